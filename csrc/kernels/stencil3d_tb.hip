// K explicit 3D diffusion steps per HBM sweep (temporal blocking) for CDNA4
// (gfx950): T2[b] = f^K(T)[b] on a list of boxes, the intermediate levels being
// f on the interior [1,n-1)^3 and T on the six faces. Bitwise equal to K
// launches of stencil3d.hip on the full interior followed by a crop to the
// boxes (StencilCoef3's expression, compiled without contraction). K = 2 is
// instantiated; the kernel is a template over K.
//
// Design (the z register march of stencil3d.hip, skewed in time):
//   * Model traffic per pass: one read of T, one read of 1/Cp, one write of T2,
//     24 B per cell for K steps.
//   * One 64-lane wave owns an x-strip of 64*V cells and R output rows. It loads
//     R + 2K rows of every plane (rows ya-K .. ya+R+K-1) and recomputes the lower
//     levels at the band seams itself: no LDS, no barrier, waves independent.
//     Level l lives on the rows [l, R+2K-l) of that window.
//   * Along z the levels are skewed: when plane p of level 0 arrives, level l
//     computes its plane p-l from the planes p-l-1, p-l, p-l+1 of level l-1, so
//     plane p-K of level K is stored. Each level keeps three planes in registers,
//     1/Cp one plane per level. A chunk loads K planes before and K planes after
//     its output planes (the first two before the march starts).
//   * In x a strip loads 64*V columns plus one edge column per side for level 0
//     (lanes 0-31 the cell left of the strip, 32-63 the cell right of it), so
//     level 1 is valid on the whole strip and level l on the columns
//     [l-1, 64V-l]; x neighbours come from the adjacent lane. Strips advance by
//     64*V - 2(K-1) columns (126 at V = 2, K = 2: even, a lane's pair stays
//     16-byte aligned). At an array face every level is exact (the face cell
//     keeps T), so a strip that touches it is valid up to it.
//   * A level-l cell on an array face takes the level l-1 value (T) unchanged.
//     Planes, rows and lanes past the array edge load clamped and store masked;
//     what they compute feeds only masked cells. All offsets are 64-bit.
//   * T2 stores and 1/Cp loads can be non-temporal (tb_nontemporal bits 0 and 1);
//     plain accesses measured 6-7 % faster here, unlike in the one-step kernel,
//     and are the default. Blocks are ordered per XCD (xcd_remap) as in the
//     one-step kernel: four waves of a block own four adjacent bands of one strip.
//   * Odd nx or a base off 16-byte alignment runs the same march with V = 1.
//     There is no thin-box path: every box runs the strip march, unless
//     Stencil3DTuning::xface = W > 0 (opt-in) sends it to the x-face kernel below
//     (boxes at most min(W, 30) wide at K = 2, the x slabs of a two-step frame).
//
// VGPRs / waves per SIMD at K = 2 (build's resource output; no AGPRs, no scratch):
// (V, R) = (2, 2) 162 / 3, (2, 4) 230 / 2, (1, 2) 98 / 4, (1, 4) 132 / 3, the same
// for every non-temporal mask. (2, 4) measured 8-13 % ahead of (2, 2)
// (profiles/diffusion3d_temporal.md).
// With Uni (uniform 1/Cp, Stencil3DTuning::uniform: the factor is a kernel
// argument, no ic registers, no ic shift, no 1/Cp loads, 16 B per cell; the same
// expression, bitwise the field path; either store setting, no AGPRs, no scratch):
// (V, R) = (2, 2) 136 / 3, (2, 4) 184 / 2, (1, 2) 90 / 5, (1, 4) 114 / 4.
// fast7 (Stencil3DTuning::fast_math, template parameter A = kFast7; rma/kernels.h: the
// 7-point sum with the folded constants as the kernel argument, explicit fmas, no flux
// temporaries; the field path keeps ic and multiplies by gs at use, Uni takes
// g = gs * value; bitwise equal to stencil3dk7_boxes_cpu; no AGPRs, no scratch):
// (V, R) = (2, 2) 154 / 3, (2, 4) 222 / 2, (1, 2) 94 / 5, (1, 4) 128 / 4; with Uni
// (2, 2) 126 / 4, (2, 4) 180 / 2, (1, 2) 82 / 5, (1, 4) 102 / 4. (2, 4) stays at 2 waves
// (3 need 168 or fewer). Same-run against canonical: 1.01-1.06x on the field path,
// 1.15-1.24x with Uni (profiles/diffusion3d_fastmath.md).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "rma/hip_check.h"
#include "rma/kernels.h"
#include "stencil3d_device.h"

namespace rma {
namespace {
using namespace march;

// Sig (Stencil3DTuning::signal, frame-first fused passes; stencil3d_device.h
// SigArg): the blocks of the signal prefix keep dispatch order and each way out of
// the kernel counts the wave. Instantiated for R = kTbDefaultRows only. Without
// Sig sg is empty and this is the kernel it was: the 48 instantiations above keep
// their registers, scratch and occupancy (profiles/diffusion3d_fused.md).
template <int K, int V, int R, bool NTS, bool NTL, bool Uni = false, int A = kCanonical3,
          bool Sig = false>
__global__ __launch_bounds__(kBlock) void stencil3d_tb_kernel(double* __restrict__ T2,
                                                              const double* __restrict__ T,
                                                              Factor<Uni> iCp,
                                                              int64_t nx, int64_t ny, int64_t nz,
                                                              BoxList L, Coef3<A> k,
                                                              int remap, SigArg<Sig> sg) {
  constexpr int NR = R + 2 * K;                 // rows of the level-0 window
  constexpr int64_t kStep = kWave * V - 2 * (K - 1);  // strip advance
  const auto [bi, lb, wave] = locate_block(L, remap, sg);
  const Box box = L.b[bi];
  const int64_t plane = nx * ny;
  // block lb of a box: strip fastest, then the group of 4 bands, then the z chunk
  const int64_t strip = lb % L.strips[bi];
  const int64_t rest = lb / L.strips[bi];
  const int64_t band = (rest % L.groups[bi]) * kWavesPerBlock + wave;
  const int64_t zc = rest / L.groups[bi];
  if (band >= L.bands[bi]) {  // the whole wave
    if constexpr (Sig) sg.wave_done();
    return;
  }
  const int64_t xs = L.xa[bi] + strip * kStep;
  const int64_t ya = box.y0 + band * R;
  const int64_t za = box.z0 + zc * L.chunk_z[bi];
  const int64_t zb = min(box.z1, za + L.chunk_z[bi]);

  const int lane = threadIdx.x & (kWave - 1);
  const int64_t x = xs + (int64_t)lane * V;  // first cell of the lane
  const int64_t xl = min(x, nx - V);         // clamped load column
  const int64_t eidx = (lane < 32) ? max(xs - 1, (int64_t)0) : min(xs + kWave * V, nx - 1);
  // columns on which level K is valid: all the way to an array face the strip touches
  const int clo = xs == 0 ? 0 : K - 1;
  const int chi = xs + kWave * V >= nx ? kWave * V - 1 : kWave * V - K;
  bool m[V], xface[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int c = lane * V + v;
    m[v] = (x + v >= box.x0) && (x + v < box.x1) && c >= clo && c <= chi;
    xface[v] = (x + v <= 0) || (x + v >= nx - 1);
  }
  const int nrows = (int)min((int64_t)R, box.y1 - ya);  // output rows inside the box
  int64_t row[NR];  // element offset of window row j (global row ya-K+j, clamped)
  bool rface[NR];   // that row lies on (or past) an array face
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int64_t g = ya - K + j;
    row[j] = min(max(g, (int64_t)0), ny - 1) * nx;
    rface[j] = g <= 0 || g >= ny - 1;
  }

  // Lv[l][s][j]: level l, plane slot s (planes p-l-2, p-l-1, p-l when plane p of
  // level 0 is the newest), window row j. ic[l]: 1/Cp of plane p-l-1.
  double Lv[K][3][NR][V], ic[Uni ? 1 : K][Uni ? 1 : NR][V];
#pragma unroll
  for (int l = 0; l < K; ++l)
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
      for (int v = 0; v < V; ++v) {
        Lv[l][0][j][v] = Lv[l][1][j][v] = Lv[l][2][j][v] = 0.0;
        if constexpr (!Uni) ic[l][j][v] = 0.0;
      }
  int64_t p = za - K + 2;
  {
    const double* p0 = T + min(max(p - 2, (int64_t)0), nz - 1) * plane;
    const double* p1 = T + min(max(p - 1, (int64_t)0), nz - 1) * plane;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      load_row<V>(Lv[0][0][j], p0 + row[j] + xl);
      load_row<V>(Lv[0][1][j], p1 + row[j] + xl);
    }
  }
  for (; p < zb + K; ++p) {
    const int64_t pc = min(max(p - 1, (int64_t)0), nz - 1);  // centre plane of level 1
    const double* pf = T + min(max(p, (int64_t)0), nz - 1) * plane;
    double ed[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) load_row<V>(Lv[0][2][j], pf + row[j] + xl);
#pragma unroll
    for (int j = 1; j < NR - 1; ++j) {
      if constexpr (!Uni) load_row<V, NTL>(ic[0][j], iCp + pc * plane + row[j] + xl);
      ed[j] = T[pc * plane + row[j] + eidx];
    }
#pragma unroll
    for (int l = 1; l <= K; ++l) {
      const int64_t z = p - l;  // plane this level computes
      if (l == K && z < za) continue;  // warm-up: nothing to store yet
      const bool zface = z <= 0 || z >= nz - 1;
#pragma unroll
      for (int j = l; j < NR - l; ++j) {
        const double(&cu)[V] = Lv[l - 1][1][j];
        const double(&up)[V] = Lv[l - 1][1][j - 1];
        const double(&dn)[V] = Lv[l - 1][1][j + 1];
        double left = __shfl_up(cu[V - 1], 1);
        double right = __shfl_down(cu[0], 1);
        if (l == 1) {
          if (lane == 0) left = ed[j];
          if (lane == kWave - 1) right = ed[j];
        }
        double res[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const double a = v == 0 ? left : cu[v == 0 ? 0 : v - 1];
          const double c = v == V - 1 ? right : cu[v == V - 1 ? v : v + 1];
          double f;
          if constexpr (Uni) f = iCp; else f = ic[l - 1][j][v];
          res[v] = update3<A, Uni>(a, cu[v], c, up[v], dn[v], Lv[l - 1][0][j][v],
                                   Lv[l - 1][2][j][v], f, k);
        }
        if (l < K) {
#pragma unroll
          for (int v = 0; v < V; ++v)
            Lv[l < K ? l : 0][2][j][v] = (zface || rface[j] || xface[v]) ? cu[v] : res[v];
        } else if (j - K < nrows) {
          store_row<V, NTS>(T2 + z * plane + row[j] + x, res, m);
        }
      }
    }
#pragma unroll
    for (int l = 0; l < K; ++l)
#pragma unroll
      for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int v = 0; v < V; ++v) {
          Lv[l][0][j][v] = Lv[l][1][j][v];
          Lv[l][1][j][v] = Lv[l][2][j][v];
        }
    if constexpr (!Uni) {
#pragma unroll
      for (int l = K - 1; l > 0; --l)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
          for (int v = 0; v < V; ++v) ic[l][j][v] = ic[l - 1][j][v];
    }
  }
  if constexpr (Sig) sg.wave_done();
}

// ---------------------------------------------------------------------------
// x-face path (Stencil3DTuning::xface): boxes narrow in x, the x slabs of a
// frame / interior split. The strip march loads 64*V columns a row for them,
// about nine times the cells a 14-wide slab updates. Here the same march runs
// narrower in x and stacked in y:
//   * A wave is RG = 64/LX groups of LX lanes (LX = 8, 16, 32). A group owns one
//     x segment of LX columns, one cell per lane (scalar 8-byte accesses: no
//     alignment or even-nx requirement), and a band of R output rows. It holds
//     the R + 2K window rows of every level in registers exactly as the strip
//     march does, Lv[K][3][NR] and ic[K][NR] on the field path, and marches along
//     z skewed in time by level: K planes before and after a chunk, warm-up
//     without stores. y neighbours are window rows in the lane's own registers:
//     no cross-lane y traffic.
//   * The band of a group is (the block's wave band) * RG + lane / LX. A group
//     whose band is past the box is masked (it loads clamped and stores nothing);
//     the wave leaves early only when all its groups are past the box.
//   * x neighbours come from the adjacent lane (__shfl_up/down by 1); for level 1
//     the first and last lane of a group take theirs from one edge load per
//     window row (lanes i < LX/2 the column left of the segment, the others the
//     column right of it, both clamped into the array). Level l is then valid on
//     the lanes [l-1, LX-l] of the group, or up to an array face the segment
//     touches: the clo / chi rule of the strip march with LX in place of 64*V.
//   * The segment starts K-1 columns left of the box and never left of column 0;
//     a box of width W fits when W + 2(K-1) <= LX (plan_dispatch3d picks the
//     smallest class: at K = 2 widths up to 6, 14, 30). One face box is one
//     segment: there is no strip loop.
//   * A level-l cell on an array face keeps the level l-1 value. Lanes, rows and
//     planes past the array load clamped and store masked, and what they compute
//     feeds only masked cells: a stored level-K cell on lane i in [clo, chi] reads
//     level l on the lanes i-(K-l) .. i+(K-l) of its own group, all inside
//     [l-1, LX-l] or bounded by a face cell, which takes no neighbour at all; the
//     lanes 0 and LX-1, the only ones a shuffle feeds from another group (or from
//     a masked one), are outside that range at every level >= 2 and take the edge
//     load at level 1. In y a lane reads only its own window rows, whose level-l
//     rows [l, NR-l) cover what the R output rows need; rows and planes on or
//     past a face keep the lower level, so their clamped copies are never read
//     through. A masked group computes on clamped loads and stores nothing.
//   * Block list: FaceList of stencil3d_device.h, groups of wave bands fastest, then
//     the z chunk. One launch per lanes-per-segment class in use, on the same
//     stream ahead of the march of the remaining boxes. No LDS, no barrier, no
//     atomics; all offsets 64-bit.
//   * The same update3 expression in the same order: bitwise the strip march's
//     cells. T2 stores follow tb_nontemporal bit 0; bit 1 (non-temporal 1/Cp
//     loads) is not instantiated for this path, which keeps it at 48
//     instantiations: 1/Cp loads are plain, the measured default of the march.
//   * R follows tb_rows (2 or 4) and the planes per task tb_chunk_z; 0 takes the
//     face path's own defaults, 2 rows and 16 planes (profiles/diffusion3d_hide.md
//     section 4: of rows 2 / 4 x planes 16 / 32 the pair with the smallest worst
//     case over widths 2-30 and 256^3-1024^3; 4 rows x 32 planes, the march's
//     default, is up to 2.6x slower on a 256^3 face, which has few tasks).
// VGPRs / waves per SIMD at K = 2 (build's resource output; no AGPRs, no scratch,
// no LDS; the same for LX = 8, 16, 32 and both store settings):
// canonical field R = 2: 110 / 4, R = 4: 150 / 3; canonical Uni 96 / 5, 132 / 3;
// fast7 field 107 / 4, 149 / 3; fast7 Uni 94 / 5, 128 / 4.
// The 48 stencil3d_tb_kernel instantiations compile to the registers, scratch and
// occupancy listed at the top of this file, as before this path was added (the
// launcher splits the box list on the host; the strip march is untouched).
// ---------------------------------------------------------------------------
constexpr int kTbFaceDefaultRows = 2;

template <int K, int LX, int R, bool NTS, bool Uni, int A>
__global__ __launch_bounds__(kBlock) void stencil3d_tb_xface_kernel(double* __restrict__ T2,
                                                                    const double* __restrict__ T,
                                                                    Factor<Uni> iCp, int64_t nx,
                                                                    int64_t ny, int64_t nz,
                                                                    FaceList L, Coef3<A> k) {
  static_assert(LX == 8 || LX == 16 || LX == 32, "lanes per segment");
  constexpr int RG = kWave / LX;  // groups of a wave
  constexpr int NR = R + 2 * K;   // rows of the level-0 window
  const auto [bi, lb, wave] = locate_block(L, 0);
  const Box box = L.b[bi];
  const int64_t plane = nx * ny;
  // block lb of a box: the group of 4 wave bands fastest, then the z chunk
  const int64_t wband = (lb % L.groups[bi]) * kWavesPerBlock + wave;
  const int64_t zc = lb / L.groups[bi];
  if (wband * RG >= L.bands[bi]) return;  // every group of the wave is past the box
  const int lane = threadIdx.x & (kWave - 1);
  const int i = lane % LX;
  const int64_t band = wband * RG + lane / LX;
  const bool live = band < L.bands[bi];  // group-uniform
  const int64_t xs = L.xs[bi];
  const int64_t ya = box.y0 + band * R;
  const int64_t za = box.z0 + zc * L.chunk_z[bi];
  const int64_t zb = min(box.z1, za + L.chunk_z[bi]);

  const int64_t x = xs + i;             // the lane's column
  const int64_t xl = min(x, nx - 1);    // clamped load column
  const int64_t eidx = (i < LX / 2) ? max(xs - 1, (int64_t)0) : min(xs + LX, nx - 1);
  // lanes on which level K is valid: all the way to an array face the segment touches
  const int clo = xs == 0 ? 0 : K - 1;
  const int chi = xs + LX >= nx ? LX - 1 : LX - K;
  const bool m = live && x >= box.x0 && x < box.x1 && i >= clo && i <= chi;
  const bool xface = x <= 0 || x >= nx - 1;
  // output rows of the group inside the box (none for a masked group)
  const int nrows = live ? (int)min((int64_t)R, box.y1 - ya) : 0;
  int64_t row[NR];  // element offset of window row j (global row ya-K+j, clamped)
  bool rface[NR];   // that row lies on (or past) an array face
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int64_t g = ya - K + j;
    row[j] = min(max(g, (int64_t)0), ny - 1) * nx;
    rface[j] = g <= 0 || g >= ny - 1;
  }

  // Lv[l][s][j]: level l, plane slot s (planes p-l-2, p-l-1, p-l when plane p of
  // level 0 is the newest), window row j. ic[l]: 1/Cp of plane p-l-1.
  double Lv[K][3][NR], ic[Uni ? 1 : K][Uni ? 1 : NR];
#pragma unroll
  for (int l = 0; l < K; ++l)
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      Lv[l][0][j] = Lv[l][1][j] = Lv[l][2][j] = 0.0;
      if constexpr (!Uni) ic[l][j] = 0.0;
    }
  int64_t p = za - K + 2;
  {
    const double* p0 = T + min(max(p - 2, (int64_t)0), nz - 1) * plane;
    const double* p1 = T + min(max(p - 1, (int64_t)0), nz - 1) * plane;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      Lv[0][0][j] = p0[row[j] + xl];
      Lv[0][1][j] = p1[row[j] + xl];
    }
  }
  for (; p < zb + K; ++p) {
    const int64_t pc = min(max(p - 1, (int64_t)0), nz - 1);  // centre plane of level 1
    const double* pf = T + min(max(p, (int64_t)0), nz - 1) * plane;
    double ed[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) Lv[0][2][j] = pf[row[j] + xl];
#pragma unroll
    for (int j = 1; j < NR - 1; ++j) {
      if constexpr (!Uni) ic[0][j] = iCp[pc * plane + row[j] + xl];
      ed[j] = T[pc * plane + row[j] + eidx];
    }
#pragma unroll
    for (int l = 1; l <= K; ++l) {
      const int64_t z = p - l;  // plane this level computes
      if (l == K && z < za) continue;  // warm-up: nothing to store yet
      const bool zface = z <= 0 || z >= nz - 1;
#pragma unroll
      for (int j = l; j < NR - l; ++j) {
        const double cu = Lv[l - 1][1][j];
        double left = __shfl_up(cu, 1);
        double right = __shfl_down(cu, 1);
        if (l == 1) {
          if (i == 0) left = ed[j];
          if (i == LX - 1) right = ed[j];
        }
        double f;
        if constexpr (Uni) f = iCp; else f = ic[l - 1][j];
        const double res = update3<A, Uni>(left, cu, right, Lv[l - 1][1][j - 1],
                                           Lv[l - 1][1][j + 1], Lv[l - 1][0][j],
                                           Lv[l - 1][2][j], f, k);
        if (l < K) {
          Lv[l < K ? l : 0][2][j] = (zface || rface[j] || xface) ? cu : res;
        } else if (m && j - K < nrows) {
          store1<NTS>(T2 + z * plane + row[j] + x, res);
        }
      }
    }
#pragma unroll
    for (int l = 0; l < K; ++l)
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        Lv[l][0][j] = Lv[l][1][j];
        Lv[l][1][j] = Lv[l][2][j];
      }
    if constexpr (!Uni) {
#pragma unroll
      for (int l = K - 1; l > 0; --l)
#pragma unroll
        for (int j = 0; j < NR; ++j) ic[l][j] = ic[l - 1][j];
    }
  }
}

}  // namespace

bool stencil3dk_has(int K) { return K == 1 || K == 2; }
bool stencil3dk_has_rows(int rows) { return rows == 2 || rows == 4; }

void stencil3dk_boxes_gpu(int K, double* T2, const double* T, const double* iCp, int64_t nx,
                          int64_t ny, int64_t nz, const Box* boxes, int nboxes,
                          const StencilCoef3& c, const Stencil3DTuning& tune, stream_t stream) {
  RMA_CHECK_ARG(stencil3dk_has(K), "K=" << K << " steps per pass is not instantiated (1 or 2)");
  if (K == 1) {
    stencil3d_boxes_gpu(T2, T, iCp, nx, ny, nz, boxes, nboxes, c, tune, stream);
    return;
  }
  validate_boxes(T2, T, nx, ny, nz, boxes, nboxes);
  const int R = tune.tb_rows > 0 ? tune.tb_rows : kTbDefaultRows;
  RMA_CHECK_ARG(stencil3dk_has_rows(R), "tb_rows=" << tune.tb_rows << " (0: default, 2 or 4)");
  check_tuning3d(tune, c, "tb_", tune.tb_nontemporal, tune.tb_chunk_z);
  // plan_launch3d runs split_boxes3d (kernel_select.cpp), which checks tune.xface
  // and sorts the boxes by plan_dispatch3d's path: face boxes leave the list for
  // the x-face kernel, launched first on the same stream, the rest keep their
  // order in the strip march. xface = 0 has no face boxes: the caller's list,
  // launch for launch. With a signal it also checks signal_boxes and tb_rows, and
  // no box takes the face path.
  const int Rf = tune.tb_rows > 0 ? tune.tb_rows : kTbFaceDefaultRows;
  const int V = stencil3d_vec(T2, T, iCp, nx, tune);
  BoxList L{};
  Split3D sp;
  const Fused3DPlan plan =
      plan_launch3d(L, sp, K, V, boxes, nboxes, tune, tune.signal != nullptr, tune.signal_boxes);
  const int64_t total = plan.blocks;
  if (L.n == 0 && !sp.faces()) return;
  const dim3 grid = grid_of(total), block(kBlock);
  hipStream_t s = as_stream(stream);
  const int nt = tune.tb_nontemporal, remap = tune.xcd_remap ? 1 : 0;
  with_arith3(c, tune, [&](auto a, const auto& k, double fac) {
    constexpr int A = decltype(a)::value;
    // the face boxes, one launch per lanes-per-segment class in use (a wave runs
    // 64/LX group tasks of Rf rows), ahead of the march of the rest
    for_face_classes(sp, [&](auto lx, const Box* face, int nface) {
      constexpr int LX = decltype(lx)::value;
      FaceList F{};
      const dim3 fgrid = grid_of(plan_faces(F, face, nface, K, Rf, kWave / LX, tune.tb_chunk_z));
      with_value<2, 4>(Rf, [&](auto r) {
        with_access3<false>(nt, tune.uniform, [&](auto nts, auto, auto uni) {
          constexpr bool NTS = decltype(nts)::value, Uni = decltype(uni)::value;
          stencil3d_tb_xface_kernel<2, LX, decltype(r)::value, NTS, Uni, A>
              <<<fgrid, block, 0, s>>>(T2, T, factor_arg<Uni>(iCp, fac), nx, ny, nz, F, k);
        });
      });
      RMA_HIP_LAUNCH_CHECK();
    });
    if (L.n == 0) return;  // face boxes only: checked above
    if (tune.signal) {  // the default rows (plan_launch3d), the prefix blocks first
      with_value<1, 2>(V, [&](auto v) {
        with_access3<true>(nt, tune.uniform, [&](auto nts, auto ntl, auto uni) {
          constexpr bool Uni = decltype(uni)::value;
          stencil3d_tb_kernel<2, decltype(v)::value, kTbDefaultRows, decltype(nts)::value,
                              decltype(ntl)::value, Uni, A, true>
              <<<grid, block, 0, s>>>(T2, T, factor_arg<Uni>(iCp, fac), nx, ny, nz, L, k, remap,
                                      WaveSig{tune.signal, plan.prefix_blocks});
        });
      });
      RMA_HIP_LAUNCH_CHECK();
      return;
    }
    with_value<1, 2>(V, [&](auto v) {
      with_value<2, 4>(R, [&](auto r) {
        with_access3<true>(nt, tune.uniform, [&](auto nts, auto ntl, auto uni) {
          constexpr bool Uni = decltype(uni)::value;
          stencil3d_tb_kernel<2, decltype(v)::value, decltype(r)::value, decltype(nts)::value,
                              decltype(ntl)::value, Uni, A>
              <<<grid, block, 0, s>>>(T2, T, factor_arg<Uni>(iCp, fac), nx, ny, nz, L, k, remap,
                                      NoSig{});
        });
      });
    });
    RMA_HIP_LAUNCH_CHECK();
  });
}

}  // namespace rma
