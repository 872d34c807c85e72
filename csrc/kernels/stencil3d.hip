// Fused 7-point diffusion stencil on (nz, ny, nx) fields for CDNA4 (gfx950).
//
// One explicit 3D heat-diffusion step, T2 = f(T, 1/Cp), on a list of boxes
// (the whole interior by default; a frame / interior split launches the same
// kernel with other boxes). The arithmetic is StencilCoef3's in rma/common.h,
// compiled without contraction: bitwise equal to stencil3d_boxes_cpu.
//
// Design (the register march of stencil.hip, turned along z):
//   * 24 B/cell (read T, read 1/Cp, write T2) against ~25 fp64 flops: HBM
//     bound, so every byte of T should come from HBM once.
//   * One 64-lane wave owns an x-strip of 64*V cells (V = 2: one 16-byte access
//     per lane and row) and a band of R rows, and marches along z over chunk_z
//     planes. For its own cells it keeps plane z-1, plane z and plane z+1 in
//     registers, plus the two y-halo rows of plane z: (3R+2)*V doubles a lane.
//     Each step loads the R own rows of the next plane, the two halo rows, R
//     rows of 1/Cp and one wave-wide edge load per row (lanes 0-31 the cell left
//     of the strip, 32-63 the cell right of it); x neighbours otherwise come
//     from the adjacent lane. All loads of a step are issued before its
//     arithmetic; with unroll = 2 two planes' loads are in flight together.
//   * T is read (R+2)/R times per band (the halo rows) plus 2/chunk_z (the
//     planes before and after a z chunk). The four waves of a block own four
//     adjacent bands of one strip, and consecutive blocks adjacent strips, then
//     the next bands: with each XCD taking a contiguous range of blocks
//     (xcd_remap) the re-read rows were fetched moments before by a neighbour
//     on the same L2.
//   * T2 stores and 1/Cp loads are non-temporal (each byte is touched once).
//   * Lanes past the array edge load clamped and store masked; rows past the
//     end of a band likewise (wave-uniform). All offsets are 64-bit.
//   * Odd nx or a base off 16-byte alignment runs the same march with V = 1.
//     Boxes at most 8 cells wide (frame faces) run one thread per row.
//   * Stencil3DTuning::xface = W > 0 (opt-in): boxes at most W <= 32 cells wide
//     run the x-face kernel below instead (rows of 8, 16 or 32 lanes), launched on
//     the same stream ahead of the march of the remaining boxes.
//   * Uniform 1/Cp (Stencil3DTuning::uniform, template flag Uni): the factor is a
//     kernel argument, the array is never dereferenced and no ic registers are
//     held: 16 B/cell. The same expression in the same order, so bitwise the
//     field path's result. Bit 1 of nontemporal has nothing to act on there.
//   * fast7 (Stencil3DTuning::fast_math, template parameter A = kFast7; rma/kernels.h):
//     the 7-point sum with the folded constants as the kernel argument, explicit
//     fmas, no flux temporaries: bitwise equal to stencil3d7_boxes_cpu, rounding-
//     close to canonical. The field path keeps ic and multiplies by gs at use; Uni
//     takes g = gs * value. Same loads, stores and masks in both arithmetics, the
//     thin-box path included. HBM-bound either way: no faster than canonical
//     (profiles/diffusion3d_fastmath.md).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "rma/hip_check.h"
#include "rma/kernels.h"
#include "stencil3d_device.h"

namespace rma {
namespace {
using namespace march;

// Addresses and masks of one wave task, constant along the march.
template <int V, int R>
struct Task {
  int64_t row[R];        // element offset of own row r in a plane (row clamped into the array)
  int64_t halo[2];       // rows ya-1 and ya+R (clamped)
  int64_t eidx;          // edge column of this lane
  int64_t x, xl;         // first cell of the lane, clamped load column
  int64_t plane;         // ny * nx
  int nrows;             // rows of the band inside the box (wave-uniform)
  bool m[V];
  int lane;
};

// UU planes z .. z+UU-1: P[0] / P[1] hold the own rows of planes z-1 / z on
// entry and of planes z+UU-1 / z+UU on exit.
template <int V, int R, int UU, int NP, bool NTS, bool NTL, bool Uni, int A>
__device__ __forceinline__ void z_steps(double (&P)[NP][R][V], double* __restrict__ T2,
                                        const double* __restrict__ T, Factor<Uni> iCp,
                                        const Task<V, R>& t, int64_t z, const Coef3<A>& k) {
  static_assert(UU + 2 <= NP, "plane registers");
  double H[UU][2][V], ic[Uni ? 1 : UU][Uni ? 1 : R][V], ed[UU][R];
#pragma unroll
  for (int u = 0; u < UU; ++u) {
    const double* pc = T + (z + u) * t.plane;
    const double* pn = pc + t.plane;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      load_row<V>(P[u + 2][r], pn + t.row[r] + t.xl);
      if constexpr (!Uni) load_row<V, NTL>(ic[u][r], iCp + (z + u) * t.plane + t.row[r] + t.xl);
      ed[u][r] = pc[t.row[r] + t.eidx];
    }
    load_row<V>(H[u][0], pc + t.halo[0] + t.xl);
    load_row<V>(H[u][1], pc + t.halo[1] + t.xl);
  }
#pragma unroll
  for (int u = 0; u < UU; ++u) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double(&cu)[V] = P[u + 1][r];
      const double(&up)[V] = r == 0 ? H[u][0] : P[u + 1][r == 0 ? 0 : r - 1];
      const double(&dn)[V] = r == R - 1 ? H[u][1] : P[u + 1][r == R - 1 ? r : r + 1];
      double left = __shfl_up(cu[V - 1], 1);
      double right = __shfl_down(cu[0], 1);
      if (t.lane == 0) left = ed[u][r];
      if (t.lane == kWave - 1) right = ed[u][r];
      double res[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const double xl = v == 0 ? left : cu[v == 0 ? 0 : v - 1];
        const double xr = v == V - 1 ? right : cu[v == V - 1 ? v : v + 1];
        double f;
        if constexpr (Uni) f = iCp; else f = ic[u][r][v];
        res[v] = update3<A, Uni>(xl, cu[v], xr, up[v], dn[v], P[u][r][v], P[u + 2][r][v], f, k);
      }
      if (r < t.nrows) store_row<V, NTS>(T2 + (z + u) * t.plane + t.row[r] + t.x, res, t.m);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
      P[0][r][v] = P[UU][r][v];
      P[1][r][v] = P[UU + 1][r][v];
    }
  }
}

// VGPRs / waves per SIMD at V = 2 (build's resource output): (R, U) = (2, 1) 78 / 6,
// (2, 2) 139 / 3, (4, 1) 134 / 3, (4, 2) 227 / 2, (8, 1) 239 / 2; no scratch. Capping
// (2, 2) and (4, 1) at the 128 registers of 4 waves spills 12-28 bytes per lane.
// With Uni (either store setting; no AGPRs, no scratch): V = 2 (2, 1) 70 / 7, (2, 2) 115 / 4,
// (4, 1) 110 / 4, (4, 2) 179 / 2, (8, 1) 191 / 2; V = 1 (2, 1) 52 / 8, (2, 2) 88 / 5,
// (4, 1) 70 / 7, (4, 2) 137 / 3, (8, 1) 135 / 3.
// fast7 (no AGPRs, no scratch), field: V = 2 (2, 1) 74 / 6, (2, 2) 129 / 3, (4, 1) 126 / 4,
// (4, 2) 217 / 2, (8, 1) 231 / 2; V = 1 (2, 1) 54 / 8, (2, 2) 96 / 5, (4, 1) 88 / 5, (4, 2) 161 / 3,
// (8, 1) 161 / 3. fast7 with Uni: V = 2 (2, 1) 62 / 8, (2, 2) 104 / 4, (4, 1) 102 / 4,
// (4, 2) 169 / 2, (8, 1) 183 / 2; V = 1 (2, 1) 50 / 8, (2, 2) 80 / 6, (4, 1) 70 / 7, (4, 2) 129 / 3,
// (8, 1) 126-127 / 4.
// Sig (Stencil3DTuning::signal, frame-first fused passes; stencil3d_device.h
// SigArg): the blocks of the signal prefix keep dispatch order and each way out of
// the kernel counts the wave. Instantiated for R = 4, U = 2 (the shipped tuning)
// only. Without Sig sg is empty and this is the kernel it was: the 120
// instantiations above keep their registers, scratch and occupancy
// (profiles/diffusion3d_fused.md).
template <int V, int R, int U, bool NTS, bool NTL, bool Uni = false, int A = kCanonical3,
          bool Sig = false>
__global__ __launch_bounds__(kBlock) void stencil3d_march_kernel(double* __restrict__ T2,
                                                                 const double* __restrict__ T,
                                                                 Factor<Uni> iCp,
                                                                 int64_t nx, int64_t ny,
                                                                 BoxList L, Coef3<A> k,
                                                                 int remap, SigArg<Sig> sg) {
  const auto [bi, lb, wave] = locate_block(L, remap, sg);
  const Box box = L.b[bi];
  const int64_t plane = nx * ny;
  if (L.chunk_z[bi] < 0) {
    // thin box: one thread per (z, y) row, scalar accesses (a 64*V-cell strip
    // would load up to 128 times the bytes it updates)
    const int64_t rows = box.y1 - box.y0;
    const int64_t i = lb * kBlock + threadIdx.x;
    if (i >= rows * (box.z1 - box.z0)) {
      if constexpr (Sig) sg.wave_done();  // counts only where the whole wave is past the box
      return;
    }
    const int64_t z = box.z0 + i / rows, y = box.y0 + i % rows;
    const int64_t o = z * plane + y * nx;
    for (int64_t x = box.x0; x < box.x1; ++x) {
      double f;
      if constexpr (Uni) f = iCp; else f = iCp[o + x];
      const double v = update3<A, Uni>(T[o + x - 1], T[o + x], T[o + x + 1], T[o - nx + x],
                                       T[o + nx + x], T[o - plane + x], T[o + plane + x], f, k);
      // written out, not store1: through the helper the 20 plain-store uniform
      // instantiations compile to other registers and SGPR spills than they had
      if constexpr (NTS) {
        __builtin_nontemporal_store(v, T2 + o + x);
      } else {
        T2[o + x] = v;
      }
    }
    if constexpr (Sig) sg.wave_done();
    return;
  }
  // block lb of a box: strip fastest, then the group of 4 bands, then the z chunk
  const int64_t strip = lb % L.strips[bi];
  const int64_t rest = lb / L.strips[bi];
  const int64_t band = (rest % L.groups[bi]) * kWavesPerBlock + wave;
  const int64_t zc = rest / L.groups[bi];
  if (band >= L.bands[bi]) {  // the whole wave
    if constexpr (Sig) sg.wave_done();
    return;
  }
  const int64_t xs = L.xa[bi] + strip * (kWave * V);
  const int64_t ya = box.y0 + band * R;
  const int64_t za = box.z0 + zc * L.chunk_z[bi];
  const int64_t zb = min(box.z1, za + L.chunk_z[bi]);

  Task<V, R> t;
  t.lane = threadIdx.x & (kWave - 1);
  t.plane = plane;
  t.x = xs + (int64_t)t.lane * V;
  t.xl = min(t.x, nx - V);
#pragma unroll
  for (int v = 0; v < V; ++v) t.m[v] = (t.x + v >= box.x0) && (t.x + v < box.x1);
  t.eidx = (t.lane < 32) ? max(xs - 1, (int64_t)0) : min(xs + kWave * V, nx - 1);
  t.nrows = (int)min((int64_t)R, box.y1 - ya);
#pragma unroll
  for (int r = 0; r < R; ++r) t.row[r] = min(ya + r, ny - 1) * nx;
  t.halo[0] = (ya - 1) * nx;
  t.halo[1] = min(ya + R, ny - 1) * nx;

  double P[U + 2][R][V];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    load_row<V>(P[0][r], T + (za - 1) * plane + t.row[r] + t.xl);
    load_row<V>(P[1][r], T + za * plane + t.row[r] + t.xl);
  }
  int64_t z = za;
  for (; z + U <= zb; z += U) z_steps<V, R, U, U + 2, NTS, NTL, Uni, A>(P, T2, T, iCp, t, z, k);
  if constexpr (U > 1) {
    for (; z < zb; ++z) z_steps<V, R, 1, U + 2, NTS, NTL, Uni, A>(P, T2, T, iCp, t, z, k);
  }
  if constexpr (Sig) sg.wave_done();
}

// ---------------------------------------------------------------------------
// x-face path (Stencil3DTuning::xface): boxes at most 32 cells wide in x, the
// x slabs of a frame / interior split. The strip march would load 128 cells a
// row for them and the thin-box path reads stride-nx scalars; here a wave is
// 64/LX rows of LX lanes (LX = 8, 16, 32: the smallest >= the box width), lane
// (r, i) owns cell (ya + r, x0 + i) and marches along z with planes z-1, z, z+1
// of its cell in registers: every wave-level plane load is 64/LX contiguous row
// segments of LX*8 bytes, each centre value comes from memory once per task
// plus two planes per z chunk. x neighbours come from the adjacent lane; lanes
// i = 0 / LX-1 take theirs from one edge load (lanes of the low half the column
// left of the box, of the high half column x0+LX). y neighbours come from the
// lane LX away; rows r = 0 / 64/LX-1 take theirs from one halo-row load.
// Columns and rows past the box load clamped into the array, which is what the
// last cell of the box needs from its neighbour lane, and store masked. The
// loads of plane z+2 and of the edge, halo and 1/Cp values of plane z+1 are
// issued before the arithmetic of plane z. No LDS, no barrier; 64-bit offsets.
// The same update3 expression: bitwise the other paths' result.
// VGPRs / waves per SIMD (build's resource output; no AGPRs, no scratch, no LDS;
// the same for LX = 8, 16, 32 and both store settings): canonical field 42 / 8,
// canonical Uni 36 / 8, fast7 field 44 / 8, fast7 Uni 38 / 8. The 120 march
// instantiations above compile to the registers, scratch and occupancy they had
// before this path was added (the launcher splits the box list on the host; the
// march kernel is untouched).
// ---------------------------------------------------------------------------
template <int LX, bool NTS, bool Uni, int A>
__global__ __launch_bounds__(kBlock) void stencil3d_xface_kernel(double* __restrict__ T2,
                                                                 const double* __restrict__ T,
                                                                 Factor<Uni> iCp, int64_t nx,
                                                                 int64_t ny, FaceList L,
                                                                 Coef3<A> k) {
  constexpr int RG = kWave / LX;  // rows of a wave
  static_assert(LX == 8 || LX == 16 || LX == 32, "lanes per row");
  const auto [bi, lb, wave] = locate_block(L, 0);
  const Box box = L.b[bi];
  // block lb of a box: the group of 4 bands fastest, then the z chunk
  const int64_t band = (lb % L.groups[bi]) * kWavesPerBlock + wave;
  const int64_t zc = lb / L.groups[bi];
  if (band >= L.bands[bi]) return;  // the whole wave
  const int64_t plane = nx * ny;
  const int64_t ya = box.y0 + band * RG;
  const int64_t za = box.z0 + zc * L.chunk_z[bi];
  const int64_t zb = min(box.z1, za + L.chunk_z[bi]);
  const int lane = threadIdx.x & (kWave - 1);
  const int i = lane % LX, r = lane / LX;
  const int64_t x = box.x0 + i, y = ya + r;
  const bool m = x < box.x1 && y < box.y1;
  const int64_t xc = min(x, nx - 1);
  const int64_t row = min(y, ny - 1) * nx;
  const int64_t o = row + xc;
  const int64_t oe = row + (i < LX / 2 ? box.x0 - 1 : min(box.x0 + LX, nx - 1));
  const int64_t oh = (r < RG / 2 ? ya - 1 : min(ya + RG, ny - 1)) * nx + xc;

  const double* p = T + za * plane;
  double bk = p[o - plane], c = p[o], fr = p[o + plane];
  double e = p[oe], h = p[oh], f;
  if constexpr (Uni) f = iCp; else f = iCp[za * plane + o];
  for (int64_t z = za; z < zb; ++z) {
    // plane z+2 (the last step loads plane zb again, unused) and the edge, halo
    // and 1/Cp values of plane z+1 <= zb <= nz-1
    const double* pn = T + (z + 1) * plane;
    const double fr2 = T[min(z + 2, zb) * plane + o];
    const double e2 = pn[oe], h2 = pn[oh];
    double f2;
    if constexpr (Uni) f2 = iCp; else f2 = iCp[(z + 1) * plane + o];
    double left = __shfl_up(c, 1), right = __shfl_down(c, 1);
    double up = __shfl_up(c, LX), dn = __shfl_down(c, LX);
    if (i == 0) left = e;
    if (i == LX - 1) right = e;
    if (r == 0) up = h;
    if (r == RG - 1) dn = h;
    const double v = update3<A, Uni>(left, c, right, up, dn, bk, fr, f, k);
    if (m) store1<NTS>(T2 + z * plane + o, v);
    bk = c;
    c = fr;
    fr = fr2;
    e = e2;
    h = h2;
    f = f2;
  }
}

// f(R, U) for the instantiated (rows, unroll) pairs: the list stencil3d_has accepts
template <class F>
void with_rows_unroll(int R, int U, F&& f) {
  if (R == 2 && U == 1) f(int_c<2>{}, int_c<1>{});
  else if (R == 2 && U == 2) f(int_c<2>{}, int_c<2>{});
  else if (R == 4 && U == 1) f(int_c<4>{}, int_c<1>{});
  else if (R == 4 && U == 2) f(int_c<4>{}, int_c<2>{});
  else if (R == 8 && U == 1) f(int_c<8>{}, int_c<1>{});
  else RMA_CHECK_ARG(false, "rows=" << R << " unroll=" << U << " has no instantiation");
}
}  // namespace

bool stencil3d_has(int rows, int unroll) {
  return ((rows == 2 || rows == 4) && (unroll == 1 || unroll == 2)) || (rows == 8 && unroll == 1);
}

int stencil3d_vec(const double* T2, const double* T, const double* iCp, int64_t nx,
                  const Stencil3DTuning& tune) {
  // the uniform variant does not read 1/Cp: its alignment does not count
  const bool aligned = ((reinterpret_cast<uintptr_t>(T) | reinterpret_cast<uintptr_t>(T2) |
                         (tune.uniform ? 0 : reinterpret_cast<uintptr_t>(iCp))) & 15) == 0;
  return (aligned && nx % 2 == 0) ? tune.vec : 1;
}

void stencil3d_boxes_gpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                         int64_t nz, const Box* boxes, int nboxes, const StencilCoef3& c,
                         const Stencil3DTuning& tune, stream_t stream) {
  validate_boxes(T2, T, nx, ny, nz, boxes, nboxes);
  RMA_CHECK_ARG(stencil3d_has(tune.rows, tune.unroll),
                "rows=" << tune.rows << " unroll=" << tune.unroll
                        << ": rows 2 or 4 with unroll 1 or 2, or rows 8 with unroll 1");
  check_tuning3d(tune, c, "", tune.nontemporal, tune.chunk_z);
  // plan_launch3d runs split_boxes3d (kernel_select.cpp), which checks tune.xface
  // and sorts the boxes by plan_dispatch3d's path: face boxes leave the list for
  // the x-face kernel, the rest keep their order in the march launch (strips, or
  // one thread per row for thin boxes). xface = 0 has no face boxes: the caller's
  // list. With a signal it also checks signal_boxes and the tuning, and no box
  // takes the face path.
  const int V = stencil3d_vec(T2, T, iCp, nx, tune);
  BoxList L{};
  Split3D sp;
  const Fused3DPlan plan =
      plan_launch3d(L, sp, 1, V, boxes, nboxes, tune, tune.signal != nullptr, tune.signal_boxes);
  const int64_t total = plan.blocks;
  if (L.n == 0 && !sp.faces()) return;
  const dim3 grid = grid_of(total), block(kBlock);
  hipStream_t s = as_stream(stream);
  const int nt = tune.nontemporal, remap = tune.xcd_remap ? 1 : 0;
  with_arith3(c, tune, [&](auto a, const auto& k, double fac) {
    constexpr int A = decltype(a)::value;
    // the face boxes, one launch per lanes-per-row class in use (a wave task is
    // 64/LX rows), ahead of the march of the rest
    for_face_classes(sp, [&](auto lx, const Box* face, int nface) {
      constexpr int LX = decltype(lx)::value;
      FaceList F{};
      const dim3 fgrid = grid_of(plan_faces(F, face, nface, 1, kWave / LX, 1, tune.chunk_z));
      with_access3<false>(nt, tune.uniform, [&](auto nts, auto, auto uni) {
        constexpr bool NTS = decltype(nts)::value, Uni = decltype(uni)::value;
        stencil3d_xface_kernel<LX, NTS, Uni, A>
            <<<fgrid, block, 0, s>>>(T2, T, factor_arg<Uni>(iCp, fac), nx, ny, F, k);
      });
      RMA_HIP_LAUNCH_CHECK();
    });
    if (L.n == 0) return;  // face boxes only: checked above
    if (tune.signal) {  // the shipped tuning (plan_launch3d), the prefix blocks first
      with_value<1, 2>(V, [&](auto v) {
        with_access3<true>(nt, tune.uniform, [&](auto nts, auto ntl, auto uni) {
          constexpr bool Uni = decltype(uni)::value;
          stencil3d_march_kernel<decltype(v)::value, kSigRows, kSigUnroll, decltype(nts)::value,
                                 decltype(ntl)::value, Uni, A, true>
              <<<grid, block, 0, s>>>(T2, T, factor_arg<Uni>(iCp, fac), nx, ny, L, k, remap,
                                      WaveSig{tune.signal, plan.prefix_blocks});
        });
      });
      RMA_HIP_LAUNCH_CHECK();
      return;
    }
    with_value<1, 2>(V, [&](auto v) {
      with_rows_unroll(tune.rows, tune.unroll, [&](auto r, auto u) {
        with_access3<true>(nt, tune.uniform, [&](auto nts, auto ntl, auto uni) {
          constexpr bool Uni = decltype(uni)::value;
          stencil3d_march_kernel<decltype(v)::value, decltype(r)::value, decltype(u)::value,
                                 decltype(nts)::value, decltype(ntl)::value, Uni, A>
              <<<grid, block, 0, s>>>(T2, T, factor_arg<Uni>(iCp, fac), nx, ny, L, k, remap,
                                      NoSig{});
        });
      });
    });
    RMA_HIP_LAUNCH_CHECK();
  });
}

Fused3DPlan stencil3d_fused_plan(int K, int V, const Box* boxes, int nboxes,
                                 const Stencil3DTuning& tune, int signal_boxes, int64_t* map) {
  RMA_CHECK_ARG(K == 1 || K == 2, "K=" << K << " steps per pass is not instantiated (1 or 2)");
  RMA_CHECK_ARG(V == 1 || V == 2, "V=" << V << " cells per lane (1 or 2)");
  RMA_CHECK_ARG(signal_boxes >= 0, "signal_boxes=" << signal_boxes);
  // the launchers' tuning checks that the block lists depend on
  if (K == 1) {
    RMA_CHECK_ARG(stencil3d_has(tune.rows, tune.unroll),
                  "rows=" << tune.rows << " unroll=" << tune.unroll
                          << ": rows 2 or 4 with unroll 1 or 2, or rows 8 with unroll 1");
    RMA_CHECK_ARG(tune.chunk_z >= 0, "chunk_z=" << tune.chunk_z);
  } else {
    RMA_CHECK_ARG(tune.tb_rows == 0 || stencil3dk_has_rows(tune.tb_rows),
                  "tb_rows=" << tune.tb_rows << " (0: default, 2 or 4)");
    RMA_CHECK_ARG(tune.tb_chunk_z >= 0, "tb_chunk_z=" << tune.tb_chunk_z);
  }
  BoxList L{};
  Split3D sp;
  const Fused3DPlan plan =
      plan_launch3d(L, sp, K, V, boxes, nboxes, tune, signal_boxes > 0, signal_boxes);
  if (map) {
    const int remap = tune.xcd_remap ? 1 : 0;
    for (int64_t b = 0; b < plan.blocks; ++b) {
      // without a prefix this is locate_block's map: xcd_remap over the whole grid
      const BlockAt at = block_after(L, b, plan.blocks, remap, plan.prefix_blocks);
      map[2 * b] = at.bi;
      map[2 * b + 1] = at.lb;
    }
  }
  return plan;
}

}  // namespace rma
