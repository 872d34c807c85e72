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
#include "stencil_device.h"

namespace rma {
namespace {
using namespace march;

struct BoxList {
  Box b[kMaxBoxes];
  int64_t xa[kMaxBoxes];         // strip origin (x0 rounded down to the strip width)
  int64_t strips[kMaxBoxes];
  int64_t bands[kMaxBoxes];
  int64_t groups[kMaxBoxes];     // blocks along y: ceil(bands / waves per block)
  int64_t chunk_z[kMaxBoxes];    // planes per task; -1: thin box, one thread per row
  int64_t block_end[kMaxBoxes];  // inclusive prefix sum of blocks
  int n;
};

__device__ __forceinline__ double cell3(double xl, double c, double xr, double up, double dn,
                                        double bk, double fr, double ic, const StencilCoef3& k) {
  const double qxR = (k.mlam * (xr - c)) * k.rdx;
  const double qxL = (k.mlam * (c - xl)) * k.rdx;
  const double qyU = (k.mlam * (dn - c)) * k.rdy;
  const double qyD = (k.mlam * (c - up)) * k.rdy;
  const double qzF = (k.mlam * (fr - c)) * k.rdz;
  const double qzB = (k.mlam * (c - bk)) * k.rdz;
  return c + k.dt * (ic * (((-(qxR - qxL)) * k.rdx - (qyU - qyD) * k.rdy) - (qzF - qzB) * k.rdz));
}

// the update of one cell in arithmetic A (f: 1/Cp of the cell, or what Factor<true> holds)
template <int A, bool Uni>
__device__ __forceinline__ double update3(double xl, double c, double xr, double up, double dn,
                                          double bk, double fr, double f, const Coef3<A>& k) {
  if constexpr (A == kFast7) return cell7<Uni>(xl, c, xr, up, dn, bk, fr, f, k);
  else return cell3(xl, c, xr, up, dn, bk, fr, f, k);
}

// 1/Cp as the kernels take it: the array, or with Uni its one value (fast7: gs
// times that value)
template <bool Uni>
using Factor = std::conditional_t<Uni, double, const double* __restrict__>;

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
template <int V, int R, int U, bool NTS, bool NTL, bool Uni = false, int A = kCanonical3>
__global__ __launch_bounds__(kBlock) void stencil3d_march_kernel(double* __restrict__ T2,
                                                                 const double* __restrict__ T,
                                                                 Factor<Uni> iCp,
                                                                 int64_t nx, int64_t ny,
                                                                 BoxList L, Coef3<A> k,
                                                                 int remap) {
  const int64_t b = remap ? xcd_remap(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int bi = 0;
  while (bi < L.n - 1 && b >= L.block_end[bi]) ++bi;  // block-uniform, <= 8 steps
  const int64_t lb = b - (bi ? L.block_end[bi - 1] : 0);
  const Box box = L.b[bi];
  const int64_t plane = nx * ny;
  if (L.chunk_z[bi] < 0) {
    // thin box: one thread per (z, y) row, scalar accesses (a 64*V-cell strip
    // would load up to 128 times the bytes it updates)
    const int64_t rows = box.y1 - box.y0;
    const int64_t i = lb * kBlock + threadIdx.x;
    if (i >= rows * (box.z1 - box.z0)) return;
    const int64_t z = box.z0 + i / rows, y = box.y0 + i % rows;
    const int64_t o = z * plane + y * nx;
    for (int64_t x = box.x0; x < box.x1; ++x) {
      double f;
      if constexpr (Uni) f = iCp; else f = iCp[o + x];
      const double v = update3<A, Uni>(T[o + x - 1], T[o + x], T[o + x + 1], T[o - nx + x],
                                       T[o + nx + x], T[o - plane + x], T[o + plane + x], f, k);
      if constexpr (NTS) {
        __builtin_nontemporal_store(v, T2 + o + x);
      } else {
        T2[o + x] = v;
      }
    }
    return;
  }
  // block lb of a box: strip fastest, then the group of 4 bands, then the z chunk
  const int64_t strip = lb % L.strips[bi];
  const int64_t rest = lb / L.strips[bi];
  const int64_t band = (rest % L.groups[bi]) * kWavesPerBlock + wave;
  const int64_t zc = rest / L.groups[bi];
  if (band >= L.bands[bi]) return;  // the whole wave
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
}

// thin[i]: boxes[i] runs the thin-box path (plan_dispatch3d's kPathThin)
int64_t plan_boxes(BoxList& L, const Box* boxes, const bool* thin, int nboxes, int V, int R,
                   int chunk_z) {
  L = BoxList{};
  int64_t total = 0;
  const int64_t sw = (int64_t)kWave * V;
  for (int i = 0; i < nboxes; ++i) {
    const Box& b = boxes[i];
    if (b.empty()) continue;
    const int n = L.n++;
    L.b[n] = b;
    const int64_t nzb = b.z1 - b.z0, nyb = b.y1 - b.y0;
    int64_t blocks;
    if (thin[i]) {
      L.chunk_z[n] = -1;
      blocks = (nyb * nzb + kBlock - 1) / kBlock;
    } else {
      L.xa[n] = b.x0 - (b.x0 % sw);
      L.strips[n] = (b.x1 - L.xa[n] + sw - 1) / sw;
      L.bands[n] = (nyb + R - 1) / R;
      L.groups[n] = (L.bands[n] + kWavesPerBlock - 1) / kWavesPerBlock;
      // 32 planes per task (measured, profiles/diffusion3d.md: 3-8 % ahead of 128
      // at 1024^3 and 1536^3, level at 512^3); each chunk re-reads two planes
      L.chunk_z[n] = std::min<int64_t>(chunk_z > 0 ? chunk_z : 32, nzb);
      blocks = L.strips[n] * L.groups[n] * ((nzb + L.chunk_z[n] - 1) / L.chunk_z[n]);
    }
    total += blocks;
    L.block_end[n] = total;
  }
  return total;
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
struct FaceList {
  Box b[kMaxBoxes];
  int64_t bands[kMaxBoxes];      // wave tasks along y: ceil(rows / (64 / LX))
  int64_t groups[kMaxBoxes];     // blocks along y: ceil(bands / waves per block)
  int64_t chunk_z[kMaxBoxes];    // planes per task
  int64_t block_end[kMaxBoxes];  // inclusive prefix sum of blocks
  int n;
};

template <int LX, bool NTS, bool Uni, int A>
__global__ __launch_bounds__(kBlock) void stencil3d_xface_kernel(double* __restrict__ T2,
                                                                 const double* __restrict__ T,
                                                                 Factor<Uni> iCp, int64_t nx,
                                                                 int64_t ny, FaceList L,
                                                                 Coef3<A> k) {
  constexpr int RG = kWave / LX;  // rows of a wave
  static_assert(LX == 8 || LX == 16 || LX == 32, "lanes per row");
  const int64_t b = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int bi = 0;
  while (bi < L.n - 1 && b >= L.block_end[bi]) ++bi;  // block-uniform, <= 8 steps
  const int64_t lb = b - (bi ? L.block_end[bi - 1] : 0);
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
    if (m) {
      if constexpr (NTS) {
        __builtin_nontemporal_store(v, T2 + z * plane + o);
      } else {
        T2[z * plane + o] = v;
      }
    }
    bk = c;
    c = fr;
    fr = fr2;
    e = e2;
    h = h2;
    f = f2;
  }
}

// index of a lanes-per-row class (Dispatch3D::lanes): 0, 1, 2 for LX = 8, 16, 32
int face_class(int lanes) { return lanes == 8 ? 0 : lanes == 16 ? 1 : 2; }

int64_t plan_faces(FaceList& L, const Box* boxes, int nboxes, int LX, int chunk_z) {
  L = FaceList{};
  int64_t total = 0;
  const int64_t rg = kWave / LX;
  for (int i = 0; i < nboxes; ++i) {
    const Box& b = boxes[i];
    const int n = L.n++;
    L.b[n] = b;
    const int64_t nzb = b.z1 - b.z0, nyb = b.y1 - b.y0;
    L.bands[n] = (nyb + rg - 1) / rg;
    L.groups[n] = (L.bands[n] + kWavesPerBlock - 1) / kWavesPerBlock;
    // 16 planes per task by default: a face has few cells, shorter tasks keep
    // more waves in flight for the 2/16 re-read of the planes around a chunk
    L.chunk_z[n] = std::min<int64_t>(chunk_z > 0 ? chunk_z : 16, nzb);
    total += L.groups[n] * ((nzb + L.chunk_z[n] - 1) / L.chunk_z[n]);
    L.block_end[n] = total;
  }
  return total;
}

template <int LX, int A>
void launch_face(dim3 grid, hipStream_t s, int nt, double* T2, const double* T, const double* iCp,
                 int64_t nx, int64_t ny, const FaceList& L, const Coef3<A>& c, bool uni,
                 double fac) {
  const dim3 block(kBlock);
  if (uni) {
    if (nt & 1)
      stencil3d_xface_kernel<LX, true, true, A><<<grid, block, 0, s>>>(T2, T, fac, nx, ny, L, c);
    else
      stencil3d_xface_kernel<LX, false, true, A><<<grid, block, 0, s>>>(T2, T, fac, nx, ny, L, c);
  } else if (nt & 1) {
    stencil3d_xface_kernel<LX, true, false, A><<<grid, block, 0, s>>>(T2, T, iCp, nx, ny, L, c);
  } else {
    stencil3d_xface_kernel<LX, false, false, A><<<grid, block, 0, s>>>(T2, T, iCp, nx, ny, L, c);
  }
}

// the face boxes of one launch, one kernel launch per lanes-per-row class in use
template <int A>
void launch_faces(const Box (&face)[3][kMaxBoxes], const int (&nface)[3], int chunk_z,
                  hipStream_t s, int nt, double* T2, const double* T, const double* iCp,
                  int64_t nx, int64_t ny, const Coef3<A>& c, bool uni, double fac) {
  for (int cls = 0; cls < 3; ++cls) {
    if (!nface[cls]) continue;
    FaceList L{};
    const int64_t total = plan_faces(L, face[cls], nface[cls], 8 << cls, chunk_z);
    RMA_CHECK_ARG(total < (int64_t(1) << 31), "grid too large: " << total << " blocks");
    const dim3 grid((unsigned)total);
    if (cls == 0) launch_face<8, A>(grid, s, nt, T2, T, iCp, nx, ny, L, c, uni, fac);
    else if (cls == 1) launch_face<16, A>(grid, s, nt, T2, T, iCp, nx, ny, L, c, uni, fac);
    else launch_face<32, A>(grid, s, nt, T2, T, iCp, nx, ny, L, c, uni, fac);
    RMA_HIP_LAUNCH_CHECK();
  }
}

template <int V, int R, int U, int A>
void launch_nt(dim3 grid, hipStream_t s, int nt, double* T2, const double* T, const double* iCp,
               int64_t nx, int64_t ny, const BoxList& L, const Coef3<A>& c, int remap,
               bool uni, double fac) {
  const dim3 block(kBlock);
  if (uni) {  // the 1/Cp-load bit has nothing to act on
    if (nt & 1)
      stencil3d_march_kernel<V, R, U, true, false, true, A><<<grid, block, 0, s>>>(T2, T, fac, nx, ny,
                                                                                L, c, remap);
    else
      stencil3d_march_kernel<V, R, U, false, false, true, A><<<grid, block, 0, s>>>(T2, T, fac, nx,
                                                                                 ny, L, c, remap);
    return;
  }
  switch (nt & 3) {
    case 0:
      stencil3d_march_kernel<V, R, U, false, false, false, A><<<grid, block, 0, s>>>(T2, T, iCp, nx, ny, L,
                                                                           c, remap);
      break;
    case 1:
      stencil3d_march_kernel<V, R, U, true, false, false, A><<<grid, block, 0, s>>>(T2, T, iCp, nx, ny, L,
                                                                          c, remap);
      break;
    case 2:
      stencil3d_march_kernel<V, R, U, false, true, false, A><<<grid, block, 0, s>>>(T2, T, iCp, nx, ny, L,
                                                                          c, remap);
      break;
    default:
      stencil3d_march_kernel<V, R, U, true, true, false, A><<<grid, block, 0, s>>>(T2, T, iCp, nx, ny, L,
                                                                         c, remap);
  }
}

template <int V, int A>
void launch_ru(int R, int U, dim3 grid, hipStream_t s, int nt, double* T2, const double* T,
               const double* iCp, int64_t nx, int64_t ny, const BoxList& L,
               const Coef3<A>& c, int remap, bool uni, double fac) {
  if (R == 2 && U == 1) launch_nt<V, 2, 1, A>(grid, s, nt, T2, T, iCp, nx, ny, L, c, remap, uni, fac);
  else if (R == 2) launch_nt<V, 2, 2, A>(grid, s, nt, T2, T, iCp, nx, ny, L, c, remap, uni, fac);
  else if (R == 4 && U == 1) launch_nt<V, 4, 1, A>(grid, s, nt, T2, T, iCp, nx, ny, L, c, remap, uni, fac);
  else if (R == 4) launch_nt<V, 4, 2, A>(grid, s, nt, T2, T, iCp, nx, ny, L, c, remap, uni, fac);
  else launch_nt<V, 8, 1, A>(grid, s, nt, T2, T, iCp, nx, ny, L, c, remap, uni, fac);
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
  RMA_CHECK_ARG(tune.vec == 1 || tune.vec == 2, "vec=" << tune.vec << " (1 or 2)");
  RMA_CHECK_ARG(tune.nontemporal >= 0 && tune.nontemporal <= 3,
                "nontemporal=" << tune.nontemporal << " (bits 0 and 1)");
  RMA_CHECK_ARG(tune.chunk_z >= 0, "chunk_z=" << tune.chunk_z);
  RMA_CHECK_ARG(!tune.fast_math || fast7_ok(c),
                "fast_math: fast7 needs lam != 0 and finite coefficients");
  // plan_dispatch3d (kernel_select.cpp) checks tune.xface and decides the path of
  // every box: face boxes leave the list for the x-face kernel, the rest keep
  // their order in the march launch (strips, or one thread per row for thin
  // boxes). xface = 0 has no face boxes: the caller's list.
  Dispatch3D path[kMaxBoxes];
  plan_dispatch3d(1, boxes, nboxes, tune, path);
  hipStream_t s = as_stream(stream);
  Box wide[kMaxBoxes], face[3][kMaxBoxes];
  bool thin[kMaxBoxes];
  int nwide = 0, nface[3] = {0, 0, 0};
  for (int i = 0; i < nboxes; ++i) {
    if (path[i].path == kPathXface) {
      const int cls = face_class(path[i].lanes);
      face[cls][nface[cls]++] = boxes[i];
    } else if (path[i].path != kPathNone) {
      thin[nwide] = path[i].path == kPathThin;
      wide[nwide++] = boxes[i];
    }
  }
  const bool faces = nface[0] + nface[1] + nface[2] > 0;
  const int V = stencil3d_vec(T2, T, iCp, nx, tune);
  BoxList L{};
  const int64_t total = plan_boxes(L, wide, thin, nwide, V, tune.rows, tune.chunk_z);
  if (L.n == 0 && !faces) return;
  RMA_CHECK_ARG(total < (int64_t(1) << 31), "grid too large: " << total << " blocks");
  const dim3 grid((unsigned)total);
  const int remap = tune.xcd_remap ? 1 : 0;
  if (tune.fast_math) {  // the uniform variant takes g = gs * value, formed here
    const Fast7 f = fast7_constants(c);
    const double g = f.gs * tune.uniform_value;
    if (faces)
      launch_faces<kFast7>(face, nface, tune.chunk_z, s, tune.nontemporal, T2, T, iCp, nx, ny, f,
                           tune.uniform, g);
    if (L.n == 0) return;
    if (V == 2)
      launch_ru<2, kFast7>(tune.rows, tune.unroll, grid, s, tune.nontemporal, T2, T, iCp, nx, ny,
                           L, f, remap, tune.uniform, g);
    else
      launch_ru<1, kFast7>(tune.rows, tune.unroll, grid, s, tune.nontemporal, T2, T, iCp, nx, ny,
                           L, f, remap, tune.uniform, g);
  } else {
    if (faces)
      launch_faces<kCanonical3>(face, nface, tune.chunk_z, s, tune.nontemporal, T2, T, iCp, nx,
                                ny, c, tune.uniform, tune.uniform_value);
    if (L.n == 0) return;
    if (V == 2)
      launch_ru<2, kCanonical3>(tune.rows, tune.unroll, grid, s, tune.nontemporal, T2, T, iCp, nx,
                                ny, L, c, remap, tune.uniform, tune.uniform_value);
    else
      launch_ru<1, kCanonical3>(tune.rows, tune.unroll, grid, s, tune.nontemporal, T2, T, iCp, nx,
                                ny, L, c, remap, tune.uniform, tune.uniform_value);
  }
  RMA_HIP_LAUNCH_CHECK();
}

}  // namespace rma
