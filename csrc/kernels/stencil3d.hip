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

int64_t plan_boxes(BoxList& L, const Box* boxes, int nboxes, int V, int R, int chunk_z) {
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
    if (b.x1 - b.x0 <= kColMaxWidth) {
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
  const int V = stencil3d_vec(T2, T, iCp, nx, tune);
  BoxList L{};
  const int64_t total = plan_boxes(L, boxes, nboxes, V, tune.rows, tune.chunk_z);
  if (L.n == 0) return;
  RMA_CHECK_ARG(total < (int64_t(1) << 31), "grid too large: " << total << " blocks");
  const dim3 grid((unsigned)total);
  hipStream_t s = as_stream(stream);
  const int remap = tune.xcd_remap ? 1 : 0;
  if (tune.fast_math) {  // the uniform variant takes g = gs * value, formed here
    const Fast7 f = fast7_constants(c);
    const double g = f.gs * tune.uniform_value;
    if (V == 2)
      launch_ru<2, kFast7>(tune.rows, tune.unroll, grid, s, tune.nontemporal, T2, T, iCp, nx, ny,
                           L, f, remap, tune.uniform, g);
    else
      launch_ru<1, kFast7>(tune.rows, tune.unroll, grid, s, tune.nontemporal, T2, T, iCp, nx, ny,
                           L, f, remap, tune.uniform, g);
  } else if (V == 2) {
    launch_ru<2, kCanonical3>(tune.rows, tune.unroll, grid, s, tune.nontemporal, T2, T, iCp, nx,
                              ny, L, c, remap, tune.uniform, tune.uniform_value);
  } else {
    launch_ru<1, kCanonical3>(tune.rows, tune.unroll, grid, s, tune.nontemporal, T2, T, iCp, nx,
                              ny, L, c, remap, tune.uniform, tune.uniform_value);
  }
  RMA_HIP_LAUNCH_CHECK();
}

}  // namespace rma
