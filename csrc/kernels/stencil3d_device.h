// What the one-step (stencil3d.hip) and K-step (stencil3d_tb.hip) 3D diffusion
// kernels share: the cell update, the block lists and their planners, the block
// prologue, and the one place that maps a Stencil3DTuning onto template
// arguments. Included by those two units only; stencil_device.h keeps the 2D
// pieces and the row loads / stores.
#pragma once

#include <algorithm>
#include <type_traits>
#include <utility>

#include "rma/hip_check.h"
#include "rma/kernels.h"
#include "stencil_device.h"

namespace rma {
namespace march {

// Arithmetic of a 3D kernel instantiation and the coefficients it takes as its
// kernel argument: canonical the StencilCoef3 itself, fast7 the folded constants.
constexpr int kCanonical3 = 0;
constexpr int kFast7 = 1;
template <int A>
using Coef3 = std::conditional_t<A == kFast7, Fast7, StencilCoef3>;

// 1/Cp as the kernels take it: the array, or with Uni its one value (fast7: gs
// times that value)
template <bool Uni>
using Factor = std::conditional_t<Uni, double, const double* __restrict__>;

// The canonical 3D cell update (rma/common.h StencilCoef3). Compiled with
// -ffp-contract=off: every operation rounds exactly as written, in this order.
// The one copy every 3D kernel runs, which is what makes a K-step pass bitwise
// equal to K one-step launches.
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

// The fast7 cell update (rma/kernels.h): the 7-point sum, the constants folded
// on the host. The fmas are explicit (contraction is off), so std::fma on the
// host is a bitwise twin. f is 1/Cp of the cell (g = gs*f, one rounded multiply)
// or, with Uni, the product gs*value formed on the host.
template <bool Uni>
__device__ __forceinline__ double cell7(double xl, double c, double xr, double up, double dn,
                                        double bk, double fr, double f, const Fast7& k) {
  double g;
  if constexpr (Uni) g = f; else g = k.gs * f;
  const double sx = xr + xl;
  const double sy = up + dn;
  const double sz = bk + fr;
  double t = __builtin_fma(k.mkc, c, sx);
  t = __builtin_fma(k.ry, sy, t);
  t = __builtin_fma(k.rz, sz, t);
  return __builtin_fma(g, t, c);
}

// the update of one cell in arithmetic A (f: 1/Cp of the cell, or what Factor<true> holds)
template <int A, bool Uni>
__device__ __forceinline__ double update3(double xl, double c, double xr, double up, double dn,
                                          double bk, double fr, double f, const Coef3<A>& k) {
  if constexpr (A == kFast7) return cell7<Uni>(xl, c, xr, up, dn, bk, fr, f, k);
  else return cell3(xl, c, xr, up, dn, bk, fr, f, k);
}

// one scalar store, non-temporal or plain
template <bool NT>
__device__ __forceinline__ void store1(double* p, double v) {
  if constexpr (NT) {
    __builtin_nontemporal_store(v, p);
  } else {
    *p = v;
  }
}

// Boxes of a strip-march launch (plan_boxes): both marches.
struct BoxList {
  Box b[kMaxBoxes];
  int64_t xa[kMaxBoxes];         // origin of strip 0
  int64_t strips[kMaxBoxes];
  int64_t bands[kMaxBoxes];
  int64_t groups[kMaxBoxes];     // blocks along y: ceil(bands / waves per block)
  int64_t chunk_z[kMaxBoxes];    // (output) planes per task; -1: thin box, one thread per row
  int64_t block_end[kMaxBoxes];  // inclusive prefix sum of blocks
  int n;
};

// Boxes of an x-face launch (plan_faces): both face paths. The one-step kernel
// starts its rows at the box and does not read xs.
struct FaceList {
  Box b[kMaxBoxes];
  int64_t xs[kMaxBoxes];         // first column of the segment
  int64_t bands[kMaxBoxes];      // tasks along y
  int64_t groups[kMaxBoxes];     // blocks along y
  int64_t chunk_z[kMaxBoxes];    // (output) planes per task
  int64_t block_end[kMaxBoxes];  // inclusive prefix sum of blocks
  int n;
};

// The block prologue of every 3D kernel: the box a block works on (bi), the
// block's index inside it (lb) and the wave's index in the block. L: a BoxList or
// FaceList, read in place (the kernel argument; a copy of n or block_end taken
// at the call would move their loads ahead of the remap). remap: blocks in the
// XCD order of xcd_remap instead of dispatch order.
struct BlockAt {
  int bi;
  int64_t lb;
  int wave;
};
template <class List>
__device__ __forceinline__ BlockAt locate_block(const List& L, int remap) {
  const int64_t b = remap ? xcd_remap(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x;
  BlockAt at;
  at.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  at.bi = 0;
  while (at.bi < L.n - 1 && b >= L.block_end[at.bi]) ++at.bi;  // block-uniform, <= 8 steps
  at.lb = b - (at.bi ? L.block_end[at.bi - 1] : 0);
  return at;
}

// The same prologue for a signalling launch (Stencil3DTuning::signal): the first
// `first` blocks, the signal prefix, keep dispatch order and the rest is XCD-
// remapped among itself (xcd_remap_after). Block blk of nwg; the caller fills in
// the wave. Host-callable: stencil3d_fused_plan maps every block with the
// function the kernels run. Unsignalled kernels keep locate_block as it is.
template <class List>
__host__ __device__ __forceinline__ BlockAt block_after(const List& L, int64_t blk, int64_t nwg,
                                                        int remap, int64_t first) {
  const int64_t b = remap ? xcd_remap_after(blk, nwg, first) : blk;
  BlockAt at;
  at.wave = 0;
  at.bi = 0;
  while (at.bi < L.n - 1 && b >= L.block_end[at.bi]) ++at.bi;  // block-uniform, <= 8 steps
  at.lb = b - (at.bi ? L.block_end[at.bi - 1] : 0);
  return at;
}

// The trailing argument of the two march kernels, SigArg<Sig>: nothing (the
// kernels as they were; NoSig is empty and the if constexpr (Sig) statements
// vanish), or the signal words of a frame-first fused pass. The waves of these
// kernels leave independently (no barrier; waves past the last band return at
// once; thin-box threads return one by one), so every wave of every prefix
// block counts itself (signal_wave_done): each way out of a signalling
// instantiation calls wave_done() behind the wave's last store. Lane 0 counts;
// where lanes leave one by one (the thin path) lane 0 has the lowest row of its
// wave: the lanes that store run the same loop together with it, so its call is
// behind every store of the wave, and a wave whose lane 0 has no row stores
// nothing. The last of first * 4 waves re-arms the counter and raises the
// flag with a system-scope release. first comes from plan_launch3d, as the grid.
struct NoSig {};
struct WaveSig {
  uint64_t* sig;
  int64_t first;  // blocks of the signal prefix
  __device__ __forceinline__ void wave_done() const {
    if ((int64_t)blockIdx.x < first) signal_wave_done(sig, first * kWavesPerBlock);
  }
};
template <bool Sig>
using SigArg = std::conditional_t<Sig, WaveSig, NoSig>;

template <class List>
__device__ __forceinline__ BlockAt locate_block(const List& L, int remap, NoSig) {
  return locate_block(L, remap);
}
template <class List>
__device__ __forceinline__ BlockAt locate_block(const List& L, int remap, const WaveSig& s) {
  BlockAt at = block_after(L, (int64_t)blockIdx.x, (int64_t)gridDim.x, remap, s.first);
  at.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  return at;
}

// Blocks of a strip-march launch of K steps per pass, V cells per lane and R
// output rows per wave; thin[i] marks a thin box (plan_dispatch3d's kPathThin,
// one-step only). Block lb of a box: strip fastest, then the group of 4 bands,
// then the z chunk.
//   K = 1: strips start on multiples of the strip width 64*V and advance by it.
//   K > 1: strip 0 starts K-1 columns left of the box (its first valid column), on
//   a multiple of V and never left of the array (valid from the face on there);
//   strips advance by 64*V - 2(K-1) columns.
// chunk_z <= 0 takes dflt planes per task; each chunk re-reads 2K planes (and
// recomputes K-1).
inline int64_t plan_boxes(BoxList& L, const Box* boxes, const bool* thin, int nboxes, int K, int V,
                          int R, int chunk_z, int64_t dflt) {
  L = BoxList{};
  int64_t total = 0;
  const int64_t sw = (int64_t)kWave * V, step = sw - 2 * (K - 1);
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
      if (K == 1) {
        L.xa[n] = b.x0 - (b.x0 % sw);
        L.strips[n] = (b.x1 - L.xa[n] + sw - 1) / sw;
      } else {
        const int64_t x0 = std::max<int64_t>(b.x0 - (K - 1), 0);
        L.xa[n] = x0 - (x0 % V);
        const int64_t first = L.xa[n] == 0 ? 0 : L.xa[n] + (K - 1);  // first valid column
        L.strips[n] = std::max<int64_t>(1, (b.x1 - first + step - 1) / step);
      }
      L.bands[n] = (nyb + R - 1) / R;
      L.groups[n] = (L.bands[n] + kWavesPerBlock - 1) / kWavesPerBlock;
      L.chunk_z[n] = std::min<int64_t>(chunk_z > 0 ? chunk_z : dflt, nzb);
      blocks = L.strips[n] * L.groups[n] * ((nzb + L.chunk_z[n] - 1) / L.chunk_z[n]);
    }
    total += blocks;
    L.block_end[n] = total;
  }
  return total;
}

// Blocks of an x-face launch of K steps per pass: a task along y is `rows` rows
// and a wave runs `per_wave` of them (one-step: one task of 64/LX rows; K-step:
// 64/LX group tasks of R rows). The segment starts K-1 columns left of the box
// (its first valid lane) and never left of the array (valid from the face on
// there). Block lb of a box: the group of 4 wave bands fastest, then the z chunk.
// 16 planes per task by default: a face has few cells, shorter tasks keep more
// waves in flight for the re-read of the 2K planes around a chunk.
constexpr int64_t kFaceDefaultChunkZ = 16;
inline int64_t plan_faces(FaceList& L, const Box* boxes, int nboxes, int K, int64_t rows,
                          int64_t per_wave, int chunk_z) {
  L = FaceList{};
  int64_t total = 0;
  for (int i = 0; i < nboxes; ++i) {
    const Box& b = boxes[i];
    const int n = L.n++;
    L.b[n] = b;
    const int64_t nzb = b.z1 - b.z0, nyb = b.y1 - b.y0;
    L.xs[n] = std::max<int64_t>(b.x0 - (K - 1), 0);
    L.bands[n] = (nyb + rows - 1) / rows;
    const int64_t wbands = (L.bands[n] + per_wave - 1) / per_wave;
    L.groups[n] = (wbands + kWavesPerBlock - 1) / kWavesPerBlock;
    L.chunk_z[n] = std::min<int64_t>(chunk_z > 0 ? chunk_z : kFaceDefaultChunkZ, nzb);
    total += L.groups[n] * ((nzb + L.chunk_z[n] - 1) / L.chunk_z[n]);
    L.block_end[n] = total;
  }
  return total;
}

inline dim3 grid_of(int64_t blocks) {
  RMA_CHECK_ARG(blocks < (int64_t(1) << 31), "grid too large: " << blocks << " blocks");
  return dim3((unsigned)blocks);
}

// The tuning checks both launchers run before any work; pre names the launcher's
// own fields ("" or "tb_"), nt and chunk_z are their values.
inline void check_tuning3d(const Stencil3DTuning& tune, const StencilCoef3& c, const char* pre,
                           int nt, int chunk_z) {
  RMA_CHECK_ARG(tune.vec == 1 || tune.vec == 2, "vec=" << tune.vec << " (1 or 2)");
  RMA_CHECK_ARG(nt >= 0 && nt <= 3, pre << "nontemporal=" << nt << " (bits 0 and 1)");
  RMA_CHECK_ARG(chunk_z >= 0, pre << "chunk_z=" << chunk_z);
  RMA_CHECK_ARG(!tune.fast_math || fast7_ok(c),
                "fast_math: fast7 needs lam != 0 and finite coefficients");
}

// defaults of Stencil3DTuning::chunk_z = 0 (profiles/diffusion3d.md: 32 planes per
// task measured 3-8 % ahead of 128 at 1024^3 and 1536^3, level at 512^3) and of
// tb_rows / tb_chunk_z = 0 (profiles/diffusion3d_temporal.md)
constexpr int64_t kDefaultChunkZ = 32;
constexpr int kTbDefaultRows = 4;
constexpr int64_t kTbDefaultChunkZ = 32;
// the tuning the signalling kernels are instantiated for: the shipped one
constexpr int kSigRows = 4, kSigUnroll = 2;

// The march launch of a K-step pass (K = 1, 2) at V cells per lane: the box lists
// (sp, L) and the block counts, the one function both launchers and
// stencil3d_fused_plan run. signalling (Stencil3DTuning::signal set, or a plan
// asked for with signal_boxes > 0): the first signal_boxes non-empty boxes are the
// signal prefix, every box runs the march or thin path (xface is checked and then
// not applied) and the tuning must be the shipped one. Every refusal names its
// argument and comes before any work.
inline Fused3DPlan plan_launch3d(BoxList& L, Split3D& sp, int K, int V, const Box* boxes,
                                 int nboxes, const Stencil3DTuning& tune, bool signalling,
                                 int signal_boxes) {
  const int R = K == 1 ? tune.rows : (tune.tb_rows > 0 ? tune.tb_rows : kTbDefaultRows);
  Stencil3DTuning t = tune;
  if (signalling) {
    RMA_CHECK_ARG(tune.xface >= 0 && tune.xface <= kXfaceMax,
                  "xface=" << tune.xface << " (0: off, or the widest face box, up to "
                           << kXfaceMax << ")");
    t.xface = 0;
    if (K == 1)
      RMA_CHECK_ARG(tune.rows == kSigRows && tune.unroll == kSigUnroll,
                    "signal: rows=" << tune.rows << " unroll=" << tune.unroll
                                    << " (signalling launches are instantiated for rows="
                                    << kSigRows << " unroll=" << kSigUnroll << " only)");
    else
      RMA_CHECK_ARG(R == kTbDefaultRows,
                    "signal: tb_rows=" << tune.tb_rows
                                       << " (signalling launches are instantiated for tb_rows="
                                       << kTbDefaultRows << ", the default, only)");
  } else {
    RMA_CHECK_ARG(signal_boxes == 0, "signal is null with signal_boxes=" << signal_boxes);
  }
  sp = split_boxes3d(K, boxes, nboxes, t);
  if (signalling)
    RMA_CHECK_ARG(signal_boxes >= 1 && signal_boxes < sp.nwide,
                  "signal_boxes=" << signal_boxes << " (1 .. " << sp.nwide - 1
                                  << ": a prefix of the " << sp.nwide
                                  << " non-empty boxes with at least one box after it)");
  Fused3DPlan p;
  p.blocks = K == 1 ? plan_boxes(L, sp.wide, sp.thin, sp.nwide, 1, V, R, tune.chunk_z,
                                 kDefaultChunkZ)
                    : plan_boxes(L, sp.wide, sp.thin, sp.nwide, K, V, R, tune.tb_chunk_z,
                                 kTbDefaultChunkZ);
  p.boxes = L.n;
  p.prefix_blocks = signalling ? L.block_end[signal_boxes - 1] : 0;
  p.signalling_waves = p.prefix_blocks * kWavesPerBlock;
  return p;
}

// ---------------------------------------------------------------------------
// Run-time values to template arguments. f receives std::integral_constant
// objects; decltype(x)::value is the template argument. Every mapping from a
// Stencil3DTuning field to a kernel's template argument goes through these.
// ---------------------------------------------------------------------------
template <int N>
using int_c = std::integral_constant<int, N>;

template <class F>
void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// f(int_c<v>) for v among Vs (checked by the caller: anything else is a bug)
template <int... Vs, class F>
void with_value(int v, F&& f) {
  const bool hit = ((v == Vs ? (f(int_c<Vs>{}), true) : false) || ...);
  RMA_CHECK_ARG(hit, "value " << v << " has no instantiation");
}

// f(LX, boxes, n) for every lanes-per-row class of split_boxes3d that has boxes,
// narrowest first: one x-face launch each
template <class F>
void for_face_classes(const Split3D& sp, F&& f) {
  for (int cls = 0; cls < 3; ++cls)
    if (sp.nface[cls])
      with_value<8, 16, 32>(8 << cls, [&](auto lx) { f(lx, sp.face[cls], sp.nface[cls]); });
}

// f(A, k, fac): the arithmetic, the coefficient argument of its kernels and the
// uniform factor they take (fast7: g = gs * value, formed here)
template <class F>
void with_arith3(const StencilCoef3& c, const Stencil3DTuning& tune, F&& f) {
  if (tune.fast_math) {
    const Fast7 k = fast7_constants(c);
    f(int_c<kFast7>{}, k, k.gs * tune.uniform_value);
  } else {
    f(int_c<kCanonical3>{}, c, tune.uniform_value);
  }
}

// f(NTS, NTL, Uni) from a non-temporal mask and the uniform flag: NTS = bit 0
// (T2 stores), NTL = bit 1 (1/Cp loads). Uniform reads no 1/Cp, so it has the
// NTL = false kernels only; HasNTL = false (the K-step face path) has none at all.
template <bool HasNTL, class F>
void with_access3(int nt, bool uniform, F&& f) {
  with_bool(uniform, [&](auto uni) {
    with_bool(nt & 1, [&](auto nts) {
      if constexpr (decltype(uni)::value || !HasNTL) {
        f(nts, std::false_type{}, uni);
      } else {
        with_bool(nt & 2, [&](auto ntl) { f(nts, ntl, uni); });
      }
    });
  });
}

// the 1/Cp argument of a kernel: the array, or with Uni the factor
template <bool Uni>
std::conditional_t<Uni, double, const double*> factor_arg(const double* iCp, double fac) {
  if constexpr (Uni) return fac;
  else return iCp;
}

}  // namespace march
}  // namespace rma
