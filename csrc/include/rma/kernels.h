// rocm_mpi_amd native core — kernel launch API (host side).
//
// Every GPU entry point enqueues work on the given HIP stream (passed as an
// opaque pointer so this header stays HIP-free for the pybind11 layer) and
// returns immediately. The *_cpu twins are bit-identical host implementations
// used for CPU-only runs (the reference's "ap 256² single-rank CPU array path",
// BASELINE.json configs[0]) and as the numerics oracle in tests.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rma/common.h"

namespace rma {

using stream_t = void*;  // hipStream_t

// ---------------------------------------------------------------------------
// Fused 5-point stencil (K4 of SURVEY.md §2.3; reference
// scripts/diffusion_2D_perf.jl:3-13). Updates every cell of every rect in ONE
// launch: T2[r] = f(T, iCp)[r]. The split boundary/interior steps of
// perf_hide (K5, scripts/diffusion_2D_perf_hide.jl:15-29) are the same launch
// with the frame rects / interior rect, so the arithmetic is shared bitwise.
// ---------------------------------------------------------------------------
constexpr int kMaxRects = 8;

// Direct-store halos (pipelined K-step kernels only): cells of the output rect
// that are a neighbour's halo are ALSO stored straight into the neighbour's
// output field -- its own tile in the same process (loopback ranks), a mapped
// peer tile (IPC) or this tile's own periodic images. Replaces the pack /
// send / receive / unpack of an exchange (DiffusionExecutor::set_direct).
// Direction d = 0..7 is (i, j) = (kDirI[d], kDirJ[d]) of executor.h. A stored
// cell (x, y) also goes to dst[d] when dst[d] is set, x lies in the i-range
// (i = -1: [xm0, xm1), +1: [xp0, xp1), 0: any) and y in the j-range (same with
// ym / yp), at element index (y * nx + x) - i * sx - j * syr * nx: every rank
// has the same nx x ny tile, the neighbour's origin sx = nx - olx columns /
// syr = ny - oly rows away. Eight fixed ranges rather than a list of rects:
// the kernel decides per task (which ranges its window and rows touch) and per
// row with a few scalar compares; a list walked per row costs a scalar load
// chain per entry and doubled the K = 24 pass at 8192^2. Passed by value (a
// kernel argument).
struct DirectStores {
  int on = 0;  // any dst set
  int32_t xm0 = 0, xm1 = 0, xp0 = 0, xp1 = 0;
  int32_t ym0 = 0, ym1 = 0, yp0 = 0, yp1 = 0;
  int64_t sx = 0, syr = 0;
  double* dst[8] = {};
};

struct StencilTuning {
  int chunk_rows = 4;      // rows marched by one wave-task
  int nontemporal = 3;     // bit 0: NT T2 stores; bit 1: NT 1/Cp loads; bit 2: NT T loads
  int kernel = 0;          // 0 = register march (default), 1 = LDS-tiled
  int unroll = 4;          // rows per march iteration whose loads are issued together
  int vec = 2;             // cells per lane (2: one 16-B access per row, 4: two; 6: three,
                           // uniform-factor pipelined kernels only, pipe_vec_uniform)
  int xcd_remap = -1;      // 1: each XCD takes a contiguous 1/8 of the tasks; 0: chunk rows
                           // padded to 8-block multiples (same-XCD neighbours); -1: by size
  int stages = 0;          // pipelined K-step kernels 9/10: waves per strip (0: default)
  int cols = 0;            // pipelined kernels: column waves per stage (0: default, 1, 2)
  // Frame-first fused pass (pipelined kernels only): signal != nullptr makes
  // the first signal_rects rects' tasks dispatch first (never XCD-remapped)
  // and count their completion in signal[0] (device memory, zero); the last
  // one resets it and stores 1 into signal[1] with system-scope release. A
  // flag_wait_gpu(signal + 1, 1, ...) on another stream then orders work after
  // those rects without waiting for the rest of the launch.
  // Without signal, signal_rects > 0 only gives the first rects their own
  // rows per task (the direct-store one-launch pass: shorter edge tasks).
  uint64_t* signal = nullptr;
  int signal_rects = 0;
  int signal_chunk_rows = 0;  // rows per task of the signal rects (0: chunk_rows)
  // Graded task rows (pipelined kernels only): rect_rows[i] > 0 is the rows
  // per task of rect i (nrects entries; else chunk_rows / signal_chunk_rows),
  // and the last `bands` rects are row bands of one region with descending
  // rows per task (plan.h plan_row_bands): dispatched in that order, each
  // XCD-remapped among its own blocks, so every XCD walks long, then medium,
  // then short tasks and the short ones fill the end of the launch. The band
  // rects must be non-empty and follow the signal rects. Speed only: any task
  // mapping computes the same cells.
  const int* rect_rows = nullptr;
  int bands = 0;
  // direct-store halos of this launch (pipelined kernels; nullptr: none)
  const DirectStores* direct = nullptr;
  // 1/Cp is bit-for-bit the one value uniform_value in every cell (the caller
  // vouches for it; DiffusionExecutor scans the array): the register-factor
  // pipelined kernels (12 / 22) at 2 or 4 cells per lane then run their
  // uniform-factor variant, which does not read the array (16 instead of 24
  // bytes per cell and pass), bitwise equal to the field path. Launches the
  // variant does not cover (1 cell per lane, direct stores, other kernels)
  // run the field path.
  bool uniform = false;
  double uniform_value = 0.0;
};

void stencil_rects_gpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                       const Rect* rects, int nrects, const StencilCoef& c,
                       const StencilTuning& tune, stream_t stream);
void stencil_rects_cpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                       const Rect* rects, int nrects, const StencilCoef& c);

// Two steps per pass (temporal blocking, stencil_tb.hip): T2[r] = f(f(T))[r],
// where the intermediate step is f(T) on the interior [1,nx-1)x[1,ny-1) and T
// elsewhere. Bitwise equal to two one-step launches. T2 != T; unroll 2 or 4;
// no column mode (every rect is marched in 64*V-cell strips).
void stencil2_rects_gpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                        const Rect* rects, int nrects, const StencilCoef& c,
                        const StencilTuning& tune, stream_t stream);
void stencil2_rects_cpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                        const Rect* rects, int nrects, const StencilCoef& c);

// K steps per pass (K = 2, 3, 4, 6, 8: stencil_kstep.hip kernel 3; others: csrc/lab): T2[r] = f^K(T)[r], the
// intermediate levels being f on the interior and T elsewhere; face fluxes
// shared between neighbouring cells (same rounding). Bitwise equal to K
// one-step launches.
void stencilk_rects_gpu(int K, double* T2, const double* T, const double* iCp, int64_t nx,
                        int64_t ny, const Rect* rects, int nrects, const StencilCoef& c,
                        const StencilTuning& tune, stream_t stream);
void stencilk_rects_cpu(int K, double* T2, const double* T, const double* iCp, int64_t nx,
                        int64_t ny, const Rect* rects, int nrects, const StencilCoef& c);
// StencilTuning::kernel of the K-step launcher: 0 march, 1 LDS 1/Cp ring, 2 DPP,
// 3 LDS ring + DPP (bitwise default), 4 fast (reassociated fluxes, 7 fp64 ops
// per cell update), 5 fast5 (5-point sum, constants folded into one per-cell
// factor, 5 ops). 4 and 5 are not bitwise equal to the canonical update.
// fast5_ok: kernel 5 divides by lam/dx^2, so it needs lam != 0.
bool fast5_ok(const StencilCoef& c);
//   9 pipe  (fast5 arithmetic) / 10 pipec (canonical): stage-pipelined strips
//     for ANY K in 1..kPipeMaxK (stencil_pipe.h); stencilk_rects_gpu routes
//     kernels 9/10 here. stages = waves per strip (0: pipe_default_stages).
//     pipe is bitwise equal to kernel 5 and to stencilk5_rects_cpu; pipec to K
//     one-step launches and stencilk_rects_cpu.
//   12 piper / 22 piper_nosb: pipe with register-resident factors (K = 10..24
//     / K = 20, 24), bitwise equal to pipe. Kernel = 9 + arithmetic id
//     (pipe_arith.h); 11 and 13-21, 23-29 are retired (docs/TUNING.md).
constexpr int kPipeMaxK = 24;
int pipe_default_stages(int K);
bool pipe_has(int K, int stages, int arith = 0);
// Column waves per stage: 2 = blocks of 2 x stages waves over ~500 columns
// (V = 4 only, fast5 K = 16/20/24, csrc/lab/stencil_pipe_lab.hip, an experiment: slower
// than 1); pipe_has_cols says whether (K, S, arith, cols) is instantiated,
// pipe_default_cols is what a tuning of cols = 0 runs.
bool pipe_has_cols(int K, int stages, int arith, int cols);
int pipe_default_cols(int K, int stages, int arith);
// Cells per lane the pipelined kernel runs for a requested tuning.vec: 5
// (fast5, K = 16..20, nx % 5 == 0: lanes never straddle the array edge; 8-B
// aligned accesses), else 4 / 2 with 16-B aligned arrays and nx % 4 / % 2,
// else 1. The executor's frame geometry uses the same answer.
int pipe_vec(int K, int stages, int arith, int64_t nx, int requested, bool aligned16);
// ... of a launch that may run the uniform-factor variant (uniform: 1/Cp is one
// value and the launch stores no halos directly). requested = 6 then runs six
// cells per lane (384-column windows) where the instantiation exists (piper K =
// 17..23, piper_nosb K = 24), the arrays are 16-B aligned and nx is even (loads
// are clamped per 16-byte pair, so nx need not be a multiple of 6); every
// other case resolves as pipe_vec does, a request of 6 as one of 4. This is
// what stencil_pipe_rects_gpu runs; pipe_vec callers that do not know about
// uniformity (the benchmark's kstep_kernel report) keep answering 4.
int pipe_vec_uniform(int K, int stages, int arith, int64_t nx, int requested, bool aligned16,
                     bool uniform);
// Blocks per CU of the core pipelined kernel (occ[0]) and of its direct-store
// variant (occ[1]; 0 when it has none; both 0 outside the core library) for
// (K, stages, arith, V): the
// executor prices direct-store passes with it (DiffusionExecutor::set_direct).
void stencil_pipe_occupancy(int K, int stages, int arith, int V, int occ[2]);
// arith: the ids of pipe_arith.h (0 fast5, 1 canonical, 3 / 13 register factors)
void stencil_pipe_rects_gpu(int K, int stages, int arith, double* T2, const double* T,
                            const double* iCp, int64_t nx, int64_t ny, const Rect* rects,
                            int nrects, const StencilCoef& c, const StencilTuning& tune,
                            stream_t stream);
// The task of every block of a pipelined launch, computed on the host by the
// function the kernel itself runs (stencil_device.h locate_strip_task over
// plan_strip_tasks): out[3 b .. 3 b + 2] = (rect index among the non-empty
// rects, strip, chunk) of block b; returns the block count (out == nullptr:
// only counts). halo = K, V cells per lane, sw_block input columns per strip
// task, rect_rows / bands as StencilTuning, sig_rects > 0: the blocks of the
// first sig_rects rects are a signal prefix. For the CPU test of the mapping.
int64_t pipe_task_map(const Rect* rects, int nrects, int V, int chunk_rows, int halo,
                      int64_t sw_block, const int* rect_rows, int bands, int sig_rects, int remap,
                      int64_t* out);
// The grid the last stencil_pipe_rects_gpu call of this process launched:
// out[0] = blocks, out[1] = the band count its kernel got (RectList::nbands).
// Tests read it to see that a graded pass reached the device as planned.
void pipe_last_launch(int64_t out[2]);
// CPU twins of the fast5 arithmetic (one step / K steps, same operations and
// rounding as kernels 5-9: std::fma, -ffp-contract=off); the intermediate
// levels are updated on the interior only, like stencilk_rects_cpu.
void stencil5_rects_cpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                        const Rect* rects, int nrects, const StencilCoef& c);
void stencilk5_rects_cpu(int K, double* T2, const double* T, const double* iCp, int64_t nx,
                         int64_t ny, const Rect* rects, int nrects, const StencilCoef& c);

// Cells of A[0, n) whose 64-bit pattern differs from A[0]'s (-0.0 differs from
// 0.0, NaN payloads count), for DiffusionExecutor's uniform-1/Cp verdict. GPU:
// out[0] += the count (zero it on the same stream first), out[1] = A[0]'s bits;
// device memory, no synchronisation. The host twin returns the count.
void count_differing_gpu(const double* A, int64_t n, uint64_t* out2, stream_t stream);
int64_t count_differing_cpu(const double* A, int64_t n);

// ---------------------------------------------------------------------------
// Fused 7-point stencil on (nz, ny, nx) fields (stencil3d.hip): one explicit
// 3D diffusion step, T2[b] = f(T, iCp)[b] for every cell of up to kMaxBoxes
// half-open boxes inside the interior, in ONE launch (StencilCoef3 in
// rma/common.h has the expression; with Stencil3DTuning::xface one more launch on
// the same stream per lanes-per-row class of the face boxes). Throws before any work unless nx, ny,
// nz >= 3, T2 != T and every non-empty box lies in [1, n-1) per dimension.
// ---------------------------------------------------------------------------
constexpr int kMaxBoxes = 8;

struct Stencil3DTuning {
  int rows = 4;         // R: rows of the y-band one wave keeps in registers (2, 4, 8)
  int unroll = 2;       // planes per z-march iteration whose loads are issued together
                        // (1 or 2; 1 only with rows = 8)
  int vec = 2;          // cells per lane: 2 = one 16-byte access per row, 1 = scalar (also
                        // taken for odd nx or a base that is not 16-byte aligned)
  int nontemporal = 3;  // bit 0: NT T2 stores; bit 1: NT 1/Cp loads
  int chunk_z = 0;      // planes one wave marches (0: 32, the measured default)
  int xcd_remap = 1;    // 1: each XCD takes a contiguous 1/8 of the blocks
  // the K-step kernel (stencil3d_tb.hip) shares vec and xcd_remap and has its own
  int tb_rows = 0;         // output rows per wave (0: the measured default, 4; 2 or 4)
  int tb_chunk_z = 0;      // output planes one wave marches (0: the measured default, 32)
  int tb_nontemporal = 0;  // bits as nontemporal; 0 measured 6-7 % ahead of 3 for this kernel
  // 1/Cp is bit-for-bit the one value uniform_value in every cell (the caller
  // vouches for it; Diffusion3D scans the array): both kernels then run their
  // uniform-factor variant, which takes the value as an argument and never
  // reads the array (16 instead of 24 bytes per cell and pass), bitwise equal
  // to the field path. Every launch has the variant; bit 1 of nontemporal /
  // tb_nontemporal is accepted and has nothing to act on.
  bool uniform = false;
  double uniform_value = 0.0;
  // 1: the fast7 arithmetic (below) instead of the canonical flux expression,
  // in both kernels, field and uniform paths. Not bitwise equal to canonical;
  // needs fast7_ok(coef) (an invalid argument otherwise, before any work).
  int fast_math = 0;
  // The widest box in x (0..kXfaceMax) that runs an x-face path instead of the
  // thin-box path or the strip march; bitwise the same result. One-step kernel
  // (stencil3d.hip): a wave of 64/LX rows of LX = 8, 16 or 32 lanes marching along
  // z. K-step kernel (stencil3d_tb.hip): a wave of 64/LX groups of LX lanes, each
  // group the K-step march of one x segment of LX columns; a box of width W needs
  // W + 2(K-1) <= LX, so at K = 2 boxes wider than min(xface, 30) keep the strip
  // march. 0: today's dispatch. Outside 0..kXfaceMax: an invalid argument before
  // any work. plan_dispatch3d below is the rule both launchers run.
  int xface = 0;
  // Frame-first fused pass (the 2D fields of StencilTuning above, for boxes):
  // signal != nullptr makes the blocks of the first signal_boxes non-empty boxes
  // the signal prefix of the launch. They dispatch first (never XCD-remapped; the
  // rest is remapped among itself) and every one of their waves counts its
  // completion in signal[0] (device memory, zero); the last one resets the
  // counter and stores 1 into signal[1] with system-scope release. A
  // flag_wait_gpu(signal + 1, 1, ...) on another stream then orders work after
  // those boxes without waiting for the rest of the launch. Needs
  // 1 <= signal_boxes < the number of non-empty boxes and the shipped tuning
  // (rows = 4, unroll = 2; tb_rows 0 or 4): anything else is an invalid argument
  // before any work, as is signal_boxes != 0 without a signal. The x-face kernels
  // do not signal: in a signalling launch every box runs the march or thin path
  // and xface is not applied. Without a signal the launch is today's launch.
  uint64_t* signal = nullptr;
  int signal_boxes = 0;
};
constexpr int kXfaceMax = 32;

// Which kernel path each box of a 3D launch takes (kernel_select.cpp, host only;
// both launchers call it, so what it returns is what runs). K = 1: a box at most
// tune.xface wide runs the x-face kernel on 8, 16 or 32 lanes per row (the
// smallest >= its width), any other box at most 8 wide the thin-box path (one
// thread per row), the rest the strip march. K = 2: a box at most tune.xface wide
// with W + 2(K-1) <= 32 runs the K-step x-face kernel on the smallest lanes-per-
// segment class LX in {8, 16, 32} with W + 2(K-1) <= LX, the rest the strip march.
// out[i] describes boxes[i]; an empty box has path kPathNone. lanes: the lanes
// that share one row of the box (LX; 64 for a strip; 1 for the thin path).
// Throws on K other than 1 or 2 and on tune.xface outside 0..kXfaceMax.
enum Path3D { kPathNone = 0, kPathMarch = 1, kPathThin = 2, kPathXface = 3 };
struct Dispatch3D {
  int path = kPathNone;
  int lanes = 0;
};
void plan_dispatch3d(int K, const Box* boxes, int nboxes, const Stencil3DTuning& tune,
                     Dispatch3D* out);
const char* path3d_name(int path);  // "none", "march", "thin", "xface"
// The boxes of a launch sorted by plan_dispatch3d's path (kernel_select.cpp, host
// only; both launchers run it): wide[0..nwide) the boxes of the march launch,
// thin[i] marking those on the thin-box path, and face[c][0..nface[c]) the boxes
// of the x-face launch of lanes-per-row class c (8, 16, 32 lanes). Empty boxes
// are in no list; every list keeps the caller's order, which fixes the launch order.
struct Split3D {
  Box wide[kMaxBoxes];
  bool thin[kMaxBoxes] = {};
  int nwide = 0;
  Box face[3][kMaxBoxes];
  int nface[3] = {0, 0, 0};
  bool faces() const { return nface[0] + nface[1] + nface[2] > 0; }
};
Split3D split_boxes3d(int K, const Box* boxes, int nboxes, const Stencil3DTuning& tune);
// The march launch of a K-step pass at V cells per lane (stencil3d_vec), computed
// on the host by the function both launchers run (stencil3d.hip; no GPU needed):
// its blocks, the blocks of the signal prefix (the first signal_boxes non-empty
// boxes; 0: an unsignalled launch, which applies tune.xface as usual and counts the
// march launch only) and the waves that count in signal[0]. map != nullptr:
// map[2 b], map[2 b + 1] = (box index among the launch's boxes, block inside the
// box) of block b, by the function the signalling kernels run (block_after);
// room for 2 * blocks entries, so call it once with nullptr. tune.signal is not
// read: signal_boxes > 0 asks for the signalling plan with every launcher check.
struct Fused3DPlan {
  int64_t blocks = 0;
  int64_t prefix_blocks = 0;
  int64_t signalling_waves = 0;
  int boxes = 0;  // boxes of the march launch
};
Fused3DPlan stencil3d_fused_plan(int K, int V, const Box* boxes, int nboxes,
                                 const Stencil3DTuning& tune, int signal_boxes, int64_t* map);
// is (rows, unroll) an instantiated march?
bool stencil3d_has(int rows, int unroll);
// Cells per lane both 3D launchers run: tune.vec with even nx and 16-byte
// aligned T and T2 (and iCp, unless tune.uniform: the array is not read), else 1.
int stencil3d_vec(const double* T2, const double* T, const double* iCp, int64_t nx,
                  const Stencil3DTuning& tune);

void stencil3d_boxes_gpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                         int64_t nz, const Box* boxes, int nboxes, const StencilCoef3& c,
                         const Stencil3DTuning& tune, stream_t stream);
void stencil3d_boxes_cpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                         int64_t nz, const Box* boxes, int nboxes, const StencilCoef3& c);
// the argument checks both twins run before any work
void validate_boxes(const double* T2, const double* T, int64_t nx, int64_t ny, int64_t nz,
                    const Box* boxes, int nboxes);

// K steps per pass (temporal blocking, stencil3d_tb.hip): T2[b] = f^K(T)[b], the
// intermediate levels being f on the interior [1,n-1)^3 and T on the six faces.
// Bitwise equal to K full-interior calls of stencil3d_boxes_* followed by a crop
// to the boxes. T2 != T; cells outside the boxes are not written. K = 1 forwards
// to the one-step kernel; a K that stencil3dk_has() denies is an invalid
// argument before any work. Every box runs the strip march (no thin-box path)
// unless Stencil3DTuning::xface sends it to the K-step x-face kernel.
bool stencil3dk_has(int K);
bool stencil3dk_has_rows(int rows);  // Stencil3DTuning::tb_rows values instantiated
void stencil3dk_boxes_gpu(int K, double* T2, const double* T, const double* iCp, int64_t nx,
                          int64_t ny, int64_t nz, const Box* boxes, int nboxes,
                          const StencilCoef3& c, const Stencil3DTuning& tune, stream_t stream);
// the one-step twin applied K times through two scratch arrays (any K >= 1)
void stencil3dk_boxes_cpu(int K, double* T2, const double* T, const double* iCp, int64_t nx,
                          int64_t ny, int64_t nz, const Box* boxes, int nboxes,
                          const StencilCoef3& c);

// fast7: the 7-point sum with the constants folded into one per-cell factor
// (the 3D counterpart of fast5; 8 fp64 operations per update, 7 with uniform
// 1/Cp, against ~30 of the canonical flux expression). On the host, in double,
//   ax = (-mlam)*rdx*rdx   ay = (-mlam)*rdy*rdy   az = (-mlam)*rdz*rdz
//   ry = ay/ax   rz = az/ax   mkc = -2.0*((1.0 + ry) + rz)   gs = dt*ax
// and per cell, c = T[z][y][x],
//   sx = T[x+1] + T[x-1]   sy = T[y-1] + T[y+1]   sz = T[z-1] + T[z+1]
//   t = fma(mkc, c, sx);  t = fma(ry, sy, t);  t = fma(rz, sz, t)
//   T2 = fma(gs*iCp, t, c)            (gs*iCp is one rounded multiply)
// With uniform 1/Cp the kernels take g = gs*value, the same product, formed
// once on the host. Explicit fmas under -ffp-contract=off: the std::fma twins
// below are bitwise equal to the GPU kernels (Stencil3DTuning::fast_math).
// fast7_ok: ax != 0 and ay/ax, az/ax and dt*ax finite.
bool fast7_ok(const StencilCoef3& c);
struct Fast7 {
  double mkc, ry, rz, gs;
};
Fast7 fast7_constants(const StencilCoef3& c);
// Same signatures and argument checks as the canonical twins, plus fast7_ok;
// the K-step twin applies the one-step twin K times through two scratch arrays.
void stencil3d7_boxes_cpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                          int64_t nz, const Box* boxes, int nboxes, const StencilCoef3& c);
void stencil3dk7_boxes_cpu(int K, double* T2, const double* T, const double* iCp, int64_t nx,
                           int64_t ny, int64_t nz, const Box* boxes, int nboxes,
                           const StencilCoef3& c);

// Width (in cells) of one wave's x-strip in the march kernel; perf_hide rounds
// its x-frame so the interior rect starts on a strip boundary.
int stencil_vec(int64_t nx, const StencilTuning& tune);
int stencil_strip_cells(int64_t nx, const StencilTuning& tune);

// ---------------------------------------------------------------------------
// kp: the three-kernel formulation (K1-K3; scripts/diffusion_2D_kp.jl:16-54).
// QX, QY, D are full (ny, nx) buffers indexed like T (see kp.hip):
//   QX[y][x] = reference qx[y-1][x]   (rows 1..ny-2, cols 0..nx-2)
//   QY[y][x] = reference qy[y][x-1]   (rows 0..ny-2, cols 1..nx-2)
//   D [y][x] = reference dTdt[y-1][x-1] (interior)
// The GPU versions use 16-byte accesses for even nx and aligned buffers and a
// scalar path otherwise.
// ---------------------------------------------------------------------------
void flux_gpu(double* QX, double* QY, const double* T, int64_t nx, int64_t ny, double mlam,
              double rdx, double rdy, stream_t stream);
void residual_gpu(double* D, const double* QX, const double* QY, const double* iCp, int64_t nx,
                  int64_t ny, double rdx, double rdy, stream_t stream);
void update_gpu(double* T, const double* D, int64_t nx, int64_t ny, double dt, stream_t stream);
void flux_cpu(double* QX, double* QY, const double* T, int64_t nx, int64_t ny, double mlam,
              double rdx, double rdy);
void residual_cpu(double* D, const double* QX, const double* QY, const double* iCp, int64_t nx,
                  int64_t ny, double rdx, double rdy);
void update_cpu(double* T, const double* D, int64_t nx, int64_t ny, double dt);
bool kp_native_layout_ok(int64_t nx);

// ---------------------------------------------------------------------------
// Initial conditions (K9/K10). Device-side so a 288 GB tile never touches the
// host.
// ---------------------------------------------------------------------------
// Geometry of a local tile inside the implicit global grid: global coordinate
// of local cell ix is x = (gx0 + ix)*dx + xoff, wrapped into [0, nxg*dx) when
// periodic (ImplicitGlobalGrid x_g semantics).
struct TileGeom {
  int64_t gx0, gy0;    // global index of local cell (0,0)
  int64_t nxg, nyg;    // global grid size
  double dx, dy;
  double xoff, yoff;   // staggering offsets 0.5*(n - size(A))*d
  int periodx, periody;
};

// T = exp(-(x+dx/2-lx/2)^2 - (y+dy/2-ly/2)^2)   (ap.jl:28)
void init_gaussian_gpu(double* T, int64_t nx, int64_t ny, const TileGeom& g, double lx, double ly,
                       stream_t stream);
void init_gaussian_cpu(double* T, int64_t nx, int64_t ny, const TileGeom& g, double lx, double ly);
// Counter-based uniform [lo,hi) keyed by the GLOBAL cell index, so every
// decomposition of the same global grid sees the same field (bitwise) and the
// overlap cells of neighbouring ranks agree.
void init_random_gpu(double* A, int64_t nx, int64_t ny, const TileGeom& g, uint64_t seed,
                     double lo, double hi, stream_t stream);
void init_random_cpu(double* A, int64_t nx, int64_t ny, const TileGeom& g, uint64_t seed,
                     double lo, double hi);
void fill_gpu(double* A, int64_t n, double value, stream_t stream);

// The same for a (nz, ny, nx) tile of a 3D global grid.
struct TileGeom3 {
  int64_t gx0, gy0, gz0;
  int64_t nxg, nyg, nzg;
  double dx, dy, dz;
  double xoff, yoff, zoff;
  int periodx, periody, periodz;
};
// T = exp(-(a*a) - (b*b) - (c*c)), a, b as in 2D, c = (z + dz/2) - lz/2
void init_gaussian3d_gpu(double* T, int64_t nx, int64_t ny, int64_t nz, const TileGeom3& g,
                         double lx, double ly, double lz, stream_t stream);
void init_gaussian3d_cpu(double* T, int64_t nx, int64_t ny, int64_t nz, const TileGeom3& g,
                         double lx, double ly, double lz);
// uniform01(seed, (gz*nyg + gy)*nxg + gx) over the wrapped global indices
void init_random3d_gpu(double* A, int64_t nx, int64_t ny, int64_t nz, const TileGeom3& g,
                       uint64_t seed, double lo, double hi, stream_t stream);
void init_random3d_cpu(double* A, int64_t nx, int64_t ny, int64_t nz, const TileGeom3& g,
                       uint64_t seed, double lo, double hi);

// ---------------------------------------------------------------------------
// Halo pack / unpack (K7/K8): strided 2D block copy. Both sides have a
// contiguous inner dimension of n_k elements; outer rows are dst_ld / src_ld
// elements apart. Element size in bytes: 2, 4, 8 or 16.
// ---------------------------------------------------------------------------
void copy2d_gpu(void* dst, int64_t dst_ld, const void* src, int64_t src_ld, int64_t n_o,
                int64_t n_k, int elem_bytes, stream_t stream);
void copy2d_cpu(void* dst, int64_t dst_ld, const void* src, int64_t src_ld, int64_t n_o,
                int64_t n_k, int elem_bytes);
// Up to kCopy2dBatch independent copies of one element size in ONE launch
// (the halo engine issues all packs of a dimension, then all its unpacks, as
// one batch each). Empty copies are skipped.
constexpr int kCopy2dBatch = 8;
struct Copy2d {
  void* dst;
  int64_t dst_ld;
  const void* src;
  int64_t src_ld, n_o, n_k;
};
void copy2d_batch_gpu(const Copy2d* copies, int n, int elem_bytes, stream_t stream);
void copy2d_batch_cpu(const Copy2d* copies, int n, int elem_bytes);

// ---------------------------------------------------------------------------
// Batched strided 3D block copy (blocks.hip): the pack (strided view -> dense
// send buffer) and place (rank-major staging -> Cartesian A_global) primitive
// of the C ABI's gather (rma/gather.h), and the device crop
// Array(T[2:end-1,2:end-1]) of the reference scripts. Each block is nz planes
// of ny rows of nx contiguous elements on both sides; pitches and extents in
// elements, x fastest. Element size 4 or 8 bytes. A pitch along an extent of
// 1 is never used and may be anything. Blocks of one call must not overlap in
// dst. The GPU launcher splits n blocks into launches of <= kCopyBlocksBatch
// descriptors of one access path (16-byte vectors when every row length, base
// address and used pitch of the block is a multiple of 16 bytes, single
// elements otherwise), in the order given. copy_blocks_cpu is the bitwise twin.
// ---------------------------------------------------------------------------
struct BlockCopy {
  void* dst;
  const void* src;
  int64_t dst_row, dst_plane, src_row, src_plane;
  int64_t nx, ny, nz;
};
constexpr int kCopyBlocksBatch = 32;  // 32 x 72 B of kernel arguments per launch
// throws unless elem_bytes is 4 or 8, every pointer is set, every extent is
// > 0 and every used pitch holds its extent (both twins call it before any work)
void validate_block_copies(const BlockCopy* blocks, int64_t n, int elem_bytes);
void copy_blocks_gpu(const BlockCopy* blocks, int64_t n, int elem_bytes, stream_t stream);
void copy_blocks_cpu(const BlockCopy* blocks, int64_t n, int elem_bytes);

// ---------------------------------------------------------------------------
// Streaming roofline probes (same-box HBM ceiling for the T_eff comparison):
//   copy : b[i] = a[i]              (1 read + 1 write)
//   triad: c[i] = a[i] + s*b[i]     (2 reads + 1 write = the stencil's mix)
// 16-byte vector accesses, grid-stride.
// ---------------------------------------------------------------------------
void stream_copy_gpu(double* b, const double* a, int64_t n, int nt, int blocks, stream_t stream);
void stream_triad_gpu(double* c, const double* a, const double* b, double s, int64_t n, int nt,
                      int blocks, stream_t stream);

// ---------------------------------------------------------------------------
// Stream-ordered flags in host-registered shared memory (flags.hip; the HIP
// IPC transport's stream mode): wait until *flag == want (bounded: after
// timeout_s the kernel stores `code` into *err and exits), or store value
// with system-scope release. One 64-lane workgroup each; graph-capturable.
// ---------------------------------------------------------------------------
void flag_wait_gpu(const uint64_t* flag, uint64_t want, double timeout_s, uint32_t* err,
                   uint32_t code, stream_t stream);
void flag_write_gpu(uint64_t* flag, uint64_t value, stream_t stream);
// Direct-store halo passes: wait until every flags[i] with bit i of mask set
// is >= want (bounded, as flag_wait_gpu); store value into every non-null
// dst[i] (system-scope release), i < 8. One 64-lane workgroup each.
void flags_wait_ge_gpu(const uint64_t* flags, uint32_t mask, uint64_t want, double timeout_s,
                       uint32_t* err, uint32_t code, stream_t stream);
struct FlagTargets {
  uint64_t* dst[8] = {};
};
void flags_write_gpu(const FlagTargets& t, uint64_t value, stream_t stream);

// ---------------------------------------------------------------------------
// Reductions for verification / NaN guards. Result is written
// to out (device memory, 1 double). workspace must hold reduce_workspace_doubles().
// ---------------------------------------------------------------------------
enum ReduceOp : int { kSum = 0, kMax = 1, kMin = 2, kMaxAbs = 3, kNonFinite = 4 };
int64_t reduce_workspace_doubles();
void reduce_gpu(const double* A, int64_t n, int op, double* out, double* workspace,
                stream_t stream);
double reduce_cpu(const double* A, int64_t n, int op);
// One pass over a field: out3 = {non-finite count, min, max of the finite cells}
// (device memory; workspace: field_stats_workspace_doubles()). The full-field
// check of a timed run (bench.py).
int64_t field_stats_workspace_doubles();
void field_stats_gpu(const double* A, int64_t n, double* out3, double* workspace,
                     stream_t stream);
void field_stats_cpu(const double* A, int64_t n, double* out3);

}  // namespace rma
