// Native time loop of 3D heat diffusion: what Diffusion3D.step enqueues
// (rocm_mpi_amd/models/diffusion3d.py), issued from C++ so that a pass costs its
// launches and nothing else on the host. No kernel of its own: every pass is one
// or two launches of stencil3d_boxes_gpu / stencil3dk_boxes_gpu plus
// HaloExchanger::exchange, and the field is bitwise the Python-issued one.
//
//   perf      : [owned box of the pass] -> swap -> [exchange(new field)], all on
//               the caller's stream.
//   perf_hide : H (high priority): [frame slabs] ............ [exchange(T2)]
//               L (normal)       :      [interior box]
//               per pass, enqueued frame, interior, exchange (a transport whose
//               exchange blocks the host still overlaps), then swap. Ordering is
//               by events only: H and L wait for the caller's stream at entry,
//               the caller's stream waits for both at exit; between passes, with
//               X the buffer pass p writes and Y the one it reads,
//                 * H's frame of pass p+1 waits for L's interior of pass p (it
//                   reads interior cells of X and overwrites frame cells of Y,
//                   which that interior read); the exchange of pass p precedes
//                   it on H in stream order;
//                 * L's interior of pass p+1 waits for H's frame kernel of pass
//                   p, not for its exchange: it reads X at least overlap - K >=
//                   halo width cells from the array edge, never a halo cell, and
//                   writes interior cells of Y, which the exchange does not touch.
//               A pass without a frame slab or without an interior box is the
//               perf pass, kept ordered on H while another depth of the same run
//               overlaps, on the caller's stream otherwise.
//
//   perf_hide, fused = 1 (frame-first single-launch passes): a pass that splits
//               is ONE launch on L, the frame slabs as its signal prefix and the
//               interior after them (Stencil3DTuning::signal); the last frame wave
//               raises a device flag that H waits on:
//                 H : ......[wait flag][lower flag][exchange(T2)]
//                 L : [frame blocks | interior blocks ............]
//               per pass, enqueued in this order: L waits for the event of H's
//               previous exchange (the frame blocks read the halo); the launch on
//               L; on H flag_wait_gpu(signal + 1, 1), flag_write_gpu(signal + 1, 0),
//               the exchange of the new field, its event. The launch is always
//               enqueued before the wait on it, so a wait depends only on work
//               enqueued earlier. The flag is lowered before the next launch can
//               start (that launch waits for this exchange), the counter is
//               re-armed by the wave that raises the flag. In such a launch no
//               box takes the x-face path. Passes that do not split stay the perf
//               pass, ordered as above. The wait is bounded (fused_timeout_s);
//               a timeout is recorded in a mapped host word and reported as an
//               invalid argument by the next run(), by check() and at destruction
//               (on stderr there: a destructor does not throw).
//
// run(n) plans n / K passes of K = steps_per_pass steps, then n % K one-step
// passes. The exchange is the per-dimension one with exact corners.
//
// Out of scope (the 2D executor, rma/executor.h, has them): hipGraph replay, a
// pass planner, direct-store halos, passes deeper than two steps, and the x-face
// path inside a fused launch.
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "rma/halo.h"
#include "rma/kernels.h"
#include "rma/plan3d.h"

namespace rma {

struct Exec3DParams {
  int mode = 0;  // 0 = perf, 1 = perf_hide
  StencilCoef3 coef{};
  int steps_per_pass = 1;  // K: 1 or 2
  int fast_math = 0;       // every pass, the one-step remainder included, runs fast7
  std::array<int64_t, 3> b_width{16, 2, 2};  // perf_hide boundary width from the array edge
  // perf_hide: widest frame box on the kernels' x-face paths, 0..kXfaceMax;
  // -1: min(max(b_width[0], overlap_x), kXfaceMax). It applies to the frame launch
  // of one- and two-step passes; in a two-step frame boxes wider than 30 keep the
  // strip march (plan_dispatch3d).
  int xface = 0;
  bool uniform_factor = true;  // uniform-1/Cp kernel variants where the scan allows
  Stencil3DTuning tune{};      // uniform*, fast_math and xface are set per launch
  // of the grid: overlap and halo width per dimension (x, y, z)
  std::array<int64_t, 3> overlaps{2, 2, 2};
  std::array<int64_t, 3> halowidths{1, 1, 1};
  // perf_hide: 1 = frame-first single-launch passes (above), 0 = two launches on
  // two streams. The default is decided by profiles/diffusion3d_fused.md.
  int fused = 0;
  // bound of the exchange stream's wait for the frame flag, seconds; the
  // environment's RMA_EXEC_FUSED_TIMEOUT, where set, replaces it (as in 2D)
  double fused_timeout_s = 60.0;
};

class Diffusion3DExecutor {
 public:
  // T, T2, iCp: (nz, ny, nx) device fields, x fastest; T holds the field, T2 a
  // copy of it (at least of its boundary cells). halo may be null for a tile
  // without neighbours. Refused before any launch (an invalid argument naming
  // what is wrong): mode outside {0, 1}, steps_per_pass outside {1, 2}, an
  // extent < 3, along a dimension with a neighbour an overlap below 2K or a halo
  // width other than K, fast_math with coefficients that fail fast7_ok, a
  // b_width < 1, xface outside -1..kXfaceMax, null or overlapping T / T2 / iCp,
  // fused outside {0, 1}, fused = 1 with mode = perf or a tuning the signalling
  // kernels are not instantiated for (rows 4, unroll 2, tb_rows 0 or 4).
  // Synchronises the device once (the 1/Cp scan) and prepares the exchanger's
  // pack buffers for both fields.
  Diffusion3DExecutor(double* T, double* T2, const double* iCp, int64_t nx, int64_t ny, int64_t nz,
                      const Exec3DParams& p, HaloExchanger* halo);
  ~Diffusion3DExecutor();
  Diffusion3DExecutor(const Diffusion3DExecutor&) = delete;
  Diffusion3DExecutor& operator=(const Diffusion3DExecutor&) = delete;

  // Enqueue n steps after the work already on caller_stream; caller_stream is
  // made to wait for them. Asynchronous: no host synchronisation.
  void run(int64_t nsteps, stream_t caller_stream);
  std::vector<int> plan(int64_t nsteps) const;
  // Number of completed buffer swaps mod 2: 0 -> the field is in T, 1 -> in T2.
  int parity() const { return parity_; }
  int64_t steps_done() const { return steps_; }
  int64_t passes_done() const { return passes_; }
  // passes enqueued as one frame-first launch (fused = 1 and the pass splits)
  int64_t fused_passes() const { return fused_passes_; }
  double fused_timeout_s() const { return fused_timeout_s_; }
  // Throws (an invalid argument) if a fused pass's wait for the frame flag has
  // timed out since construction: the halos of that pass are wrong. run() calls
  // it first; call it after synchronising to learn about the passes just run.
  void check() const;
  // The verdict of the last scan of 1/Cp (count_differing_gpu): every cell holds
  // bit for bit one value, which the passes then take as a kernel argument
  // instead of reading the array. False with Exec3DParams::uniform_factor off
  // or RMA_DIAG=uniform_factor=off. run() does not re-examine the array: after
  // writing to 1/Cp call rescan_factor() (synchronises the device).
  bool uniform() const { return uniform_; }
  double uniform_value() const { return c0_; }
  bool rescan_factor();
  int frame_xface() const { return xface_; }
  Box owned(int K) const { return owned_box3d({nx_, ny_, nz_}, nbr_, K); }
  HideBoxes3 hide_boxes(int K) const;

 private:
  void launch(int K, const Box* boxes, int n, bool frame, double* Tin, double* Tout,
              stream_t s, int signal_boxes = 0) const;
  void exchange(double* A, stream_t s);
  HaloField field(double* A) const;
  void scan_factor();
  void release();

  double* T_;
  double* T2_;
  const double* iCp_;
  int64_t nx_, ny_, nz_;
  Exec3DParams p_;
  HaloExchanger* halo_;
  Neighbors nbr_{{{-1, -1}, {-1, -1}, {-1, -1}}};
  int xface_ = 0;
  bool uniform_ = false;
  double c0_ = 0.0;
  void* s_hi_ = nullptr;  // hipStream_t, perf_hide only
  void* s_lo_ = nullptr;
  void* ev_in_ = nullptr;  // hipEvent_t
  void* ev_frame_ = nullptr;
  void* ev_inner_ = nullptr;
  void* ev_halo_ = nullptr;
  int parity_ = 0;
  int64_t steps_ = 0;
  int64_t passes_ = 0;
  int64_t fused_passes_ = 0;
  double fused_timeout_s_ = 60.0;
  uint64_t* sig_ = nullptr;        // device: [frame wave counter, frame flag], fused only
  uint32_t* ferr_host_ = nullptr;  // mapped host word: 1 = a frame wait timed out
  uint32_t* ferr_dev_ = nullptr;
};

}  // namespace rma
