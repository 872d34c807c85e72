// Native time loop of 3D heat diffusion (see rma/executor3d.h).
#include "rma/executor3d.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rma/config.h"
#include "rma/hip_check.h"

namespace rma {

namespace {
hipStream_t S(void* p) { return reinterpret_cast<hipStream_t>(p); }
hipEvent_t E(void* p) { return reinterpret_cast<hipEvent_t>(p); }

bool overlap(const double* a, const double* b, int64_t cells) {
  const auto a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  const uintptr_t bytes = (uintptr_t)cells * sizeof(double);
  return a0 < b0 + bytes && b0 < a0 + bytes;
}
}  // namespace

Diffusion3DExecutor::Diffusion3DExecutor(double* T, double* T2, const double* iCp, int64_t nx,
                                         int64_t ny, int64_t nz, const Exec3DParams& p,
                                         HaloExchanger* halo)
    : T_(T), T2_(T2), iCp_(iCp), nx_(nx), ny_(ny), nz_(nz), p_(p), halo_(halo) {
  // every refusal comes before the first HIP call
  RMA_CHECK_ARG(p.mode == 0 || p.mode == 1, "mode " << p.mode << " (0 perf, 1 perf_hide)");
  const int K = p.steps_per_pass;
  RMA_CHECK_ARG(K == 1 || K == 2, "steps_per_pass " << K << " (1 or 2)");
  RMA_CHECK_ARG(nx >= 3 && ny >= 3 && nz >= 3,
                "nx, ny, nz >= 3 required, got " << nx << ", " << ny << ", " << nz);
  RMA_CHECK_ARG(T != nullptr && T2 != nullptr && iCp != nullptr, "T, T2 or iCp is NULL");
  const int64_t cells = nx * ny * nz;
  RMA_CHECK_ARG(!overlap(T, T2, cells), "T2 must not alias T (double buffering)");
  RMA_CHECK_ARG(!overlap(T, iCp, cells) && !overlap(T2, iCp, cells), "iCp must not alias T or T2");
  for (int d = 0; d < 3; ++d)
    RMA_CHECK_ARG(p.b_width[d] >= 1, "b_width[" << d << "] = " << p.b_width[d] << " (>= 1)");
  RMA_CHECK_ARG(p.xface >= -1 && p.xface <= kXfaceMax,
                "xface " << p.xface << " (-1, or 0.." << kXfaceMax << ")");
  RMA_CHECK_ARG(!p.fast_math || fast7_ok(p.coef),
                "fast_math: the fast7 arithmetic needs lam != 0 and finite coefficients");
  RMA_CHECK_ARG(p.fused == 0 || p.fused == 1,
                "fused " << p.fused << " (0 two launches, 1 frame-first single launch)");
  RMA_CHECK_ARG(!p.fused || p.mode == 1, "fused " << p.fused << " needs mode 1 (perf_hide), got "
                                                          << "mode " << p.mode);
  // the signalling kernels exist for the shipped tuning only (plan_launch3d refuses
  // the rest per launch; here it is refused once, before any work)
  RMA_CHECK_ARG(!p.fused || (p.tune.rows == 4 && p.tune.unroll == 2 &&
                             (p.tune.tb_rows == 0 || p.tune.tb_rows == 4)),
                "fused 1 needs rows 4, unroll 2 and tb_rows 0 or 4, got rows "
                    << p.tune.rows << ", unroll " << p.tune.unroll << ", tb_rows "
                    << p.tune.tb_rows);
  RMA_CHECK_ARG(p.fused_timeout_s > 0.0, "fused_timeout_s " << p.fused_timeout_s << " (> 0)");
  // bounded wait of the exchange stream for the frame flag (seconds); the
  // environment's value, where set, replaces the parameter, as in the 2D executor
  fused_timeout_s_ = std::getenv("RMA_EXEC_FUSED_TIMEOUT")
                         ? env_double("RMA_EXEC_FUSED_TIMEOUT", 60.0, 1e-9, 1e6)
                         : p.fused_timeout_s;
  if (halo_) nbr_ = halo_->neighbors();
  for (int d = 0; d < 3; ++d) {
    if (nbr_[d][0] < 0 && nbr_[d][1] < 0) continue;
    RMA_CHECK_ARG(p.overlaps[d] >= 2 * K, "steps_per_pass " << K << " needs a grid overlap >= "
                                              << 2 * K << " along dim " << d << ", got "
                                              << p.overlaps[d]);
    RMA_CHECK_ARG(p.halowidths[d] == K, "steps_per_pass " << K << " needs halo width " << K
                                            << " along dim " << d << ", got " << p.halowidths[d]);
  }
  const std::string v = diag_value("uniform_factor");
  RMA_CHECK_ARG(v.empty() || v == "off", "RMA_DIAG uniform_factor=" << v << " (off)");
  xface_ = p.xface >= 0
               ? p.xface
               : (int)std::min<int64_t>(std::max(p.b_width[0], p.overlaps[0]), kXfaceMax);
  try {
    if (p_.mode == 1) {
      int least = 0, greatest = 0;
      RMA_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
      // the model's pair: the highest priority for the frame and the exchange,
      // the default one (0) for the interior
      hipStream_t hi = nullptr, lo = nullptr;
      RMA_HIP_CHECK(hipStreamCreateWithPriority(&hi, hipStreamNonBlocking, greatest));
      s_hi_ = hi;
      RMA_HIP_CHECK(hipStreamCreateWithPriority(&lo, hipStreamNonBlocking, 0));
      s_lo_ = lo;
      for (void** e : {&ev_in_, &ev_frame_, &ev_inner_, &ev_halo_})
        RMA_HIP_CHECK(
            hipEventCreateWithFlags(reinterpret_cast<hipEvent_t*>(e), hipEventDisableTiming));
      if (p_.fused) {
        RMA_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&sig_), 2 * sizeof(uint64_t)));
        // zeroed on the stream the signalling launches run on and waited for: a
        // null-stream memset is not ordered before work on a non-blocking stream
        RMA_HIP_CHECK(hipMemsetAsync(sig_, 0, 2 * sizeof(uint64_t), lo));
        RMA_HIP_CHECK(hipStreamSynchronize(lo));
        RMA_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&ferr_host_), sizeof(uint32_t),
                                    hipHostMallocMapped));
        *ferr_host_ = 0;
        RMA_HIP_CHECK(
            hipHostGetDevicePointer(reinterpret_cast<void**>(&ferr_dev_), ferr_host_, 0));
      }
    }
    scan_factor();
    // the pack buffers exist before the first run (no allocation inside it)
    if (halo_) {
      halo_->prepare({field(T_)}, 7);
      halo_->prepare({field(T2_)}, 7);
    }
  } catch (...) {
    release();
    throw;
  }
}

Diffusion3DExecutor::~Diffusion3DExecutor() {
  // drain first: a timeout of the last run is known only then
  if (s_hi_) (void)hipStreamSynchronize(S(s_hi_));
  if (ferr_host_ && __atomic_load_n(ferr_host_, __ATOMIC_ACQUIRE) != 0)
    std::fprintf(stderr,
                 "rma: Diffusion3DExecutor: a fused pass's wait for the frame flag timed out "
                 "after %g s (RMA_EXEC_FUSED_TIMEOUT); the halos of that pass are wrong\n",
                 fused_timeout_s_);
  release();
}

void Diffusion3DExecutor::check() const {
  if (!ferr_host_) return;
  const uint32_t e = __atomic_load_n(ferr_host_, __ATOMIC_ACQUIRE);
  RMA_CHECK_ARG(e == 0, "frame-first fused pass: the exchange stream's wait for the frame flag "
                        "timed out after "
                            << fused_timeout_s_
                            << " s (RMA_EXEC_FUSED_TIMEOUT); the halos of that pass are wrong");
}

void Diffusion3DExecutor::release() {
  // work of the last run may still be queued on the two streams
  if (s_hi_) (void)hipStreamSynchronize(S(s_hi_));
  if (s_lo_) (void)hipStreamSynchronize(S(s_lo_));
  for (void** e : {&ev_in_, &ev_frame_, &ev_inner_, &ev_halo_}) {
    if (*e) (void)hipEventDestroy(E(*e));
    *e = nullptr;
  }
  if (s_hi_) (void)hipStreamDestroy(S(s_hi_));
  if (s_lo_) (void)hipStreamDestroy(S(s_lo_));
  s_hi_ = s_lo_ = nullptr;
  // the streams' flag kernels and launches are drained: the words can go
  if (sig_) (void)hipFree(sig_);
  if (ferr_host_) (void)hipHostFree(ferr_host_);
  sig_ = nullptr;
  ferr_host_ = ferr_dev_ = nullptr;
}

void Diffusion3DExecutor::scan_factor() {
  uniform_ = false;
  c0_ = 0.0;
  const std::string v = diag_value("uniform_factor");
  RMA_CHECK_ARG(v.empty() || v == "off", "RMA_DIAG uniform_factor=" << v << " (off)");
  if (!p_.uniform_factor || v == "off") return;
  // whoever wrote 1/Cp did so on a stream of their own: wait for the device
  RMA_HIP_CHECK(hipDeviceSynchronize());
  uint64_t* d = nullptr;
  RMA_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d), 2 * sizeof(uint64_t)));
  uint64_t h[2] = {1, 0};
  try {
    // the device is idle: the null stream orders the three operations
    RMA_HIP_CHECK(hipMemsetAsync(d, 0, 2 * sizeof(uint64_t), nullptr));
    count_differing_gpu(iCp_, nx_ * ny_ * nz_, d, nullptr);
    RMA_HIP_CHECK(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, nullptr));
    RMA_HIP_CHECK(hipStreamSynchronize(nullptr));
  } catch (...) {
    (void)hipStreamSynchronize(nullptr);
    (void)hipFree(d);
    throw;
  }
  RMA_HIP_CHECK(hipFree(d));
  if (h[0] != 0) return;
  uniform_ = true;
  std::memcpy(&c0_, &h[1], sizeof c0_);
}

bool Diffusion3DExecutor::rescan_factor() {
  scan_factor();
  return uniform_;
}

HideBoxes3 Diffusion3DExecutor::hide_boxes(int K) const {
  return hide_boxes3d({nx_, ny_, nz_}, owned(K), sides3d(nbr_), p_.overlaps, p_.b_width);
}

std::vector<int> Diffusion3DExecutor::plan(int64_t nsteps) const {
  RMA_CHECK_ARG(nsteps >= 0, "nsteps " << nsteps);
  const int K = p_.steps_per_pass;
  std::vector<int> out((size_t)(nsteps / K), K);
  out.insert(out.end(), (size_t)(nsteps % K), 1);
  return out;
}

HaloField Diffusion3DExecutor::field(double* A) const {
  HaloField f;
  f.ptr = A;
  f.size = {nx_, ny_, nz_};
  f.elem_bytes = 8;
  f.ol = p_.overlaps;
  f.hw = p_.halowidths;
  return f;
}

void Diffusion3DExecutor::exchange(double* A, stream_t s) {
  if (halo_) halo_->exchange({field(A)}, s, 7);
}

void Diffusion3DExecutor::launch(int K, const Box* boxes, int n, bool frame, double* Tin,
                                 double* Tout, stream_t s, int signal_boxes) const {
  Box b[kMaxBoxes];
  int m = 0;
  for (int i = 0; i < n; ++i)
    if (!boxes[i].empty()) b[m++] = boxes[i];
  if (m == 0) return;
  Stencil3DTuning tn = p_.tune;
  tn.fast_math = p_.fast_math ? 1 : 0;
  tn.uniform = uniform_;
  tn.uniform_value = uniform_ ? c0_ : 0.0;
  tn.xface = frame ? xface_ : 0;  // one- and two-step frames (plan_dispatch3d caps the width)
  if (signal_boxes > 0) {  // a fused pass: the first boxes are the signal prefix, no face path
    tn.signal = sig_;
    tn.signal_boxes = signal_boxes;
    tn.xface = 0;
  }
  if (K == 1)
    stencil3d_boxes_gpu(Tout, Tin, iCp_, nx_, ny_, nz_, b, m, p_.coef, tn, s);
  else
    stencil3dk_boxes_gpu(K, Tout, Tin, iCp_, nx_, ny_, nz_, b, m, p_.coef, tn, s);
}

void Diffusion3DExecutor::run(int64_t nsteps, stream_t caller) {
  check();
  const std::vector<int> passes = plan(nsteps);
  if (passes.empty()) return;
  // the depths of this run: K and, with a remainder, 1
  HideBoxes3 split[3];
  bool overlapped = false;
  if (p_.mode == 1)
    for (int k : {passes.front(), passes.back()}) {
      split[k] = hide_boxes(k);
      overlapped = overlapped || split[k].split();
    }
  hipStream_t cur = S(caller), H = S(s_hi_), L = S(s_lo_);
  if (overlapped) {
    RMA_HIP_CHECK(hipEventRecord(E(ev_in_), cur));
    RMA_HIP_CHECK(hipStreamWaitEvent(H, E(ev_in_), 0));
    RMA_HIP_CHECK(hipStreamWaitEvent(L, E(ev_in_), 0));
    // the first pass waits on these as on "the pass before"
    RMA_HIP_CHECK(hipEventRecord(E(ev_inner_), L));
    RMA_HIP_CHECK(hipEventRecord(E(ev_frame_), H));
  }
  for (int k : passes) {
    double* Tin = parity_ ? T2_ : T_;
    double* Tout = parity_ ? T_ : T2_;
    if (p_.mode == 0 || !split[k].split()) {
      // one launch, swap, exchange of the new field: the perf pass
      Box one = owned(k);
      const Box* boxes = &one;
      int n = 1;
      if (p_.mode == 1 && !split[k].has_interior) {
        boxes = split[k].frame.data();
        n = (int)split[k].frame.size();
      }
      if (overlapped) {  // another depth of this run overlaps: stay ordered on H
        RMA_HIP_CHECK(hipStreamWaitEvent(H, E(ev_inner_), 0));
        launch(k, boxes, n, false, Tin, Tout, H);
        exchange(Tout, H);
        RMA_HIP_CHECK(hipEventRecord(E(ev_frame_), H));
        RMA_HIP_CHECK(hipStreamWaitEvent(L, E(ev_frame_), 0));
        RMA_HIP_CHECK(hipEventRecord(E(ev_inner_), L));
      } else {
        launch(k, boxes, n, false, Tin, Tout, cur);
        exchange(Tout, cur);
      }
    } else if (p_.fused) {
      // Frame-first single launch (rma/executor3d.h). ev_frame_ is the event of
      // H's previous exchange here (the unsplit pass above records it there too):
      // the frame blocks read the halo. The launch follows the previous one on L
      // in stream order, which covers what the frame of a split pass waits for.
      const HideBoxes3& sp = split[k];
      Box b[kMaxBoxes];
      int m = 0;
      for (const Box& f : sp.frame)
        if (!f.empty()) b[m++] = f;
      const int nframe = m;
      b[m++] = sp.interior;
      RMA_HIP_CHECK(hipStreamWaitEvent(L, E(ev_frame_), 0));
      launch(k, b, m, false, Tin, Tout, L, nframe);
      RMA_HIP_CHECK(hipEventRecord(E(ev_inner_), L));
      // exchange stream: the frame flag (bounded wait), lowered for the next pass;
      // the launch it waits on is already enqueued
      flag_wait_gpu(sig_ + 1, 1, fused_timeout_s_, ferr_dev_, 1, H);
      flag_write_gpu(sig_ + 1, 0, H);
      exchange(Tout, H);
      RMA_HIP_CHECK(hipEventRecord(E(ev_frame_), H));
      ++fused_passes_;
    } else {
      const HideBoxes3& sp = split[k];
      // interior of the pass before: the frame reads its cells and overwrites
      // cells it read
      RMA_HIP_CHECK(hipStreamWaitEvent(H, E(ev_inner_), 0));
      launch(k, sp.frame.data(), (int)sp.frame.size(), true, Tin, Tout, H);
      // frame kernel of the pass before, not its exchange
      RMA_HIP_CHECK(hipStreamWaitEvent(L, E(ev_frame_), 0));
      RMA_HIP_CHECK(hipEventRecord(E(ev_frame_), H));
      launch(k, &sp.interior, 1, false, Tin, Tout, L);
      RMA_HIP_CHECK(hipEventRecord(E(ev_inner_), L));
      exchange(Tout, H);
    }
    parity_ ^= 1;
    steps_ += k;
    ++passes_;
  }
  if (overlapped) {
    RMA_HIP_CHECK(hipEventRecord(E(ev_halo_), H));
    RMA_HIP_CHECK(hipStreamWaitEvent(cur, E(ev_halo_), 0));
    RMA_HIP_CHECK(hipStreamWaitEvent(cur, E(ev_inner_), 0));
  }
}

}  // namespace rma
