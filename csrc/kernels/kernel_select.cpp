// Host-side kernel-selection rules of the stencil launchers: which
// pipelined (K, stages, arithmetic, cols) instantiations exist, the cells per
// lane a launch runs, the one-step march kernel's strip width, the path of every
// box of a 3D launch (plan_dispatch3d) and the box lists both 3D launchers
// build from it (split_boxes3d). Plain host code
// (moved out of stencil_pipe.hip / stencil.hip) so the executor's planning
// compiles and runs without HIP, e.g. in tests/native/executor_selftest.cpp
// under ThreadSanitizer / AddressSanitizer.
#include <cstdint>

#include "pipe_arith.h"
#include "rma/kernels.h"

namespace rma {

int pipe_default_stages(int K) {
  // Waves per strip: 1, 2 or 4 only. A block of 3, 5 or 6 waves puts two of
  // its stages on one SIMD (waves are dealt round-robin over the 4 SIMDs of a
  // CU) and the per-row barrier then runs the whole block at that SIMD's pace:
  // K=17..20 with 5 stages took 103-118 ms per pass at 101376^2 against 76 ms
  // for K=20 on 4 stages of 5 levels (profiles/pass_sweep_r2.json). Deeper
  // stages amortise the per-row barrier and hand-off: K=24 on 4 stages of 6
  // levels (2 waves per SIMD) has the lowest time per step of all depths.
  if (K <= 4) return 1;
  if (K <= 9) return 2;  // K=9 on 4 stages would leave the last one empty
  return 4;
}

bool pipe_has(int K, int S, int arith) {
  if (K < 1 || K > kPipeMaxK) return false;
  if (arith == pipe::kArFast5Reg) return S == 4 && K >= 10 && K <= 24;
  if (arith == pipe::kArFast5RegNoSB) return S == 4 && (K == 20 || K == 24);
  if (arith != pipe::kArFast5 && arith != pipe::kArCanon) return false;  // retired ids
  if (S == pipe_default_stages(K)) return true;
  // alternative stage splits instantiated for sweeps (csrc/lab/stencil_pipe_lab.hip)
  return (K == 12 && S == 3) || (K == 16 && S == 8) || (K == 24 && S == 8) ||
         (K == 8 && S == 4) || (K == 8 && S == 1);
}

bool pipe_has_cols(int K, int S, int arith, int cols) {
  if (cols <= 1) return pipe_has(K, S, arith);
  if (cols != 2 || S != 4) return false;
  return (arith == pipe::kArFast5 || arith == pipe::kArFast5Reg) && (K == 16 || K == 20 || K == 24);
}

int pipe_default_cols(int K, int S, int arith) {
  // one column wave: the 2-column blocks (csrc/lab/stencil_pipe_lab.hip) do 6-8 % less
  // arithmetic but run one 8-wave block per CU and lose more to the unhidden
  // per-row barrier: ring kernel 5-20 % (profiles/pass_sweep_cols2_r2.json), piper
  // +5.3 % at K=20 and +11.9 % at K=24 even with the retired rotated map, +34-38 % wait cycles
  // (profiles/r6/cols2_piper.md)
  (void)K;
  (void)S;
  (void)arith;
  return 1;
}

int pipe_vec(int K, int stages, int arith, int64_t nx, int requested, bool aligned16) {
  const int S = stages > 0 ? stages : pipe_default_stages(K);
  if (requested == 5 && nx % 5 == 0 && pipe::pipe_has_v5(K, S, arith)) return 5;
  if (aligned16 && nx % 2 == 0) return (requested >= 4 && nx % 4 == 0) ? 4 : 2;
  return 1;
}

int pipe_vec_uniform(int K, int stages, int arith, int64_t nx, int requested, bool aligned16,
                     bool uniform) {
  const int S = stages > 0 ? stages : pipe_default_stages(K);
  // the load position is clamped per 16-byte pair, so any even nx will do
  if (requested == 6 && uniform && aligned16 && nx % 2 == 0 && pipe::pipe_has_v6(K, S, arith))
    return 6;
  return pipe_vec(K, stages, arith, nx, requested == 6 ? 4 : requested, aligned16);
}

int stencil_vec(int64_t nx, const StencilTuning& tune) {
  // cells per lane: 16-byte rows need an even nx; V=4 also needs nx % 4 == 0
  // (a clamped lane past the row end must still load its own cells)
  if (nx % 2) return 1;
  if (tune.vec == 4 && nx % 4 == 0) return 4;
  return 2;
}

int stencil_strip_cells(int64_t nx, const StencilTuning& tune) {
  constexpr int kWave = 64;
  return kWave * stencil_vec(nx, tune);
}

void plan_dispatch3d(int K, const Box* boxes, int nboxes, const Stencil3DTuning& tune,
                     Dispatch3D* out) {
  constexpr int64_t kThinMaxWidth = 8;  // one-step boxes at most this wide: one thread per row
  RMA_CHECK_ARG(K == 1 || K == 2, "K=" << K << " steps per pass is not instantiated (1 or 2)");
  RMA_CHECK_ARG(tune.xface >= 0 && tune.xface <= kXfaceMax,
                "xface=" << tune.xface << " (0: off, or the widest face box, up to "
                         << kXfaceMax << ")");
  RMA_CHECK_ARG(nboxes >= 0 && nboxes <= kMaxBoxes,
                "nboxes=" << nboxes << " (at most " << kMaxBoxes << " boxes per launch)");
  for (int i = 0; i < nboxes; ++i) {
    const Box& b = boxes[i];
    out[i] = Dispatch3D{};
    if (b.empty()) continue;
    const int64_t w = b.x1 - b.x0;
    // columns a face segment needs: the box and, per side, the K-1 columns on
    // which the lower levels are recomputed (none for the one-step kernel)
    const int64_t need = w + 2 * (K - 1);
    if (w <= tune.xface && need <= 32) {
      out[i].path = kPathXface;
      out[i].lanes = need <= 8 ? 8 : need <= 16 ? 16 : 32;
    } else if (K == 1 && w <= kThinMaxWidth) {
      out[i].path = kPathThin;
      out[i].lanes = 1;
    } else {
      out[i].path = kPathMarch;
      out[i].lanes = 64;
    }
  }
}

Split3D split_boxes3d(int K, const Box* boxes, int nboxes, const Stencil3DTuning& tune) {
  Dispatch3D path[kMaxBoxes];
  plan_dispatch3d(K, boxes, nboxes, tune, path);
  Split3D s;
  for (int i = 0; i < nboxes; ++i) {
    if (path[i].path == kPathXface) {
      const int cls = path[i].lanes == 8 ? 0 : path[i].lanes == 16 ? 1 : 2;
      s.face[cls][s.nface[cls]++] = boxes[i];
    } else if (path[i].path != kPathNone) {
      s.thin[s.nwide] = path[i].path == kPathThin;
      s.wide[s.nwide++] = boxes[i];
    }
  }
  return s;
}

const char* path3d_name(int path) {
  switch (path) {
    case kPathMarch: return "march";
    case kPathThin: return "thin";
    case kPathXface: return "xface";
    default: return "none";
  }
}

}  // namespace rma
