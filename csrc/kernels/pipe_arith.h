// Arithmetic variants of the stage-pipelined K-step kernel (stencil_pipe.h
// template parameter Ar) and the host-side predicates over them. Host-safe (no
// HIP): the kernel-selection rules (kernel_select.cpp) compile with any host
// compiler, e.g. the sanitizer builds of tests/native.
#pragma once

namespace rma {
namespace pipe {

// kArFast5 (kernel 9, "pipe"): T2 = fma(g, fma(r, U+D, fma(-2(1+r), c, L+R)), c)
// with the factors g in an LDS ring; kArCanon (10): the canonical flux form.
// kArFast5Reg (12, "piper"): fast5 with the factor rows in registers, one
// factor hand-off row per stage. kArFast5RegNoSB (22): piper without the
// sched_barriers between the phases of a level's arithmetic (the scheduler
// free to overlap levels); bitwise equal to piper, the executor's K = 24 kernel.
// Kernel number = 9 + id. Ids 2, 4-12 and 14-20 are retired: docs/TUNING.md,
// "Retired kernel experiments".
constexpr int kArFast5 = 0, kArCanon = 1, kArFast5Reg = 3, kArFast5RegNoSB = 13;
constexpr bool ar_reg(int Ar) { return Ar == kArFast5Reg || Ar == kArFast5RegNoSB; }

// 5 cells per lane: fast5, S = 4, K = 16..20, in the lab library
// (csrc/lab/stencil_pipe5_lab.hip)
inline bool pipe_has_v5(int K, int S, int ar) {
  return ar == kArFast5 && S == 4 && K >= 16 && K <= 20;
}

// 6 cells per lane: the uniform-factor variant of the register-factor kernels,
// S = 4, K = 17..23 (piper) and K = 24 (piper_nosb), in the core units r / r20 / r24
inline bool pipe_has_v6(int K, int S, int ar) {
  return S == 4 && ((ar == kArFast5Reg && K >= 17 && K <= 23) || (ar == kArFast5RegNoSB && K == 24));
}

}  // namespace pipe
}  // namespace rma
