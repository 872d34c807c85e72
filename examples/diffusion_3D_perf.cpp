// Standalone native driver of 3D heat diffusion (no Python, no torch):
// ImplicitGlobalGrid's flagship example on one rank, written against the C ABI
// of librma_core.so (rma/capi.h) only: grid, device-side Gaussian, the native
// time loop, barrier timers.
//
//   ./build/examples/diffusion_3D_perf [nx] [nt] [periodic] [steps_per_pass] [fast_math] [hide]
//                                      [fused]
//   (nx: cube edge, halo included; periodic 1: the rank is its own neighbour on
//    all six sides; steps_per_pass 1 or 2; fast_math 1: the fast7 arithmetic;
//    hide 1: perf_hide with b_width (16, 2, 2), 0: perf; fused 1 (with hide 1):
//    frame-first single-launch passes)
//
// Prints the reference line with T_eff = 3*nx*ny*nz*8 B / t_it. The first
// min(10, nt - 1) steps are untimed, as in the reference scripts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "rma/capi.h"

#define CK(x)                                                        \
  do {                                                               \
    if ((x) != 0) {                                                  \
      std::fprintf(stderr, "%s failed: %s\n", #x, rma_last_error()); \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)
#define HK(x)                                                             \
  do {                                                                    \
    hipError_t e_ = (x);                                                  \
    if (e_ != hipSuccess) {                                               \
      std::fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_)); \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? std::atoll(argv[1]) : 256;
  const int nt = argc > 2 ? std::atoi(argv[2]) : 100;
  const int periodic = argc > 3 ? std::atoi(argv[3]) : 0;
  const int K = argc > 4 ? std::atoi(argv[4]) : 1;
  const int fast = argc > 5 ? std::atoi(argv[5]) : 0;
  const int hide = argc > 6 ? std::atoi(argv[6]) : 0;
  const int fused = argc > 7 ? std::atoi(argv[7]) : 0;
  if (n < 3 || nt < 1 || (K != 1 && K != 2)) {
    std::fprintf(stderr, "usage: %s [nx >= 3] [nt >= 1] [periodic 0|1] [steps_per_pass 1|2] "
                         "[fast_math 0|1] [hide 0|1] [fused 0|1]\n", argv[0]);
    return 2;
  }
  HK(hipSetDevice(0));
  rma_grid* g = nullptr;
  int me = 0, dims[3], coords[3];
  const int dims_in[3] = {1, 1, 1};
  const int per[3] = {periodic, periodic, periodic};
  const int ol[3] = {2 * K, 2 * K, 2 * K};  // K steps per pass: overlap 2K, halo width K
  const int hw[3] = {K, K, K};
  CK(rma_init_global_grid((int)n, (int)n, (int)n, dims_in, per, ol, hw, 1, 0, nullptr, 0, &g, &me,
                          dims, coords));
  const double lx = 10, ly = 10, lz = 10, lam = 1, Cp0 = 1;
  const double dx = lx / rma_nx_g(g), dy = ly / rma_ny_g(g), dz = lz / rma_nz_g(g);
  const double dt = std::min(dx * dx, std::min(dy * dy, dz * dz)) * Cp0 / lam / 6.1;
  const double coef[5] = {-lam, 1 / dx, 1 / dy, 1 / dz, dt};
  double *T, *T2, *iCp;
  const int64_t cells = n * n * n;
  const size_t bytes = (size_t)cells * sizeof(double);
  HK(hipMalloc(&T, bytes));
  HK(hipMalloc(&T2, bytes));
  HK(hipMalloc(&iCp, bytes));
  hipStream_t s;
  HK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  CK(rma_fill(iCp, cells, 1.0 / Cp0, s));
  CK(rma_init_gaussian3d(g, T, n, n, n, dx, dy, dz, lx, ly, lz, s));
  HK(hipMemcpyAsync(T2, T, bytes, hipMemcpyDeviceToDevice, s));
  HK(hipStreamSynchronize(s));
  rma_executor3d* ex = nullptr;
  const int64_t b_width[3] = {16, 2, 2};
  CK(rma_executor3d_create_f(g, hide ? 1 : 0, T, T2, iCp, n, n, n, coef, b_width, K, fast, 0,
                             fused, &ex));
  std::printf("Global grid: %ldx%ldx%ld (nprocs: 1, dims: %dx%dx%d)\n", (long)rma_nx_g(g),
              (long)rma_ny_g(g), (long)rma_nz_g(g), dims[0], dims[1], dims[2]);
  std::printf("[loop] native %s%s, %d step(s) per pass, %s, 1/Cp %s\n",
              hide ? "perf_hide" : "perf", fused ? " fused" : "", K, fast ? "fast7" : "canonical",
              rma_executor3d_uniform(ex) ? "uniform (kernel argument)" : "read per cell");
  const int warm = nt > 1 ? std::min(10, nt - 1) : 0;
  if (warm) CK(rma_executor3d_run(ex, warm, s));
  CK(rma_tic(g, s));
  CK(rma_executor3d_run(ex, nt - warm, s));
  double wtime = 0;
  CK(rma_toc(g, s, &wtime));
  const double A_eff = 3.0 / 1e9 * (double)cells * sizeof(double);
  const double T_eff = A_eff / (wtime / (nt - warm));
  std::printf("Executed %d steps in = %1.3e sec (@ T_eff = %1.2f GB/s) \n", nt, wtime, T_eff);
  // the centre cell of the current field: a finite value says the run was real
  const double* cur = rma_executor3d_parity(ex) ? T2 : T;
  double c = 0;
  HK(hipMemcpy(&c, cur + ((n / 2) * n + n / 2) * n + n / 2, sizeof c, hipMemcpyDeviceToHost));
  std::printf("T[centre] = %.17g\n", c);
  CK(rma_executor3d_check(ex));  // a fused pass's wait that timed out
  if (fused)
    std::printf("[hide] %lld fused passes\n", (long long)rma_executor3d_fused_passes(ex));
  CK(rma_executor3d_destroy(ex));
  HK(hipFree(T));
  HK(hipFree(T2));
  HK(hipFree(iCp));
  HK(hipStreamDestroy(s));
  CK(rma_finalize_global_grid(g));
  return 0;
}
