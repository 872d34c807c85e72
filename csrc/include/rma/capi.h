/* C ABI of the native core — ImplicitGlobalGrid-compatible names.
 *
 * For non-Python hosts (a Julia `ccall` shim: julia/ImplicitGlobalGridMI355X.jl,
 * C/C++/Fortran drivers: examples/diffusion_2D_perf_hide.cpp). Mirrors the IGG
 * calls the reference scripts make: init_global_grid,
 * update_halo!, gather!, nx_g/ny_g, x_g/y_g, tic/toc, finalize_global_grid.
 *
 * Bootstrap is the caller's: rank 0 calls rma_unique_id() and the 128 bytes
 * reach every rank by whatever the host uses (MPI.Bcast in Julia, a file, a
 * TCP store); world size 1 needs no id (pass NULL).
 * All functions return 0 on success, non-zero on error; rma_last_error()
 * gives the message (thread-local). Device pointers / streams are opaque.
 */
#ifndef RMA_CAPI_H
#define RMA_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rma_grid rma_grid;

const char* rma_last_error(void);
int rma_unique_id(char out[128]);

/* nxyz: local sizes (halo incl.); dims: 0 = let Dims_create choose; periods;
 * overlaps (default 2) and halowidths (default 1) per dim. out_* may be NULL. */
int rma_init_global_grid(int nx, int ny, int nz, const int dims[3], const int periods[3],
                         const int overlaps[3], const int halowidths[3], int nprocs, int rank,
                         const char* unique_id, int device, rma_grid** out_grid, int* out_me,
                         int out_dims[3], int out_coords[3]);
/* Executors created on a grid pin it: with executors still alive the teardown
 * is deferred to the last rma_executor_destroy (any order is safe). */
int rma_finalize_global_grid(rma_grid* g);

int64_t rma_nx_g(const rma_grid* g);
int64_t rma_ny_g(const rma_grid* g);
int64_t rma_nz_g(const rma_grid* g);
/* global coordinate of 0-based local index ix of an array of extent size_A (IGG x_g(ix+1,...)) */
double rma_x_g(const rma_grid* g, int64_t ix, double dx, int64_t size_A);
double rma_y_g(const rma_grid* g, int64_t iy, double dy, int64_t size_A);
double rma_z_g(const rma_grid* g, int64_t iz, double dz, int64_t size_A);
int rma_neighbors(const rma_grid* g, int out[6]);

/* update_halo!: nfields device arrays, sizes[3*i..] = (nx_A, ny_A, nz_A) with x
 * fastest; elem_bytes per field. Enqueued on `stream` (asynchronous). */
int rma_update_halo(rma_grid* g, int nfields, void* const* fields, const int64_t* sizes,
                    const int* elem_bytes, void* stream);
/* The RANK-MAJOR gather (not IGG's layout): root receives nprocs*bytes, rank
 * r's buffer at byte offset r*bytes. Both buffers must be device memory.
 * Asynchronous on `stream`. For ImplicitGlobalGrid's gather! use
 * rma_gather_igg. */
int rma_gather(rma_grid* g, const void* sendbuf, void* recvbuf, size_t bytes, int root,
               void* stream);
/* ImplicitGlobalGrid gather!: root assembles every rank's A (size_A = nx,ny,nz,
 * x fastest) at its Cartesian coordinates into A_global (dims .* size_A).
 * pitch_A = {row pitch, plane pitch} in elements, NULL = dense. A and A_global
 * may each be host or device memory; A_global may be NULL off-root. Blocking.
 *
 * Collective: every rank calls it with the same size_A, elem_bytes (4 or 8)
 * and root (equal size_A on all ranks is a precondition, as in IGG). Host or
 * device is found per pointer (hipPointerGetAttributes; an unknown pointer is
 * host memory); host data passes through device buffers the grid owns, so
 * RCCL only ever sees device memory. A strided device A (pitch_A: e.g. the
 * interior T[2:end-1,2:end-1] of a field) is packed on the device. On return
 * A_global is complete on root and every rank may reuse A; the wait is bounded
 * by RMA_COMM_TIMEOUT. Refused before any communication, with the argument
 * named in rma_last_error: NULL A_global on root, elem_bytes other than 4 / 8,
 * an extent <= 0, a pitch smaller than the extent, root out of range, and an
 * A_global of more than RMA_GATHER_MAX_BYTES (default 8 GiB). Only tested
 * between ranks sharing one GPU and on one rank; a gather between distinct
 * GPUs over xGMI has not run on any machine yet. */
int rma_gather_igg(rma_grid* g, const void* A, const int64_t size_A[3], const int64_t pitch_A[2],
                   int elem_bytes, void* A_global, int root, void* stream);
/* barrier-synchronised timers (the barrier's wait is bounded by
 * RMA_COMM_TIMEOUT seconds, read once at rma_init_global_grid; default 300) */
int rma_tic(rma_grid* g, void* stream);
int rma_toc(rma_grid* g, void* stream, double* seconds);

/* the fused 5-point diffusion step of the reference (perf.jl) on one tile:
 * T2[interior] = f(T, iCp); coef = {-lam, 1/dx, 1/dy, dt}. */
int rma_diffusion_step(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                       const double coef[4], void* stream);

/* device-side initial conditions of a local tile of the global grid */
int rma_init_gaussian(rma_grid* g, double* T, int64_t nx, int64_t ny, double dx, double dy,
                      double lx, double ly, void* stream);
int rma_init_random(rma_grid* g, double* A, int64_t nx, int64_t ny, double dx, double dy,
                    uint64_t seed, void* stream);
int rma_fill(double* A, int64_t n, double value, void* stream);

/* native time-loop executor: mode 0 = perf (fused), 1 = perf_hide (boundary on a
 * high-priority stream + halo exchange overlapped with the interior), 2 = kp
 * (needs qx, qy, dTdt). Enqueues n steps after the work on `stream`.
 * iCp (1/Cp) is EXAMINED WHEN THE EXECUTOR IS CREATED (after a device
 * synchronisation): where every cell holds bit-for-bit one value, the
 * fast-math K-step passes take that value as a kernel argument and no longer
 * read the array (16 instead of 24 bytes per cell and pass, the same results).
 * After writing to iCp, destroy the executor and create a new one; an
 * executor that found a uniform array does not see later changes. */
typedef struct rma_executor rma_executor;
int rma_executor_create(rma_grid* g, int mode, double* T, double* T2, const double* iCp,
                        int64_t nx, int64_t ny, const double coef[4], int64_t bwx, int64_t bwy,
                        double* qx, double* qy, double* dTdt, rma_executor** out);
// Same with temporal blocking: at most `steps_per_pass` (1..24) time steps per
// kernel pass (rma_executor_run plans passes of 1..steps_per_pass steps) (needs a grid created with overlaps >= 2*steps_per_pass and
// halowidths = steps_per_pass along every dimension with a neighbour).
int rma_executor_create_k(rma_grid* g, int mode, double* T, double* T2, const double* iCp,
                          int64_t nx, int64_t ny, const double coef[4], int64_t bwx, int64_t bwy,
                          int steps_per_pass, double* qx, double* qy, double* dTdt,
                          rma_executor** out);
// Same with `fast_math` != 0: every pass uses the 5-point-sum arithmetic (5 fp64
// operations per cell update instead of 14; rounding-level, not bitwise, equal to
// the canonical update; the bench default). Both arithmetics run any depth 1..24.
int rma_executor_create_kf(rma_grid* g, int mode, double* T, double* T2, const double* iCp,
                           int64_t nx, int64_t ny, const double coef[4], int64_t bwx,
                           int64_t bwy, int steps_per_pass, int fast_math, double* qx,
                           double* qy, double* dTdt, rma_executor** out);
// Same with `graph_steps` > 0: steps are replayed from a hipGraph capturing
// `graph_steps` steps (the host enqueue cost of a step drops to a graph launch);
// needs a capturable halo transport (RCCL: RMA_DIAG=rccl_graph, see README).
int rma_executor_create_g(rma_grid* g, int mode, double* T, double* T2, const double* iCp,
                          int64_t nx, int64_t ny, const double coef[4], int64_t bwx, int64_t bwy,
                          int steps_per_pass, int fast_math, int graph_steps, double* qx,
                          double* qy, double* dTdt, rma_executor** out);
/* Single-rank grid: route the periodic self-neighbours through a 1-rank RCCL
 * communicator (send/recv to itself) instead of local copies -- the GPU-direct
 * P2P path on one GPU (tests, probes). Call before creating executors: it
 * fails while an executor of this grid is alive. */
int rma_grid_self_via_rccl(rma_grid* g);
int rma_executor_run(rma_executor* e, int64_t nsteps, void* stream);
int rma_executor_parity(const rma_executor* e);
/* After the caller synchronised: nonzero (with rma_last_error) if a
 * frame-first fused pass's bounded wait for its frame flag timed out (the
 * halos of that pass are wrong); also reported by the next rma_executor_run.
 * out_fused (may be NULL): passes run as fused launches so far. */
int rma_executor_check(const rma_executor* e, int64_t* out_fused);
int rma_executor_destroy(rma_executor* e);

/* ---- 3D heat diffusion: (nz, ny, nx) fields, x fastest (Julia's A[ix,iy,iz]) ----
 * coef = {-lam, 1/dx, 1/dy, 1/dz, dt} (StencilCoef3, rma/common.h).
 * One fused 7-point step on the whole interior [1,n-1)^3 of one tile. */
int rma_diffusion3d_step(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                         int64_t nz, const double coef[5], void* stream);
/* K steps (1 or 2) in one pass on nboxes (at most 8) half-open boxes of cells,
 * boxes[6*i..] = (x0, x1, y0, y1, z0, z1) inside the interior; cells outside the
 * boxes keep T2's values. fast_math != 0: the fast7 arithmetic (rounding-close
 * to the canonical update, not bitwise equal to it). */
int rma_diffusion3d_boxes(int K, double* T2, const double* T, const double* iCp, int64_t nx,
                          int64_t ny, int64_t nz, const int64_t* boxes, int nboxes,
                          const double coef[5], int fast_math, void* stream);
/* device-side initial conditions of a local 3D tile of the global grid */
int rma_init_gaussian3d(rma_grid* g, double* T, int64_t nx, int64_t ny, int64_t nz, double dx,
                        double dy, double dz, double lx, double ly, double lz, void* stream);
int rma_init_random3d(rma_grid* g, double* A, int64_t nx, int64_t ny, int64_t nz, double dx,
                      double dy, double dz, uint64_t seed, void* stream);

/* Native 3D time loop (rma/executor3d.h): mode 0 = perf (one kernel per pass,
 * then the halo exchange), 1 = perf_hide (boundary frame and exchange on a
 * high-priority stream next to the interior box; b_width = boundary width per
 * dimension, from the array edge). T holds the field and T2 a copy of it.
 * steps_per_pass = 1 or 2: two steps per pass need a grid with overlaps >= 4
 * and halowidths = 2 along every dimension with a neighbour. fast_math != 0:
 * every pass runs the fast7 arithmetic. xface: 0..32, the widest frame box on
 * the kernels' x-face paths, -1 = min(max(b_width[0], overlap_x), 32); it
 * applies to one- and two-step frames (two-step: boxes up to 30 wide).
 * iCp is examined when the executor is created (after a device
 * synchronisation): where every cell holds bit for bit one value the passes
 * take it as a kernel argument and do not read the array (the same field).
 * After writing to iCp call rma_executor3d_rescan_factor. Bad arguments are
 * refused before any launch, named in rma_last_error. The executor pins its
 * grid like the 2D ones: finalize and destroy may come in any order.
 * rma_executor3d_create_f adds fused (the 2D _k / _kf / _g naming):
 * 0 = perf_hide's two launches on two streams, what rma_executor3d_create
 * means; 1 = frame-first single-launch passes (mode 1 only): a pass that splits
 * is one launch, the frame boxes dispatched first, whose last frame wave raises
 * a device flag the exchange stream waits on (bounded by RMA_EXEC_FUSED_TIMEOUT,
 * 60 s). The same field bit for bit. A wait that timed out fails the next
 * rma_executor3d_run and rma_executor3d_check with the reason in rma_last_error,
 * and is printed on stderr when the executor is destroyed. Other values of
 * fused are refused.
 * Not here: hipGraph replay, a pass planner, direct-store halos, more than two
 * steps per pass. */
typedef struct rma_executor3d rma_executor3d;
int rma_executor3d_create(rma_grid* g, int mode, double* T, double* T2, const double* iCp,
                          int64_t nx, int64_t ny, int64_t nz, const double coef[5],
                          const int64_t b_width[3], int steps_per_pass, int fast_math, int xface,
                          rma_executor3d** out);
int rma_executor3d_create_f(rma_grid* g, int mode, double* T, double* T2, const double* iCp,
                            int64_t nx, int64_t ny, int64_t nz, const double coef[5],
                            const int64_t b_width[3], int steps_per_pass, int fast_math,
                            int xface, int fused, rma_executor3d** out);
/* enqueue nsteps after the work on `stream`; `stream` waits for them (asynchronous) */
int rma_executor3d_run(rma_executor3d* e, int64_t nsteps, void* stream);
/* nonzero (the reason in rma_last_error) if a fused pass's wait has timed out */
int rma_executor3d_check(rma_executor3d* e);
/* passes enqueued as one frame-first launch so far */
int64_t rma_executor3d_fused_passes(const rma_executor3d* e);
/* 0: the field is in T, 1: in T2 */
int rma_executor3d_parity(const rma_executor3d* e);
/* nonzero: the last scan found one value in every cell of iCp */
int rma_executor3d_uniform(const rma_executor3d* e);
/* scan iCp again (synchronises the device); out_uniform may be NULL */
int rma_executor3d_rescan_factor(rma_executor3d* e, int* out_uniform);
int rma_executor3d_destroy(rma_executor3d* e);

#ifdef __cplusplus
}
#endif
#endif
