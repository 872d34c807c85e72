// Host (CPU) twins of the GPU kernels. Same expressions, same operation order,
// compiled with -ffp-contract=off, so CPU and GPU results agree bitwise (the
// exp() of init_gaussian excepted: libm vs OCML may differ by one ulp).
// These serve the CPU array path (BASELINE.json configs[0]: "ap 256x256 fp64
// single-rank CPU array path") and multi-rank CPU runs over gloo.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include <vector>

#include "rma/kernels.h"
#include "rma/parallel_for.h"

namespace rma {

namespace {
inline double cell(double xl, double c, double xr, double up, double dn, double ic,
                   const StencilCoef& k) {
  const double qxR = (k.mlam * (xr - c)) * k.rdx;
  const double qxL = (k.mlam * (c - xl)) * k.rdx;
  const double qyU = (k.mlam * (dn - c)) * k.rdy;
  const double qyD = (k.mlam * (c - up)) * k.rdy;
  return c + k.dt * (ic * ((-(qxR - qxL)) * k.rdx - (qyU - qyD) * k.rdy));
}
}  // namespace

void stencil_rects_cpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                       const Rect* rects, int nrects, const StencilCoef& c) {
  RMA_CHECK_ARG(nrects >= 0 && nrects <= kMaxRects, "nrects=" << nrects);
  for (int i = 0; i < nrects; ++i) {
    const Rect r = rects[i];
    if (r.empty()) continue;
    RMA_CHECK_ARG(r.x0 >= 1 && r.x1 <= nx - 1 && r.y0 >= 1 && r.y1 <= ny - 1,
                  "rect outside interior");
    parallel_for(r.y0, r.y1, 64, [&](int64_t y) {
      const double* up = T + (y - 1) * nx;
      const double* cu = T + y * nx;
      const double* dn = T + (y + 1) * nx;
      const double* ic = iCp + y * nx;
      double* out = T2 + y * nx;
      for (int64_t x = r.x0; x < r.x1; ++x)
        out[x] = cell(cu[x - 1], cu[x], cu[x + 1], up[x], dn[x], ic[x], c);
    });
  }
}

void stencil2_rects_cpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                        const Rect* rects, int nrects, const StencilCoef& c) {
  RMA_CHECK_ARG(T2 != T, "two-step update cannot run in place");
  std::vector<double> S1(T, T + nx * ny);  // step 1 on the interior, T elsewhere
  const Rect interior{1, nx - 1, 1, ny - 1};
  stencil_rects_cpu(S1.data(), T, iCp, nx, ny, &interior, 1, c);
  stencil_rects_cpu(T2, S1.data(), iCp, nx, ny, rects, nrects, c);
}

void stencilk_rects_cpu(int K, double* T2, const double* T, const double* iCp, int64_t nx,
                        int64_t ny, const Rect* rects, int nrects, const StencilCoef& c) {
  RMA_CHECK_ARG(K >= 1, "K=" << K);
  RMA_CHECK_ARG(T2 != T, "multi-step update cannot run in place");
  std::vector<double> a(T, T + nx * ny), b(a);
  const Rect interior{1, nx - 1, 1, ny - 1};
  for (int j = 1; j < K; ++j) {  // levels 1..K-1 on the interior, T elsewhere
    stencil_rects_cpu(b.data(), a.data(), iCp, nx, ny, &interior, 1, c);
    a.swap(b);
  }
  stencil_rects_cpu(T2, a.data(), iCp, nx, ny, rects, nrects, c);
}

void validate_boxes(const double* T2, const double* T, int64_t nx, int64_t ny, int64_t nz,
                    const Box* boxes, int nboxes) {
  RMA_CHECK_ARG(nboxes >= 0 && nboxes <= kMaxBoxes,
                "nboxes=" << nboxes << " (at most " << kMaxBoxes << " boxes per launch)");
  RMA_CHECK_ARG(nx >= 3 && ny >= 3 && nz >= 3,
                "grid too small: nx=" << nx << " ny=" << ny << " nz=" << nz);
  RMA_CHECK_ARG(T2 != T, "the 3D update cannot run in place (T2 aliases T)");
  for (int i = 0; i < nboxes; ++i) {
    const Box& b = boxes[i];
    if (b.empty()) continue;
    RMA_CHECK_ARG(b.x0 >= 1 && b.x1 <= nx - 1 && b.y0 >= 1 && b.y1 <= ny - 1 && b.z0 >= 1 &&
                      b.z1 <= nz - 1,
                  "box " << i << " [" << b.x0 << "," << b.x1 << ")x[" << b.y0 << "," << b.y1
                         << ")x[" << b.z0 << "," << b.z1 << ") outside the interior of " << nx
                         << "x" << ny << "x" << nz);
  }
}

// CPU twin of stencil3d_boxes_gpu (stencil3d.hip): StencilCoef3's expression
void stencil3d_boxes_cpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                         int64_t nz, const Box* boxes, int nboxes, const StencilCoef3& k) {
  validate_boxes(T2, T, nx, ny, nz, boxes, nboxes);
  const int64_t plane = nx * ny;
  for (int i = 0; i < nboxes; ++i) {
    const Box b = boxes[i];
    if (b.empty()) continue;
    const int64_t rows = b.y1 - b.y0;
    parallel_for(0, rows * (b.z1 - b.z0), 64, [&](int64_t j) {
      const int64_t o = (b.z0 + j / rows) * plane + (b.y0 + j % rows) * nx;
      const double* cu = T + o;
      for (int64_t x = b.x0; x < b.x1; ++x) {
        const double c = cu[x];
        const double qxR = (k.mlam * (cu[x + 1] - c)) * k.rdx;
        const double qxL = (k.mlam * (c - cu[x - 1])) * k.rdx;
        const double qyU = (k.mlam * (cu[x + nx] - c)) * k.rdy;
        const double qyD = (k.mlam * (c - cu[x - nx])) * k.rdy;
        const double qzF = (k.mlam * (cu[x + plane] - c)) * k.rdz;
        const double qzB = (k.mlam * (c - cu[x - plane])) * k.rdz;
        T2[o + x] = c + k.dt * (iCp[o + x] * (((-(qxR - qxL)) * k.rdx - (qyU - qyD) * k.rdy) -
                                              (qzF - qzB) * k.rdz));
      }
    });
  }
}

// CPU twin of stencil3dk_boxes_gpu (stencil3d_tb.hip): no kernel code shared
void stencil3dk_boxes_cpu(int K, double* T2, const double* T, const double* iCp, int64_t nx,
                          int64_t ny, int64_t nz, const Box* boxes, int nboxes,
                          const StencilCoef3& c) {
  RMA_CHECK_ARG(K >= 1, "K=" << K);
  validate_boxes(T2, T, nx, ny, nz, boxes, nboxes);
  if (K == 1) {
    stencil3d_boxes_cpu(T2, T, iCp, nx, ny, nz, boxes, nboxes, c);
    return;
  }
  std::vector<double> a(T, T + nx * ny * nz), b(a);
  const Box interior{1, nx - 1, 1, ny - 1, 1, nz - 1};
  for (int j = 1; j < K; ++j) {  // levels 1..K-1 on the interior, T on the faces
    stencil3d_boxes_cpu(b.data(), a.data(), iCp, nx, ny, nz, &interior, 1, c);
    a.swap(b);
  }
  stencil3d_boxes_cpu(T2, a.data(), iCp, nx, ny, nz, boxes, nboxes, c);
}

bool fast7_ok(const StencilCoef3& c) {
  const double ax = (-c.mlam) * c.rdx * c.rdx, ay = (-c.mlam) * c.rdy * c.rdy,
               az = (-c.mlam) * c.rdz * c.rdz;
  return ax != 0.0 && std::isfinite(ax) && std::isfinite(ay) && std::isfinite(az) &&
         std::isfinite(ay / ax) && std::isfinite(az / ax) && std::isfinite(c.dt * ax);
}

Fast7 fast7_constants(const StencilCoef3& c) {
  const double ax = (-c.mlam) * c.rdx * c.rdx;
  const double ay = (-c.mlam) * c.rdy * c.rdy;
  const double az = (-c.mlam) * c.rdz * c.rdz;
  Fast7 f;
  f.ry = ay / ax;
  f.rz = az / ax;
  f.mkc = -2.0 * ((1.0 + f.ry) + f.rz);
  f.gs = c.dt * ax;
  return f;
}

// fast7 arithmetic (rma/kernels.h): the 7-point sum with one folded per-cell
// factor. std::fma rounds once like v_fma_f64, so this twin is bitwise equal to
// the fast7 instantiations of stencil3d.hip / stencil3d_tb.hip
// (tests/test_stencil3d_fast_cpu.py pins it to an exact-rational model).
void stencil3d7_boxes_cpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                          int64_t nz, const Box* boxes, int nboxes, const StencilCoef3& k) {
  validate_boxes(T2, T, nx, ny, nz, boxes, nboxes);
  RMA_CHECK_ARG(fast7_ok(k), "fast7 needs lam != 0 and finite coefficients");
  const Fast7 f = fast7_constants(k);
  const int64_t plane = nx * ny;
  for (int i = 0; i < nboxes; ++i) {
    const Box b = boxes[i];
    if (b.empty()) continue;
    const int64_t rows = b.y1 - b.y0;
    parallel_for(0, rows * (b.z1 - b.z0), 64, [&](int64_t j) {
      const int64_t o = (b.z0 + j / rows) * plane + (b.y0 + j % rows) * nx;
      const double* cu = T + o;
      for (int64_t x = b.x0; x < b.x1; ++x) {
        const double c = cu[x];
        const double g = f.gs * iCp[o + x];
        const double sx = cu[x + 1] + cu[x - 1];
        const double sy = cu[x - nx] + cu[x + nx];
        const double sz = cu[x - plane] + cu[x + plane];
        double t = std::fma(f.mkc, c, sx);
        t = std::fma(f.ry, sy, t);
        t = std::fma(f.rz, sz, t);
        T2[o + x] = std::fma(g, t, c);
      }
    });
  }
}

void stencil3dk7_boxes_cpu(int K, double* T2, const double* T, const double* iCp, int64_t nx,
                           int64_t ny, int64_t nz, const Box* boxes, int nboxes,
                           const StencilCoef3& c) {
  RMA_CHECK_ARG(K >= 1, "K=" << K);
  validate_boxes(T2, T, nx, ny, nz, boxes, nboxes);
  RMA_CHECK_ARG(fast7_ok(c), "fast7 needs lam != 0 and finite coefficients");
  if (K == 1) {
    stencil3d7_boxes_cpu(T2, T, iCp, nx, ny, nz, boxes, nboxes, c);
    return;
  }
  std::vector<double> a(T, T + nx * ny * nz), b(a);
  const Box interior{1, nx - 1, 1, ny - 1, 1, nz - 1};
  for (int j = 1; j < K; ++j) {  // levels 1..K-1 on the interior, T on the faces
    stencil3d7_boxes_cpu(b.data(), a.data(), iCp, nx, ny, nz, &interior, 1, c);
    a.swap(b);
  }
  stencil3d7_boxes_cpu(T2, a.data(), iCp, nx, ny, nz, boxes, nboxes, c);
}

bool fast5_ok(const StencilCoef& c) {
  const double ax = (-c.mlam) * c.rdx * c.rdx, ay = (-c.mlam) * c.rdy * c.rdy;
  return ax != 0.0 && std::isfinite(ax) && std::isfinite(ay) && std::isfinite(ay / ax) &&
         std::isfinite(c.dt * ax);
}

// fast5 arithmetic (csrc/lab/stencil_kstep_lab.hip kernel 5, stencil_pipe.h): the 5-point sum
// with the constants folded into one per-cell factor g = dt*lam/dx^2 * 1/Cp,
//   T2 = fma(g, fma(r, U+D, fma(-2(1+r), c, R+L)), c),  r = (lam/dy^2)/(lam/dx^2).
// std::fma rounds once like v_fma_f64, so this twin is bitwise equal to the
// GPU kernels (tests/test_fast5_cpu.py, tests/test_pipe_gpu.py).
void stencil5_rects_cpu(double* T2, const double* T, const double* iCp, int64_t nx, int64_t ny,
                        const Rect* rects, int nrects, const StencilCoef& c) {
  RMA_CHECK_ARG(nrects >= 0 && nrects <= kMaxRects, "nrects=" << nrects);
  RMA_CHECK_ARG(fast5_ok(c), "fast5 needs lam != 0 and finite coefficients");
  const double ax = (-c.mlam) * c.rdx * c.rdx;
  const double ay = (-c.mlam) * c.rdy * c.rdy;
  const double ry = ay / ax;
  const double mkc = -2.0 * (1.0 + ry);
  const double gs = c.dt * ax;
  for (int i = 0; i < nrects; ++i) {
    const Rect r = rects[i];
    if (r.empty()) continue;
    RMA_CHECK_ARG(r.x0 >= 1 && r.x1 <= nx - 1 && r.y0 >= 1 && r.y1 <= ny - 1,
                  "rect outside interior");
    parallel_for(r.y0, r.y1, 64, [&](int64_t y) {
      const double* up = T + (y - 1) * nx;
      const double* cu = T + y * nx;
      const double* dn = T + (y + 1) * nx;
      const double* ic = iCp + y * nx;
      double* out = T2 + y * nx;
      for (int64_t x = r.x0; x < r.x1; ++x) {
        const double g = gs * ic[x];
        const double sx = cu[x + 1] + cu[x - 1];
        const double sy = up[x] + dn[x];
        double t = std::fma(mkc, cu[x], sx);
        t = std::fma(ry, sy, t);
        out[x] = std::fma(g, t, cu[x]);
      }
    });
  }
}

void stencilk5_rects_cpu(int K, double* T2, const double* T, const double* iCp, int64_t nx,
                         int64_t ny, const Rect* rects, int nrects, const StencilCoef& c) {
  RMA_CHECK_ARG(K >= 1, "K=" << K);
  RMA_CHECK_ARG(T2 != T, "multi-step update cannot run in place");
  std::vector<double> a(T, T + nx * ny), b(a);
  const Rect interior{1, nx - 1, 1, ny - 1};
  for (int j = 1; j < K; ++j) {
    stencil5_rects_cpu(b.data(), a.data(), iCp, nx, ny, &interior, 1, c);
    a.swap(b);
  }
  stencil5_rects_cpu(T2, a.data(), iCp, nx, ny, rects, nrects, c);
}

void flux_cpu(double* QX, double* QY, const double* T, int64_t nx, int64_t ny, double mlam,
              double rdx, double rdy) {
  parallel_for(0, ny - 1, 64, [&](int64_t y) {
    const double* r0 = T + y * nx;
    const double* r1 = r0 + nx;
    for (int64_t x = 1; x < nx - 1; ++x) QY[y * nx + x] = (mlam * (r1[x] - r0[x])) * rdy;
    if (y >= 1)
      for (int64_t x = 0; x < nx - 1; ++x) QX[y * nx + x] = (mlam * (r0[x + 1] - r0[x])) * rdx;
  });
}

void residual_cpu(double* D, const double* QX, const double* QY, const double* iCp, int64_t nx,
                  int64_t ny, double rdx, double rdy) {
  parallel_for(1, ny - 1, 64, [&](int64_t y) {
    for (int64_t x = 1; x < nx - 1; ++x) {
      const int64_t o = y * nx + x;
      const double ddx = (QX[o] - QX[o - 1]) * rdx;
      const double ddy = (QY[o] - QY[o - nx]) * rdy;
      D[o] = iCp[o] * (-(ddx + ddy));
    }
  });
}

void update_cpu(double* T, const double* D, int64_t nx, int64_t ny, double dt) {
  parallel_for(1, ny - 1, 64, [&](int64_t y) {
    for (int64_t x = 1; x < nx - 1; ++x) {
      double* p = T + y * nx + x;
      *p = *p + dt * D[y * nx + x];
    }
  });
}

void copy2d_cpu(void* dst, int64_t dst_ld, const void* src, int64_t src_ld, int64_t n_o,
                int64_t n_k, int elem_bytes) {
  RMA_CHECK_ARG(elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8 || elem_bytes == 16,
                "unsupported element size " << elem_bytes);
  char* d = static_cast<char*>(dst);
  const char* s = static_cast<const char*>(src);
  for (int64_t o = 0; o < n_o; ++o)
    std::memcpy(d + o * dst_ld * elem_bytes, s + o * src_ld * elem_bytes, n_k * elem_bytes);
}

void copy2d_batch_cpu(const Copy2d* copies, int n, int elem_bytes) {
  RMA_CHECK_ARG(n >= 0 && n <= kCopy2dBatch, "copy2d batch of " << n);
  for (int i = 0; i < n; ++i) {
    const Copy2d& c = copies[i];
    if (c.n_o <= 0 || c.n_k <= 0) continue;
    RMA_CHECK_ARG(c.dst_ld >= c.n_k && c.src_ld >= c.n_k, "leading dims smaller than row length");
    copy2d_cpu(c.dst, c.dst_ld, c.src, c.src_ld, c.n_o, c.n_k, elem_bytes);
  }
}

void validate_block_copies(const BlockCopy* blocks, int64_t n, int elem_bytes) {
  RMA_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8,
                "copy_blocks: unsupported elem_bytes " << elem_bytes << " (4 or 8)");
  RMA_CHECK_ARG(n >= 0 && (n == 0 || blocks != nullptr), "copy_blocks: " << n << " blocks");
  for (int64_t i = 0; i < n; ++i) {
    const BlockCopy& c = blocks[i];
    RMA_CHECK_ARG(c.dst && c.src, "copy_blocks: null pointer in block " << i);
    RMA_CHECK_ARG(c.nx > 0 && c.ny > 0 && c.nz > 0,
                  "copy_blocks: block " << i << " has extents " << c.nx << " x " << c.ny << " x "
                                        << c.nz);
    RMA_CHECK_ARG(c.ny == 1 || (c.dst_row >= c.nx && c.src_row >= c.nx),
                  "copy_blocks: row pitch of block " << i << " smaller than nx=" << c.nx);
    // a plane ends at its last row's last element
    const int64_t dspan = (c.ny - 1) * (c.ny > 1 ? c.dst_row : 0) + c.nx;
    const int64_t sspan = (c.ny - 1) * (c.ny > 1 ? c.src_row : 0) + c.nx;
    RMA_CHECK_ARG(c.nz == 1 || (c.dst_plane >= dspan && c.src_plane >= sspan),
                  "copy_blocks: plane pitch of block " << i << " smaller than a plane");
  }
}

// CPU twin of copy_blocks_gpu (blocks.hip)
void copy_blocks_cpu(const BlockCopy* blocks, int64_t n, int elem_bytes) {
  validate_block_copies(blocks, n, elem_bytes);
  for (int64_t i = 0; i < n; ++i) {
    const BlockCopy& c = blocks[i];
    char* d = static_cast<char*>(c.dst);
    const char* s = static_cast<const char*>(c.src);
    for (int64_t z = 0; z < c.nz; ++z)
      for (int64_t y = 0; y < c.ny; ++y)
        std::memcpy(d + (z * c.dst_plane + y * c.dst_row) * elem_bytes,
                    s + (z * c.src_plane + y * c.src_row) * elem_bytes, (size_t)c.nx * elem_bytes);
  }
}

double reduce_cpu(const double* A, int64_t n, int op) {
  double v = (op == kMax) ? -std::numeric_limits<double>::infinity()
                          : (op == kMin ? std::numeric_limits<double>::infinity() : 0.0);
  for (int64_t i = 0; i < n; ++i) {
    const double a = A[i];
    switch (op) {
      case kSum: v += a; break;
      case kMax: v = std::fmax(v, a); break;
      case kMin: v = std::fmin(v, a); break;
      case kMaxAbs: v = std::fmax(v, std::fabs(a)); break;
      case kNonFinite: v += std::isfinite(a) ? 0.0 : 1.0; break;
      default: RMA_CHECK_ARG(false, "bad reduce op " << op);
    }
  }
  return v;
}

// CPU twin of count_differing_gpu (misc.hip): bit patterns, not values
int64_t count_differing_cpu(const double* A, int64_t n) {
  int64_t cnt = 0;
  uint64_t first = 0, v = 0;
  if (n > 0) std::memcpy(&first, A, sizeof first);
  for (int64_t i = 0; i < n; ++i) {
    std::memcpy(&v, A + i, sizeof v);
    cnt += v != first ? 1 : 0;
  }
  return cnt;
}

// Host builds of the runtime without device code (the sanitizer programs of
// tests/native, where "device" memory is host memory) resolve the launch to
// this twin; in the core library the definition of misc.hip takes its place.
__attribute__((weak)) void count_differing_gpu(const double* A, int64_t n, uint64_t* out2,
                                               stream_t) {
  out2[0] += (uint64_t)count_differing_cpu(A, n);
  std::memcpy(&out2[1], A, sizeof(uint64_t));
}

// CPU twin of field_stats_gpu (misc.hip)
void field_stats_cpu(const double* A, int64_t n, double* out3) {
  double bad = 0.0, lo = INFINITY, hi = -INFINITY;
  for (int64_t i = 0; i < n; ++i) {
    const double v = A[i];
    if (!std::isfinite(v)) {
      bad += 1.0;
      continue;
    }
    lo = std::fmin(lo, v);
    hi = std::fmax(hi, v);
  }
  out3[0] = bad;
  out3[1] = lo;
  out3[2] = hi;
}

}  // namespace rma
