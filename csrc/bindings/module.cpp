// pybind11 bindings of the native core: rocm_mpi_amd._C
//
// Pure C++ (no HIP headers): pointers travel as integers (torch
// Tensor.data_ptr()), streams as integers (torch.cuda.Stream.cuda_stream).
// Shape/dtype/device validation happens in rocm_mpi_amd/ops before any call.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <string>
#include <tuple>
#include <vector>

#include "rma/config.h"
#include "rma/comm.h"
#include "rma/common.h"
#include "rma/executor.h"
#include "rma/executor3d.h"
#include "rma/gather.h"
#include "rma/halo.h"
#include "rma/ipc.h"
#include "rma/kernels.h"
#include "rma/loopback.h"
#include "rma/p2p.h"
#include "rma/plan.h"
#include "rma/topology.h"
#include "rma/trace.h"

namespace py = pybind11;
using namespace rma;

namespace {

template <typename T>
T* P(uintptr_t p) {
  return reinterpret_cast<T*>(p);
}
stream_t S(uintptr_t s) { return reinterpret_cast<stream_t>(s); }

using Rect4 = std::tuple<int64_t, int64_t, int64_t, int64_t>;
using Coef4 = std::tuple<double, double, double, double>;  // mlam, rdx, rdy, dt
using Geom = std::tuple<int64_t, int64_t, int64_t, int64_t, double, double, double, double, int,
                        int>;  // gx0 gy0 nxg nyg dx dy xoff yoff periodx periody

std::vector<Rect> to_rects(const std::vector<Rect4>& v) {
  std::vector<Rect> r;
  for (auto& t : v) r.push_back({std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t)});
  return r;
}
StencilCoef to_coef(const Coef4& c) {
  return {std::get<0>(c), std::get<1>(c), std::get<2>(c), std::get<3>(c)};
}
TileGeom to_geom(const Geom& g) {
  TileGeom t;
  std::tie(t.gx0, t.gy0, t.nxg, t.nyg, t.dx, t.dy, t.xoff, t.yoff, t.periodx, t.periody) = g;
  return t;
}
Rect4 from_rect(const Rect& r) { return {r.x0, r.x1, r.y0, r.y1}; }

using Box6 = std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>;
using Coef5 = std::tuple<double, double, double, double, double>;  // mlam, rdx, rdy, rdz, dt
using Geom3 = std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, double, double,
                         double, double, double, double, int, int,
                         int>;  // g{x,y,z}0 n{x,y,z}g d{x,y,z} {x,y,z}off period{x,y,z}
std::vector<Box> to_boxes(const std::vector<Box6>& v) {
  std::vector<Box> b;
  for (auto& t : v)
    b.push_back({std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t), std::get<4>(t),
                 std::get<5>(t)});
  return b;
}
Box6 from_box(const Box& b) { return {b.x0, b.x1, b.y0, b.y1, b.z0, b.z1}; }
StencilCoef3 to_coef3(const Coef5& c) {
  return {std::get<0>(c), std::get<1>(c), std::get<2>(c), std::get<3>(c), std::get<4>(c)};
}
TileGeom3 to_geom3(const Geom3& g) {
  TileGeom3 t;
  std::tie(t.gx0, t.gy0, t.gz0, t.nxg, t.nyg, t.nzg, t.dx, t.dy, t.dz, t.xoff, t.yoff, t.zoff,
           t.periodx, t.periody, t.periodz) = g;
  return t;
}

using FieldT = std::tuple<uintptr_t, std::array<int64_t, 3>, int, std::array<int64_t, 3>,
                          std::array<int64_t, 3>>;
std::vector<HaloField> to_fields(const std::vector<FieldT>& v) {
  std::vector<HaloField> out;
  for (auto& t : v) {
    HaloField f;
    f.ptr = reinterpret_cast<void*>(std::get<0>(t));
    f.size = std::get<1>(t);
    f.elem_bytes = std::get<2>(t);
    f.ol = std::get<3>(t);
    f.hw = std::get<4>(t);
    out.push_back(f);
  }
  return out;
}

}  // namespace

PYBIND11_MODULE(_C, m) {
  m.doc() = "rocm_mpi_amd native core (HIP kernels for gfx950, RCCL halo exchange, executor)";
  static py::exception<Error> exc(m, "NativeError", PyExc_RuntimeError);
  py::register_exception_translator([](std::exception_ptr p) {
    try {
      if (p) std::rethrow_exception(p);
    } catch (const Error& e) {
      exc(e.what());
    }
  });

  m.def("set_rank_for_errors", &set_rank_for_errors);
  m.def("rccl_version", &rccl_version);
  m.def("rccl_library", &rccl_library);
  m.def("device_pci_bus_id", &device_pci_bus_id, py::arg("device"));
  m.def(
      "stencil_strip_cells",
      [](int64_t nx, int vec) {
        StencilTuning t;
        t.vec = vec;
        return stencil_strip_cells(nx, t);
      },
      py::arg("nx"), py::arg("vec") = 2);

  // ---------------- kernels ----------------
  m.def(
      "stencil_rects",
      [](uintptr_t T2, uintptr_t T, uintptr_t iCp, int64_t nx, int64_t ny,
         const std::vector<Rect4>& rects, const Coef4& coef, int chunk_rows, int nontemporal,
         int kernel, uintptr_t stream, bool gpu, int unroll, int vec, int xcd_remap) {
        auto r = to_rects(rects);
        StencilTuning tn;
        tn.chunk_rows = chunk_rows;
        tn.nontemporal = nontemporal;
        tn.kernel = kernel;
        tn.unroll = unroll;
        tn.vec = vec;
        tn.xcd_remap = xcd_remap;
        if (gpu)
          stencil_rects_gpu(P<double>(T2), P<const double>(T), P<const double>(iCp), nx, ny,
                            r.data(), (int)r.size(), to_coef(coef), tn, S(stream));
        else {
          py::gil_scoped_release nogil;
          stencil_rects_cpu(P<double>(T2), P<const double>(T), P<const double>(iCp), nx, ny,
                            r.data(), (int)r.size(), to_coef(coef));
        }
      },
      py::arg("T2"), py::arg("T"), py::arg("iCp"), py::arg("nx"), py::arg("ny"), py::arg("rects"),
      py::arg("coef"), py::arg("chunk_rows") = 4, py::arg("nontemporal") = 3,
      py::arg("kernel") = 0, py::arg("stream") = 0, py::arg("gpu") = true,
      py::arg("unroll") = 4, py::arg("vec") = 2, py::arg("xcd_remap") = -1);
  m.def(
      "stencil2_rects",
      [](uintptr_t T2, uintptr_t T, uintptr_t iCp, int64_t nx, int64_t ny,
         const std::vector<Rect4>& rects, const Coef4& coef, int chunk_rows, int nontemporal,
         uintptr_t stream, bool gpu, int unroll, int xcd_remap) {
        auto r = to_rects(rects);
        StencilTuning tn;
        tn.chunk_rows = chunk_rows;
        tn.nontemporal = nontemporal;
        tn.unroll = unroll;
        tn.xcd_remap = xcd_remap;
        if (gpu)
          stencil2_rects_gpu(P<double>(T2), P<const double>(T), P<const double>(iCp), nx, ny,
                             r.data(), (int)r.size(), to_coef(coef), tn, S(stream));
        else {
          py::gil_scoped_release nogil;
          stencil2_rects_cpu(P<double>(T2), P<const double>(T), P<const double>(iCp), nx, ny,
                             r.data(), (int)r.size(), to_coef(coef));
        }
      },
      py::arg("T2"), py::arg("T"), py::arg("iCp"), py::arg("nx"), py::arg("ny"), py::arg("rects"),
      py::arg("coef"), py::arg("chunk_rows") = 8, py::arg("nontemporal") = 3,
      py::arg("stream") = 0, py::arg("gpu") = true, py::arg("unroll") = 2,
      py::arg("xcd_remap") = -1);
  m.def(
      "stencilk_rects",
      [](int K, uintptr_t T2, uintptr_t T, uintptr_t iCp, int64_t nx, int64_t ny,
         const std::vector<Rect4>& rects, const Coef4& coef, int chunk_rows, int nontemporal,
         uintptr_t stream, bool gpu, int xcd_remap, int vec, int kernel, int stages, int cols,
         bool uniform, double uniform_value, const std::vector<int>& rect_rows, int bands) {
        auto r = to_rects(rects);
        StencilTuning tn;
        if (!rect_rows.empty() && rect_rows.size() != r.size())
          throw std::invalid_argument("rect_rows: one entry per rect");
        tn.rect_rows = rect_rows.empty() ? nullptr : rect_rows.data();
        tn.bands = bands;
        tn.cols = cols;
        tn.uniform = uniform;
        tn.uniform_value = uniform_value;
        tn.chunk_rows = chunk_rows;
        tn.nontemporal = nontemporal;
        tn.xcd_remap = xcd_remap;
        tn.vec = vec;
        tn.kernel = kernel;
        tn.stages = stages;
        if (gpu)
          stencilk_rects_gpu(K, P<double>(T2), P<const double>(T), P<const double>(iCp), nx, ny,
                             r.data(), (int)r.size(), to_coef(coef), tn, S(stream));
        else {
          // the CPU twin of the kernel's arithmetic: fast5 (kernels 5-9, 12, 22) or canonical
          const bool f5 = (kernel >= 5 && kernel <= 9) || kernel == 12 || kernel == 22;
          py::gil_scoped_release nogil;
          if (f5)
            stencilk5_rects_cpu(K, P<double>(T2), P<const double>(T), P<const double>(iCp), nx,
                                ny, r.data(), (int)r.size(), to_coef(coef));
          else
            stencilk_rects_cpu(K, P<double>(T2), P<const double>(T), P<const double>(iCp), nx,
                               ny, r.data(), (int)r.size(), to_coef(coef));
        }
      },
      py::arg("K"), py::arg("T2"), py::arg("T"), py::arg("iCp"), py::arg("nx"), py::arg("ny"),
      py::arg("rects"), py::arg("coef"), py::arg("chunk_rows") = 16, py::arg("nontemporal") = 3,
      py::arg("stream") = 0, py::arg("gpu") = true, py::arg("xcd_remap") = -1,
      py::arg("vec") = 2, py::arg("kernel") = 0, py::arg("stages") = 0, py::arg("cols") = 0,
      py::arg("uniform") = false, py::arg("uniform_value") = 0.0,
      py::arg("rect_rows") = std::vector<int>{}, py::arg("bands") = 0);
  m.def(
      "stencil3d_boxes",
      [](uintptr_t T2, uintptr_t T, uintptr_t iCp, int64_t nx, int64_t ny, int64_t nz,
         const std::vector<Box6>& boxes, const Coef5& coef, int rows, int unroll, int vec,
         int nontemporal, int chunk_z, int xcd_remap, uintptr_t stream, bool gpu, bool uniform,
         double uniform_value, bool fast_math, int xface, uintptr_t signal, int signal_boxes) {
        auto b = to_boxes(boxes);
        if (gpu) {
          Stencil3DTuning tn;
          tn.signal = P<uint64_t>(signal);
          tn.signal_boxes = signal_boxes;
          tn.fast_math = fast_math ? 1 : 0;
          tn.xface = xface;
          tn.uniform = uniform;
          tn.uniform_value = uniform_value;
          tn.rows = rows;
          tn.unroll = unroll;
          tn.vec = vec;
          tn.nontemporal = nontemporal;
          tn.chunk_z = chunk_z;
          tn.xcd_remap = xcd_remap;
          stencil3d_boxes_gpu(P<double>(T2), P<const double>(T), P<const double>(iCp), nx, ny, nz,
                              b.data(), (int)b.size(), to_coef3(coef), tn, S(stream));
        } else {
          py::gil_scoped_release nogil;  // the CPU twin of the arithmetic
          if (fast_math)
            stencil3d7_boxes_cpu(P<double>(T2), P<const double>(T), P<const double>(iCp), nx, ny,
                                 nz, b.data(), (int)b.size(), to_coef3(coef));
          else
            stencil3d_boxes_cpu(P<double>(T2), P<const double>(T), P<const double>(iCp), nx, ny,
                                nz, b.data(), (int)b.size(), to_coef3(coef));
        }
      },
      py::arg("T2"), py::arg("T"), py::arg("iCp"), py::arg("nx"), py::arg("ny"), py::arg("nz"),
      py::arg("boxes"), py::arg("coef"), py::arg("rows") = 4, py::arg("unroll") = 2,
      py::arg("vec") = 2, py::arg("nontemporal") = 3, py::arg("chunk_z") = 0,
      py::arg("xcd_remap") = 1, py::arg("stream") = 0, py::arg("gpu") = true,
      py::arg("uniform") = false, py::arg("uniform_value") = 0.0, py::arg("fast_math") = false,
      py::arg("xface") = 0, py::arg("signal") = 0, py::arg("signal_boxes") = 0);
  m.def(
      "fast7_ok", [](const Coef5& coef) { return fast7_ok(to_coef3(coef)); }, py::arg("coef"));
  // cells per lane a GPU launch with these arrays runs (stencil3d_vec)
  m.def(
      "stencil3d_vec",
      [](uintptr_t T2, uintptr_t T, uintptr_t iCp, int64_t nx, int vec, bool uniform) {
        Stencil3DTuning tn;
        tn.vec = vec;
        tn.uniform = uniform;
        return stencil3d_vec(P<const double>(T2), P<const double>(T), P<const double>(iCp), nx,
                             tn);
      },
      py::arg("T2"), py::arg("T"), py::arg("iCp"), py::arg("nx"), py::arg("vec") = 2,
      py::arg("uniform") = false);
  m.def("stencil3d_has", &stencil3d_has, py::arg("rows"), py::arg("unroll"));
  m.def(
      "stencil3dk_boxes",
      [](int K, uintptr_t T2, uintptr_t T, uintptr_t iCp, int64_t nx, int64_t ny, int64_t nz,
         const std::vector<Box6>& boxes, const Coef5& coef, int rows, int unroll, int vec,
         int nontemporal, int chunk_z, int xcd_remap, int tb_rows, int tb_chunk_z,
         int tb_nontemporal, uintptr_t stream, bool gpu, bool uniform, double uniform_value,
         bool fast_math, int xface, uintptr_t signal, int signal_boxes) {
        auto b = to_boxes(boxes);
        if (gpu) {
          Stencil3DTuning tn;
          tn.signal = P<uint64_t>(signal);
          tn.signal_boxes = signal_boxes;
          tn.fast_math = fast_math ? 1 : 0;
          tn.xface = xface;
          tn.uniform = uniform;
          tn.uniform_value = uniform_value;
          tn.rows = rows;
          tn.unroll = unroll;
          tn.vec = vec;
          tn.nontemporal = nontemporal;
          tn.chunk_z = chunk_z;
          tn.xcd_remap = xcd_remap;
          tn.tb_rows = tb_rows;
          tn.tb_chunk_z = tb_chunk_z;
          tn.tb_nontemporal = tb_nontemporal;
          stencil3dk_boxes_gpu(K, P<double>(T2), P<const double>(T), P<const double>(iCp), nx, ny,
                               nz, b.data(), (int)b.size(), to_coef3(coef), tn, S(stream));
        } else {
          py::gil_scoped_release nogil;
          if (fast_math)
            stencil3dk7_boxes_cpu(K, P<double>(T2), P<const double>(T), P<const double>(iCp), nx,
                                  ny, nz, b.data(), (int)b.size(), to_coef3(coef));
          else
            stencil3dk_boxes_cpu(K, P<double>(T2), P<const double>(T), P<const double>(iCp), nx,
                                 ny, nz, b.data(), (int)b.size(), to_coef3(coef));
        }
      },
      py::arg("K"), py::arg("T2"), py::arg("T"), py::arg("iCp"), py::arg("nx"), py::arg("ny"),
      py::arg("nz"), py::arg("boxes"), py::arg("coef"), py::arg("rows") = 4,
      py::arg("unroll") = 2, py::arg("vec") = 2, py::arg("nontemporal") = 3,
      py::arg("chunk_z") = 0, py::arg("xcd_remap") = 1, py::arg("tb_rows") = 0,
      py::arg("tb_chunk_z") = 0, py::arg("tb_nontemporal") = 0, py::arg("stream") = 0,
      py::arg("gpu") = true, py::arg("uniform") = false, py::arg("uniform_value") = 0.0,
      py::arg("fast_math") = false, py::arg("xface") = 0, py::arg("signal") = 0,
      py::arg("signal_boxes") = 0);
  // The march launch of a K-step pass with these boxes, V cells per lane, by the
  // function both launchers run (stencil3d_fused_plan; host only): (blocks,
  // prefix_blocks, signalling_waves, boxes of the launch, [(box, local block), ...]
  // per block). signal_boxes > 0: the signalling launch, with every launcher check.
  m.def(
      "stencil3d_fused_plan",
      [](int K, int V, const std::vector<Box6>& boxes, int signal_boxes, int rows, int unroll,
         int chunk_z, int xcd_remap, int tb_rows, int tb_chunk_z, int xface) {
        auto b = to_boxes(boxes);
        Stencil3DTuning tn;
        tn.rows = rows;
        tn.unroll = unroll;
        tn.chunk_z = chunk_z;
        tn.xcd_remap = xcd_remap;
        tn.tb_rows = tb_rows;
        tn.tb_chunk_z = tb_chunk_z;
        tn.xface = xface;
        RMA_CHECK_ARG(b.size() <= (size_t)kMaxBoxes,
                      "nboxes=" << b.size() << " (at most " << kMaxBoxes << " boxes per launch)");
        const Fused3DPlan p =
            stencil3d_fused_plan(K, V, b.data(), (int)b.size(), tn, signal_boxes, nullptr);
        std::vector<int64_t> map((size_t)(2 * p.blocks));
        stencil3d_fused_plan(K, V, b.data(), (int)b.size(), tn, signal_boxes, map.data());
        std::vector<std::pair<int64_t, int64_t>> pairs((size_t)p.blocks);
        for (int64_t i = 0; i < p.blocks; ++i) pairs[(size_t)i] = {map[2 * i], map[2 * i + 1]};
        return py::make_tuple(p.blocks, p.prefix_blocks, p.signalling_waves, p.boxes, pairs);
      },
      py::arg("K"), py::arg("V"), py::arg("boxes"), py::arg("signal_boxes"), py::arg("rows") = 4,
      py::arg("unroll") = 2, py::arg("chunk_z") = 0, py::arg("xcd_remap") = 1,
      py::arg("tb_rows") = 0, py::arg("tb_chunk_z") = 0, py::arg("xface") = 0);
  // the kernel path of every non-empty box of a K-step launch with this xface
  // (plan_dispatch3d, the rule both launchers run): [(path, lanes), ...] with path
  // "march", "thin" or "xface". Host only.
  m.def(
      "stencil3d_dispatch",
      [](int K, const std::vector<Box6>& boxes, int xface) {
        auto b = to_boxes(boxes);
        Stencil3DTuning tn;
        tn.xface = xface;
        std::vector<Dispatch3D> d(b.size());
        plan_dispatch3d(K, b.data(), (int)b.size(), tn, d.data());
        std::vector<std::pair<std::string, int>> out;
        for (const Dispatch3D& e : d)
          if (e.path != kPathNone) out.emplace_back(path3d_name(e.path), e.lanes);
        return out;
      },
      py::arg("K"), py::arg("boxes"), py::arg("xface") = 0);
  m.def("stencil3dk_has", &stencil3dk_has, py::arg("K"));
  m.def("stencil3dk_has_rows", &stencil3dk_has_rows, py::arg("rows"));
  // Cells of A[0, n) whose bit pattern differs from A[0]'s. GPU: out2 is device
  // memory (two 64-bit words: the count is added to out2[0], zero it on the same
  // stream first; out2[1] = A[0]'s bits), nothing synchronises, returns 0. CPU:
  // returns the count.
  m.def(
      "count_differing",
      [](uintptr_t A, int64_t n, uintptr_t out2, uintptr_t stream, bool gpu) -> int64_t {
        if (gpu) {
          count_differing_gpu(P<const double>(A), n, P<uint64_t>(out2), S(stream));
          return 0;
        }
        py::gil_scoped_release nogil;
        return count_differing_cpu(P<const double>(A), n);
      },
      py::arg("A"), py::arg("n"), py::arg("out2") = 0, py::arg("stream") = 0,
      py::arg("gpu") = true);
  m.def("init_gaussian3d", [](uintptr_t T, int64_t nx, int64_t ny, int64_t nz, const Geom3& g,
                              double lx, double ly, double lz, uintptr_t stream, bool gpu) {
    if (gpu)
      init_gaussian3d_gpu(P<double>(T), nx, ny, nz, to_geom3(g), lx, ly, lz, S(stream));
    else
      init_gaussian3d_cpu(P<double>(T), nx, ny, nz, to_geom3(g), lx, ly, lz);
  });
  m.def("init_random3d", [](uintptr_t A, int64_t nx, int64_t ny, int64_t nz, const Geom3& g,
                            uint64_t seed, double lo, double hi, uintptr_t stream, bool gpu) {
    if (gpu)
      init_random3d_gpu(P<double>(A), nx, ny, nz, to_geom3(g), seed, lo, hi, S(stream));
    else
      init_random3d_cpu(P<double>(A), nx, ny, nz, to_geom3(g), seed, lo, hi);
  });
  m.def(
      "stream_copy",
      [](uintptr_t b, uintptr_t a, int64_t n, uintptr_t s, int nt, int blocks) {
        stream_copy_gpu(P<double>(b), P<const double>(a), n, nt, blocks, S(s));
      },
      py::arg("b"), py::arg("a"), py::arg("n"), py::arg("stream"), py::arg("nt") = 0,
      py::arg("blocks") = 0);
  m.def(
      "stream_triad",
      [](uintptr_t c, uintptr_t a, uintptr_t b, double x, int64_t n, uintptr_t s, int nt,
         int blocks) {
        stream_triad_gpu(P<double>(c), P<const double>(a), P<const double>(b), x, n, nt, blocks,
                         S(s));
      },
      py::arg("c"), py::arg("a"), py::arg("b"), py::arg("x"), py::arg("n"), py::arg("stream"),
      py::arg("nt") = 0, py::arg("blocks") = 0);

  m.def("flux", [](uintptr_t qx, uintptr_t qy, uintptr_t T, int64_t nx, int64_t ny, double mlam,
                   double rdx, double rdy, uintptr_t stream, bool gpu) {
    if (gpu)
      flux_gpu(P<double>(qx), P<double>(qy), P<const double>(T), nx, ny, mlam, rdx, rdy,
               S(stream));
    else
      flux_cpu(P<double>(qx), P<double>(qy), P<const double>(T), nx, ny, mlam, rdx, rdy);
  });
  m.def("residual", [](uintptr_t dTdt, uintptr_t qx, uintptr_t qy, uintptr_t iCp, int64_t nx,
                       int64_t ny, double rdx, double rdy, uintptr_t stream, bool gpu) {
    if (gpu)
      residual_gpu(P<double>(dTdt), P<const double>(qx), P<const double>(qy),
                   P<const double>(iCp), nx, ny, rdx, rdy, S(stream));
    else
      residual_cpu(P<double>(dTdt), P<const double>(qx), P<const double>(qy),
                   P<const double>(iCp), nx, ny, rdx, rdy);
  });
  m.def("update", [](uintptr_t T, uintptr_t dTdt, int64_t nx, int64_t ny, double dt,
                     uintptr_t stream, bool gpu) {
    if (gpu)
      update_gpu(P<double>(T), P<const double>(dTdt), nx, ny, dt, S(stream));
    else
      update_cpu(P<double>(T), P<const double>(dTdt), nx, ny, dt);
  });
  m.def("init_gaussian", [](uintptr_t T, int64_t nx, int64_t ny, const Geom& g, double lx,
                            double ly, uintptr_t stream, bool gpu) {
    if (gpu)
      init_gaussian_gpu(P<double>(T), nx, ny, to_geom(g), lx, ly, S(stream));
    else
      init_gaussian_cpu(P<double>(T), nx, ny, to_geom(g), lx, ly);
  });
  m.def("init_random", [](uintptr_t A, int64_t nx, int64_t ny, const Geom& g, uint64_t seed,
                          double lo, double hi, uintptr_t stream, bool gpu) {
    if (gpu)
      init_random_gpu(P<double>(A), nx, ny, to_geom(g), seed, lo, hi, S(stream));
    else
      init_random_cpu(P<double>(A), nx, ny, to_geom(g), seed, lo, hi);
  });
  m.def("fill", [](uintptr_t A, int64_t n, double v, uintptr_t stream) {
    fill_gpu(P<double>(A), n, v, S(stream));
  });
  m.def("copy2d", [](uintptr_t dst, int64_t dst_ld, uintptr_t src, int64_t src_ld, int64_t n_o,
                     int64_t n_k, int elem_bytes, uintptr_t stream, bool gpu) {
    if (gpu)
      copy2d_gpu(P<void>(dst), dst_ld, P<const void>(src), src_ld, n_o, n_k, elem_bytes,
                 S(stream));
    else
      copy2d_cpu(P<void>(dst), dst_ld, P<const void>(src), src_ld, n_o, n_k, elem_bytes);
  });
  // copies: [(dst, dst_ld, src, src_ld, n_o, n_k)], one element size, one launch
  m.def("copy2d_batch", [](const std::vector<std::tuple<uintptr_t, int64_t, uintptr_t, int64_t,
                                                        int64_t, int64_t>>& copies,
                           int elem_bytes, uintptr_t stream, bool gpu) {
    std::vector<Copy2d> c;
    for (const auto& t : copies)
      c.push_back({P<void>(std::get<0>(t)), std::get<1>(t), P<const void>(std::get<2>(t)),
                   std::get<3>(t), std::get<4>(t), std::get<5>(t)});
    if (gpu)
      copy2d_batch_gpu(c.data(), (int)c.size(), elem_bytes, S(stream));
    else
      copy2d_batch_cpu(c.data(), (int)c.size(), elem_bytes);
  });
  m.def("copy2d_batch_max", [] { return kCopy2dBatch; });
  // blocks: [(dst, src, dst_row, dst_plane, src_row, src_plane, nx, ny, nz)] in elements,
  // any number (launches of <= copy_blocks_max() descriptors of one access path)
  m.def("copy_blocks", [](const std::vector<std::tuple<uintptr_t, uintptr_t, int64_t, int64_t,
                                                       int64_t, int64_t, int64_t, int64_t,
                                                       int64_t>>& blocks,
                          int elem_bytes, uintptr_t stream, bool gpu) {
    std::vector<BlockCopy> c;
    for (const auto& t : blocks)
      c.push_back({P<void>(std::get<0>(t)), P<const void>(std::get<1>(t)), std::get<2>(t),
                   std::get<3>(t), std::get<4>(t), std::get<5>(t), std::get<6>(t),
                   std::get<7>(t), std::get<8>(t)});
    if (gpu)
      copy_blocks_gpu(c.data(), (int64_t)c.size(), elem_bytes, S(stream));
    else
      copy_blocks_cpu(c.data(), (int64_t)c.size(), elem_bytes);
  });
  m.def("copy_blocks_max", [] { return kCopyBlocksBatch; });
  // where every rank's block of the IGG-style gather sits in A_global (rma/gather.h)
  m.def(
      "gather_plan",
      [](const std::array<int, 3>& dims, const std::array<int64_t, 3>& size, int elem_bytes) {
        const GatherPlan p = plan_gather(dims, size, elem_bytes);
        py::dict d;
        d["nprocs"] = p.nprocs;
        d["size_g"] = p.size_g;
        d["row_pitch_g"] = p.row_pitch_g;
        d["plane_pitch_g"] = p.plane_pitch_g;
        d["block_elems"] = p.block_elems;
        d["coords"] = p.coords;
        d["offsets"] = p.offset;
        d["contiguous_in_global"] = p.contiguous_in_global;
        return d;
      },
      py::arg("dims"), py::arg("size"), py::arg("elem_bytes"));
  // the IPC transport's stream-ordered flag kernels (csrc/kernels/flags.hip)
  m.def(
      "flag_wait",
      [](uintptr_t flag, uint64_t want, double timeout_s, uintptr_t err, uint32_t code,
         uintptr_t stream) {
        flag_wait_gpu(P<const uint64_t>(flag), want, timeout_s, P<uint32_t>(err), code, S(stream));
      },
      py::call_guard<py::gil_scoped_release>());
  m.def(
      "flag_write",
      [](uintptr_t flag, uint64_t value, uintptr_t stream) {
        flag_write_gpu(P<uint64_t>(flag), value, S(stream));
      },
      py::call_guard<py::gil_scoped_release>());
  m.def("reduce_workspace_doubles", &reduce_workspace_doubles);
  m.def("reduce_gpu", [](uintptr_t A, int64_t n, int op, uintptr_t out, uintptr_t ws,
                         uintptr_t stream) {
    reduce_gpu(P<const double>(A), n, op, P<double>(out), P<double>(ws), S(stream));
  });
  m.def("reduce_cpu",
        [](uintptr_t A, int64_t n, int op) { return reduce_cpu(P<const double>(A), n, op); });
  m.def("diag_string", &diag_string);  // RMA_DIAG, validated (unknown key: error)
  m.def("diag_value", [](const std::string& k) { return diag_value(k.c_str()); });
  m.def("env_double", &env_double);
  m.def("env_choice", &env_choice);
  m.def("field_stats_workspace_doubles", &field_stats_workspace_doubles);
  m.def("field_stats_gpu", [](uintptr_t A, int64_t n, uintptr_t out3, uintptr_t ws,
                              uintptr_t stream) {
    field_stats_gpu(P<const double>(A), n, P<double>(out3), P<double>(ws), S(stream));
  });
  m.def("field_stats_cpu", [](uintptr_t A, int64_t n) {
    double o[3];
    field_stats_cpu(P<const double>(A), n, o);
    return std::make_tuple(o[0], o[1], o[2]);
  });

  // ---------------- topology ----------------
  m.def("dims_create", &dims_create, py::arg("nprocs"), py::arg("dims"));
  m.attr("PROC_NULL") = kProcNull;
  py::class_<CartTopology>(m, "CartTopology")
      .def(py::init<int, std::array<int, 3>, std::array<int, 3>>(), py::arg("nprocs"),
           py::arg("dims"), py::arg("periods"))
      .def_property_readonly("nprocs", &CartTopology::nprocs)
      .def_property_readonly("dims", &CartTopology::dims)
      .def_property_readonly("periods", &CartTopology::periods)
      .def("coords", &CartTopology::coords)
      .def("rank_of", &CartTopology::rank_of)
      .def("shift", &CartTopology::shift)
      .def("neighbors", &CartTopology::neighbors)
      .def("diagonals", &CartTopology::diagonals);

  // ---------------- communication ----------------
  py::enum_<DType>(m, "DType")
      .value("float64", DType::kFloat64)
      .value("float32", DType::kFloat32)
      .value("int64", DType::kInt64)
      .value("int32", DType::kInt32)
      .value("uint8", DType::kUInt8);
  py::enum_<RedOp>(m, "RedOp")
      .value("sum", RedOp::kSum)
      .value("max", RedOp::kMax)
      .value("min", RedOp::kMin)
      .value("prod", RedOp::kProd);
  py::class_<P2PTransport>(m, "P2PTransport")
      .def_property_readonly("rank", &P2PTransport::rank)
      .def_property_readonly("size", &P2PTransport::size)
      .def("group_start", &P2PTransport::group_start)
      .def("group_end", &P2PTransport::group_end, py::call_guard<py::gil_scoped_release>())
      .def("send", [](P2PTransport& c, uintptr_t buf, size_t bytes, int peer,
                      uintptr_t s) { c.send(P<const void>(buf), bytes, peer, S(s)); },
           py::call_guard<py::gil_scoped_release>())
      .def("recv", [](P2PTransport& c, uintptr_t buf, size_t bytes, int peer,
                      uintptr_t s) { c.recv(P<void>(buf), bytes, peer, S(s)); },
           py::call_guard<py::gil_scoped_release>());
  py::class_<LoopbackHub, std::shared_ptr<LoopbackHub>>(m, "LoopbackHub")
      .def(py::init<int, double>(), py::arg("nranks"), py::arg("timeout_s") = 60.0)
      .def_property_readonly("size", &LoopbackHub::size);
  py::class_<LoopbackEndpoint, P2PTransport>(m, "LoopbackEndpoint")
      .def(py::init<std::shared_ptr<LoopbackHub>, int>(), py::arg("hub"), py::arg("rank"));
  py::class_<IpcTransport, P2PTransport>(m, "IpcTransport")
      .def(py::init<int, int, int, const std::vector<int>&, size_t, const std::string&, double,
                    int>(),
           py::arg("rank"), py::arg("size"), py::arg("device"), py::arg("peers"),
           py::arg("mailbox_bytes"), py::arg("token"), py::arg("timeout_s") = 300.0,
           py::arg("mode") = -1)
      .def("export_for", [](const IpcTransport& t, int p) { return py::bytes(t.export_for(p)); })
      .def("connect", [](IpcTransport& t, int p, py::bytes blob) { t.connect(p, blob); })
      .def("unlink_shm", &IpcTransport::unlink_shm)
      .def("abort_waits", &IpcTransport::abort_waits)
      .def("check_error", &IpcTransport::check_error)
      .def_property_readonly("connected", &IpcTransport::connected)
      .def_property_readonly("mailbox_bytes", &IpcTransport::mailbox_bytes)
      .def_property_readonly("mode",
                             [](const IpcTransport& t) {
                               return t.mode() == IpcTransport::Mode::kStream ? "stream" : "host";
                             })
      .def_property_readonly("poisoned", &IpcTransport::poisoned)
      .def_property_readonly("host_waits", &IpcTransport::host_waits);
  py::class_<IpcMap>(m, "IpcMap")
      .def(py::init<>())
      .def_static("export_ptr",
                  [](uintptr_t p) { return py::bytes(IpcMap::export_ptr((const void*)p)); })
      .def("open", [](IpcMap& m, py::bytes blob) { return (uintptr_t)m.open(blob); })
      .def("close_all", &IpcMap::close_all)
      .def_property_readonly("mappings", &IpcMap::mappings);
  py::class_<RcclComm, P2PTransport>(m, "RcclComm")
      .def_static("unique_id", []() { return py::bytes(RcclComm::unique_id()); })
      .def(py::init([](int nranks, int rank, py::bytes uid, int device, double init_timeout_s) {
             std::string s = uid;
             py::gil_scoped_release nogil;
             return new RcclComm(nranks, rank, s, device, init_timeout_s);
           }),
           py::arg("nranks"), py::arg("rank"), py::arg("uid"), py::arg("device"),
           py::arg("init_timeout_s") = 0.0)
      .def_property_readonly("nonblocking", &RcclComm::nonblocking)
      .def_property_readonly("data_blocking", &RcclComm::data_blocking)
      .def_property_readonly("device", &RcclComm::device)
      .def("count", &RcclComm::count)
      .def("allreduce",
           [](RcclComm& c, uintptr_t sb, uintptr_t rb, size_t count, DType dt, RedOp op,
              uintptr_t s) { c.allreduce(P<const void>(sb), P<void>(rb), count, dt, op, S(s)); })
      .def("broadcast",
           [](RcclComm& c, uintptr_t sb, uintptr_t rb, size_t count, DType dt, int root,
              uintptr_t s) { c.broadcast(P<const void>(sb), P<void>(rb), count, dt, root, S(s)); })
      .def("gather", [](RcclComm& c, uintptr_t sb, uintptr_t rb, size_t bytes, int root,
                        uintptr_t s) { c.gather(P<const void>(sb), P<void>(rb), bytes, root, S(s)); })
      .def(
          "barrier", [](RcclComm& c, uintptr_t s, double t) { c.barrier(S(s), t); },
          py::arg("stream"), py::arg("timeout_s") = 300.0, py::call_guard<py::gil_scoped_release>())
      .def(
          "wait", [](RcclComm& c, uintptr_t s, double t) { c.wait(S(s), t); }, py::arg("stream"),
          py::arg("timeout_s") = 300.0, py::call_guard<py::gil_scoped_release>())
      .def("check_async", &RcclComm::check_async)
      .def("abort", &RcclComm::abort)
      .def_property_readonly("aborted", &RcclComm::aborted);

  py::class_<HaloExchanger>(m, "HaloExchanger")
      .def(py::init([](P2PTransport* comm, int self_rank,
                       std::array<std::array<int, 2>, 3> nbr) {
             return new HaloExchanger(comm, self_rank, nbr);
           }),
           py::arg("comm").none(true), py::arg("self_rank"), py::arg("neighbors"),
           py::keep_alive<1, 2>())
      .def(
          "exchange",
          [](HaloExchanger& h, const std::vector<FieldT>& fields, uintptr_t s, int mask) {
            auto f = to_fields(fields);
            py::gil_scoped_release nogil;  // loopback transports block on peer threads
            h.exchange(f, S(s), mask);
          },
          py::arg("fields"), py::arg("stream"), py::arg("dims_mask") = 7)
      .def(
          "prepare",
          [](HaloExchanger& h, const std::vector<FieldT>& fields, int mask) {
            h.prepare(to_fields(fields), mask);
          },
          py::arg("fields"), py::arg("dims_mask") = 7)
      .def(
          "exchange_merged",
          [](HaloExchanger& h, const std::vector<FieldT>& fields, uintptr_t s) {
            auto f = to_fields(fields);
            py::gil_scoped_release nogil;
            h.exchange_merged(f, S(s));
          },
          py::arg("fields"), py::arg("stream"))
      .def("set_diagonals", &HaloExchanger::set_diagonals)
      .def_property_readonly("has_diagonals", &HaloExchanger::has_diagonals)
      .def_property_readonly("diagonals", &HaloExchanger::diagonals)
      .def("active", &HaloExchanger::active)
      .def("capturable", &HaloExchanger::capturable)
      .def("set_self_via_transport", &HaloExchanger::set_self_via_transport)
      .def_property_readonly("neighbors", &HaloExchanger::neighbors)
      .def_property_readonly("bytes_sent_last", &HaloExchanger::bytes_sent_last)
      .def_property_readonly("plan_hits", &HaloExchanger::plan_hits)
      .def_property_readonly("plan_misses", &HaloExchanger::plan_misses);

  // ---------------- executor ----------------
  m.def("pipe_chunk_rows", &pipe_chunk_rows, py::arg("K"), py::arg("ny"),
        py::arg("canonical") = false);
  m.def("default_chunk_k", [](int K, int64_t ny) { return default_tune_k(K, ny).chunk_rows; },
        py::arg("K"), py::arg("ny"));
  m.def("plan_passes", &plan_passes, py::arg("nsteps"), py::arg("costs"));
  m.def("uniform_pass_costs", &uniform_pass_costs, py::arg("kmax"), py::arg("cells") = 0.0);
  m.def("pipe_uniform_cells", &pipe_uniform_cells, py::arg("K"), py::arg("cells"));
  m.def("default_pass_costs", &default_pass_costs, py::arg("kmax"), py::arg("fast5"),
        py::arg("cells") = 0.0);
  m.def(
      "plan_row_bands",
      [](int64_t y0, int64_t y1, int64_t strips, int64_t slots, const std::array<int, 3>& rows,
         int uniform_rows, double fill) {
        std::vector<std::tuple<int64_t, int64_t, int>> out;
        for (const RowBand& b : plan_row_bands(y0, y1, strips, slots, rows, uniform_rows, fill))
          out.emplace_back(b.y0, b.y1, b.rows);
        return out;
      },
      py::arg("y0"), py::arg("y1"), py::arg("strips"), py::arg("slots"), py::arg("rows"),
      py::arg("uniform_rows"), py::arg("fill") = kBandFill);
  m.def("pipe_band_rows", &pipe_band_rows, py::arg("K"), py::arg("ny"));
  m.def("pipe_strip_count", &pipe_strip_count, py::arg("x0"), py::arg("x1"), py::arg("K"),
        py::arg("V"));
  m.def(
      "parse_task_rows",
      [](const std::string& spec) {
        std::array<int, 3> rows{{0, 0, 0}};
        double fill = kBandFill;
        bool uniform = false;
        const bool forced = parse_task_rows(spec, rows, fill, uniform);
        return std::make_tuple(forced, uniform, rows, fill);
      },
      py::arg("spec"));
  m.def(
      "pipe_task_map",
      [](const std::vector<Rect4>& rects, int V, int chunk_rows, int halo, int64_t sw_block,
         const std::vector<int>& rect_rows, int bands, int sig_rects, int remap) {
        auto r = to_rects(rects);
        if (!rect_rows.empty() && rect_rows.size() != r.size())
          throw std::invalid_argument("rect_rows: one entry per rect");
        const int* rr = rect_rows.empty() ? nullptr : rect_rows.data();
        const int64_t n = pipe_task_map(r.data(), (int)r.size(), V, chunk_rows, halo, sw_block, rr,
                                        bands, sig_rects, remap, nullptr);
        std::vector<int64_t> flat((size_t)(3 * n));
        pipe_task_map(r.data(), (int)r.size(), V, chunk_rows, halo, sw_block, rr, bands,
                      sig_rects, remap, flat.data());
        std::vector<std::tuple<int64_t, int64_t, int64_t>> out;
        for (int64_t b = 0; b < n; ++b)
          out.emplace_back(flat[3 * b], flat[3 * b + 1], flat[3 * b + 2]);
        return out;
      },
      py::arg("rects"), py::arg("V"), py::arg("chunk_rows"), py::arg("halo"),
      py::arg("sw_block") = 0, py::arg("rect_rows") = std::vector<int>{}, py::arg("bands") = 0,
      py::arg("sig_rects") = 0, py::arg("remap") = 1);
  m.def("pipe_last_launch", []() {
    int64_t v[2] = {0, 0};
    pipe_last_launch(v);
    return std::make_tuple(v[0], v[1]);
  });
  m.def(
      "stencil_pipe_occupancy",
      [](int K, int stages, int arith, int V) {
        int occ[2] = {0, 0};
        stencil_pipe_occupancy(K, stages, arith, V, occ);
        return std::make_tuple(occ[0], occ[1]);
      },
      py::arg("K"), py::arg("stages"), py::arg("arith"), py::arg("V"));
  m.def("pipe_default_stages", &pipe_default_stages, py::arg("K"));
  m.def("pipe_default_cols", &pipe_default_cols, py::arg("K"), py::arg("stages"),
        py::arg("arith") = 0);
  m.def("pipe_has_cols", &pipe_has_cols, py::arg("K"), py::arg("stages"), py::arg("arith"),
        py::arg("cols"));
  m.def("pipe_vec", &pipe_vec, py::arg("K"), py::arg("stages"), py::arg("arith"), py::arg("nx"),
        py::arg("requested"), py::arg("aligned16") = true);
  m.def("pipe_vec_uniform", &pipe_vec_uniform, py::arg("K"), py::arg("stages"), py::arg("arith"),
        py::arg("nx"), py::arg("requested"), py::arg("aligned16") = true,
        py::arg("uniform") = false);
  m.def("pipe_max_k", []() { return kPipeMaxK; });
  m.def(
      "pass_geometry",
      [](int64_t nx, int64_t ny, int K, std::array<std::array<int, 2>, 3> nbr, bool hide,
         int64_t bwx, int64_t bwy, int64_t olx, int64_t oly) {
        const PassGeom g = pass_geometry(nx, ny, K, nbr, hide, bwx, bwy, olx, oly);
        std::vector<Rect4> fr;
        for (auto& r : g.frame) fr.push_back(from_rect(r));
        return std::make_tuple(from_rect(g.out), fr, from_rect(g.interior));
      },
      py::arg("nx"), py::arg("ny"), py::arg("K"), py::arg("neighbors"), py::arg("hide"),
      py::arg("bwx"), py::arg("bwy"), py::arg("olx"), py::arg("oly"));
  m.def(
      "frame_layout",
      [](int64_t ny, std::array<std::array<int, 2>, 3> nbr) {
        const FrameLayout f = frame_layout(ny, nbr);
        return std::make_tuple(f.chunk_div, f.bands);
      },
      py::arg("ny"), py::arg("neighbors"));
  m.def(
      "canonical_kernel_k",
      [](int K, int64_t ny) {
        const StencilTuning t = canonical_tune_k(K, ny);
        return std::make_tuple(t.kernel, t.vec, t.chunk_rows);
      },
      py::arg("K"), py::arg("ny"));
  m.def(
      "fast_kernel_k",
      [](int K, int64_t ny, const Coef4& coef) {
        const StencilTuning t = fast_tune_k(K, ny, to_coef(coef));
        return std::make_tuple(t.kernel, t.vec, t.chunk_rows);
      },
      py::arg("K"), py::arg("ny"), py::arg("coef"));
  py::class_<DiffusionExecutor>(m, "Executor")
      .def(py::init([](uintptr_t T, uintptr_t T2, uintptr_t iCp, int64_t nx, int64_t ny, int mode,
                       const Coef4& coef, int chunk_rows, int nontemporal, int kernel,
                       int64_t bwx, int64_t bwy, int use_graph, int graph_steps,
                       HaloExchanger* halo, uintptr_t qx, uintptr_t qy, uintptr_t dTdt,
                       int unroll, int vec, int temporal, int64_t olx, int64_t oly,
                       int chunk2, int unroll2, int fast_math) {
             ExecParams p;
             p.fast_math = fast_math;
             p.temporal = temporal;
             p.olx = olx;
             p.oly = oly;
             p.tune2 = default_tune_k(temporal, ny);  // measured defaults
             if (chunk2 > 0) p.tune2.chunk_rows = chunk2;
             p.chunk_rows2 = chunk2;  // 0: per pass depth
             if (temporal == 2) p.tune2.unroll = unroll2;
             p.tune2.nontemporal = nontemporal & 3;
             p.mode = static_cast<Mode>(mode);
             p.coef = to_coef(coef);
             p.tune.chunk_rows = chunk_rows;
             p.tune.nontemporal = nontemporal;
             p.tune.kernel = kernel;
             p.tune.unroll = unroll;
             p.tune.vec = vec;
             p.bwx = bwx;
             p.bwy = bwy;
             p.use_graph = use_graph;
             p.graph_steps = graph_steps;
             return new DiffusionExecutor(P<double>(T), P<double>(T2), P<const double>(iCp), nx,
                                          ny, p, halo, P<double>(qx), P<double>(qy),
                                          P<double>(dTdt));
           }),
           py::arg("T"), py::arg("T2"), py::arg("iCp"), py::arg("nx"), py::arg("ny"),
           py::arg("mode"), py::arg("coef"), py::arg("chunk_rows") = 4,
           py::arg("nontemporal") = 3, py::arg("kernel") = 0, py::arg("bwx") = 1,
           py::arg("bwy") = 1, py::arg("use_graph") = 0, py::arg("graph_steps") = 0,
           py::arg("halo").none(true) = nullptr, py::arg("qx") = 0, py::arg("qy") = 0,
           py::arg("dTdt") = 0, py::arg("unroll") = 4, py::arg("vec") = 2,
           py::arg("temporal") = 1, py::arg("olx") = 2, py::arg("oly") = 2,
           py::arg("chunk2") = 0, py::arg("unroll2") = 2, py::arg("fast_math") = 0,
           py::keep_alive<1, 16>())
      .def(
          "run", [](DiffusionExecutor& e, int64_t n, uintptr_t s) { e.run(n, S(s)); },
          py::arg("nsteps"), py::arg("stream"), py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("parity", &DiffusionExecutor::parity)
      .def_property_readonly("steps_done", &DiffusionExecutor::steps_done)
      .def_property_readonly("passes_done", &DiffusionExecutor::passes_done)
      .def_property_readonly("fused_passes", &DiffusionExecutor::fused_passes)
      .def_property_readonly("graded_passes", &DiffusionExecutor::graded_passes)
      .def(
          "row_bands",
          [](DiffusionExecutor& e, int K, const Rect4& r) {
            std::vector<std::tuple<int64_t, int64_t, int>> out;
            for (const RowBand& b : e.row_bands(K, to_rects({r})[0]))
              out.emplace_back(b.y0, b.y1, b.rows);
            return out;
          },
          py::arg("K"), py::arg("rect"))
      .def_property_readonly("uniform_factor", &DiffusionExecutor::uniform_factor)
      .def("rescan_factor", &DiffusionExecutor::rescan_factor,
           py::call_guard<py::gil_scoped_release>())
      .def("check_error", &DiffusionExecutor::check_error)
      .def("plan", &DiffusionExecutor::plan, py::arg("nsteps"))
      .def_property_readonly("pass_costs", &DiffusionExecutor::pass_costs)
      .def("prime", &DiffusionExecutor::prime, py::call_guard<py::gil_scoped_release>())
      .def("set_timing", &DiffusionExecutor::set_timing, py::arg("on"),
           py::call_guard<py::gil_scoped_release>())
      .def("timings",
           [](DiffusionExecutor& e) {
             std::vector<py::dict> out;
             std::vector<PassTiming> ts;
             {
               py::gil_scoped_release nogil;
               ts = e.timings();
             }
             for (const auto& t : ts) {
               py::dict d;
               d["K"] = t.K;
               d["frame_ms"] = t.frame_ms;
               d["halo_ms"] = t.halo_ms;
               d["interior_ms"] = t.interior_ms;
               d["pass_ms"] = t.pass_ms;
               d["exposed_halo_ms"] = t.exposed_halo_ms;
               out.push_back(d);
             }
             return out;
           })
      .def(
          "set_direct",
          // peers: 8 tuples (rank, T ptr, T2 ptr, flag ptr) in DiffusionExecutor::kDirI/J
          // order; in_flags: this rank's 8 device words (0: none)
          [](DiffusionExecutor& e, const std::vector<std::tuple<int, uintptr_t, uintptr_t, uintptr_t>>& peers,
             uintptr_t in_flags, bool host_wait) {
            RMA_CHECK_ARG(peers.size() == 8, "set_direct: 8 directions, got " << peers.size());
            std::array<DiffusionExecutor::DirectPeer, 8> a{};
            for (int d = 0; d < 8; ++d) {
              a[d].rank = std::get<0>(peers[d]);
              a[d].T = P<double>(std::get<1>(peers[d]));
              a[d].T2 = P<double>(std::get<2>(peers[d]));
              a[d].flag = P<uint64_t>(std::get<3>(peers[d]));
            }
            e.set_direct(a, P<uint64_t>(in_flags), host_wait);
          },
          py::arg("peers"), py::arg("in_flags"), py::arg("host_wait") = false,
          py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("direct", &DiffusionExecutor::direct)
      .def_property_readonly("direct_passes", &DiffusionExecutor::direct_passes)
      .def_property_readonly_static("direct_dirs", [](py::object) {
        std::vector<std::pair<int, int>> v;
        for (int d = 0; d < 8; ++d)
          v.emplace_back(DiffusionExecutor::kDirI[d], DiffusionExecutor::kDirJ[d]);
        return v;
      })
      .def("set_solo", &DiffusionExecutor::set_solo, py::arg("on"),
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("solo", &DiffusionExecutor::solo)
      .def_property_readonly("frame_rects",
                             [](const DiffusionExecutor& e) {
                               std::vector<Rect4> v;
                               for (auto& r : e.frame_rects()) v.push_back(from_rect(r));
                               return v;
                             })
      .def_property_readonly("interior_rect",
                             [](const DiffusionExecutor& e) { return from_rect(e.interior_rect()); })
      .def(
          "geometry",
          [](DiffusionExecutor& e, int K) {
            const PassGeom& g = e.geometry(K);
            auto rl = [](const std::vector<Rect>& v) {
              std::vector<Rect4> o;
              for (auto& r : v) o.push_back(from_rect(r));
              return o;
            };
            py::dict d;
            d["aligned"] = g.aligned;
            d["out"] = from_rect(g.out);
            d["frame"] = rl(g.frame);
            d["frame_wide"] = rl(g.frame_wide);
            d["frame_tall"] = rl(g.frame_tall);
            d["interior"] = from_rect(g.interior);
            d["tasks"] = g.tasks();  // the interior grid's tasks (fused / one-launch policy)
            d["task_w"] = g.task_w;  // output columns per strip of the pass's kernel
            return d;
          },
          py::arg("K"));

  // ---------------- 3D diffusion: pass geometry and the native time loop ----------------
  // the C++ twins of Diffusion3D.owned_box and ops.hide_boxes3d (rma/plan3d.h)
  m.def(
      "owned_box3d",
      [](const std::array<int64_t, 3>& n, const Neighbors& nbr, int k) {
        return from_box(owned_box3d(n, nbr, k));
      },
      py::arg("n"), py::arg("neighbors"), py::arg("k"));
  m.def(
      "hide_boxes3d",
      [](const std::array<int64_t, 3>& n, const Box6& owned, const Sides3& sides,
         const std::array<int64_t, 3>& overlaps, const std::array<int64_t, 3>& b_width) {
        const HideBoxes3 h = hide_boxes3d(n, to_boxes({owned})[0], sides, overlaps, b_width);
        std::vector<Box6> frame;
        for (const Box& b : h.frame) frame.push_back(from_box(b));
        py::object inner = py::none();
        if (h.has_interior) inner = py::cast(from_box(h.interior));
        return py::make_tuple(frame, inner);
      },
      py::arg("n"), py::arg("owned"), py::arg("sides"), py::arg("overlaps"), py::arg("b_width"));
  py::class_<Diffusion3DExecutor>(m, "Executor3D")
      .def(py::init([](uintptr_t T, uintptr_t T2, uintptr_t iCp, int64_t nx, int64_t ny,
                       int64_t nz, int mode, const Coef5& coef, HaloExchanger* halo,
                       const std::array<int64_t, 3>& overlaps,
                       const std::array<int64_t, 3>& halowidths, int steps_per_pass,
                       bool fast_math, const std::array<int64_t, 3>& b_width, int xface,
                       bool uniform_factor, int rows, int unroll, int vec, int nontemporal,
                       int chunk_z, int xcd_remap, int tb_rows, int tb_chunk_z,
                       int tb_nontemporal, int fused, double fused_timeout_s) {
             Exec3DParams p;
             p.fused = fused;
             p.fused_timeout_s = fused_timeout_s;
             p.mode = mode;
             p.coef = to_coef3(coef);
             p.steps_per_pass = steps_per_pass;
             p.fast_math = fast_math ? 1 : 0;
             p.b_width = b_width;
             p.xface = xface;
             p.uniform_factor = uniform_factor;
             p.overlaps = overlaps;
             p.halowidths = halowidths;
             p.tune.rows = rows;
             p.tune.unroll = unroll;
             p.tune.vec = vec;
             p.tune.nontemporal = nontemporal;
             p.tune.chunk_z = chunk_z;
             p.tune.xcd_remap = xcd_remap;
             p.tune.tb_rows = tb_rows;
             p.tune.tb_chunk_z = tb_chunk_z;
             p.tune.tb_nontemporal = tb_nontemporal;
             py::gil_scoped_release nogil;  // the 1/Cp scan synchronises the device
             return new Diffusion3DExecutor(P<double>(T), P<double>(T2), P<const double>(iCp), nx,
                                            ny, nz, p, halo);
           }),
           py::arg("T"), py::arg("T2"), py::arg("iCp"), py::arg("nx"), py::arg("ny"),
           py::arg("nz"), py::arg("mode"), py::arg("coef"), py::arg("halo").none(true) = nullptr,
           py::arg("overlaps") = std::array<int64_t, 3>{2, 2, 2},
           py::arg("halowidths") = std::array<int64_t, 3>{1, 1, 1},
           py::arg("steps_per_pass") = 1, py::arg("fast_math") = false,
           py::arg("b_width") = std::array<int64_t, 3>{16, 2, 2}, py::arg("xface") = 0,
           py::arg("uniform_factor") = true, py::arg("rows") = 4, py::arg("unroll") = 2,
           py::arg("vec") = 2, py::arg("nontemporal") = 3, py::arg("chunk_z") = 0,
           py::arg("xcd_remap") = 1, py::arg("tb_rows") = 0, py::arg("tb_chunk_z") = 0,
           py::arg("tb_nontemporal") = 0, py::arg("fused") = 0,
           py::arg("fused_timeout_s") = 60.0, py::keep_alive<1, 10>())
      .def(
          "run", [](Diffusion3DExecutor& e, int64_t n, uintptr_t s) { e.run(n, S(s)); },
          py::arg("nsteps"), py::arg("stream"), py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("parity", &Diffusion3DExecutor::parity)
      .def_property_readonly("uniform", &Diffusion3DExecutor::uniform)
      .def_property_readonly("uniform_value", &Diffusion3DExecutor::uniform_value)
      .def("rescan_factor", &Diffusion3DExecutor::rescan_factor,
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("steps_done", &Diffusion3DExecutor::steps_done)
      .def_property_readonly("passes_done", &Diffusion3DExecutor::passes_done)
      .def_property_readonly("fused_passes", &Diffusion3DExecutor::fused_passes)
      .def_property_readonly("fused_timeout_s", &Diffusion3DExecutor::fused_timeout_s)
      .def("check", &Diffusion3DExecutor::check)
      .def_property_readonly("frame_xface", &Diffusion3DExecutor::frame_xface)
      .def("plan", &Diffusion3DExecutor::plan, py::arg("nsteps"));

  // ---------------- tracing ----------------
  m.def("trace_enable", &trace_enable);
  m.def("trace_enabled", &trace_enabled);
  m.def("trace_push", [](const std::string& s) { trace_push(s.c_str()); });
  m.def("trace_pop", &trace_pop);
  m.def("trace_mark", [](const std::string& s) { trace_mark(s.c_str()); });
}
