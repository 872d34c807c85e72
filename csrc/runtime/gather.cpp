// Host-only plan of the IGG-style gather (rma/gather.h): no HIP, no RCCL.
#include "rma/gather.h"

#include "rma/common.h"

namespace rma {

GatherPlan plan_gather(const std::array<int, 3>& dims, const std::array<int64_t, 3>& size_A,
                       int elem_bytes) {
  RMA_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8,
                "gather: unsupported elem_bytes " << elem_bytes << " (4 or 8)");
  for (int d = 0; d < 3; ++d) {
    RMA_CHECK_ARG(dims[d] >= 1, "gather: dims[" << d << "] = " << dims[d]);
    RMA_CHECK_ARG(size_A[d] >= 1, "gather: size_A[" << d << "] = " << size_A[d]);
  }
  GatherPlan p;
  p.nprocs = dims[0] * dims[1] * dims[2];
  p.elem_bytes = elem_bytes;
  p.size_A = size_A;
  for (int d = 0; d < 3; ++d) p.size_g[d] = (int64_t)dims[d] * size_A[d];
  p.row_pitch_g = p.size_g[0];
  p.plane_pitch_g = p.size_g[0] * p.size_g[1];
  p.block_elems = size_A[0] * size_A[1] * size_A[2];
  p.total_elems = p.block_elems * p.nprocs;
  const CartTopology topo(p.nprocs, dims, {0, 0, 0});
  p.coords.resize(p.nprocs);
  p.offset.resize(p.nprocs);
  for (int r = 0; r < p.nprocs; ++r) {
    const std::array<int, 3> c = topo.coords(r);
    p.coords[r] = c;
    p.offset[r] = (int64_t)c[2] * size_A[2] * p.plane_pitch_g +
                  (int64_t)c[1] * size_A[1] * p.row_pitch_g + (int64_t)c[0] * size_A[0];
  }
  p.contiguous_in_global = (size_A[1] == 1 && size_A[2] == 1) ||
                           (dims[0] == 1 && (dims[1] == 1 || size_A[2] == 1));
  return p;
}

}  // namespace rma
