// The IGG-style gather over RCCL send/recv (rma/gather.h).
//
// Sender: a dense device source is sent as it is; a strided device source is
// packed by the block-copy kernel into the grid's send buffer; a host source
// is copied there (a strided one packed on the CPU first). Root: all receives
// in one RCCL group; when every block is one contiguous range of A_global
// they land in place (no staging, no kernel), otherwise rank-major in the
// grid's staging and ONE placement pass of the block-copy kernel moves them to
// their Cartesian positions. A host A_global is assembled on the device and
// leaves with one copy. RCCL never sees a host pointer.
#include "rma/gather.h"

#include <hip/hip_runtime.h>

#include <cstring>

#include "rma/comm.h"
#include "rma/config.h"
#include "rma/hip_check.h"

namespace rma {

namespace {

// device memory only; an unknown pointer (the error return: plain malloc /
// a Julia Array), unregistered and pinned host memory are all host
bool is_device_pointer(const void* p) {
  hipPointerAttribute_t a{};
  const hipError_t e = hipPointerGetAttributes(&a, p);
  (void)hipGetLastError();  // an unknown pointer leaves a sticky error behind
  if (e != hipSuccess) return false;
  return a.type == hipMemoryTypeDevice;
}

void grow(void*& p, size_t& have, size_t want) {
  if (have >= want) return;
  if (p) RMA_HIP_CHECK(hipFree(p));
  p = nullptr;
  have = 0;
  RMA_HIP_CHECK(hipMalloc(&p, want));
  have = want;
}

}  // namespace

void GatherBuffers::release() {
  // hipFree waits for the device, so work a failed call left behind is over
  if (send) (void)hipFree(send);
  if (stage) (void)hipFree(stage);
  if (assembled) (void)hipFree(assembled);
  send = stage = assembled = nullptr;
  send_bytes = stage_bytes = assembled_bytes = 0;
  host_pack.clear();
  host_pack.shrink_to_fit();
  in_flight = false;
}

void gather_blocks(RcclComm* comm, const GridDesc& grid, double timeout_s, GatherBuffers& buf,
                   const void* A, const int64_t size_A[3], const int64_t pitch_A[2],
                   int elem_bytes, void* A_global, int root, stream_t stream) {
  // ---- every refusal comes before anything is enqueued or sent ----
  RMA_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8,
                "gather: unsupported elem_bytes " << elem_bytes << " (4 or 8)");
  RMA_CHECK_ARG(size_A != nullptr, "gather: size_A is NULL");
  for (int d = 0; d < 3; ++d)
    RMA_CHECK_ARG(size_A[d] > 0, "gather: size_A[" << d << "] = " << size_A[d] << " (must be > 0)");
  RMA_CHECK_ARG(A != nullptr, "gather: A is NULL");
  RMA_CHECK_ARG(root >= 0 && root < grid.nprocs,
                "gather: root " << root << " out of range (nprocs " << grid.nprocs << ")");
  const int64_t nx = size_A[0], ny = size_A[1], nz = size_A[2];
  const int64_t row = pitch_A ? pitch_A[0] : nx;
  const int64_t plane = pitch_A ? pitch_A[1] : nx * ny;
  if (pitch_A) {
    RMA_CHECK_ARG(row >= nx, "gather: pitch_A[0] = " << row << " smaller than nx = " << nx);
    RMA_CHECK_ARG(nz == 1 || plane >= (ny - 1) * row + nx,
                  "gather: pitch_A[1] = " << plane << " smaller than a plane of " << ny
                                          << " rows at pitch_A[0] = " << row);
  }
  const bool is_root = grid.me == root;
  RMA_CHECK_ARG(!is_root || A_global != nullptr, "gather: A_global is NULL on the root");
  const GatherPlan plan = plan_gather(grid.dims, {nx, ny, nz}, elem_bytes);
  const double max_bytes =
      env_double("RMA_GATHER_MAX_BYTES", (double)(8ull << 30), 1.0, 9.0e18);
  const double total_bytes = (double)plan.total_elems * elem_bytes;
  RMA_CHECK_ARG(total_bytes <= max_bytes,
                "gather: A_global would hold " << total_bytes << " bytes, more than "
                                               << "RMA_GATHER_MAX_BYTES = " << max_bytes);
  RMA_CHECK_ARG(!buf.in_flight, "gather: an earlier gather on this grid did not complete");
  RMA_CHECK_ARG(comm != nullptr || grid.nprocs == 1, "gather: no communicator");

  hipStream_t s = as_stream(stream);
  const size_t eb = (size_t)elem_bytes;
  const size_t block_bytes = (size_t)plan.block_elems * eb;
  const bool dense = (ny == 1 || row == nx) && (nz == 1 || plane == nx * ny);
  const bool a_dev = is_device_pointer(A);
  const bool g_dev = is_root && is_device_pointer(A_global);

  // the dense host image of a strided host source
  const void* host_src = A;
  if (!a_dev && !dense) {
    buf.host_pack.resize(block_bytes);
    const BlockCopy c{buf.host_pack.data(), A, nx, nx * ny, row, plane, nx, ny, nz};
    copy_blocks_cpu(&c, 1, elem_bytes);
    host_src = buf.host_pack.data();
  }

  // buffers grow before anything is enqueued (nothing of an earlier call is pending)
  if (!is_root && (!a_dev || !dense)) grow(buf.send, buf.send_bytes, block_bytes);
  if (is_root && !plan.contiguous_in_global)
    grow(buf.stage, buf.stage_bytes, block_bytes * (size_t)plan.nprocs);
  if (is_root && !g_dev)
    grow(buf.assembled, buf.assembled_bytes, block_bytes * (size_t)plan.nprocs);

  buf.in_flight = true;
  if (!is_root) {
    const void* sendp = A;
    if (!a_dev) {
      RMA_HIP_CHECK(hipMemcpyAsync(buf.send, host_src, block_bytes, hipMemcpyHostToDevice, s));
      sendp = buf.send;
    } else if (!dense) {
      const BlockCopy c{buf.send, A, nx, nx * ny, row, plane, nx, ny, nz};
      copy_blocks_gpu(&c, 1, elem_bytes, stream);
      sendp = buf.send;
    }
    comm->group_start();
    comm->send(sendp, block_bytes, root, stream);
    comm->group_end();
  } else {
    char* out = static_cast<char*>(g_dev ? A_global : buf.assembled);
    const bool in_place = plan.contiguous_in_global;
    char* stage = static_cast<char*>(buf.stage);
    auto slot = [&](int r) {  // where rank r's block is received
      return in_place ? out + (size_t)plan.offset[r] * eb : stage + (size_t)r * block_bytes;
    };
    // the root's own block: a host source goes to its slot like a received
    // one; a device source is copied (in place) or joins the placement pass
    std::vector<BlockCopy> place;
    auto placed = [&](int r, const void* src, int64_t srow, int64_t splane) {
      return BlockCopy{out + (size_t)plan.offset[r] * eb, src, plan.row_pitch_g,
                       plan.plane_pitch_g, srow, splane, nx, ny, nz};
    };
    if (!a_dev) {
      RMA_HIP_CHECK(hipMemcpyAsync(slot(root), host_src, block_bytes, hipMemcpyHostToDevice, s));
      if (!in_place) place.push_back(placed(root, slot(root), nx, nx * ny));
    } else if (in_place && dense) {
      RMA_HIP_CHECK(hipMemcpyAsync(slot(root), A, block_bytes, hipMemcpyDeviceToDevice, s));
    } else {
      place.push_back(placed(root, A, row, plane));
    }
    if (plan.nprocs > 1) {
      comm->group_start();
      for (int r = 0; r < plan.nprocs; ++r)
        if (r != root) comm->recv(slot(r), block_bytes, r, stream);
      comm->group_end();
    }
    if (!in_place)
      for (int r = 0; r < plan.nprocs; ++r)
        if (r != root) place.push_back(placed(r, slot(r), nx, nx * ny));
    if (!place.empty()) copy_blocks_gpu(place.data(), (int64_t)place.size(), elem_bytes, stream);
    if (!g_dev)
      RMA_HIP_CHECK(hipMemcpyAsync(A_global, out, block_bytes * (size_t)plan.nprocs,
                                   hipMemcpyDeviceToHost, s));
  }
  if (comm)
    comm->wait(stream, timeout_s);
  else
    RMA_HIP_CHECK(hipStreamSynchronize(s));
  buf.in_flight = false;
}

}  // namespace rma
