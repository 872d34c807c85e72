// ImplicitGlobalGrid gather!: the root assembles every rank's block at its
// Cartesian coordinates (reference scripts/diffusion_2D_ap.jl:31-34,45-47:
// T_v of size dims .* size(T_nh), gather!(T_nh, T_v)).
//
// Two parts:
//  * plan_gather (gather.cpp, host-only, no HIP): where every rank's block
//    sits in A_global. Coordinates come from CartTopology, the same ordering
//    update_halo uses, so the two cannot drift apart.
//  * gather_blocks (gather_blocks.cpp): the collective itself over RCCL
//    send/recv, with the strided block-copy kernel (kernels.h copy_blocks_gpu)
//    for the pack on the senders and the placement on the root.
//
// Layout: x fastest; A is (nz, ny, nx) row-major, A_global is
// (dims[2]*nz, dims[1]*ny, dims[0]*nx). Every rank passes the same size_A
// (the precondition of IGG's gather!).
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rma/kernels.h"
#include "rma/topology.h"

namespace rma {

struct GatherPlan {
  int nprocs = 1;
  int elem_bytes = 8;
  std::array<int64_t, 3> size_A{1, 1, 1};   // nx, ny, nz of one block
  std::array<int64_t, 3> size_g{1, 1, 1};   // dims .* size_A
  int64_t row_pitch_g = 1, plane_pitch_g = 1;  // of A_global, in elements
  int64_t block_elems = 1, total_elems = 1;
  std::vector<std::array<int, 3>> coords;   // of rank r (CartTopology::coords)
  std::vector<int64_t> offset;              // element offset of rank r's block in A_global
  // every block is ONE contiguous byte range of A_global (the root can then
  // receive in place): a block is a single row, or blocks span whole global
  // rows (dims[0] == 1) and are one plane deep or span whole planes
  // (size_A[2] == 1 or dims[1] == 1)
  bool contiguous_in_global = true;
};

GatherPlan plan_gather(const std::array<int, 3>& dims, const std::array<int64_t, 3>& size_A,
                       int elem_bytes);

class RcclComm;

// Device buffers of the gather, owned by the grid: grown on demand at the
// start of a call (the previous call ended with a completed wait), released
// with the grid.
struct GatherBuffers {
  void* send = nullptr;      // dense copy of a strided or host source
  void* stage = nullptr;     // root: rank-major blocks before the placement
  void* assembled = nullptr; // root: A_global on the device when the caller's is host memory
  size_t send_bytes = 0, stage_bytes = 0, assembled_bytes = 0;
  std::vector<char> host_pack;  // dense copy of a strided host source
  bool in_flight = false;    // a call enqueued work and its wait did not complete
  void release();
  ~GatherBuffers() { release(); }
};

// Collective and blocking. comm == nullptr: a single-rank grid (same path
// without send / receive). A / A_global may each be device or host memory
// (classified with hipPointerGetAttributes); A_global may be null off-root.
// pitch_A = {row pitch, plane pitch} in elements, nullptr = dense. RCCL is
// only handed device memory: the caller's device pointers or `buf`. Every
// argument is checked before anything is enqueued or sent. On return (after
// the communicator's bounded wait of timeout_s on `stream`) A_global is
// complete on the root and every rank may reuse A.
void gather_blocks(RcclComm* comm, const GridDesc& grid, double timeout_s, GatherBuffers& buf,
                   const void* A, const int64_t size_A[3], const int64_t pitch_A[2],
                   int elem_bytes, void* A_global, int root, stream_t stream);

}  // namespace rma
