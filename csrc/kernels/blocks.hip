// Batched strided 3D block copy (gfx950): one kernel for both directions of
// the C ABI's gather (rma/gather.h) and for the device crop of the reference
// scripts (Array(T[2:end-1,2:end-1]), scripts/diffusion_2D_ap.jl:45):
//  * pack : a strided view of a rank's field -> the dense send buffer;
//  * place: the root's rank-major staging -> every block at its Cartesian
//    position in A_global, all blocks in one launch (up to kCopyBlocksBatch).
//
// blockIdx.y selects the descriptor; descriptors travel by value (the style
// of Copy2dBatchArgs in misc.hip). 64-bit indexing; no division per element:
// a lane takes a fixed column once and strides over rows, keeping (y, z) of
// its row by addition. Rows narrower than half a block share the block
// between several rows; wider rows take kColsPerLane columns per lane, the
// loads issued before the stores, and the launch's cx column groups share a
// row. Plain C++ vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rma/hip_check.h"
#include "rma/kernels.h"

namespace rma {
namespace {

// 16 bytes as a native vector: the kColsPerLane values of a lane stay in registers
typedef uint32_t E16 __attribute__((ext_vector_type(4)));

struct CopyBlocksArgs {
  BlockCopy c[kCopyBlocksBatch];  // pitches and nx in elements of the launch's E
};
static_assert(sizeof(CopyBlocksArgs) <= 2560, "kernel arguments stay well under 4 KB");

constexpr int kBlock = 256;
constexpr int kColsPerLane = 4;
constexpr int kMaxBlocksX = 2048;  // per descriptor; rows are grid-strided beyond it

// gridDim.x = cx * nrg: block b works on column group b % cx of row group b / cx
template <typename E>
__global__ __launch_bounds__(kBlock) void copy_blocks_kernel(CopyBlocksArgs a, unsigned cx) {
  const BlockCopy c = a.c[blockIdx.y];
  const unsigned t = threadIdx.x;
  // lanes per row W and rows per block R of this descriptor
  const unsigned W = c.nx * 2 <= kBlock ? (unsigned)c.nx : (unsigned)kBlock;
  const unsigned R = kBlock / W;
  if (t >= R * W) return;
  const unsigned r0 = t / W, k0 = t - r0 * W;
  const unsigned rg = blockIdx.x / cx, cg = blockIdx.x - rg * cx, nrg = gridDim.x / cx;
  const int64_t rows = c.ny * c.nz;
  const int64_t step = (int64_t)nrg * R;
  int64_t row = (int64_t)rg * R + r0;
  if (row >= rows) return;
  // (y, z) of the lane's row: one division here, additions afterwards
  int64_t z = row / c.ny, y = row - z * c.ny;
  const int64_t sz = step / c.ny, sy = step - sz * c.ny;
  const int64_t kstep = (int64_t)kBlock * cx;
  const int64_t kbeg = (int64_t)cg * kBlock + k0;
  E* __restrict__ dst = static_cast<E*>(c.dst);
  const E* __restrict__ src = static_cast<const E*>(c.src);
  for (; row < rows; row += step) {
    const E* __restrict__ s = src + z * c.src_plane + y * c.src_row;
    E* __restrict__ d = dst + z * c.dst_plane + y * c.dst_row;
    for (int64_t k = kbeg; k < c.nx; k += kColsPerLane * kstep) {
      E v[kColsPerLane];
#pragma unroll
      for (int j = 0; j < kColsPerLane; ++j) {
        const int64_t kk = k + j * kstep;
        if (kk < c.nx) v[j] = s[kk];
      }
#pragma unroll
      for (int j = 0; j < kColsPerLane; ++j) {
        const int64_t kk = k + j * kstep;
        if (kk < c.nx) d[kk] = v[j];
      }
    }
    y += sy;
    z += sz;
    if (y >= c.ny) {
      y -= c.ny;
      ++z;
    }
  }
}

// 16-byte path: row length, both bases and every used pitch are multiples of 16 B
bool vec16_ok(const BlockCopy& c, int eb) {
  const int64_t per = 16 / eb;
  if (c.nx % per) return false;
  if ((reinterpret_cast<uintptr_t>(c.dst) | reinterpret_cast<uintptr_t>(c.src)) & 15) return false;
  if (c.ny > 1 && (c.dst_row % per || c.src_row % per)) return false;
  if (c.nz > 1 && (c.dst_plane % per || c.src_plane % per)) return false;
  return true;
}

void launch(const CopyBlocksArgs& a, int m, int elem_bytes, hipStream_t s) {
  // column groups per row: what the widest row can use at kColsPerLane columns
  // per lane; row groups: what the block with most rows can use, capped
  int64_t cx = 1, nrg = 1;
  for (int i = 0; i < m; ++i) {
    const BlockCopy& c = a.c[i];
    const int64_t rows = c.ny * c.nz;
    if (c.nx * 2 <= kBlock) {
      const int64_t R = kBlock / c.nx;
      nrg = std::max(nrg, (rows + R - 1) / R);
    } else {
      cx = std::max(cx, (c.nx + kBlock * kColsPerLane - 1) / (kBlock * kColsPerLane));
      nrg = std::max(nrg, rows);
    }
  }
  cx = std::min<int64_t>(cx, 16);
  nrg = std::min<int64_t>(nrg, std::max<int64_t>(1, kMaxBlocksX / cx));
  const dim3 grid((unsigned)(cx * nrg), (unsigned)m);
  switch (elem_bytes) {
    case 4: copy_blocks_kernel<uint32_t><<<grid, kBlock, 0, s>>>(a, (unsigned)cx); break;
    case 8: copy_blocks_kernel<uint64_t><<<grid, kBlock, 0, s>>>(a, (unsigned)cx); break;
    default: copy_blocks_kernel<E16><<<grid, kBlock, 0, s>>>(a, (unsigned)cx); break;
  }
  RMA_HIP_LAUNCH_CHECK();
}

}  // namespace

void copy_blocks_gpu(const BlockCopy* blocks, int64_t n, int elem_bytes, stream_t stream) {
  validate_block_copies(blocks, n, elem_bytes);
  hipStream_t s = as_stream(stream);
  CopyBlocksArgs a{};
  int m = 0;
  bool wide = false;  // path of the descriptors collected in `a`
  for (int64_t i = 0; i < n; ++i) {
    BlockCopy c = blocks[i];
    const bool w = vec16_ok(c, elem_bytes);
    // a launch holds descriptors of one path, at most kCopyBlocksBatch of them
    if (m > 0 && (w != wide || m == kCopyBlocksBatch)) {
      launch(a, m, wide ? 16 : elem_bytes, s);
      m = 0;
    }
    wide = w;
    if (w) {
      const int64_t per = 16 / elem_bytes;
      c.nx /= per;
      c.dst_row /= per;
      c.src_row /= per;
      c.dst_plane /= per;
      c.src_plane /= per;
    }
    // pitches along an extent of 1 are never used: keep them out of the kernel
    if (c.ny == 1) c.dst_row = c.src_row = 0;
    if (c.nz == 1) c.dst_plane = c.src_plane = 0;
    a.c[m++] = c;
  }
  if (m > 0) launch(a, m, wide ? 16 : elem_bytes, s);
}

}  // namespace rma
