// Host-only geometry of the 3D diffusion passes (no HIP): the box a K-step pass
// owns and perf_hide's split of it into a boundary frame and an interior box.
// The rule is that of the Python model (ops.hide_boxes3d, Diffusion3D.owned_box),
// which tests/test_plan3d_cpu.py compares case by case; a HIP-free translation
// unit so that a sanitizer build runs it (tests/native/plan3d_selftest.cpp).
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "rma/common.h"
#include "rma/plan.h"  // Neighbors

namespace rma {

// Cells a K-step pass writes on an (nz, ny, nx) tile, n = {nx, ny, nz}: next to
// a neighbour the K cells [0,K) are halo (the exchange refreshes them),
// elsewhere the fixed boundary cell 0 stays.
Box owned_box3d(const std::array<int64_t, 3>& n, const Neighbors& nbr, int K);

using Sides3 = std::array<std::array<bool, 2>, 3>;  // (dim, lo/hi) -> has a neighbour
Sides3 sides3d(const Neighbors& nbr);

struct HideBoxes3 {
  std::vector<Box> frame;  // at most six disjoint slabs, computed ahead of the exchange
  Box interior{};          // valid when has_interior
  bool has_interior = false;
  // a frame AND an interior: the pass can overlap its exchange with the interior
  bool split() const { return has_interior && !frame.empty(); }
};

// Frame / interior split of `owned` (ImplicitGlobalGrid's @hide_communication
// with boundary width b_width[d] >= 1, counted from the array edge). On a side
// with a neighbour the interior starts max(b_width[d], overlaps[d]) cells in, so
// the send planes [ol-hw, ol) and [n-ol, n-ol+hw) lie in the frame; a side
// without a neighbour has no slab and the interior reaches the owned bound.
// Slabs: z over the full owned x-y extent, y over the interior's z range, x
// over the interior's y and z range; empty slabs are dropped. An interior empty
// in some dimension gives frame = {owned} and no interior ("no split"); no
// neighbour at all gives no frame and interior = owned.
HideBoxes3 hide_boxes3d(const std::array<int64_t, 3>& n, const Box& owned, const Sides3& sides,
                        const std::array<int64_t, 3>& overlaps,
                        const std::array<int64_t, 3>& b_width);

}  // namespace rma
