// Geometry of the 3D diffusion passes (see rma/plan3d.h). Host only.
#include "rma/plan3d.h"

#include <algorithm>

namespace rma {

Box owned_box3d(const std::array<int64_t, 3>& n, const Neighbors& nbr, int K) {
  RMA_CHECK_ARG(K >= 1, "pass depth " << K);
  int64_t b[6];
  for (int d = 0; d < 3; ++d) {
    RMA_CHECK_ARG(n[d] >= 3, "tile extent " << n[d] << " along dim " << d << " (>= 3)");
    b[2 * d] = nbr[d][0] >= 0 ? K : 1;
    b[2 * d + 1] = n[d] - (nbr[d][1] >= 0 ? K : 1);
  }
  return {b[0], b[1], b[2], b[3], b[4], b[5]};
}

Sides3 sides3d(const Neighbors& nbr) {
  Sides3 s{};
  for (int d = 0; d < 3; ++d)
    for (int k = 0; k < 2; ++k) s[d][k] = nbr[d][k] >= 0;
  return s;
}

HideBoxes3 hide_boxes3d(const std::array<int64_t, 3>& n, const Box& owned, const Sides3& sides,
                        const std::array<int64_t, 3>& overlaps,
                        const std::array<int64_t, 3>& b_width) {
  for (int d = 0; d < 3; ++d)
    RMA_CHECK_ARG(b_width[d] >= 1, "b_width[" << d << "] = " << b_width[d] << " (>= 1)");
  HideBoxes3 out;
  bool any = false;
  for (int d = 0; d < 3; ++d) any = any || sides[d][0] || sides[d][1];
  if (!any) {
    out.interior = owned;
    out.has_interior = true;
    return out;
  }
  const int64_t own[6] = {owned.x0, owned.x1, owned.y0, owned.y1, owned.z0, owned.z1};
  int64_t in[6];
  for (int d = 0; d < 3; ++d) {
    int64_t lo = own[2 * d], hi = own[2 * d + 1];
    const int64_t m = std::max(b_width[d], overlaps[d]);
    if (sides[d][0]) lo = std::max(lo, m);
    if (sides[d][1]) hi = std::min(hi, n[d] - m);
    if (hi <= lo) {  // nothing to overlap the exchange with
      out.frame.push_back(owned);
      return out;
    }
    in[2 * d] = lo;
    in[2 * d + 1] = hi;
  }
  const Box slabs[6] = {{own[0], own[1], own[2], own[3], own[4], in[4]},
                        {own[0], own[1], own[2], own[3], in[5], own[5]},
                        {own[0], own[1], own[2], in[2], in[4], in[5]},
                        {own[0], own[1], in[3], own[3], in[4], in[5]},
                        {own[0], in[0], in[2], in[3], in[4], in[5]},
                        {in[1], own[1], in[2], in[3], in[4], in[5]}};
  for (const Box& b : slabs)
    if (!b.empty()) out.frame.push_back(b);
  out.interior = {in[0], in[1], in[2], in[3], in[4], in[5]};
  out.has_interior = true;
  return out;
}

}  // namespace rma
