// Stand-alone self test of the 3D pass geometry (csrc/runtime/plan3d.cpp) and of
// the launchers' box split (split_boxes3d, csrc/kernels/kernel_select.cpp), built
// with -fsanitize=address,undefined by tests/test_plan3d_host_sanitized_cpu.py.
// The hand cases of tests/test_plan3d_cpu.py plus a sweep of small tiles; every
// split is checked as a partition of the owned box on a cell count array.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rma/kernels.h"
#include "rma/plan3d.h"

using namespace rma;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static bool same(const Box& a, const Box& b) {
  return a.x0 == b.x0 && a.x1 == b.x1 && a.y0 == b.y0 && a.y1 == b.y1 && a.z0 == b.z0 &&
         a.z1 == b.z1;
}

// frame + interior == owned, no cell twice
static void check_partition(const std::array<int64_t, 3>& n, const Box& own, const HideBoxes3& h) {
  std::vector<int> cnt((size_t)(n[0] * n[1] * n[2]), 0);
  auto add = [&](const Box& b, int v) {
    CHECK(!b.empty());
    CHECK(b.x0 >= 0 && b.y0 >= 0 && b.z0 >= 0 && b.x1 <= n[0] && b.y1 <= n[1] && b.z1 <= n[2]);
    for (int64_t z = b.z0; z < b.z1; ++z)
      for (int64_t y = b.y0; y < b.y1; ++y)
        for (int64_t x = b.x0; x < b.x1; ++x) cnt[(size_t)((z * n[1] + y) * n[0] + x)] += v;
  };
  for (const Box& b : h.frame) add(b, 1);
  add(h.interior, 1);
  add(own, -1);
  for (int c : cnt) CHECK(c == 0);
}

int main() {
  const Neighbors all{{{0, 0}, {0, 0}, {0, 0}}}, none{{{-1, -1}, {-1, -1}, {-1, -1}}};
  {  // no neighbour: no frame, the owned box is the interior
    const std::array<int64_t, 3> n{20, 12, 9};
    const Box own = owned_box3d(n, none, 1);
    CHECK(same(own, Box{1, 19, 1, 11, 1, 8}));
    const HideBoxes3 h = hide_boxes3d(n, own, sides3d(none), {2, 2, 2}, {16, 2, 2});
    CHECK(h.frame.empty() && h.has_interior && same(h.interior, own) && !h.split());
  }
  // interior empty in one dimension: no split
  for (const std::array<int64_t, 3>& n :
       {std::array<int64_t, 3>{20, 13, 9}, {130, 4, 9}, {130, 13, 8}}) {
    const Box own = owned_box3d(n, all, 2);
    const HideBoxes3 h = hide_boxes3d(n, own, sides3d(all), {4, 4, 4}, {16, 2, 2});
    CHECK(!h.has_interior && h.frame.size() == 1 && same(h.frame[0], own) && !h.split());
  }
  {  // b_width below the overlap: the interior starts at the overlap
    const std::array<int64_t, 3> n{130, 13, 9};
    const Box own = owned_box3d(n, all, 2);
    CHECK(same(own, Box{2, 128, 2, 11, 2, 7}));
    HideBoxes3 h = hide_boxes3d(n, own, sides3d(all), {4, 4, 4}, {1, 1, 1});
    CHECK(h.split() && h.frame.size() == 6 && same(h.interior, Box{4, 126, 4, 9, 4, 5}));
    check_partition(n, own, h);
    h = hide_boxes3d(n, own, sides3d(all), {4, 4, 4}, {16, 2, 2});
    CHECK(h.split() && same(h.interior, Box{16, 114, 4, 9, 4, 5}));
    check_partition(n, own, h);
  }
  // every subset of the six sides on small tiles, both overlaps, a few widths
  int splits = 0;
  for (int mask = 0; mask < 64; ++mask) {
    Neighbors nb = none;
    for (int d = 0; d < 3; ++d)
      for (int s = 0; s < 2; ++s)
        if (mask >> (2 * d + s) & 1) nb[d][s] = 0;
    for (int K = 1; K <= 2; ++K)
      for (int64_t nx : {3, 9, 14, 40})
        for (int64_t bw : {1, 3, 7, 20}) {
          const std::array<int64_t, 3> n{nx, 11, 10};
          const Box own = owned_box3d(n, nb, K);
          const HideBoxes3 h =
              hide_boxes3d(n, own, sides3d(nb), {2 * K, 2 * K, 2 * K}, {bw, 2, 3});
          CHECK(h.frame.size() <= 6);
          if (!h.split()) continue;
          ++splits;
          check_partition(n, own, h);
        }
  }
  CHECK(splits > 100);
  bool refused = false;
  try {
    (void)hide_boxes3d({9, 9, 9}, Box{1, 8, 1, 8, 1, 8}, sides3d(all), {2, 2, 2}, {2, 0, 2});
  } catch (const Error&) {
    refused = true;
  }
  CHECK(refused);
  {  // split_boxes3d: empty, thin, march and the three face classes; every list
     // keeps the input order, which fixes the launch order
    const Box in[8] = {{1, 7, 1, 5, 1, 5},    {2, 2, 1, 5, 1, 5},    {1, 34, 1, 5, 1, 5},
                       {3, 17, 1, 5, 1, 5},   {4, 34, 2, 5, 1, 5},   {5, 11, 1, 5, 1, 5},
                       {6, 39, 1, 5, 1, 5},   {7, 21, 1, 5, 1, 5}};  // widths 6 0 33 14 30 6 33 14
    auto is = [&](const Box& b, int i) { return same(b, in[i]); };
    Stencil3DTuning tn;
    Split3D s = split_boxes3d(1, in, 8, tn);  // xface = 0: widths up to 8 thin, the rest march
    CHECK(!s.faces() && s.nwide == 7);
    const int w0[7] = {0, 2, 3, 4, 5, 6, 7};
    for (int i = 0; i < 7; ++i) CHECK(is(s.wide[i], w0[i]) && s.thin[i] == (w0[i] == 0 || w0[i] == 5));
    tn.xface = 32;
    s = split_boxes3d(1, in, 8, tn);  // K = 1: 6 -> 8 lanes, 14 -> 16, 30 -> 32, 33 marches
    CHECK(s.nwide == 2 && is(s.wide[0], 2) && is(s.wide[1], 6) && !s.thin[0] && !s.thin[1]);
    CHECK(s.nface[0] == 2 && is(s.face[0][0], 0) && is(s.face[0][1], 5));
    CHECK(s.nface[1] == 2 && is(s.face[1][0], 3) && is(s.face[1][1], 7));
    CHECK(s.nface[2] == 1 && is(s.face[2][0], 4));
    s = split_boxes3d(2, in, 8, tn);  // K = 2 needs W + 2 lanes: the same classes
    CHECK(s.nwide == 2 && is(s.wide[0], 2) && is(s.wide[1], 6) && !s.thin[0] && !s.thin[1]);
    CHECK(s.nface[0] == 2 && is(s.face[0][0], 0) && is(s.face[0][1], 5));
    CHECK(s.nface[1] == 2 && is(s.face[1][0], 3) && is(s.face[1][1], 7));
    CHECK(s.nface[2] == 1 && is(s.face[2][0], 4));
    tn.xface = 14;
    s = split_boxes3d(2, in, 8, tn);  // width 30 is past xface: it marches, no thin path at K = 2
    CHECK(s.nwide == 3 && is(s.wide[0], 2) && is(s.wide[1], 4) && is(s.wide[2], 6));
    CHECK(!s.thin[0] && !s.thin[1] && !s.thin[2] && s.nface[0] == 2 && s.nface[1] == 2 && !s.nface[2]);
  }
  std::printf("plan3d selftest OK (%d splits)\n", splits);
  return 0;
}
