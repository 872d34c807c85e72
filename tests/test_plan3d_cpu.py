"""The C++ frame / interior split of the 3D passes (csrc/runtime/plan3d.cpp,
bound as ``_C.owned_box3d`` / ``_C.hide_boxes3d``) against the Python model's
rule (``ops.hide_boxes3d``, ``Diffusion3D.owned_box``): 200 seeded random cases
and the hand cases, and for every case with a frame and an interior the
partition property: frame + interior is the owned box, pairwise disjoint."""
import itertools
import random

import numpy as np
import pytest

from rocm_mpi_amd import ops
from rocm_mpi_amd._native import native


def owned_rule(n, nb, k):
    """Diffusion3D.owned_box: next to a neighbour the k cells [0,k) are halo."""
    box = []
    for d in (0, 1, 2):
        box += [k if nb[d][0] >= 0 else 1, n[d] - (k if nb[d][1] >= 0 else 1)]
    return tuple(box)


def both(n, nb, k, ol, bw):
    """(frame, inner) of the C++ twin after it agreed with the Python rule."""
    own = owned_rule(n, nb, k)
    assert tuple(native().owned_box3d(list(n), [list(p) for p in nb], k)) == own
    sides = [(nb[d][0] >= 0, nb[d][1] >= 0) for d in (0, 1, 2)]
    want_frame, want_inner = ops.hide_boxes3d(n, own, sides, ol, bw)
    frame, inner = native().hide_boxes3d(list(n), own, sides, list(ol), list(bw))
    assert [tuple(b) for b in frame] == [tuple(b) for b in want_frame]
    assert (None if inner is None else tuple(inner)) == want_inner
    assert len(frame) <= 6
    return own, [tuple(b) for b in frame], None if inner is None else tuple(inner)


def check_partition(n, own, frame, inner):
    """frame + interior == owned, no cell twice (counted on the whole tile)."""
    cnt = np.zeros((n[2], n[1], n[0]), dtype=np.int32)
    for x0, x1, y0, y1, z0, z1 in frame + [inner]:
        assert x0 < x1 and y0 < y1 and z0 < z1
        cnt[z0:z1, y0:y1, x0:x1] += 1
    want = np.zeros_like(cnt)
    want[own[4]:own[5], own[2]:own[3], own[0]:own[1]] = 1
    assert np.array_equal(cnt, want)


def cases():
    rng = random.Random(20260)
    out = []
    for _ in range(200):
        n = tuple(rng.randint(3, 40) for _ in range(3))
        nb = tuple(tuple(rng.choice((-1, 0)) for _ in range(2)) for _ in range(3))
        o = rng.choice((2, 4))
        bw = tuple(rng.randint(1, 20) for _ in range(3))
        out.append((n, nb, o // 2, (o, o, o), bw))
    return out


def test_random_cases_agree_with_the_python_rule_and_partition_the_owned_box():
    split = 0
    for n, nb, k, ol, bw in cases():
        own, frame, inner = both(n, nb, k, ol, bw)
        if frame and inner is not None:
            split += 1
            check_partition(n, own, frame, inner)
    assert split >= 20  # the random cases do reach the split


ALL = ((0, 0), (0, 0), (0, 0))
NONE = ((-1, -1), (-1, -1), (-1, -1))


def test_no_neighbour_gives_no_frame_and_the_owned_interior():
    own, frame, inner = both((20, 12, 9), NONE, 1, (2, 2, 2), (16, 2, 2))
    assert frame == [] and inner == own == (1, 19, 1, 11, 1, 8)


@pytest.mark.parametrize("n", [(20, 13, 9), (130, 4, 9), (130, 13, 8)])
def test_interior_empty_in_one_dimension_gives_no_split(n):
    # b_width (16, 2, 2) at overlap 4: x needs n > 32, y and z n > 8
    own, frame, inner = both(n, ALL, 2, (4, 4, 4), (16, 2, 2))
    assert inner is None and frame == [own]


def test_b_width_below_the_overlap_starts_at_the_overlap():
    n = (130, 13, 9)
    own, frame, inner = both(n, ALL, 2, (4, 4, 4), (1, 1, 1))
    assert inner == (4, 126, 4, 9, 4, 5) and len(frame) == 6
    check_partition(n, own, frame, inner)
    own, frame, inner = both(n, ALL, 2, (4, 4, 4), (16, 2, 2))
    assert inner == (16, 114, 4, 9, 4, 5)
    check_partition(n, own, frame, inner)


@pytest.mark.parametrize("nb", list(itertools.product(((-1, -1), (0, -1), (-1, 0), (0, 0)),
                                                      repeat=3)))
def test_every_subset_of_the_six_sides(nb):
    n = (40, 11, 10)
    own, frame, inner = both(n, nb, 1, (2, 2, 2), (3, 2, 4))
    sides = sum(p >= 0 for pair in nb for p in pair)
    assert len(frame) == sides and inner is not None  # a slab per side with a neighbour
    if frame:
        check_partition(n, own, frame, inner)


def test_a_bad_b_width_is_refused():
    with pytest.raises(RuntimeError, match="b_width"):
        native().hide_boxes3d([9, 9, 9], (1, 8, 1, 8, 1, 8), [(True, True)] * 3, [2, 2, 2],
                              [2, 0, 2])
