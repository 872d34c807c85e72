"""``ops.hide_boxes3d``: the frame / interior split of a 3D pass. The boxes tile
the owned box exactly once, the send planes of every neighbour side lie in the
frame, at most six frame boxes, the degenerate returns and the refusals."""
import itertools

import numpy as np
import pytest

from rocm_mpi_amd import ops

B_WIDTHS = [(1, 1, 1), (2, 2, 2), (16, 2, 2), (3, 5, 4)]
# {9..14}^3 subsampled: every size in every dimension, mixed among the dimensions
SIZES = [(9, 9, 9), (10, 12, 14), (11, 13, 9), (12, 14, 10), (13, 9, 11), (14, 10, 12),
         (14, 14, 14)]
SIDES = list(itertools.product((False, True), repeat=6))  # every subset of neighbour sides


def owned_box(n, sides, k):
    """Diffusion3D.owned_box(k) of a rank with these neighbour sides."""
    box = []
    for d in range(3):
        box += [k if sides[d][0] else 1, n[d] - (k if sides[d][1] else 1)]
    return tuple(box)


def mark(cover, b):
    x0, x1, y0, y1, z0, z1 = b
    assert x0 < x1 and y0 < y1 and z0 < z1, f"empty box {b} returned"
    cover[z0:z1, y0:y1, x0:x1] += 1


@pytest.mark.parametrize("ol", [2, 4])
@pytest.mark.parametrize("bw", B_WIDTHS)
def test_boxes_tile_the_owned_box_and_hold_the_send_planes(bw, ol):
    k = hw = ol // 2
    for n, flat in itertools.product(SIZES, SIDES):
        sides = [flat[0:2], flat[2:4], flat[4:6]]
        own = owned_box(n, sides, k)
        frame, inner = ops.hide_boxes3d(n, own, sides, (ol,) * 3, bw)
        assert len(frame) <= 6
        cover = np.zeros(n[::-1], dtype=np.int32)
        fr = np.zeros(n[::-1], dtype=np.int32)
        for b in frame:
            mark(cover, b)
            mark(fr, b)
        if inner is not None:
            mark(cover, inner)
        want = np.zeros(n[::-1], dtype=np.int32)
        want[own[4]:own[5], own[2]:own[3], own[0]:own[1]] = 1
        assert np.array_equal(cover, want), (n, sides, bw, ol)  # each owned cell once, none outside
        # degenerate returns
        if not any(flat):
            assert frame == [] and inner == own
            continue
        lo_hi = []
        for d in range(3):
            m = max(bw[d], ol)
            lo_hi.append((m if sides[d][0] else own[2 * d],
                          n[d] - m if sides[d][1] else own[2 * d + 1]))
        if any(hi <= lo for lo, hi in lo_hi):
            assert frame == [own] and inner is None
        else:
            assert inner == tuple(v for p in lo_hi for v in p)
            # the slabs' extents: z over the owned x-y extent, y over the inner z range,
            # x over the inner y and z range
            for b in frame:
                if (b[4], b[5]) != lo_hi[2]:
                    assert b[:4] == own[:4]
                elif (b[2], b[3]) != lo_hi[1]:
                    assert b[:2] == own[:2]
                else:
                    assert (b[2], b[3]) == lo_hi[1] and (b[4], b[5]) == lo_hi[2]
        # the owned part of the send planes [ol-hw, ol) and [n-ol, n-ol+hw) is frame
        for d in range(3):
            for s, (a, b_) in enumerate(((ol - hw, ol), (n[d] - ol, n[d] - ol + hw))):
                if not sides[d][s]:
                    continue
                sl = [slice(None)] * 3
                sl[2 - d] = slice(a, b_)
                sl = tuple(sl)
                assert np.array_equal(fr[sl], want[sl]), (n, sides, bw, ol, d, s)


def test_refusals():
    n, own, sides = (12, 12, 12), (1, 11, 1, 11, 1, 11), [(True, True)] * 3
    for bw in [(0, 1, 1), (1, -2, 1), (1, 1, 0)]:
        with pytest.raises(ValueError, match="b_width >= 1"):
            ops.hide_boxes3d(n, own, sides, (2, 2, 2), bw)
    with pytest.raises(ValueError, match="three dimensions"):
        ops.hide_boxes3d(n, own, sides, (2, 2, 2), (1, 1))
    with pytest.raises(ValueError, match="three dimensions"):
        ops.hide_boxes3d((12, 12), own, sides, (2, 2, 2), (1, 1, 1))


def test_the_reference_example_split():
    """b_width (16, 2, 2) on a 64^3 tile with neighbours on every side, overlap 2."""
    frame, inner = ops.hide_boxes3d((64, 64, 64), (1, 63, 1, 63, 1, 63), [(True, True)] * 3,
                                    (2, 2, 2), (16, 2, 2))
    assert inner == (16, 48, 2, 62, 2, 62)
    assert frame == [(1, 63, 1, 63, 1, 2), (1, 63, 1, 63, 62, 63), (1, 63, 1, 2, 2, 62),
                     (1, 63, 62, 63, 2, 62), (1, 16, 2, 62, 2, 62), (48, 63, 2, 62, 2, 62)]
