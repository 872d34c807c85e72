"""Block -> (rect, strip, chunk) mapping of the pipelined kernels
(csrc/kernels/stencil_device.h locate_strip_task), run on the host through
native().pipe_task_map: with row bands the XCD remap stays inside each band.
Seeded launches with 1-3 bands, with and without rects before the bands and a
signal prefix: every task exactly once; one band or none maps exactly as the
single-segment remap (xcd_remap_after) does."""
import random

import pytest

from rocm_mpi_amd._native import native


@pytest.fixture(scope="module")
def N():
    return native()


def xcd_remap(b, nwg):
    """Each of the 8 XCDs (block b runs on XCD b % 8) takes a contiguous eighth."""
    if nwg < 8:
        return b
    q, r = divmod(nwg, 8)
    xcd, slot = b % 8, b // 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + slot


def xcd_remap_after(b, nwg, first):
    return b if b < first else first + xcd_remap(b - first, nwg - first)


def plan(rects, rect_rows, chunk_rows, V, halo):
    """(strips, chunks, first block) per rect, as plan_strip_tasks lays them out."""
    step = (64 * V - 2 * halo) // V * V
    out, total = [], 0
    for (x0, x1, y0, y1), rr in zip(rects, rect_rows):
        xa = (x0 - halo) - (x0 - halo) % V
        strips = -(-(x1 - (xa + halo)) // step)
        cr = rr or chunk_rows
        chunks = -(-(y1 - y0) // cr)
        out.append((strips, chunks, total))
        total += strips * chunks
    return out, total


def linear(layout, b):
    """The task of logical block b: rects in order, chunk-major, strip fastest."""
    for ri, (strips, chunks, first) in enumerate(layout):
        if b < first + strips * chunks:
            return ri, (b - first) % strips, (b - first) // strips
    raise AssertionError(b)


def case(seed):
    r = random.Random(31_000 + seed)
    V = r.choice((2, 4, 6))
    K = r.randint(3, 24)
    step = (64 * V - 2 * K) // V * V
    nbands = seed % 3 + 1
    lead = r.choice((0, 0, 1, 2))        # rects before the bands
    sig = r.randint(0, lead)             # ... of which signal rects
    x0 = r.randint(1, 40)
    small = seed % 4 == 1                # a launch whose bands have fewer than 8 blocks
    strips = r.choice((1, 2)) if small else r.choice((1, 2, 3, 5, 9))
    x1 = x0 + r.randint((strips - 1) * step + 1, strips * step - 2 * V)
    rects, rows = [], []
    for _ in range(lead):                # frame-like rects elsewhere on the tile
        fy = r.randint(1, 50)
        rects.append((r.randint(1, 30), r.randint(31, 400), fy, fy + r.randint(1, 70)))
        rows.append(r.choice((0, 5, 16)))
    y = r.randint(1, 30)
    band_rows = sorted(r.sample((4, 8, 16, 32, 96, 200), nbands), reverse=True)
    for i, br in enumerate(band_rows):
        n = r.randint(1, 2 if small else 12) * br  # whole tasks but for the last band
        if i == nbands - 1:
            n += r.randint(0, br - 1)
        rects.append((x0, x1, y, y + n))
        rows.append(br)
        y += n
    return dict(V=V, K=K, rects=rects, rows=rows, bands=nbands, sig=sig, lead=lead,
                chunk=r.choice((8, 64)))


@pytest.mark.parametrize("seed", range(48))
def test_every_task_exactly_once(N, seed):
    c = case(seed)
    layout, total = plan(c["rects"], c["rows"], c["chunk"], c["V"], c["K"])
    got = N.pipe_task_map(c["rects"], c["V"], c["chunk"], c["K"], 0, c["rows"], c["bands"],
                          c["sig"], 1)
    assert len(got) == total
    want = sorted(linear(layout, b) for b in range(total))
    assert sorted(got) == want and len(set(got)) == total
    # segments: the signal prefix keeps dispatch order; the other lead rects, and
    # each band, are permuted among their own blocks only
    nlead = c["lead"]
    first = layout[c["sig"]][2] if c["sig"] < len(layout) else total
    assert got[:first] == [linear(layout, b) for b in range(first)]
    if c["bands"] > 1:
        bounds = [first, layout[nlead][2]] + [s[2] for s in layout[nlead + 1:]] + [total]
    else:
        bounds = [first, total]
    for s, e in zip(bounds, bounds[1:]):
        assert got[s:e] == [linear(layout, s + xcd_remap(b - s, e - s)) for b in range(s, e)]
    # without the remap: dispatch order
    plain = N.pipe_task_map(c["rects"], c["V"], c["chunk"], c["K"], 0, c["rows"], c["bands"],
                            c["sig"], 0)
    assert plain == [linear(layout, b) for b in range(total)]


@pytest.mark.parametrize("seed", range(0, 48, 3))  # the one-band cases
def test_one_band_maps_as_the_single_segment_remap(N, seed):
    c = case(seed)
    assert c["bands"] == 1
    layout, total = plan(c["rects"], c["rows"], c["chunk"], c["V"], c["K"])
    first = layout[c["sig"]][2]
    want = [linear(layout, xcd_remap_after(b, total, first)) for b in range(total)]
    for bands in (0, 1):
        assert N.pipe_task_map(c["rects"], c["V"], c["chunk"], c["K"], 0, c["rows"], bands,
                               c["sig"], 1) == want


def test_block_counts_cover_the_edge_cases():
    """The seeds hold bands under 8 blocks, block counts that are no multiple of
    8 and launches with a signal prefix."""
    small = odd = sig = 0
    for seed in range(48):
        c = case(seed)
        layout, _ = plan(c["rects"], c["rows"], c["chunk"], c["V"], c["K"])
        counts = [s * ch for s, ch, _ in layout[c["lead"]:]]
        small += any(n < 8 for n in counts) and c["bands"] > 1
        odd += any(n % 8 for n in counts) and c["bands"] > 1
        sig += c["sig"] > 0 and c["bands"] > 1
    assert small >= 3 and odd >= 10 and sig >= 3


def test_bands_each_walk_every_xcd_in_dispatch_order(N):
    """Three bands of 15, 9 and 9 blocks: block b of a band runs on XCD b % 8, and
    each XCD's blocks of a band are one contiguous run of the band's tasks."""
    rects = [(1, 500, 1, 321), (1, 500, 321, 417), (1, 500, 417, 459)]
    rows = [64, 32, 16]
    layout, total = plan(rects, rows, 64, 4, 24)
    assert [s * c for s, c, _ in layout] == [15, 9, 9]
    got = N.pipe_task_map(rects, 4, 64, 24, 0, rows, 3, 0, 1)
    order = {linear(layout, b): b for b in range(total)}
    for ri, (strips, chunks, first) in enumerate(layout):
        blocks = range(first, first + strips * chunks)
        assert {got[b][0] for b in blocks} == {ri}  # the band's blocks run its own tasks
        for xcd in range(8):
            mine = sorted(order[got[b]] for b in blocks if b % 8 == xcd)
            assert mine and mine == list(range(mine[0], mine[0] + len(mine)))


def test_bad_band_arguments_are_refused(N):
    rects = [(1, 500, 1, 65), (1, 500, 65, 97)]
    with pytest.raises(Exception):
        N.pipe_task_map(rects, 4, 64, 24, 0, [64, 32], 3, 0, 1)  # more bands than rects
    with pytest.raises(Exception):
        N.pipe_task_map(rects, 4, 64, 24, 0, [64, 32], 2, 1, 1)  # a band inside the signal prefix
    with pytest.raises(Exception):
        N.pipe_task_map(rects + [(1, 500, 97, 97)], 4, 64, 24, 0, [64, 32, 8], 3, 0, 1)  # empty band
    with pytest.raises(Exception):
        N.pipe_task_map(rects, 4, 64, 24, 0, [64], 2, 0, 1)  # one rows entry per rect
