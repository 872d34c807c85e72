"""Graded task rows, host side (csrc/runtime/plan.cpp plan_row_bands): the row
range of a pipelined launch split into at most three bands of descending rows
per task. Seeded ranges: the bands partition the range, every band but the last
is whole tasks, short ranges keep today's single band; the RMA_DIAG task_rows
grammar; the default table."""
import random

import pytest

from rocm_mpi_amd import config
from rocm_mpi_amd._native import native


@pytest.fixture(scope="module")
def N():
    return native()


def case(seed):
    r = random.Random(9_000 + seed)
    K = r.randint(5, 24)
    r2 = r.choice((4, 8, 24, 96, 384))
    r1 = r2 * r.choice((2, 3, 4))
    r0 = r1 * r.choice((2, 4, 5))
    rows = [r0, r1, r2]
    if seed % 5 == 3:
        rows[r.choice((1, 2))] = 0  # two bands only
    y0 = r.randint(1, 60)
    span = r.choice((r.randint(1, r0), r.randint(r0, 6 * r0), r.randint(6 * r0, 40 * r0)))
    return dict(K=K, y0=y0, y1=y0 + span, strips=r.randint(1, 400),
                slots=r.choice((1, 7, 256, 512, 1024)), rows=rows,
                uniform=r.choice((16, 64, 3072)), fill=r.choice((1.0, 2.0, 3.5)))


def bands_of(N, c):
    return N.plan_row_bands(c["y0"], c["y1"], c["strips"], c["slots"], c["rows"], c["uniform"],
                            c["fill"])


@pytest.mark.parametrize("seed", range(60))
def test_bands_partition_descend_and_are_whole_tasks(N, seed):
    c = case(seed)
    b = bands_of(N, c)
    assert 1 <= len(b) <= 3
    assert b[0][0] == c["y0"] and b[-1][1] == c["y1"]
    for (a0, a1, _), (b0, _, _) in zip(b, b[1:]):
        assert a1 == b0  # seams: no gap, no overlap
    assert all(y1 > y0 and rows >= 1 for y0, y1, rows in b)
    if len(b) == 1:
        assert b[0] == (c["y0"], c["y1"], c["uniform"])  # today's geometry
        return
    rows = [r for _, _, r in b]
    assert rows == sorted(rows, reverse=True) and len(set(rows)) == len(rows)
    assert set(rows) <= {r for r in c["rows"] if r > 0} and rows[0] == c["rows"][0]
    for y0, y1, r in b[:-1]:
        assert (y1 - y0) % r == 0
    # the long band keeps at least half of the range less one of its tasks
    assert b[0][1] - b[0][0] > (c["y1"] - c["y0"]) // 2 - rows[0]


def test_short_ranges_keep_the_single_band(N):
    rows = [96, 32, 8]
    for span in (1, 8, 62, 95, 96, 127):
        # a task of 96 rows beside the two short bands (a quarter of the range each)
        assert N.plan_row_bands(1, 1 + span, 3, 512, rows, 48, 2.0) == [(1, 1 + span, 48)]
    b = N.plan_row_bands(1, 202, 3, 512, rows, 48, 2.0)
    assert b == [(1, 97, 96), (97, 129, 32), (129, 202, 8)]
    assert N.plan_row_bands(1, 202, 3, 512, [0, 0, 0], 48, 2.0) == [(1, 202, 48)]
    assert N.plan_row_bands(1, 202, 3, 512, [96, 0, 0], 48, 2.0) == [(1, 202, 48)]
    for bad in ([8, 32, 96], [96, 96, 8], [96, 8, 8], [96, 0, 96]):
        with pytest.raises(Exception):
            N.plan_row_bands(1, 2000, 3, 512, bad, 48, 2.0)


def test_the_bench_tile_bands(N):
    """The 288 GB class at K = 20..24: the table's bands, sized from 512 resident
    blocks (256 CUs x 2) at 301 six-cell strips; smaller classes and shallower
    passes stay uniform."""
    rows = list(N.pipe_band_rows(24, 101120))
    assert rows == list(N.pipe_band_rows(20, 98304)) and rows[0] > rows[1] > rows[2] > 0
    assert list(N.pipe_band_rows(19, 101120)) == [0, 0, 0]
    assert list(N.pipe_band_rows(24, 65536)) == [0, 0, 0]
    strips = N.pipe_strip_count(1, 101119, 24, 6)
    assert strips == 301 and N.pipe_strip_count(1, 769, 24, 6) == 3
    assert N.pipe_strip_count(1, 769, 20, 4) == -(-768 // 216)
    b = N.plan_row_bands(1, 101119, strips, 512, rows, 3072)
    assert len(b) == 3 and [r for _, _, r in b] == rows
    chunks = -(-2 * 512 // strips)
    assert chunks * rows[1] <= b[1][1] - b[1][0] < (chunks + 1) * rows[1] + rows[0]
    assert chunks * rows[2] <= b[2][1] - b[2][0] < (chunks + 1) * rows[2] + rows[1]


def test_task_rows_grammar(N):
    assert "task_rows" in config.DIAG_KEYS
    assert N.parse_task_rows("") == (False, False, [0, 0, 0], 2.0)
    assert N.parse_task_rows("uniform")[:2] == (False, True)
    assert N.parse_task_rows("96/32/8") == (True, False, [96, 32, 8], 2.0)
    assert N.parse_task_rows("6144/0/384/1.5") == (True, False, [6144, 0, 384], 1.5)
    assert N.parse_task_rows("6144/768/0")[2] == [6144, 768, 0]
    for bad in ("96", "96/32", "a/b/c", "96/32/8/", "96/32/8/0", "0/32/8", "96/32/8/2/1",
                "96.5/32/8", "-96/32/8", "graded",
                "8/32/96", "96/96/8", "96/8/8", "96/0/96", "96/0/0"):  # rows must descend
        with pytest.raises(Exception):
            N.parse_task_rows(bad)
