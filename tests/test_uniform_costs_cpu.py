"""The planner's row for uniform-factor passes (csrc/runtime/plan.cpp
``uniform_pass_costs``, ``pipe_uniform_cells``): measured for the 288 GB tile
class only, the field-path rows untouched, plans that minimise the row."""
import itertools

import pytest

from rocm_mpi_amd._native import native

BIG = 101120.0 * 101120.0
# default_pass_costs(24, True, 288 GB class) as it was before the uniform row existed
FIELD_288 = [1.235, 1.230, 1.215, 1.163, 1.232, 1.210, 1.199, 1.126, 1.149, 1.138, 1.144, 1.119,
             1.244, 1.306, 1.371, 1.399, 1.595, 1.640, 1.676, 1.658, 1.886, 1.903, 1.971, 1.962]


def test_field_path_row_is_not_repriced():
    N = native()
    assert list(N.default_pass_costs(24, True, BIG))[1:] == FIELD_288
    assert list(N.default_pass_costs(24, True))[1:] == FIELD_288


def test_field_path_plans_unchanged():
    N = native()
    c = N.default_pass_costs(24, True, BIG)
    assert list(N.plan_passes(20, c)) == [20]
    assert list(N.plan_passes(1000, c)) == [24] * 40 + [20, 20]  # the benchmark's, as before
    assert list(N.plan_passes(1010, c)) == [24] * 37 + [22] + [20] * 5
    assert list(N.plan_passes(45, c)) == [24, 21]
    assert list(N.plan_passes(37, c)) == [24, 13]


@pytest.mark.parametrize("n", [4096, 8192, 16384, 40000, 98303])
def test_smaller_tiles_have_no_uniform_row_and_keep_four_cells(n):
    N = native()
    assert list(N.uniform_pass_costs(24, float(n) * n)) == list(
        N.default_pass_costs(24, True, float(n) * n))
    assert all(N.pipe_uniform_cells(K, float(n) * n) == 4 for K in range(1, 25))


def test_large_tile_row_and_cells():
    N = native()
    u = list(N.uniform_pass_costs(24, BIG))
    f = list(N.default_pass_costs(24, True, BIG))
    assert u[1:10] == f[1:10]  # K <= 9: no uniform kernel
    assert all(u[K] < f[K] for K in range(10, 25))
    # the measured times: K = 24 60.93 ms over the 39.415 ms one-step pass
    assert u[24] == pytest.approx(60.929 / 39.415, abs=1e-3)
    assert u[16] == pytest.approx(45.003 / 39.415, abs=1e-3)
    assert [N.pipe_uniform_cells(K, BIG) for K in (9, 16, 17, 20, 24)] == [4, 4, 6, 6, 6]
    assert list(N.uniform_pass_costs(12, BIG)) == u[:13]
    with pytest.raises(Exception):
        N.uniform_pass_costs(25, BIG)


def brute(n, cost, kmax):
    """Cheapest multiset of depths summing to n (exhaustive for small n)."""
    best = {0: 0.0}
    for s in range(1, n + 1):
        best[s] = min(best[s - K] + cost[K] for K in range(1, min(kmax, s) + 1))
    return best[n]


@pytest.mark.parametrize("n", [20, 37, 45, 100, 1000, 1010])
def test_plans_minimise_the_uniform_row(n):
    N = native()
    u = list(N.uniform_pass_costs(24, BIG))
    plan = list(N.plan_passes(n, u))
    assert sum(plan) == n
    assert sum(u[K] for K in plan) == pytest.approx(brute(n, u, 24), abs=1e-9)


def test_benchmark_plan_on_the_uniform_row():
    N = native()
    u = N.uniform_pass_costs(24, BIG)
    assert list(N.plan_passes(1000, u)) == [24] * 41 + [16]
    assert list(N.plan_passes(20, u)) == [20]
