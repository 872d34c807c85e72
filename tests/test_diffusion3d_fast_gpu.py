"""Diffusion3D(fast_math=True) on one MI355X (the fast7 instantiations of the 3D
kernels): rank threads over the device loopback against the one-rank run of the
same global grid (bitwise), independence of the plan and of the uniform-factor
path, the device field against the CPU twin's, and the app's report."""
import numpy as np
import pytest

from test_diffusion3d_fast_cpu import (CASES, bits, plan_and_factor_independence,
                                       rank_threads_equal_one_rank, run_app, single)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("temporal", [1, 2])
@pytest.mark.parametrize("dims,periods", CASES)
def test_rank_threads_equal_the_one_rank_run_bitwise(dims, periods, temporal):
    rank_threads_equal_one_rank(dims, periods, temporal, "cuda")


def test_field_is_independent_of_the_plan_the_factor_path_and_the_device():
    """temporal=2 with an odd nt == temporal=1; the uniform-factor kernels (the
    default: 1/Cp is one value) == the field path; the GPU == the CPU twin."""
    a = plan_and_factor_independence("cuda")
    assert np.array_equal(bits(a), bits(single("cpu", temporal=2)))
    canon = single("cuda", temporal=2, fast_math=False)
    assert not np.array_equal(a, canon) and float(np.abs(a - canon).max()) < 1e-14


def test_app_reports_the_arithmetic(tmp_path):
    plan, rec = run_app(tmp_path, "--fast-math", "--temporal", "2")
    assert "cuda" in rec["device"]
    assert rec["extra"]["fast_math"] is True and rec["extra"]["uniform_passes"] == [1, 2]
    assert len(plan) == 1 and "fast-math (fast7" in plan[0], plan
