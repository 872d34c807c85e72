"""Randomised decomposition-invariance of ``Diffusion3D`` on one MI355X: the first
configurations of ``fuzz3d_cases.model_case`` with rank threads over the device
loopback transport, the Python-issued pass loop or the native executor as drawn.
Every cell of every rank's tile equals, bitwise, the same cell of the global field:
the NumPy golden model (canonical arithmetic) or a one-rank CPU run (fast7)."""
import pytest

from fuzz3d_cases import N_MODEL_GPU, model_case, model_check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(N_MODEL_GPU))
def test_random_decompositions_match_the_global_field(seed):
    model_check(seed, "cuda:0")


def test_seed_set_runs_both_pass_loops():
    cases = [model_case(s) for s in range(N_MODEL_GPU)]
    assert {c["native"] for c in cases if c["variant"] != "ap"} == {False, True}
    assert {c["variant"] for c in cases} == {"perf", "perf_hide", "ap"}
