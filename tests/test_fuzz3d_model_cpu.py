"""Randomised decomposition-invariance of ``Diffusion3D`` on CPU tensors (loopback
rank threads, the C++ CPU twins): the configurations of ``fuzz3d_cases.model_case``
(process grid, periodic dimensions, tile size, variant, steps per pass, arithmetic,
frame width, x-face limit, uniform or random 1/Cp) against the NumPy golden model
of the global grid (canonical arithmetic) or a one-rank run (fast7), every cell of
every rank's tile bitwise. test_fuzz3d_model_gpu.py runs the first seeds on the GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

import golden3d
from fuzz3d_cases import N_MODEL_CPU, bits, expect_inner, model_case, model_check


@pytest.mark.parametrize("seed", range(N_MODEL_CPU))
def test_random_decompositions_match_the_global_field(seed):
    model_check(seed, "cpu")


def test_seed_set_covers_the_model_axes():
    cases = [model_case(s) for s in range(N_MODEL_CPU)]
    assert {c["variant"] for c in cases} == {"perf", "perf_hide", "ap"}
    assert {c["temporal"] for c in cases} == {1, 2}
    assert {c["fast"] for c in cases} == {False, True}
    assert {c["icp"] for c in cases} == {"uniform", "random"}
    assert any(any(c["periods"]) for c in cases) and any(not any(c["periods"]) for c in cases)
    assert any(c["n"][0] > 130 for c in cases)
    inner = set()
    for c in cases:
        if c["variant"] != "perf_hide":
            continue
        inner |= {expect_inner(c, (x, y, z)) for x in range(c["dims"][0])
                  for y in range(c["dims"][1]) for z in range(c["dims"][2])}
    assert inner == {False, True}  # perf_hide with and without an interior box
    for d in range(3):  # at least three distinct multi-rank process grids per axis
        assert len({c["dims"] for c in cases if c["dims"][d] > 1}) >= 3, d
    for c in cases:
        assert c["variant"] != "ap" or (c["temporal"] == 1 and not c["fast"] and not c["native"])
        assert c["temporal"] == 1 or c["nt"] % 2 == 1 and c["nt"] >= 3


def test_numpy_random_field_equals_the_integer_model():
    """golden3d.random_field3_np (the global fields above) == the Python-integer
    random_field3 that ties init_random3d to splitmix64, on a periodic tile."""
    geom = SimpleNamespace(gx0=5, gy0=0, gz0=3, nxg=11, nyg=7, nzg=6, periodx=1, periody=0,
                           periodz=1)
    for seed, lo, hi in ((1234, 0.0, 1.0), (2**64 - 3, 0.5, 1.0)):
        a = golden3d.random_field3(9, 7, 6, geom, seed, lo, hi)
        b = golden3d.random_field3_np(9, 7, 6, geom, seed, lo, hi)
        assert np.array_equal(bits(a), bits(b))
