"""Seeded differential fuzz of the 2D kernels' CPU twins (fuzz2d_cases.py) against
references that share no code with the package: the canonical twins (march, two-step,
lds_dpp, pipec) against K applications of ``golden.step`` on the whole field, bitwise
on every cell; the fast5 twin against ``golden.run5`` (exact rationals) on every cell
of the tiny cases (tier A) and, through the dependence cone, on up to 16 sampled cells
of every seam-shaped case with K <= 4 (tier B). test_fuzz2d_gpu.py runs the same seeds
on the gfx950 kernels. The coverage the seed set must reach is asserted here from the
launchers' host-side rules, with no kernel run."""
from collections import Counter

import numpy as np
import pytest

from fuzz2d_cases import (CHUNKS, FAST, MAX_CELLS, MAX_RECTS, MAX_SAMPLES, MAX_TINY_UPDATES,
                          N_MODEL_CPU, N_MODEL_GPU, N_SEEDS, N_TINY, ROWS, SENTINEL, bits, canonical_reference,
                          describe, exact_reference, fast5_sample_reference, first_difference,
                          inside_mask, kernel_case, model_case, model_check, seams, tiny_case, twin)
from rocm_mpi_amd import ops

GROUP = 20
TINY_GROUP = 20
# seeds the fuzz has exposed a bug with: run by both files, always
REGRESSION_SEEDS: tuple = ()


def check_twin(seed):
    c = kernel_case(seed)
    got = twin(c)
    inside = inside_mask(c)
    msg = f"seed {seed}: {describe(c)}"
    assert (got[~inside] == SENTINEL).all() and not (got[inside] == SENTINEL).any(), msg
    if c["kernel"] not in FAST:
        same = bits(got) == bits(canonical_reference(c))
        assert same.all(), (f"{int((~same).sum())} cells differ, first (y, x) = "
                            f"{first_difference(same)}; {msg}")
    elif c["K"] <= 4:
        for cell, want in fast5_sample_reference(c):
            assert inside[cell] and np.isfinite(want), msg
            assert got[cell] == want, f"first differing cell (y, x) = {cell}: {got[cell]!r} != {want!r}; {msg}"


def check_tiny_twin(seed):
    c = tiny_case(seed)
    got, want = twin(c), exact_reference(c)
    assert np.isfinite(want).all() and np.isfinite(got).all(), seed
    same = got == want
    assert same.all(), (f"tiny seed {seed}: {int((~same).sum())} cells differ, first (y, x) = "
                        f"{first_difference(same)}; {describe(c)}")


@pytest.mark.parametrize("group", range(N_SEEDS // GROUP))
def test_cpu_twins_equal_the_independent_references(group):
    for seed in range(group * GROUP, (group + 1) * GROUP):
        check_twin(seed)


@pytest.mark.parametrize("group", range(N_TINY // TINY_GROUP))
def test_fast5_twin_equals_the_exact_model_on_tiny_fields(group):
    for seed in range(group * TINY_GROUP, (group + 1) * TINY_GROUP):
        check_tiny_twin(seed)


def test_regression_seeds():
    for seed in REGRESSION_SEEDS:
        check_twin(seed)


@pytest.mark.parametrize("seed", range(N_MODEL_CPU))
def test_model_tiles_equal_the_one_rank_run_bitwise(seed):
    model_check(seed, "cpu")


def _valid(c, seed):
    tiny = np.finfo(np.float64).tiny
    ny, nx = c["shape"]
    assert min(ny, nx) >= 3 and ny * nx <= MAX_CELLS, seed
    assert 1 <= len(c["rects"]) <= MAX_RECTS
    assert ops.validate_rects(c["rects"], nx, ny) == c["rects"], seed  # none empty, inside
    inside_mask(c)  # disjoint
    for a in (c["T"], c["iCp"]):
        assert a.dtype == np.float64 and a.shape == c["shape"]
        assert np.isfinite(a).all() and ((a == 0) | (np.abs(a) >= tiny)).all(), seed
    assert c["iCp"].min() >= 0.5 and c["iCp"].max() <= 2.0
    if c["uniform"]:
        assert (c["iCp"] == c["value"]).all()
    coef = ops.StencilCoef(*c["coef"])
    assert ops.fast5_ok(coef), seed
    lam, dx, dy = -coef.mlam, 1.0 / coef.rdx, 1.0 / coef.rdy
    limit = 1.0 / (2.0 * lam * float(c["iCp"].max()) * (1 / dx**2 + 1 / dy**2))
    assert 0.0 < coef.dt <= c["limit"] and coef.dt < limit * (1 + 1e-12), seed
    assert c["tuning"]["chunk_rows"] in CHUNKS and c["tuning"]["xcd_remap"] in (0, 1)


def test_cases_are_valid_and_reproducible():
    """Every seed gives a launchable case: shape, rect and tuning bounds, finite and
    normal inputs with both zeros somewhere in the set, coefficients the fast5
    arithmetic accepts with dt below the explicit limit."""
    zeros = Counter()
    for seed in range(N_SEEDS):
        c = kernel_case(seed)
        _valid(c, seed)
        assert c["V"] == c["want"], (seed, describe(c))  # the shape gives the cells drawn
        assert 1 <= len(c["samples"]) <= MAX_SAMPLES
        zeros["+0"] += bool(((c["T"] == 0) & ~np.signbit(c["T"])).any())
        zeros["-0"] += bool(((c["T"] == 0) & np.signbit(c["T"])).any())
    assert zeros["+0"] >= 20 and zeros["-0"] >= 20, zeros
    for seed in range(N_TINY):
        c = tiny_case(seed)
        _valid(c, seed)
        ny, nx = c["shape"]
        assert max(ny, nx) <= 14 and (nx - 2) * (ny - 2) * c["K"] <= MAX_TINY_UPDATES
        assert c["kernel"] in FAST and c["rects"] == [ops.interior_rect(nx, ny)]
    a, b = kernel_case(7), kernel_case(7)
    assert describe(a) == describe(b) and np.array_equal(bits(a["T"]), bits(b["T"]))


def coverage():
    cov = dict(rows=Counter(), depth=Counter(), piper=Counter(), V=Counter(), strips2=0, strips3=0,
               seam_edge=0, cone=0, cone_strips2=0, iso=0, misaligned=0, short=0, many=0, cases=0, uniform=0,
               tuning=Counter())
    for seed in range(N_SEEDS):
        c = kernel_case(seed)
        cov["cases"] += 1
        kernel, K, V = c["kernel"], c["K"], c["V"]
        ny, nx = c["shape"]
        cov["rows"][kernel] += 1
        if kernel in ("pipe", "pipec"):
            cov["depth"][K] += 1
        if kernel == "piper":
            cov["piper"][K] += 1
        cov["V"][V] += 1
        cov["uniform"] += c["uniform"]
        strips = max(1 + len(seams(kernel, K, V, x0, x1)) for x0, x1, _, _ in c["rects"])
        cov["cone"] += kernel in FAST and K <= 4
        cov["cone_strips2"] += kernel in FAST and K <= 4 and strips >= 2
        cov["strips2"] += strips >= 2
        cov["strips3"] += strips >= 3
        # seams past the first strip: of the interior's tiling and of each rect's own
        deep = set(seams(kernel, K, V, 1, nx - 1)) | set(seams(kernel, K, V, K, max(K + 1, nx - K)))
        near = False
        for x0, x1, _, _ in c["rects"]:
            own = set(seams(kernel, K, V, x0, x1 + 2))
            near |= any(abs(x1 - s) <= 1 for s in own | deep) or any(abs(x0 - s) <= 1 for s in deep)
        cov["seam_edge"] += near
        coef = ops.StencilCoef(*c["coef"])
        cov["iso"] += ops.fast5_constants(coef)[0] == 1.0
        cov["misaligned"] += not c["aligned"]
        chunk = c["tuning"]["chunk_rows"]
        cov["short"] += ny - 2 < K or 0 < (ny - 2) % chunk < K
        cov["many"] += len(c["rects"]) >= 5
        for k in ("nontemporal", "unroll"):
            if k in c["tuning"]:
                entry = kernel if kernel in ("march", "tb2") else "kstep"
                cov["tuning"][(entry, k, c["tuning"][k])] += 1
    return cov


def test_seed_set_reaches_every_kernel_depth_and_seam():
    cov = coverage()
    assert cov["cases"] == N_SEEDS  # zero cases left out
    for kernel, _ in ROWS:
        assert cov["rows"][kernel] >= 10, (kernel, cov["rows"])
    assert set(cov["rows"]) == {k for k, _ in ROWS}
    assert all(cov["depth"][K] >= 1 for K in range(1, 25)), cov["depth"]
    assert all(cov["piper"][K] >= 1 for K in range(10, 25)), cov["piper"]
    for V in (1, 2, 4, 6):
        assert cov["V"][V] >= 15, cov["V"]
    assert cov["strips2"] >= 40 and cov["strips3"] >= 15, cov
    assert cov["seam_edge"] >= 60, cov
    assert cov["iso"] >= 30, cov
    assert cov["misaligned"] >= 40, cov
    assert cov["short"] >= 40, cov
    assert cov["many"] >= 30, cov
    assert cov["uniform"] >= 20, cov
    assert cov["cone"] >= 10 and cov["cone_strips2"] >= 3, cov  # tier B against the exact model
    # every value the entry points accept
    for nt in range(8):
        assert cov["tuning"][("march", "nontemporal", nt)] >= 1, cov["tuning"]
    for nt in range(4):
        assert cov["tuning"][("tb2", "nontemporal", nt)] >= 1, cov["tuning"]
    for u in (2, 4, 8):
        assert cov["tuning"][("march", "unroll", u)] >= 1, cov["tuning"]
    for u in (2, 4):
        assert cov["tuning"][("tb2", "unroll", u)] >= 1, cov["tuning"]
    for nt in range(4):
        assert cov["tuning"][("kstep", "nontemporal", nt)] >= 5, cov["tuning"]


def test_model_seeds_reach_both_arithmetics_rank_splits_and_the_six_cell_passes():
    cs = [model_case(s) for s in range(N_MODEL_GPU)]
    assert all(300 <= c["nx"] <= 1100 and 4 * c["K"] + 6 <= c["ny"] <= 4 * c["K"] + 90 and
               1 <= c["nt"] <= 2 * c["K"] + 3 for c in cs)
    assert sum(c["dims"] != (1, 1) for c in cs) >= 4 and sum(c["dims"] == (1, 1) for c in cs) >= 2
    assert sum(c["fast"] for c in cs) >= 4 and sum(not c["fast"] for c in cs) >= 3
    assert sum(c["fast"] and c["icp"] == "random" for c in cs) >= 2
    assert {c["variant"] for c in cs} == {"perf", "perf_hide"}
    assert sum(max(c["periods"]) for c in cs) >= 2
    # uniform 1/Cp, fast-math, a six-cell depth, an even nx: passes at six cells per lane
    assert sum(c["fast"] and c["icp"] == "uniform" and c["K"] >= 17 and c["cells"] == 6 and
               c["nx"] % 2 == 0 for c in cs) >= 1


def test_seams_mirror_the_launchers_on_known_rects():
    """The strip seams used above, on rects whose strips the kernels' design fixes
    (``seam_of`` / ``step_of`` of test_pipe_v6_gpu.py; 64 V columns on multiples of
    64 V for the one- and two-step kernels)."""
    for K in (17, 20, 24):
        step = (384 - 2 * K) // 6 * 6
        first = (1 - K) // 6 * 6 + K + step
        assert seams("piper", K, 6, 1, first + step + 1) == [first, first + step]
        assert seams("piper", K, 6, 1, first) == []
    assert seams("pipe", 24, 1, 1, 40) == [17, 33] and seams("pipe", 24, 4, 1, 210) == [208]
    assert seams("lds_dpp", 8, 2, 1, 300) == [112, 224]
    assert seams("march", 1, 2, 130, 256) == [] and seams("march", 1, 2, 127, 129) == [128]
    assert seams("tb2", 2, 1, 1, 129) == [64, 128]
