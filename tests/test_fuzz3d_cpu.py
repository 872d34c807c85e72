"""Seeded differential fuzz of the 3D kernels' CPU twins (fuzz3d_cases.py) against
references that share no code with the package: the canonical twin against K
applications of ``golden3d.step3`` on the whole field, bitwise on every cell; the
fast7 twin against ``golden3d_fast.cell7`` (exact rationals) on a sample of every
case. test_fuzz3d_gpu.py runs the same seeds on the gfx950 kernels. The coverage
the seed set must reach is asserted here through the launchers' host-side rules
(``ops.stencil3d_dispatch``, ``native().stencil3d_vec``)."""
from collections import Counter

import numpy as np
import pytest

from fuzz3d_cases import (MAX_BOXES, MAX_CELLS, MAX_SAMPLES, N_SEEDS, SENTINEL, bits,
                          canonical_reference, describe, fast7_sample_reference, inside_mask, kernel_case,
                          march_strips, tuning_of, twin)
from rocm_mpi_amd import ops
from rocm_mpi_amd._native import native

GROUP = 20
# seeds the fuzz has exposed a bug with, kept as named regression cases
REGRESSIONS: dict = {}


def check_twin(seed):
    c = kernel_case(seed)
    got = twin(c)
    inside = inside_mask(c)
    msg = f"seed {seed}: {describe(c)}"
    assert (got[~inside] == SENTINEL).all() and not (got[inside] == SENTINEL).any(), msg
    if not c["fast"]:
        want = canonical_reference(c)
        same = bits(got) == bits(want)
        assert same.all(), f"{int((~same).sum())} cells differ, first {np.argwhere(~same)[0]}; {msg}"
        return
    for cell, want in fast7_sample_reference(c):
        assert inside[cell], msg
        assert bits(np.float64(got[cell])) == bits(np.float64(want)), (cell, got[cell], want, msg)


@pytest.mark.parametrize("group", range(N_SEEDS // GROUP))
def test_cpu_twins_equal_the_independent_references_bitwise(group):
    for seed in range(group * GROUP, (group + 1) * GROUP):
        check_twin(seed)


def test_regression_seeds():
    for name in sorted(REGRESSIONS):
        check_twin(REGRESSIONS[name])


def test_cases_are_valid_and_reproducible():
    """Every seed gives a launchable case: shape, box and tuning bounds, finite and
    normal inputs with equal neighbours and both zeros somewhere in the set."""
    tiny = np.finfo(np.float64).tiny
    zeros = Counter()
    for seed in range(N_SEEDS):
        c = kernel_case(seed)
        nz, ny, nx = c["shape"]
        assert min(nz, ny, nx) >= 3 and nz * ny * nx <= MAX_CELLS, seed
        assert 1 <= len(c["boxes"]) <= MAX_BOXES
        assert ops.validate_boxes(c["boxes"], nx, ny, nz) == c["boxes"], seed  # none empty
        inside_mask(c)  # disjoint
        assert 1 <= len(c["samples"]) <= MAX_SAMPLES
        for a in (c["T"], c["iCp"]):
            assert a.dtype == np.float64 and a.shape == c["shape"]
            assert np.isfinite(a).all() and ((a == 0) | (np.abs(a) >= tiny)).all(), seed
        assert c["iCp"].min() >= 0.5 and c["iCp"].max() <= 2.0
        assert ops.fast7_ok(ops.StencilCoef3(*c["coef"]))
        tn = c["tuning"]
        assert (tn["rows"], tn["unroll"]) in ops.TUNINGS_3D and 0 <= tn["xface"] <= ops.XFACE_MAX
        zeros["+0"] += bool(((c["T"] == 0) & ~np.signbit(c["T"])).any())
        zeros["-0"] += bool(((c["T"] == 0) & np.signbit(c["T"])).any())
    assert zeros["+0"] >= 20 and zeros["-0"] >= 20, zeros
    a, b = kernel_case(7), kernel_case(7)
    assert describe(a) == describe(b) and np.array_equal(bits(a["T"]), bits(b["T"]))


def coverage():
    """Counts over the seed set, from the launchers' own host-side rules."""
    cov = dict(paths=Counter(), lanes=Counter(), rows=Counter(), tb_rows=Counter(),
               chunk1=Counter(), deep=0, deep_multi=0, deep_k2=0, cases=0)
    vec = native().stencil3d_vec
    for seed in range(N_SEEDS):
        c = kernel_case(seed)
        cov["cases"] += 1
        K, tn = c["K"], c["tuning"]
        nx = c["shape"][2]
        base = 0x10000 + (0 if c["aligned"] else 8)  # host-only: the rule looks at the low bits
        V = vec(base, base, base, nx, tn["vec"], c["uniform"])
        assert vec(base, base, base, nx, 2, c["uniform"]) == (2 if c["aligned"] and nx % 2 == 0
                                                              else 1)
        plan = ops.stencil3d_dispatch(K, c["shape"], c["boxes"], tuning_of(c))
        assert [b for b, _, _ in plan] == c["boxes"]
        combo = ("fast7" if c["fast"] else "canonical", "uniform" if c["uniform"] else "field")
        chunk = tn["chunk_z"] if K == 1 else tn["tb_chunk_z"]
        marches = 0
        for (x0, x1, y0, y1, z0, z1), path, lanes in plan:
            name = path if path != "xface" else f"xface-{lanes}"
            cov["paths"][(K, name) + combo] += 1
            if path != "thin" and chunk == 1 and z0 > 1 and z1 - z0 >= 2:
                cov["chunk1"][K] += 1
            if path != "march":
                continue
            marches += 1
            if x0 >= 126:
                strips = march_strips(K, V, x0, x1)
                cov["deep"] += 1
                cov["deep_multi"] += strips >= 2
                cov["deep_k2"] += K == 2
        if marches:  # the march launch: cells per lane and the rows it instantiates
            cause = ("two" if V == 2 else "one-odd-nx" if nx % 2 else
                     "one-unaligned" if not c["aligned"] else "one-requested")
            cov["lanes"][cause] += 1
            if K == 1:
                cov["rows"][(tn["rows"], tn["unroll"])] += 1
            else:
                cov["tb_rows"][tn["tb_rows"]] += 1
    return cov


def test_seed_set_reaches_every_path_and_seam():
    cov = coverage()
    n = cov["cases"]
    assert n == N_SEEDS  # zero cases left out
    paths = {1: ("march", "thin", "xface-8", "xface-16", "xface-32"),
             2: ("march", "xface-8", "xface-16", "xface-32")}
    for K, names in paths.items():
        for name in names:
            for arith in ("canonical", "fast7"):
                for factor in ("field", "uniform"):
                    key = (K, name, arith, factor)
                    assert cov["paths"][key] >= 3, (key, cov["paths"][key])
    assert not [k for k in cov["paths"] if k[1] not in paths[k[0]]]
    lanes = cov["lanes"]
    one = lanes["one-odd-nx"] + lanes["one-unaligned"] + lanes["one-requested"]
    assert lanes["two"] >= 0.25 * n and one >= 0.25 * n, lanes
    assert lanes["one-odd-nx"] >= 0.10 * n and lanes["one-unaligned"] >= 0.10 * n, lanes
    assert cov["deep"] >= 30 and cov["deep_multi"] >= 15 and cov["deep_k2"] >= 10, cov
    for ru in ops.TUNINGS_3D:
        assert cov["rows"][ru] >= 5, (ru, cov["rows"])
    for R in (0,) + tuple(ops.TB_ROWS_3D):
        assert cov["tb_rows"][R] >= 5, (R, cov["tb_rows"])
    assert cov["chunk1"][1] >= 5 and cov["chunk1"][2] >= 5, cov["chunk1"]


def test_march_strips_mirrors_the_launchers_on_known_boxes():
    """The strip count used above, on boxes whose strips the kernels' design fixes:
    128 (64) cells a strip from a strip-aligned origin in the one-step kernel, an
    advance of 126 (62) from one column left of the box in the two-step kernel."""
    assert march_strips(1, 2, 130, 256) == 1 and march_strips(1, 2, 127, 129) == 2
    assert march_strips(1, 1, 126, 129) == 2 and march_strips(1, 1, 128, 192) == 1
    assert march_strips(2, 2, 1, 126) == 1 and march_strips(2, 2, 1, 127) == 2
    assert march_strips(2, 2, 128, 253) == 1 and march_strips(2, 2, 128, 254) == 2
    assert march_strips(2, 1, 127, 189) == 1 and march_strips(2, 1, 127, 190) == 2
