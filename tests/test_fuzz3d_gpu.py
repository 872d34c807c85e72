"""Seeded differential fuzz of the gfx950 3D kernels (csrc/kernels/stencil3d.hip,
stencil3d_tb.hip): the cases of fuzz3d_cases.py, one launch each with the drawn
tuning on canary-guarded device buffers. Canonical results are compared bitwise on
every cell with K applications of ``golden3d.step3`` (NumPy), fast7 results with
``golden3d_fast.cell7`` (exact rationals) on the case's sample and with the fast7
CPU twin on every cell (test_fuzz3d_cpu.py ties that twin to ``cell7`` on the same
samples). Margins, inputs and the cells outside the boxes must stay as they were;
a uniform-factor launch (1/Cp array full of NaN) must equal the field-path launch
on an array filled with the value."""
import numpy as np
import pytest
import torch

from fuzz3d_cases import (CANARY, N_SEEDS, SENTINEL, bits, canonical_reference, describe,
                          fast7_sample_reference, inside_mask, kernel_case, tuning_of, twin)
from rocm_mpi_amd import ops
from rocm_mpi_amd._native import native
from test_fuzz3d_cpu import REGRESSIONS

pytestmark = pytest.mark.gpu
GROUP = 20


def guarded(src, margin, aligned):
    """src inside a larger device buffer with canary margins on both sides, on a
    16-byte boundary or 8 bytes off it."""
    n, off = src.size, 0 if aligned else 1
    base = torch.full((n + 2 * margin + 2,), CANARY, dtype=torch.float64, device="cuda")
    assert base.data_ptr() % 16 == 0
    v = base[margin + off:margin + off + n].view(src.shape)
    v.copy_(torch.from_numpy(src))
    assert v.data_ptr() % 16 == (0 if aligned else 8)
    return base, v, (margin + off, margin + off + n)


def margins_intact(base, span):
    return bool((base[:span[0]] == CANARY).all()) and bool((base[span[1]:] == CANARY).all())


def launch(c, T2, T, iCp, tuning):
    ops.stencil3dk_step(c["K"], T2, T, iCp, ops.StencilCoef3(*c["coef"]), c["boxes"],
                        tuning=tuning)
    torch.cuda.synchronize()


def check_gpu(seed):
    c = kernel_case(seed)
    msg = f"seed {seed}: {describe(c)}"
    nz, ny, nx = c["shape"]
    margin = (ny * nx + 1) // 2 * 2 + 2 * nx  # more than a plane, even: the alignment holds
    assert margin % 2 == 0 and margin > ny * nx
    sentinel = np.full(c["shape"], SENTINEL)
    # the uniform variant must not read the array: it holds NaN on the device
    bT, vT, sT = guarded(c["T"], margin, c["aligned"])
    bI, vI, sI = guarded(np.full(c["shape"], np.nan) if c["uniform"] else c["iCp"], margin,
                         c["aligned"])
    b2, v2, s2 = guarded(sentinel, margin, c["aligned"])
    tn = tuning_of(c)
    V = native().stencil3d_vec(v2.data_ptr(), vT.data_ptr(), vI.data_ptr(), nx, tn.vec,
                               c["uniform"])
    assert V == (tn.vec if c["aligned"] and nx % 2 == 0 else 1), msg
    launch(c, v2, vT, vI, tn)
    assert margins_intact(b2, s2) and margins_intact(bT, sT) and margins_intact(bI, sI), msg
    assert np.array_equal(bits(vT.cpu().numpy()), bits(c["T"])), msg  # inputs unchanged
    if not c["uniform"]:
        assert np.array_equal(bits(vI.cpu().numpy()), bits(c["iCp"])), msg
    else:
        assert bool(torch.isnan(bI[sI[0]:sI[1]]).all()), msg
    got = v2.cpu().numpy()
    inside = inside_mask(c)
    assert (got[~inside] == SENTINEL).all() and not (got[inside] == SENTINEL).any(), msg
    if c["fast"]:
        for cell, want in fast7_sample_reference(c):
            assert bits(np.float64(got[cell])) == bits(np.float64(want)), (cell, got[cell], want,
                                                                            msg)
        want = twin(c)
    else:
        want = canonical_reference(c)
    same = bits(got) == bits(want)
    assert same.all(), f"{int((~same).sum())} cells differ, first {np.argwhere(~same)[0]}; {msg}"
    if c["uniform"]:  # bitwise the field path on an array filled with the value
        v2.copy_(torch.from_numpy(sentinel))
        vI.copy_(torch.from_numpy(c["iCp"]))
        launch(c, v2, vT, vI, tuning_of(c, uniform=False, uniform_value=None))
        assert margins_intact(b2, s2), msg
        assert np.array_equal(bits(v2.cpu().numpy()), bits(got)), msg


@pytest.mark.parametrize("group", range(N_SEEDS // GROUP))
def test_gpu_kernels_equal_the_independent_references_bitwise(group):
    for seed in range(group * GROUP, (group + 1) * GROUP):
        check_gpu(seed)


def test_regression_seeds():
    for name in sorted(REGRESSIONS):
        check_gpu(REGRESSIONS[name])
