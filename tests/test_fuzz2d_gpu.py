"""Seeded differential fuzz of the gfx950 2D kernels (csrc/kernels/stencil.hip,
stencil_tb.hip, stencil_kstep.hip, stencil_pipe*.hip): the cases of fuzz2d_cases.py,
one launch each with the drawn tuning on canary-guarded device buffers. Canonical
results (march, two-step, lds_dpp, pipec) are compared bitwise on every cell with K
applications of ``golden.step`` (NumPy); fast5 results (pipe, piper, piper_nosb) with
the fast5 CPU twin on every cell, bitwise (test_fuzz2d_cpu.py ties that twin to the
exact-rational model), and on the tiny cases with ``golden.run5`` itself on every
cell. Margins, inputs and the cells outside the rects must stay as they were. A
uniform-factor launch gets its value as an argument and an array full of NaN (at one
cell per lane there is no uniform variant and the launcher documents that it reads
the array: it gets the array); it must equal the field-path launch on the array, and
a six-cell launch the four-cell one. The model tier runs ``Diffusion2D`` with the
native executor on tiles two to five strips wide."""
import numpy as np
import pytest
import torch

from fuzz2d_cases import (ARITH, CANARY, FAST, N_MODEL_GPU, N_SEEDS, N_TINY, PIPE, SENTINEL, bits,
                          canonical_reference, describe, exact_reference, first_difference,
                          inside_mask, kernel_case, model_case, model_check, run_kernel, tiny_case,
                          tuning_of, twin)
from rocm_mpi_amd._native import native
from test_fuzz2d_cpu import REGRESSION_SEEDS

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
    run_kernel(c, T2, T, iCp, tuning)
    torch.cuda.synchronize()


def check_gpu(c, tag):
    msg = f"{tag} {c['seed']}: {describe(c)}"
    ny, nx = c["shape"]
    margin = 2 * nx + 2  # two rows, even: the alignment holds
    sentinel = np.full(c["shape"], SENTINEL)
    tn = tuning_of(c)
    if c["kernel"] in PIPE:  # the cells per lane these arrays get == the case's
        N = native()
        V = (N.pipe_vec_uniform(c["K"], 0, ARITH[c["kernel"]], nx, tn.vec, c["aligned"], True)
             if c["uniform"] else N.pipe_vec(c["K"], 0, ARITH[c["kernel"]], nx, tn.vec, c["aligned"]))
        assert V == c["V"], msg
    # the uniform variant must not read the array: it holds NaN on the device
    blind = c["uniform"] and c["V"] >= 2
    bT, vT, sT = guarded(c["T"], margin, c["aligned"])
    bI, vI, sI = guarded(np.full(c["shape"], np.nan) if blind else c["iCp"], margin, c["aligned"])
    b2, v2, s2 = guarded(sentinel, margin, c["aligned"])
    launch(c, v2, vT, vI, tn)
    assert margins_intact(b2, s2) and margins_intact(bT, sT) and margins_intact(bI, sI), msg
    assert np.array_equal(bits(vT.cpu().numpy()), bits(c["T"])), msg  # inputs unchanged
    if blind:
        assert bool(torch.isnan(bI[sI[0]:sI[1]]).all()), msg
    else:
        assert np.array_equal(bits(vI.cpu().numpy()), bits(c["iCp"])), msg
    got = v2.cpu().numpy()
    inside = inside_mask(c)
    assert (got[~inside] == SENTINEL).all() and not (got[inside] == SENTINEL).any(), msg
    if tag == "tiny seed":  # tier A: the exact model on every cell
        want = exact_reference(c)
        assert np.isfinite(got).all() and np.isfinite(want).all(), msg
        same = got == want
        assert same.all(), (f"{int((~same).sum())} cells differ from the exact model, first "
                            f"(y, x) = {first_difference(same)}; {msg}")
    want = twin(c) if c["kernel"] in FAST else canonical_reference(c)
    same = bits(got) == bits(want)
    assert same.all(), (f"{int((~same).sum())} cells differ, first (y, x) = "
                        f"{first_difference(same)}; {msg}")
    again = []
    if c["uniform"]:  # bitwise the field path on the array
        again.append(tuning_of(c, uniform=False, uniform_value=None))
    if c["V"] == 6:  # bitwise the four-cell uniform kernel
        again.append(tuning_of(c, vec=4))
    for other in again:
        v2.copy_(torch.from_numpy(sentinel))
        vI.copy_(torch.from_numpy(c["iCp"]))
        launch(c, v2, vT, vI, other)
        assert margins_intact(b2, s2), msg
        same = bits(v2.cpu().numpy()) == bits(got)
        assert same.all(), (f"{other}: {int((~same).sum())} cells differ, first (y, x) = "
                            f"{first_difference(same)}; {msg}")


@pytest.mark.parametrize("group", range(N_SEEDS // GROUP))
def test_gpu_kernels_equal_the_independent_references_bitwise(group):
    for seed in range(group * GROUP, (group + 1) * GROUP):
        check_gpu(kernel_case(seed), "seed")


@pytest.mark.parametrize("group", range(N_TINY // GROUP))
def test_gpu_fast5_kernels_equal_the_exact_model_on_tiny_fields(group):
    for seed in range(group * GROUP, (group + 1) * GROUP):
        check_gpu(tiny_case(seed), "tiny seed")


def test_regression_seeds():
    for seed in REGRESSION_SEEDS:
        check_gpu(kernel_case(seed), "seed")


@pytest.mark.parametrize("seed", range(N_MODEL_GPU))
def test_model_tiles_equal_the_one_rank_cpu_run_bitwise(monkeypatch, seed):
    monkeypatch.setenv("RMA_DIAG", f"pipe_cells={model_case(seed)['cells']}")
    model_check(seed, "cuda")
