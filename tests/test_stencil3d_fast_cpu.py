"""The fast7 arithmetic of the 3D kernels on the CPU: the C++ twins
(``stencil3d7_boxes_cpu`` / ``stencil3dk7_boxes_cpu``, reached through
``Stencil3DTuning(fast_math=True)`` on CPU tensors) against the exact-rational
model of tests/golden3d_fast.py, bitwise; the K-step twin against one-step calls;
the distance from the canonical twin; the refusals."""
import numpy as np
import pytest
import torch

import golden3d_fast
from rocm_mpi_amd import ops
from rocm_mpi_amd._native import native

LAM, DX, DY, DZ = 1.3, 0.037, 0.041, 0.053  # anisotropic
# half the explicit 3D stability limit 1 / (2 lam (1/dx^2 + 1/dy^2 + 1/dz^2)) at 1/Cp <= 1
DT = 0.5 / (2.0 * LAM * (1.0 / DX**2 + 1.0 / DY**2 + 1.0 / DZ**2))
COEF = ops.StencilCoef3.from_physics(LAM, DX, DY, DZ, DT)
FAST = ops.Stencil3DTuning(fast_math=True)
SENTINEL = -7.25
NZ, NY, NX = 9, 10, 11

BOX_LISTS = {
    "interior": [ops.interior_box(NX, NY, NZ)],
    # x-width 1 and 3 (thin x-boxes), a wide box between them, gaps everywhere
    "thin_and_gaps": [(1, 2, 1, NY - 1, 1, NZ - 1), (4, 7, 2, NY - 2, 1, NZ - 2),
                      (8, NX - 1, 1, NY - 2, 2, NZ - 1), (2, 3, 3, NY - 1, 1, 3)],
}


def fields(shape, seed):
    rng = np.random.default_rng(seed)
    T = torch.from_numpy(rng.uniform(0.0, 1.0, shape))
    iCp = torch.from_numpy(rng.uniform(0.5, 1.0, shape))
    return T, iCp


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def step(K, T2, T, iCp, boxes=None, tuning=FAST, coef=COEF, forward=False):
    if K == 1 and not forward:
        ops.stencil3d_step(T2, T, iCp, coef, boxes, tuning)
    else:
        ops.stencil3dk_step(K, T2, T, iCp, coef, boxes, tuning)


@pytest.mark.parametrize("boxes", sorted(BOX_LISTS))
@pytest.mark.parametrize("K", [1, 2])
def test_twin_equals_the_exact_golden_model_bitwise(K, boxes):
    T, iCp = fields((NZ, NY, NX), 11)
    bl = BOX_LISTS[boxes]
    want = np.full((NZ, NY, NX), SENTINEL)
    golden3d_fast.pass7(K, want, T.numpy(), iCp.numpy(), bl, *COEF)
    inside = torch.zeros((NZ, NY, NX), dtype=torch.bool)
    for x0, x1, y0, y1, z0, z1 in bl:
        inside[z0:z1, y0:y1, x0:x1] = True
    for forward in (False, True):  # K = 1 also through stencil3dk_step
        got = torch.full((NZ, NY, NX), SENTINEL, dtype=torch.float64)
        step(K, got, T, iCp, bl, forward=forward)
        assert same_bits(got, torch.from_numpy(want)), (K, boxes, forward)
        assert bool((got[~inside] == SENTINEL).all())  # cells outside the boxes untouched
        assert not bool((got[inside] == SENTINEL).any())


@pytest.mark.parametrize("boxes", sorted(BOX_LISTS))
def test_two_step_pass_equals_two_one_step_calls(boxes):
    T, iCp = fields((NZ, NY, NX), 12)
    bl = BOX_LISTS[boxes]
    mid = T.clone()  # step 1 on the interior, T on the six faces
    step(1, mid, T, iCp)
    want = torch.full((NZ, NY, NX), SENTINEL, dtype=torch.float64)
    step(1, want, mid, iCp, bl)
    got = torch.full((NZ, NY, NX), SENTINEL, dtype=torch.float64)
    step(2, got, T, iCp, bl)
    assert same_bits(got, want)


def test_fast7_differs_from_canonical_and_stays_rounding_close():
    """Six full-interior steps of either twin on a 12 x 13 x 14 field. The bound is
    the project's own for the 2D fast5 / canonical pair."""
    shape = (12, 13, 14)
    T, iCp = fields(shape, 13)
    res = {}
    for name, tn in (("canonical", None), ("fast7", FAST)):
        a, b = T.clone(), T.clone()
        for _ in range(6):
            step(1, b, a, iCp, tuning=tn)
            a, b = b, a
        res[name] = a
    diff = (res["fast7"] - res["canonical"]).abs()
    frac = float((diff != 0).double().mean())
    print(f"fast7 vs canonical after 6 steps on {shape}: max |diff| = {float(diff.max()):.3e}, "
          f"{100 * frac:.1f} % of the cells differ")
    assert not torch.equal(res["fast7"], res["canonical"])
    assert float(diff.max()) < 1e-14


def test_fast_math_is_off_by_default_and_leaves_canonical_alone():
    assert ops.Stencil3DTuning().fast_math is False
    T, iCp = fields((NZ, NY, NX), 14)
    a, b = T.clone(), T.clone()
    step(2, a, T, iCp, tuning=None)
    step(2, b, T, iCp, tuning=ops.Stencil3DTuning(fast_math=False))
    assert same_bits(a, b)


def test_refusals():
    assert ops.fast7_ok(COEF) and native().fast7_ok(tuple(COEF))
    bad = [ops.StencilCoef3.from_physics(0.0, DX, DY, DZ, DT),  # lam = 0: ax = 0
           ops.StencilCoef3.from_physics(LAM, DX, DY, DZ, float("inf")),  # dt*ax
           ops.StencilCoef3(-LAM, 1.0 / DX, float("inf"), 1.0 / DZ, DT),  # ay/ax
           ops.StencilCoef3(-LAM, 1.0 / DX, 1.0 / DY, float("nan"), DT)]  # az/ax
    T, iCp = fields((NZ, NY, NX), 15)
    T2 = torch.full((NZ, NY, NX), SENTINEL, dtype=torch.float64)
    box = [ops.interior_box(NX, NY, NZ)]
    for c in bad:
        assert not ops.fast7_ok(c) and not native().fast7_ok(tuple(c)), c
        for K, forward in ((1, False), (1, True), (2, False)):
            with pytest.raises(ValueError, match="fast7"):
                step(K, T2, T, iCp, coef=c, forward=forward)
        # the C++ entry points themselves (an invalid argument before any work)
        with pytest.raises(RuntimeError, match="invalid argument"):
            native().stencil3d_boxes(T2.data_ptr(), T.data_ptr(), iCp.data_ptr(), NX, NY, NZ, box,
                                     tuple(c), gpu=False, fast_math=True)
        for K in (1, 2):
            with pytest.raises(RuntimeError, match="invalid argument"):
                native().stencil3dk_boxes(K, T2.data_ptr(), T.data_ptr(), iCp.data_ptr(), NX, NY,
                                          NZ, box, tuple(c), gpu=False, fast_math=True)
    assert bool((T2 == SENTINEL).all())
    # lam = 0 is a fine canonical coefficient set: only fast_math refuses it
    step(2, T2, T, iCp, coef=bad[0], tuning=None)
    assert same_bits(T2[1:-1, 1:-1, 1:-1], T[1:-1, 1:-1, 1:-1])
    # the twins keep the canonical twins' argument checks
    with pytest.raises(RuntimeError, match="invalid argument"):
        native().stencil3d_boxes(T.data_ptr(), T.data_ptr(), iCp.data_ptr(), NX, NY, NZ, box,
                                 tuple(COEF), gpu=False, fast_math=True)  # in place
    with pytest.raises(RuntimeError, match="invalid argument"):
        native().stencil3dk_boxes(2, T2.data_ptr(), T.data_ptr(), iCp.data_ptr(), NX, NY, NZ,
                                  [(0, NX, 1, 2, 1, 2)], tuple(COEF), gpu=False, fast_math=True)
