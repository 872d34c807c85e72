"""The two-step 3D pass on the CPU: the C++ twin and the torch fallback against
two steps of the NumPy golden model (bitwise), box lists with gaps against the
crop of two full-interior one-step calls, argument refusals, and K = 1."""
import numpy as np
import pytest
import torch

import golden3d
from rocm_mpi_amd import ops

SHAPES = [(3, 3, 3), (3, 4, 5), (4, 5, 7), (5, 3, 4), (11, 9, 12)]  # (nz, ny, nx)
COEF = ops.StencilCoef3.from_physics(1.3, 0.11, 0.07, 0.05, 3.1e-4)  # dx != dy != dz
SENTINEL = -7.25


def fields(shape, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, shape), rng.uniform(0.5, 2.0, shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def golden2(T, iCp):
    return golden3d.step3(golden3d.step3(T, iCp, *COEF), iCp, *COEF)


@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_twin_equals_two_golden_steps_bitwise(shape):
    T, iCp = fields(shape, 1)
    want = golden2(T, iCp)
    T2 = torch.from_numpy(T.copy())  # the pass leaves the faces: they start as T's
    ops.stencil3dk_step(2, T2, torch.from_numpy(T), torch.from_numpy(iCp), COEF)
    assert np.array_equal(bits(T2.numpy()), bits(want))


@pytest.mark.parametrize("shape", SHAPES)
def test_torch_fallback_equals_two_golden_steps_bitwise(shape):
    T, iCp = fields(shape, 2)
    nz, ny, nx = shape
    want = golden2(T, iCp)
    T2 = torch.from_numpy(T.copy())
    ops.stencil3dk_torch(2, T2, torch.from_numpy(T), torch.from_numpy(iCp), COEF,
                         [ops.interior_box(nx, ny, nz)])
    assert np.array_equal(bits(T2.numpy()), bits(want))


def gap_boxes(nx, ny, nz):
    """Boxes with gaps between them, one of them 1 cell wide."""
    return [(1, 2, 1, ny - 1, 1, nz - 1), (4, 7, 2, ny - 2, 1, nz - 2),
            (8, nx - 2, 1, ny - 2, 2, nz - 1), (nx - 2, nx - 1, 3, ny - 1, 1, 3)]


@pytest.mark.parametrize("fn", ["native", "torch"])
def test_box_lists_with_gaps(fn):
    nz, ny, nx = 11, 9, 12
    T, iCp = fields((nz, ny, nx), 3)
    Tt, It = torch.from_numpy(T), torch.from_numpy(iCp)
    # two full-interior one-step calls
    S1, S2 = Tt.clone(), Tt.clone()
    ops.stencil3d_step(S1, Tt, It, COEF)
    ops.stencil3d_step(S2, S1, It, COEF)
    boxes = gap_boxes(nx, ny, nz)
    inside = np.zeros((nz, ny, nx), dtype=bool)
    for x0, x1, y0, y1, z0, z1 in boxes:
        inside[z0:z1, y0:y1, x0:x1] = True
    assert inside.any() and not inside[1:-1, 1:-1, 1:-1].all()
    T2 = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64)
    if fn == "native":
        ops.stencil3dk_step(2, T2, Tt, It, COEF, boxes)
    else:
        ops.stencil3dk_torch(2, T2, Tt, It, COEF, boxes)
    got = T2.numpy()
    assert (got[~inside] == SENTINEL).all()
    assert np.array_equal(bits(got[inside]), bits(S2.numpy()[inside]))
    assert np.array_equal(bits(Tt.numpy()), bits(T)) and np.array_equal(bits(It.numpy()), bits(iCp))


def test_refusals_before_any_write():
    nz, ny, nx = 5, 6, 7
    T = torch.zeros((nz, ny, nx), dtype=torch.float64)
    iCp = T.clone()
    T2 = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64)
    for K in (0, 3, 4, -1):
        with pytest.raises(ValueError, match="not instantiated"):
            ops.stencil3dk_step(K, T2, T, iCp, COEF)
    with pytest.raises(ValueError, match="must not alias"):
        ops.stencil3dk_step(2, T, T, iCp, COEF)
    for box in [(0, 3, 1, 3, 1, 3), (1, nx, 1, 3, 1, 3), (1, 3, 0, 3, 1, 3), (1, 3, 1, ny, 1, 3),
                (1, 3, 1, 3, 0, 3), (1, 3, 1, 3, 1, nz)]:
        with pytest.raises(ValueError, match="outside the interior"):
            ops.stencil3dk_step(2, T2, T, iCp, COEF, [(1, 2, 1, 2, 1, 2), box])
    with pytest.raises(ValueError, match="at most 8 boxes"):
        ops.stencil3dk_step(2, T2, T, iCp, COEF, [(1, 2, 1, 2, 1, 2)] * 9)
    with pytest.raises(TypeError, match="float64"):
        ops.stencil3dk_step(2, T2, T.float(), iCp, COEF)
    with pytest.raises(ValueError, match="shape"):
        ops.stencil3dk_step(2, T2, T, iCp[:-1].contiguous(), COEF)
    small = torch.zeros((2, ny, nx), dtype=torch.float64)
    with pytest.raises(ValueError, match=">= 3 required"):
        ops.stencil3dk_step(2, small.clone(), small, small.clone(), COEF)
    assert (T2 == SENTINEL).all()


def test_native_twin_refuses_on_its_own():
    from rocm_mpi_amd._native import native

    T = torch.zeros((5, 6, 7), dtype=torch.float64)
    T2 = torch.full((5, 6, 7), SENTINEL, dtype=torch.float64)
    args = (T.data_ptr(), T.data_ptr(), 7, 6, 5)
    with pytest.raises(RuntimeError, match="outside the interior"):
        native().stencil3dk_boxes(2, T2.data_ptr(), *args, [(1, 7, 1, 2, 1, 2)], tuple(COEF),
                                  gpu=False)
    with pytest.raises(RuntimeError, match="at most 8 boxes"):
        native().stencil3dk_boxes(2, T2.data_ptr(), *args, [(1, 2, 1, 2, 1, 2)] * 9, tuple(COEF),
                                  gpu=False)
    with pytest.raises(RuntimeError, match="in place"):
        native().stencil3dk_boxes(2, T.data_ptr(), *args, [(1, 2, 1, 2, 1, 2)], tuple(COEF),
                                  gpu=False)
    with pytest.raises(RuntimeError, match="invalid argument"):
        native().stencil3dk_boxes(0, T2.data_ptr(), *args, [(1, 2, 1, 2, 1, 2)], tuple(COEF),
                                  gpu=False)
    assert (T2 == SENTINEL).all()
    assert native().stencil3dk_has(1) and native().stencil3dk_has(2)
    assert not native().stencil3dk_has(3) and not native().stencil3dk_has(0)
    assert tuple(k for k in range(8) if native().stencil3dk_has(k)) == ops.TEMPORAL_3D
    assert tuple(r for r in range(10) if native().stencil3dk_has_rows(r)) == ops.TB_ROWS_3D


def test_k1_is_the_one_step_op():
    nz, ny, nx = 11, 9, 12
    T, iCp = fields((nz, ny, nx), 4)
    Tt, It = torch.from_numpy(T), torch.from_numpy(iCp)
    boxes = gap_boxes(nx, ny, nz)
    for bl in (None, boxes):
        a = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64)
        b = a.clone()
        ops.stencil3dk_step(1, a, Tt, It, COEF, bl)
        ops.stencil3d_step(b, Tt, It, COEF, bl)
        assert np.array_equal(bits(a.numpy()), bits(b.numpy()))
