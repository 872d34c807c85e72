"""The 3D (7-point) update on the CPU: the C++ twin and the torch twin against the
NumPy golden model (bitwise), box lists, argument refusals and the 3D initial
conditions against Python-integer / exact-rational oracles (tests/golden3d.py)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import golden3d
from rocm_mpi_amd import ops

SHAPES = [(3, 3, 3), (4, 5, 7), (9, 6, 130), (5, 11, 129)]  # (nz, ny, nx)
COEF = ops.StencilCoef3.from_physics(1.3, 0.11, 0.07, 0.05, 3.1e-4)  # dx != dy != dz


def fields(shape, seed=0):
    rng = np.random.default_rng(seed)
    T = rng.uniform(-1.0, 1.0, shape)
    iCp = rng.uniform(0.5, 2.0, shape)
    return T, iCp


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_twin_equals_golden_bitwise(shape):
    T, iCp = fields(shape, 1)
    want = golden3d.step3(T, iCp, *COEF)
    T2 = torch.from_numpy(T.copy())  # the twin leaves the faces: they start as T's
    ops.stencil3d_step(T2, torch.from_numpy(T), torch.from_numpy(iCp), COEF)
    assert np.array_equal(bits(T2.numpy()), bits(want))


@pytest.mark.parametrize("shape", SHAPES)
def test_torch_twin_equals_golden_bitwise(shape):
    T, iCp = fields(shape, 2)
    nz, ny, nx = shape
    want = golden3d.step3(T, iCp, *COEF)
    T2 = torch.from_numpy(T.copy())
    ops.stencil3d_torch(T2, torch.from_numpy(T), torch.from_numpy(iCp), COEF,
                        [ops.interior_box(nx, ny, nz)])
    assert np.array_equal(bits(T2.numpy()), bits(want))


def eight_boxes(nx, ny, nz):
    """8 disjoint boxes tiling the interior: every dimension cut once."""
    cx, cy, cz = 1 + (nx - 2) // 3, 1 + (ny - 2) // 2, 1 + (nz - 1) // 2
    xs, ys, zs = [(1, cx), (cx, nx - 1)], [(1, cy), (cy, ny - 1)], [(1, cz), (cz, nz - 1)]
    return [(x0, x1, y0, y1, z0, z1) for z0, z1 in zs for y0, y1 in ys for x0, x1 in xs]


@pytest.mark.parametrize("fn", ["native", "torch"])
def test_eight_boxes_equal_one_interior_launch(fn):
    nz, ny, nx = 9, 6, 130
    T, iCp = fields((nz, ny, nx), 3)
    Tt, It = torch.from_numpy(T), torch.from_numpy(iCp)
    sentinel = -7.25
    boxes = eight_boxes(nx, ny, nz)
    assert len(boxes) == 8 and all(b[1] > b[0] and b[3] > b[2] and b[5] > b[4] for b in boxes)
    outs = []
    for bl in ([ops.interior_box(nx, ny, nz)], boxes):
        T2 = torch.full((nz, ny, nx), sentinel, dtype=torch.float64)
        if fn == "native":
            ops.stencil3d_step(T2, Tt, It, COEF, bl)
        else:
            ops.stencil3d_torch(T2, Tt, It, COEF, bl)
        outs.append(T2.numpy())
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    want = golden3d.step3(T, iCp, *COEF)
    assert np.array_equal(bits(outs[1][1:-1, 1:-1, 1:-1]), bits(want[1:-1, 1:-1, 1:-1]))
    face = np.ones((nz, ny, nx), dtype=bool)
    face[1:-1, 1:-1, 1:-1] = False
    assert (outs[1][face] == sentinel).all()
    # a partial list: the cells of the boxes left out keep the sentinel
    T2 = torch.full((nz, ny, nx), sentinel, dtype=torch.float64)
    ops.stencil3d_step(T2, Tt, It, COEF, boxes[:3])
    inside = np.zeros((nz, ny, nx), dtype=bool)
    for x0, x1, y0, y1, z0, z1 in boxes[:3]:
        inside[z0:z1, y0:y1, x0:x1] = True
    assert (T2.numpy()[~inside] == sentinel).all()
    assert np.array_equal(bits(T2.numpy()[inside]), bits(want[inside]))


def test_refusals():
    nz, ny, nx = 5, 6, 7
    T = torch.zeros((nz, ny, nx), dtype=torch.float64)
    T2, iCp = T.clone(), T.clone()
    for box in [(0, 3, 1, 3, 1, 3), (1, nx, 1, 3, 1, 3), (1, 3, 0, 3, 1, 3), (1, 3, 1, ny, 1, 3),
                (1, 3, 1, 3, 0, 3), (1, 3, 1, 3, 1, nz)]:
        with pytest.raises(ValueError, match="outside the interior"):
            ops.stencil3d_step(T2, T, iCp, COEF, [box])
    with pytest.raises(ValueError, match="at most 8 boxes"):
        ops.stencil3d_step(T2, T, iCp, COEF, [(1, 2, 1, 2, 1, 2)] * 9)
    with pytest.raises(ValueError, match="must not alias"):
        ops.stencil3d_step(T, T, iCp, COEF)
    with pytest.raises(TypeError, match="float64"):
        ops.stencil3d_step(T2, T.float(), iCp, COEF)
    with pytest.raises(ValueError, match="contiguous"):
        ops.stencil3d_step(T2, torch.zeros((nz, ny, 2 * nx), dtype=torch.float64)[:, :, ::2], iCp,
                           COEF)
    small = torch.zeros((2, ny, nx), dtype=torch.float64)
    with pytest.raises(ValueError, match=">= 3 required"):
        ops.stencil3d_step(small.clone(), small, small.clone(), COEF)
    with pytest.raises(ValueError, match="shape"):
        ops.stencil3d_step(T2, T, iCp[:-1].contiguous(), COEF)
    # empty boxes are skipped, not refused
    T2.fill_(5.0)
    ops.stencil3d_step(T2, T, iCp, COEF, [(3, 3, 1, 2, 1, 2), (1, 2, 4, 2, 1, 2)])
    assert (T2 == 5.0).all()


def test_native_twin_refuses_on_its_own():
    """The C++ layer validates before any work too (callers outside ops)."""
    from rocm_mpi_amd._native import native

    T = torch.zeros((5, 6, 7), dtype=torch.float64)
    T2 = T.clone()
    args = (T.data_ptr(), T.data_ptr(), 7, 6, 5)
    with pytest.raises(RuntimeError, match="outside the interior"):
        native().stencil3d_boxes(T2.data_ptr(), *args, [(1, 7, 1, 2, 1, 2)], tuple(COEF), gpu=False)
    with pytest.raises(RuntimeError, match="at most 8 boxes"):
        native().stencil3d_boxes(T2.data_ptr(), *args, [(1, 2, 1, 2, 1, 2)] * 9, tuple(COEF),
                                 gpu=False)
    with pytest.raises(RuntimeError, match="in place"):
        native().stencil3d_boxes(T.data_ptr(), *args, [(1, 2, 1, 2, 1, 2)], tuple(COEF), gpu=False)
    with pytest.raises(RuntimeError, match="grid too small"):
        native().stencil3d_boxes(T2.data_ptr(), T.data_ptr(), T.data_ptr(), 7, 6, 2, [],
                                 tuple(COEF), gpu=False)


# ---------------------------------------------------------------------------
# initial conditions
# ---------------------------------------------------------------------------
def tile_geoms(nx, ny, nz, periodz=1):
    """Two z-neighbouring tiles (overlap 2) of a 2x2x2 grid, offset in all three
    dimensions; z periodic: the second tile runs over the far edge."""
    nxg, nyg = 2 * (nx - 2) + 2, 2 * (ny - 2) + 2
    nzg = 2 * (nz - 2) if periodz else 2 * (nz - 2) + 2
    common = dict(nxg=nxg, nyg=nyg, nzg=nzg, dx=10.0 / nxg, dy=7.0 / nyg, dz=5.0 / nzg,
                  xoff=0.0, yoff=0.0, zoff=0.0, periodx=0, periody=0, periodz=periodz)
    return [SimpleNamespace(gx0=nx - 2, gy0=ny - 2, gz0=c * (nz - 2), **common) for c in (0, 1)]


@pytest.mark.parametrize("periodz", [0, 1])
def test_init_random3d_against_python_integers(periodz):
    nz, ny, nx = 6, 5, 9
    seed = 2**63 + 12345
    tiles = []
    for g in tile_geoms(nx, ny, nz, periodz):
        A = torch.empty((nz, ny, nx), dtype=torch.float64)
        ops.init_random3d_(A, ops.TileGeometry3(**vars(g)), seed=seed, lo=-1.0, hi=2.0)
        want = golden3d.random_field3(nx, ny, nz, g, seed, -1.0, 2.0)
        assert np.array_equal(bits(A.numpy()), bits(want))
        tiles.append(A.numpy())
    # the overlap cells of the two z-neighbours agree
    assert np.array_equal(bits(tiles[0][-2:]), bits(tiles[1][:2]))
    if periodz:  # and around the period: the second tile's end is the first one's start
        assert np.array_equal(bits(tiles[1][-2:]), bits(tiles[0][:2]))
    assert len(np.unique(tiles[0])) == tiles[0].size  # no accidental repeats inside a tile


@pytest.mark.parametrize("periodz", [0, 1])
def test_init_gaussian3d_against_separable_product(periodz):
    nz, ny, nx = 6, 5, 9
    lx, ly, lz = 10.0, 7.0, 5.0
    for g in tile_geoms(nx, ny, nz, periodz):
        A = torch.empty((nz, ny, nx), dtype=torch.float64)
        ops.init_gaussian3d_(A, ops.TileGeometry3(**vars(g)), lx, ly, lz)
        want = golden3d.gaussian_product3(nx, ny, nz, g, lx, ly, lz)
        tol = golden3d.gaussian_tolerance3(nx, ny, nz, g, lx, ly, lz)
        dev = float(np.max(np.abs(A.numpy() - want) / want))
        print(f"gaussian3d periodz={periodz} gz0={g.gz0}: max rel dev {dev:.3e}, bound {tol:.3e}")
        assert tol < 1e-12
        assert dev <= tol
