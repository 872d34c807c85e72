"""The gfx950 z-march kernel (csrc/kernels/stencil3d.hip) against its CPU twin,
bitwise: strip edges, masked tails, the scalar and unaligned paths, every
instantiated tuning, guard bands, thin boxes, 64-bit offsets; and the 3D initial
conditions on the GPU."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import golden3d
from rocm_mpi_amd import ops

pytestmark = pytest.mark.gpu

COEF = ops.StencilCoef3.from_physics(1.3, 0.11, 0.07, 0.05, 3.1e-4)  # dx != dy != dz
NXS = [3, 5, 127, 128, 129, 130, 131, 258]
_ref_cache: dict = {}


def case(nx, ny, nz, uniform):
    """(T, iCp, CPU-twin result) of one shape, computed once; T2 starts as a
    sentinel so the faces must stay untouched."""
    key = (nx, ny, nz, uniform)
    if key not in _ref_cache:
        rng = np.random.default_rng(hash(key) & 0xFFFF)
        T = torch.from_numpy(rng.uniform(-1.0, 1.0, (nz, ny, nx)))
        iCp = (torch.full((nz, ny, nx), 0.75, dtype=torch.float64) if uniform
               else torch.from_numpy(rng.uniform(0.5, 2.0, (nz, ny, nx))))
        want = torch.full((nz, ny, nx), -7.25, dtype=torch.float64)
        ops.stencil3d_step(want, T, iCp, COEF)
        _ref_cache[key] = (T, iCp, want)
    return _ref_cache[key]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.mark.parametrize("nx", NXS)
@pytest.mark.parametrize("R,U", ops.TUNINGS_3D)
def test_gpu_equals_cpu_twin_bitwise(R, U, nx):
    tn = ops.Stencil3DTuning(rows=R, unroll=U)
    for ny, nz, uniform in itertools.product(sorted({3, 4, R + 2, R + 3, 2 * R + 3}),
                                             sorted({3, 4, 5, U + 2, U + 3}), (True, False)):
        T, iCp, want = case(nx, ny, nz, uniform)
        T2 = torch.full((nz, ny, nx), -7.25, dtype=torch.float64, device="cuda")
        ops.stencil3d_step(T2, T.cuda(), iCp.cuda(), COEF, tuning=tn)
        assert same_bits(T2.cpu(), want), (R, U, nx, ny, nz, uniform)


def test_unaligned_views_take_the_scalar_path():
    """Fields 8 bytes off the 16-byte alignment, even nx."""
    nz, ny, nx = 5, 7, 130
    T, iCp, want = case(nx, ny, nz, False)
    n = nz * ny * nx

    def view(src):
        base = torch.empty(n + 2, dtype=torch.float64, device="cuda")
        assert base.data_ptr() % 16 == 0
        v = base[1:n + 1].view(nz, ny, nx)
        v.copy_(src)
        assert v.data_ptr() % 16 == 8
        return v

    T2 = view(torch.full((nz, ny, nx), -7.25, dtype=torch.float64))
    ops.stencil3d_step(T2, view(T), view(iCp), COEF)
    assert same_bits(T2.cpu(), want)


def test_every_instantiated_tuning():
    nz, ny, nx = 7, 13, 258
    T, iCp, want = case(nx, ny, nz, False)
    Tg, Ig = T.cuda(), iCp.cuda()
    for (R, U), vec, nt, cz, remap in itertools.product(ops.TUNINGS_3D, (1, 2), (0, 1, 2, 3),
                                                        (0, 2, 3), (0, 1)):
        tn = ops.Stencil3DTuning(rows=R, unroll=U, vec=vec, nontemporal=nt, chunk_z=cz,
                                 xcd_remap=remap)
        T2 = torch.full((nz, ny, nx), -7.25, dtype=torch.float64, device="cuda")
        ops.stencil3d_step(T2, Tg, Ig, COEF, tuning=tn)
        assert same_bits(T2.cpu(), want), tn
    for bad in (dict(rows=3), dict(rows=8, unroll=2), dict(vec=4), dict(nontemporal=4)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.stencil3d_step(torch.empty_like(Tg), Tg, Ig, COEF,
                               tuning=ops.Stencil3DTuning(**bad))


CANARY, SENTINEL = 1234.5, -7.25


def guarded(src, margin):
    """src inside a larger device buffer with canary margins on both sides."""
    n = src.numel()
    base = torch.full((n + 2 * margin,), CANARY, dtype=torch.float64, device="cuda")
    v = base[margin:margin + n].view(src.shape)
    v.copy_(src)
    return base, v


def margins_intact(base, margin):
    return bool((base[:margin] == CANARY).all()) and bool((base[-margin:] == CANARY).all())


BOX_LISTS = {
    "interior": lambda nx, ny, nz: [ops.interior_box(nx, ny, nz)],
    # x-width 1 and 3 (one thread per row), a strip box between them, gaps everywhere
    "thin_and_gaps": lambda nx, ny, nz: [(1, 2, 1, ny - 1, 1, nz - 1), (4, 7, 2, ny - 2, 1, nz - 2),
                                         (9, nx - 3, 1, ny - 2, 2, nz - 1),
                                         (nx - 2, nx - 1, 3, ny - 1, 1, 3)],
}


@pytest.mark.parametrize("boxes", sorted(BOX_LISTS))
@pytest.mark.parametrize("R,U", ops.TUNINGS_3D)
@pytest.mark.parametrize("nx", [131, 258])
def test_guard_bands_and_cells_outside_the_boxes(R, U, nx, boxes):
    nz, ny = 6, 2 * R + 3
    T, iCp, _ = case(nx, ny, nz, False)
    bl = BOX_LISTS[boxes](nx, ny, nz)
    margin = (ny * nx + 1) // 2 * 2 + 2 * nx  # more than a plane, even: the fields stay aligned
    want = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64)
    ops.stencil3d_step(want, T, iCp, COEF, bl)
    inside = torch.zeros((nz, ny, nx), dtype=torch.bool)
    for x0, x1, y0, y1, z0, z1 in bl:
        inside[z0:z1, y0:y1, x0:x1] = True
    assert bool((want[~inside] == SENTINEL).all()) and not bool((want[inside] == SENTINEL).any())
    bT, vT = guarded(T, margin)
    bI, vI = guarded(iCp, margin)
    b2, v2 = guarded(torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64), margin)
    ops.stencil3d_step(v2, vT, vI, COEF, bl, ops.Stencil3DTuning(rows=R, unroll=U))
    torch.cuda.synchronize()
    assert margins_intact(b2, margin) and margins_intact(bT, margin) and margins_intact(bI, margin)
    assert same_bits(vT.cpu(), T) and same_bits(vI.cpu(), iCp)  # inputs unchanged
    got = v2.cpu()
    assert bool((got[~inside] == SENTINEL).all())  # all six faces and between the boxes
    assert same_bits(got, want)


@pytest.mark.parametrize("nx", [1291, 1292])
def test_offsets_beyond_2_to_31_cells(nx):
    """nz*ny*nx > 2^31 with a row width that is no strip multiple (odd: scalar
    path, even: 16-byte path): three 3-plane z-slabs against the CPU twin run on
    the slab plus its z neighbours."""
    nz = ny = 1290
    assert nz * ny * nx > 2**31
    geom = ops.TileGeometry3(0, 0, 0, nx, ny, nz, 1.0, 1.0, 1.0)
    T = torch.empty((nz, ny, nx), dtype=torch.float64, device="cuda")
    iCp = torch.empty_like(T)
    ops.init_random3d_(T, geom, seed=7, lo=-1.0, hi=1.0)
    ops.init_random3d_(iCp, geom, seed=8, lo=0.5, hi=2.0)
    T2 = torch.empty_like(T)
    ops.stencil3d_step(T2, T, iCp, COEF)
    for za in (1, nz // 2 - 1, nz - 4):
        Ts, Is = T[za - 1:za + 4].cpu(), iCp[za - 1:za + 4].cpu()
        want = torch.zeros_like(Ts)
        ops.stencil3d_step(want, Ts, Is, COEF)
        got = T2[za:za + 3, 1:-1, 1:-1].cpu()
        assert same_bits(got, want[1:4, 1:-1, 1:-1]), za
    del T, T2, iCp
    torch.cuda.empty_cache()


def tile_geoms(nx, ny, nz, periodz):
    nxg, nyg = 2 * (nx - 2) + 2, 2 * (ny - 2) + 2
    nzg = 2 * (nz - 2) if periodz else 2 * (nz - 2) + 2
    common = dict(nxg=nxg, nyg=nyg, nzg=nzg, dx=10.0 / nxg, dy=7.0 / nyg, dz=5.0 / nzg,
                  xoff=0.0, yoff=0.0, zoff=0.0, periodx=0, periody=0, periodz=periodz)
    return [SimpleNamespace(gx0=nx - 2, gy0=ny - 2, gz0=c * (nz - 2), **common) for c in (0, 1)]


@pytest.mark.parametrize("periodz", [0, 1])
def test_initial_conditions_on_the_gpu(periodz):
    nz, ny, nx = 12, 9, 67
    lx, ly, lz = 10.0, 7.0, 5.0
    for g in tile_geoms(nx, ny, nz, periodz):
        geom = ops.TileGeometry3(**vars(g))
        A = torch.empty((nz, ny, nx), dtype=torch.float64, device="cuda")
        C = torch.empty((nz, ny, nx), dtype=torch.float64)
        ops.init_random3d_(A, geom, seed=99, lo=-1.0, hi=2.0)
        ops.init_random3d_(C, geom, seed=99, lo=-1.0, hi=2.0)
        assert same_bits(A.cpu(), C)
        ops.init_gaussian3d_(A, geom, lx, ly, lz)
        want = golden3d.gaussian_product3(nx, ny, nz, g, lx, ly, lz)
        tol = golden3d.gaussian_tolerance3(nx, ny, nz, g, lx, ly, lz)
        dev = float(np.max(np.abs(A.cpu().numpy() - want) / want))
        print(f"gaussian3d gpu periodz={periodz} gz0={g.gz0}: max rel dev {dev:.3e}, "
              f"bound {tol:.3e}")
        assert dev <= tol
