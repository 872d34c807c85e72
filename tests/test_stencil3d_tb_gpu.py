"""The gfx950 two-step z-march (csrc/kernels/stencil3d_tb.hip) against its CPU
twin, bitwise, from a sentinel T2: strip, band and chunk seams, masked tails, the
scalar and unaligned paths, every instantiated tuning, guard bands, box lists
with gaps, 64-bit offsets."""
import itertools

import pytest
import torch

from rocm_mpi_amd import ops

pytestmark = pytest.mark.gpu

K = 2
COEF = ops.StencilCoef3.from_physics(1.3, 0.11, 0.07, 0.05, 3.1e-4)  # dx != dy != dz
# strips advance by 126 columns at 2 cells per lane: seams at 126 s +- 1, the
# masked tail, odd nx (1 cell per lane, seams at 62 s), a last strip of one column
NXS = [3, 4, 5, 125, 126, 127, 128, 129, 130, 252, 253, 254, 258]
NZS = [3, 4, 5, 6, 9]
CANARY, SENTINEL = 1234.5, -7.25
_ref_cache: dict = {}


def nys(R):
    return sorted({3, 4, R + 2, R + 3, 4 * R + 2, 4 * R + 3, 8 * R + 3})


def case(nx, ny, nz, uniform):
    """(T, iCp, CPU-twin result) of one shape, computed once; T2 starts as a
    sentinel so the faces must stay untouched."""
    key = (nx, ny, nz, uniform)
    if key not in _ref_cache:
        g = torch.Generator().manual_seed(hash(key) & 0xFFFF)
        T = torch.rand((nz, ny, nx), dtype=torch.float64, generator=g) * 2.0 - 1.0
        iCp = (torch.full((nz, ny, nx), 0.75, dtype=torch.float64) if uniform
               else torch.rand((nz, ny, nx), dtype=torch.float64, generator=g) * 1.5 + 0.5)
        want = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64)
        ops.stencil3dk_step(K, want, T, iCp, COEF)
        _ref_cache[key] = (T, iCp, want)
    return _ref_cache[key]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def check(nx, ny, nz, uniform, tn):
    T, iCp, want = case(nx, ny, nz, uniform)
    T2 = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64, device="cuda")
    ops.stencil3dk_step(K, T2, T.cuda(), iCp.cuda(), COEF, tuning=tn)
    assert same_bits(T2.cpu(), want), (nx, ny, nz, uniform, tn)


@pytest.mark.parametrize("nx", NXS)
@pytest.mark.parametrize("R", ops.TB_ROWS_3D)
def test_strip_seams(R, nx):
    tn = ops.Stencil3DTuning(tb_rows=R)
    for ny, nz, uniform in itertools.product((4, R + 3), (4, 6), (True, False)):
        check(nx, ny, nz, uniform, tn)


@pytest.mark.parametrize("R", ops.TB_ROWS_3D)
def test_band_seams(R):
    tn = ops.Stencil3DTuning(tb_rows=R)
    for nx, ny, uniform in itertools.product((5, 130), nys(R), (True, False)):
        check(nx, ny, 5, uniform, tn)


@pytest.mark.parametrize("chunk_z", [0, 1, 2, 3])
@pytest.mark.parametrize("R", ops.TB_ROWS_3D)
def test_chunk_seams(R, chunk_z):
    tn = ops.Stencil3DTuning(tb_rows=R, tb_chunk_z=chunk_z)
    for nx, nz, uniform in itertools.product((6, 129), NZS, (True, False)):
        check(nx, R + 3, nz, uniform, tn)


def test_every_instantiated_tuning():
    nz, ny, nx = 7, 13, 258
    T, iCp, want = case(nx, ny, nz, False)
    Tg, Ig = T.cuda(), iCp.cuda()
    for R, vec, nt, cz, remap in itertools.product(ops.TB_ROWS_3D, (1, 2), (0, 1, 2, 3),
                                                   (0, 1, 2, 3), (0, 1)):
        tn = ops.Stencil3DTuning(tb_rows=R, vec=vec, tb_nontemporal=nt, tb_chunk_z=cz,
                                 xcd_remap=remap)
        T2 = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64, device="cuda")
        ops.stencil3dk_step(K, T2, Tg, Ig, COEF, tuning=tn)
        assert same_bits(T2.cpu(), want), tn
    T2 = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64, device="cuda")
    for bad in (dict(tb_rows=3), dict(tb_rows=8), dict(vec=4), dict(tb_nontemporal=4),
                dict(tb_chunk_z=-1)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.stencil3dk_step(K, T2, Tg, Ig, COEF, tuning=ops.Stencil3DTuning(**bad))
    from rocm_mpi_amd._native import native

    with pytest.raises(RuntimeError, match="invalid argument"):  # an uninstantiated depth
        native().stencil3dk_boxes(3, T2.data_ptr(), Tg.data_ptr(), Ig.data_ptr(), nx, ny, nz,
                                  [ops.interior_box(nx, ny, nz)], tuple(COEF))
    torch.cuda.synchronize()
    assert bool((T2 == SENTINEL).all())  # refused before any work


def test_k1_forwards_to_the_one_step_kernel():
    nz, ny, nx = 7, 13, 258
    T, iCp, _ = case(nx, ny, nz, False)
    Tg, Ig = T.cuda(), iCp.cuda()
    a = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64, device="cuda")
    b = a.clone()
    ops.stencil3dk_step(1, a, Tg, Ig, COEF)
    ops.stencil3d_step(b, Tg, Ig, COEF)
    assert same_bits(a.cpu(), b.cpu())


@pytest.mark.parametrize("R", ops.TB_ROWS_3D)
def test_unaligned_views_take_the_scalar_path(R):
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

    T2 = view(torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64))
    ops.stencil3dk_step(K, T2, view(T), view(iCp), COEF, tuning=ops.Stencil3DTuning(tb_rows=R))
    assert same_bits(T2.cpu(), want)


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
    # what a pass writes on a tile with neighbours on every side
    "two_cells_in": lambda nx, ny, nz: [(2, nx - 2, 2, ny - 2, 2, nz - 2)],
    # x-width 1 and 3, a strip box between them, gaps everywhere
    "thin_and_gaps": lambda nx, ny, nz: [(1, 2, 1, ny - 1, 1, nz - 1), (4, 7, 2, ny - 2, 1, nz - 2),
                                         (9, nx - 3, 1, ny - 2, 2, nz - 1),
                                         (nx - 2, nx - 1, 3, ny - 1, 1, 3)],
}


@pytest.mark.parametrize("boxes", sorted(BOX_LISTS))
@pytest.mark.parametrize("R", ops.TB_ROWS_3D)
@pytest.mark.parametrize("nx", [131, 258])
def test_guard_bands_and_cells_outside_the_boxes(R, nx, boxes):
    nz, ny = 7, 2 * R + 3
    T, iCp, _ = case(nx, ny, nz, False)
    bl = BOX_LISTS[boxes](nx, ny, nz)
    margin = (ny * nx + 1) // 2 * 2 + 2 * nx  # more than a plane, even: the fields stay aligned
    want = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64)
    ops.stencil3dk_step(K, want, T, iCp, COEF, bl)
    inside = torch.zeros((nz, ny, nx), dtype=torch.bool)
    for x0, x1, y0, y1, z0, z1 in bl:
        inside[z0:z1, y0:y1, x0:x1] = True
    assert bool((want[~inside] == SENTINEL).all()) and not bool((want[inside] == SENTINEL).any())
    bT, vT = guarded(T, margin)
    bI, vI = guarded(iCp, margin)
    b2, v2 = guarded(torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64), margin)
    ops.stencil3dk_step(K, v2, vT, vI, COEF, bl, ops.Stencil3DTuning(tb_rows=R))
    torch.cuda.synchronize()
    assert margins_intact(b2, margin) and margins_intact(bT, margin) and margins_intact(bI, margin)
    assert same_bits(vT.cpu(), T) and same_bits(vI.cpu(), iCp)  # inputs unchanged
    got = v2.cpu()
    assert bool((got[~inside] == SENTINEL).all())  # all six faces and between the boxes
    assert same_bits(got, want)


def test_offsets_beyond_2_to_31_cells():
    """nz*ny*nx > 2^31 with a row width that is no strip multiple: three 3-plane
    z-slabs against the CPU twin run on the slab plus K z neighbours per side
    (the slab's planes are then K cells away from the sub-array's faces, or on
    the same side of the array's own face)."""
    nx, nz = 1292, 1290
    ny = 1290
    assert nz * ny * nx > 2**31
    geom = ops.TileGeometry3(0, 0, 0, nx, ny, nz, 1.0, 1.0, 1.0)
    T = torch.empty((nz, ny, nx), dtype=torch.float64, device="cuda")
    iCp = torch.empty_like(T)
    ops.init_random3d_(T, geom, seed=7, lo=-1.0, hi=1.0)
    ops.init_random3d_(iCp, geom, seed=8, lo=0.5, hi=2.0)
    T2 = torch.empty_like(T)
    ops.stencil3dk_step(K, T2, T, iCp, COEF)
    for za in (1, nz // 2 - 1, nz - 4):
        lo, hi = max(za - K, 0), min(za + 3 + K, nz)
        Ts, Is = T[lo:hi].cpu(), iCp[lo:hi].cpu()
        want = torch.zeros_like(Ts)
        ops.stencil3dk_step(K, want, Ts, Is, COEF)
        got = T2[za:za + 3, 1:-1, 1:-1].cpu()
        assert same_bits(got, want[za - lo:za - lo + 3, 1:-1, 1:-1]), za
    del T, T2, iCp
    torch.cuda.empty_cache()
