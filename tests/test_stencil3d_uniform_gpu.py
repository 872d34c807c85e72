"""The uniform-1/Cp variants of the gfx950 3D kernels (csrc/kernels/stencil3d.hip,
stencil3d_tb.hip; ``Stencil3DTuning.uniform``), bitwise against the CPU twin run
on a real array of 0.75. The kernel under test gets the value as an argument and
a device ``iCp`` full of NaN: any read of the array poisons every cell it
touches. The same launch with ``uniform=False`` and a real 0.75 array (the field
path, the parent's kernel) must give the same bits on the GPU itself."""
import dataclasses
import itertools

import pytest
import torch

from rocm_mpi_amd import ops
from rocm_mpi_amd._native import native
from test_stencil3d_gpu import COEF, case as case1, guarded, margins_intact, same_bits
from test_stencil3d_tb_gpu import BOX_LISTS, CANARY, SENTINEL, case as case2, nys

pytestmark = pytest.mark.gpu

VALUE = 0.75  # the uniform array of both imported case() helpers
# K = 1: the thin-box limit at width 8 (nx - 2 = 7, 8, 9), strip seams at 128, odd
# nx (one cell per lane); K = 2: the NXS of test_stencil3d_tb_gpu.py
NXS1 = [3, 4, 5, 9, 10, 11, 127, 128, 129, 130, 131, 257, 258]
NXS2 = [3, 4, 5, 125, 126, 127, 128, 129, 130, 252, 253, 254, 258]
CASE = {1: case1, 2: case2}
_dev_cache: dict = {}


def step(K, T2, T, iCp, boxes=None, tuning=None):
    if K == 1:
        ops.stencil3d_step(T2, T, iCp, COEF, boxes, tuning)
    else:
        ops.stencil3dk_step(K, T2, T, iCp, COEF, boxes, tuning)


def device_case(K, nx, ny, nz):
    """(T, 0.75 array, NaN array) on the device and the CPU twin's result."""
    key = (K, nx, ny, nz)
    if key not in _dev_cache:
        T, iCp, want = CASE[K](nx, ny, nz, True)
        assert bool((iCp == VALUE).all())
        _dev_cache[key] = (T.cuda(), iCp.cuda(), torch.full_like(T, float("nan")).cuda(), want)
    return _dev_cache[key]


def uni(tn):
    return dataclasses.replace(tn, uniform=True, uniform_value=VALUE)


def check(K, nx, ny, nz, tn):
    """Uniform variant with a NaN array == CPU twin == field path on the GPU."""
    T, I, Inan, want = device_case(K, nx, ny, nz)
    got = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64, device="cuda")
    step(K, got, T, Inan, tuning=uni(tn))
    assert same_bits(got.cpu(), want), (K, nx, ny, nz, tn)
    field = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64, device="cuda")
    step(K, field, T, I, tuning=tn)
    assert same_bits(got, field), (K, nx, ny, nz, tn)


# ------------------------------- one step ----------------------------------
@pytest.mark.parametrize("nx", NXS1)
@pytest.mark.parametrize("R,U", ops.TUNINGS_3D)
def test_march_strip_seams_and_thin_boxes(R, U, nx):
    tn = ops.Stencil3DTuning(rows=R, unroll=U)
    for ny, nz in itertools.product((4, R + 3), (4, U + 3)):
        check(1, nx, ny, nz, tn)


@pytest.mark.parametrize("R,U", ops.TUNINGS_3D)
def test_march_band_seams(R, U):
    tn = ops.Stencil3DTuning(rows=R, unroll=U)
    for nx, ny in itertools.product((5, 10, 130), sorted({R + 2, R + 3, 4 * R + 2, 4 * R + 3})):
        check(1, nx, ny, 5, tn)


@pytest.mark.parametrize("chunk_z", [0, 1, 2, 3])
@pytest.mark.parametrize("R,U", ops.TUNINGS_3D)
def test_march_chunk_seams(R, U, chunk_z):
    tn = ops.Stencil3DTuning(rows=R, unroll=U, chunk_z=chunk_z)
    for nx, nz in itertools.product((6, 129), range(3, 10)):
        check(1, nx, R + 3, nz, tn)


def test_march_every_instantiated_tuning():
    """Every (rows, unroll) x vec x non-temporal mask x xcd_remap; bit 1 of the
    mask (the 1/Cp loads) is accepted and has nothing to act on."""
    nz, ny, nx = 7, 13, 258
    for (R, U), vec, nt, remap in itertools.product(ops.TUNINGS_3D, (1, 2), (0, 1, 2, 3), (0, 1)):
        check(1, nx, ny, nz, ops.Stencil3DTuning(rows=R, unroll=U, vec=vec, nontemporal=nt,
                                                 xcd_remap=remap))
    T, _, Inan, _ = device_case(1, nx, ny, nz)
    T2 = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64, device="cuda")
    for bad in (dict(rows=3), dict(rows=8, unroll=2), dict(vec=4), dict(nontemporal=4)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            step(1, T2, T, Inan, tuning=uni(ops.Stencil3DTuning(**bad)))
    torch.cuda.synchronize()
    assert bool((T2 == SENTINEL).all())  # refused before any work


def test_k1_forwards_the_uniform_variant():
    nz, ny, nx = 7, 13, 258
    T, _, Inan, want = device_case(1, nx, ny, nz)
    T2 = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64, device="cuda")
    ops.stencil3dk_step(1, T2, T, Inan, COEF, tuning=uni(ops.Stencil3DTuning()))
    assert same_bits(T2.cpu(), want)


def test_uniform_value_none_reads_cell_zero():
    """``uniform_value=None``: the op reads iCp[0, 0, 0] (the 2D convention)."""
    nz, ny, nx = 5, 7, 130
    T, I, _, want = device_case(1, nx, ny, nz)
    T2 = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64, device="cuda")
    ops.stencil3d_step(T2, T, I, COEF, tuning=ops.Stencil3DTuning(uniform=True))
    assert same_bits(T2.cpu(), want)


# ------------------------------- two steps ---------------------------------
@pytest.mark.parametrize("nx", NXS2)
@pytest.mark.parametrize("R", ops.TB_ROWS_3D)
def test_tb_strip_seams(R, nx):
    tn = ops.Stencil3DTuning(tb_rows=R)
    for ny, nz in itertools.product((4, R + 3), (4, 6)):
        check(2, nx, ny, nz, tn)


@pytest.mark.parametrize("R", ops.TB_ROWS_3D)
def test_tb_band_seams(R):
    tn = ops.Stencil3DTuning(tb_rows=R)
    for nx, ny in itertools.product((5, 130), nys(R)):
        check(2, nx, ny, 5, tn)


@pytest.mark.parametrize("chunk_z", [0, 1, 2, 3])
@pytest.mark.parametrize("R", ops.TB_ROWS_3D)
def test_tb_chunk_seams(R, chunk_z):
    tn = ops.Stencil3DTuning(tb_rows=R, tb_chunk_z=chunk_z)
    for nx, nz in itertools.product((6, 129), range(3, 10)):
        check(2, nx, R + 3, nz, tn)


def test_tb_every_instantiated_tuning():
    nz, ny, nx = 7, 13, 258
    for R, vec, nt, remap in itertools.product(ops.TB_ROWS_3D, (1, 2), (0, 1, 2, 3), (0, 1)):
        check(2, nx, ny, nz, ops.Stencil3DTuning(tb_rows=R, vec=vec, tb_nontemporal=nt,
                                                 xcd_remap=remap))
    T, _, Inan, _ = device_case(2, nx, ny, nz)
    T2 = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64, device="cuda")
    for bad in (dict(tb_rows=3), dict(tb_rows=8), dict(vec=4), dict(tb_nontemporal=4),
                dict(tb_chunk_z=-1)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            step(2, T2, T, Inan, tuning=uni(ops.Stencil3DTuning(**bad)))
    torch.cuda.synchronize()
    assert bool((T2 == SENTINEL).all())


# ----------------------- alignment, guard bands ----------------------------
def off_by_8(src):
    """src in a device view 8 bytes off 16-byte alignment."""
    n = src.numel()
    base = torch.empty(n + 2, dtype=torch.float64, device="cuda")
    assert base.data_ptr() % 16 == 0
    v = base[1:n + 1].view(src.shape)
    v.copy_(src)
    assert v.data_ptr() % 16 == 8
    return v


@pytest.mark.parametrize("K", [1, 2])
def test_unaligned_icp_keeps_the_vector_path(K):
    """iCp 8 bytes off 16-byte alignment, T and T2 aligned, even nx: the uniform
    variant does not read the array, so its alignment must not demote the launch
    to one cell per lane (``stencil3d_vec`` is the launchers' own choice)."""
    nz, ny, nx = 5, 7, 130
    T, I, Inan, want = device_case(K, nx, ny, nz)
    bad = off_by_8(Inan)
    T2 = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64, device="cuda")
    assert T.data_ptr() % 16 == 0 and T2.data_ptr() % 16 == 0
    vec = native().stencil3d_vec
    assert vec(T2.data_ptr(), T.data_ptr(), bad.data_ptr(), nx, 2, True) == 2
    assert vec(T2.data_ptr(), T.data_ptr(), bad.data_ptr(), nx, 2, False) == 1  # the field path
    assert vec(T2.data_ptr(), T.data_ptr(), bad.data_ptr(), nx, 1, True) == 1
    assert vec(T2.data_ptr(), T.data_ptr(), bad.data_ptr(), nx + 1, 2, True) == 1  # odd nx
    assert vec(T2.data_ptr(), off_by_8(T).data_ptr(), I.data_ptr(), nx, 2, True) == 1
    for R in ops.TB_ROWS_3D:
        T2.fill_(SENTINEL)
        step(K, T2, T, bad, tuning=uni(ops.Stencil3DTuning(rows=R, tb_rows=R)))
        assert same_bits(T2.cpu(), want)
    # every field off alignment: the scalar march, still without a read of 1/Cp
    U2 = off_by_8(torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64))
    step(K, U2, off_by_8(T), bad, tuning=uni(ops.Stencil3DTuning()))
    assert same_bits(U2.cpu(), want)


def guard_tunings(K):
    if K == 1:
        return [ops.Stencil3DTuning(rows=R, unroll=U) for R, U in ops.TUNINGS_3D]
    return [ops.Stencil3DTuning(tb_rows=R) for R in ops.TB_ROWS_3D]


@pytest.mark.parametrize("boxes", sorted(BOX_LISTS))
@pytest.mark.parametrize("nx", [131, 258])
@pytest.mark.parametrize("K", [1, 2])
def test_guard_bands_and_cells_outside_the_boxes(K, nx, boxes):
    for tn in guard_tunings(K):
        R = tn.rows if K == 1 else tn.tb_rows
        nz, ny = 7, 2 * R + 3
        T, iCp, _ = CASE[K](nx, ny, nz, True)
        bl = BOX_LISTS[boxes](nx, ny, nz)
        margin = (ny * nx + 1) // 2 * 2 + 2 * nx  # more than a plane, even: T, T2 stay aligned
        want = torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64)
        step(K, want, T, iCp, bl)
        inside = torch.zeros((nz, ny, nx), dtype=torch.bool)
        for x0, x1, y0, y1, z0, z1 in bl:
            inside[z0:z1, y0:y1, x0:x1] = True
        assert bool((want[~inside] == SENTINEL).all())
        assert not bool((want[inside] == SENTINEL).any())
        nan = torch.full((nz, ny, nx), float("nan"), dtype=torch.float64)
        bT, vT = guarded(T, margin)
        bI, vI = guarded(nan, margin)
        b2, v2 = guarded(torch.full((nz, ny, nx), SENTINEL, dtype=torch.float64), margin)
        step(K, v2, vT, vI, bl, uni(tn))
        torch.cuda.synchronize()
        assert margins_intact(b2, margin) and margins_intact(bT, margin)
        assert margins_intact(bI, margin), tn
        assert same_bits(vT.cpu(), T) and bool(torch.isnan(vI).all())  # inputs unchanged
        got = v2.cpu()
        assert bool((got[~inside] == SENTINEL).all()), tn  # six faces and between the boxes
        assert same_bits(got, want), tn
    assert CANARY != SENTINEL


# ----------------------------- count_differing -----------------------------
CAP = 2048 * 8 * 256  # blocks x cells per thread x threads of the launcher's grid cap


@pytest.mark.parametrize("n", [1, 2, 4099, CAP + 1, 3 * CAP + 12345])
def test_count_differing_on_the_gpu(n):
    A = torch.full((n,), 0.75, dtype=torch.float64, device="cuda")
    assert ops.count_differing(A) == 0
    pos = sorted({p for p in (1, n // 2, n - 1, CAP - 1, CAP, 2 * CAP + 7) if 0 < p < n})
    for i, p in enumerate(pos):
        A[p] = 1.5
        assert ops.count_differing(A) == i + 1
    Z = torch.zeros(n, dtype=torch.float64, device="cuda")
    assert ops.count_differing(Z) == 0
    if n > 1:
        Z[n - 1] = -0.0
        assert ops.count_differing(Z) == 1
        N = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        assert ops.count_differing(N) == 0
        N.view(torch.int64)[n // 2] += 1  # another payload
        assert bool(torch.isnan(N).all()) and ops.count_differing(N) == 1
