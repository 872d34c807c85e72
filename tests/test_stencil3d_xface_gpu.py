"""The x-face path of the one-step 3D kernel (csrc/kernels/stencil3d.hip,
``Stencil3DTuning.xface``): boxes at most ``xface`` cells wide run a wave of
64/LX rows of LX = 8, 16 or 32 lanes marching along z. Bitwise against the CPU
twin and against today's dispatch (``xface = 0``) on the GPU, from a sentinel
T2: widths around every LX limit, faces at both array edges and at an odd
interior column, row counts that are no multiple of 64/LX, a z chunk seam and
a remainder, a two-box launch with a wide box, both arithmetics, field and
uniform 1/Cp (a device array full of NaN: any read of it poisons the cell),
both T2-store settings; the refusal; canary guard bands."""
import dataclasses
import itertools

import pytest
import torch

from rocm_mpi_amd import ops
from test_stencil3d_fast_cpu import COEF

pytestmark = pytest.mark.gpu

VALUE = 0.75
CANARY, SENTINEL = 1234.5, -7.25
SHAPES = [(37, 13, 70), (5, 3, 35)]  # (nz, ny, nx)
WIDTHS = [1, 7, 8, 9, 15, 16, 17, 31, 32]
_cache: dict = {}


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def fields(shape, uniform):
    """(T, iCp) of one shape on the host and the device, made once."""
    key = (shape, uniform)
    if key not in _cache:
        g = torch.Generator().manual_seed(hash(key) & 0xFFFF)
        T = torch.rand(shape, dtype=torch.float64, generator=g) * 2.0 - 1.0
        iCp = (torch.full(shape, VALUE, dtype=torch.float64) if uniform
               else torch.rand(shape, dtype=torch.float64, generator=g) * 0.5 + 0.5)
        dev_fac = torch.full(shape, float("nan"), dtype=torch.float64).cuda() if uniform \
            else iCp.cuda()
        _cache[key] = (T, iCp, T.cuda(), dev_fac)
    return _cache[key]


def tuning(fast, uniform, **kw):
    tn = ops.Stencil3DTuning(chunk_z=16, fast_math=fast, **kw)
    if uniform:
        tn = dataclasses.replace(tn, uniform=True, uniform_value=VALUE)
    return tn


def twin(shape, T, iCp, boxes, fast):
    want = torch.full(shape, SENTINEL, dtype=torch.float64)
    ops.stencil3d_step(want, T, iCp, COEF, boxes, ops.Stencil3DTuning(fast_math=fast))
    return want


def run(shape, Tg, fac, boxes, tn):
    got = torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")
    ops.stencil3d_step(got, Tg, fac, COEF, boxes, tn)
    return got


def face_boxes(shape, w):
    """Width-w boxes at x0 = 1, at x1 = nx-1 and at an odd interior x0 (those that
    fit), the last one on sub-ranges of y and z where the field has room."""
    nz, ny, nx = shape
    out = []
    for x0 in (1, nx - 1 - w, 3):
        if x0 < 1 or x0 + w > nx - 1 or any(b[0] == x0 for b in out):
            continue
        if x0 == 3 and ny > 4 and nz > 4:
            out.append((x0, x0 + w, 2, ny - 2, 2, nz - 2))
        else:
            out.append((x0, x0 + w, 1, ny - 1, 1, nz - 1))
    return out


def outside_kept(got, boxes):
    inside = torch.zeros(got.shape, dtype=torch.bool)
    for x0, x1, y0, y1, z0, z1 in boxes:
        inside[z0:z1, y0:y1, x0:x1] = True
    return bool((got[~inside] == SENTINEL).all()) and not bool((got[inside] == SENTINEL).any())


@pytest.mark.parametrize("uniform", [False, True], ids=["field", "uniform"])
@pytest.mark.parametrize("fast", [False, True], ids=["canonical", "fast7"])
@pytest.mark.parametrize("shape", SHAPES, ids=["37x13x70", "5x3x35"])
def test_face_path_equals_the_twin_and_todays_dispatch_bitwise(shape, fast, uniform):
    T, iCp, Tg, fac = fields(shape, uniform)
    for w in WIDTHS:
        for box in face_boxes(shape, w):
            want = twin(shape, T, iCp, [box], fast)
            today = run(shape, Tg, fac, [box], tuning(fast, uniform))
            assert same_bits(today.cpu(), want), ("xface=0", box)
            for nt in (0, 3):  # plain and non-temporal T2 stores
                for xf in sorted({w, 32}):
                    got = run(shape, Tg, fac, [box], tuning(fast, uniform, nontemporal=nt,
                                                            xface=xf))
                    assert same_bits(got, today), (box, nt, xf)
                    assert outside_kept(got.cpu(), [box]), (box, nt, xf)
            if w > 1:  # xface below the width: the box keeps today's path
                got = run(shape, Tg, fac, [box], tuning(fast, uniform, xface=w - 1))
                assert same_bits(got, today), (box, "xface < width")


@pytest.mark.parametrize("uniform", [False, True], ids=["field", "uniform"])
@pytest.mark.parametrize("fast", [False, True], ids=["canonical", "fast7"])
def test_a_width_33_box_falls_through_and_two_box_launches(fast, uniform):
    shape = SHAPES[0]
    nz, ny, nx = shape
    T, iCp, Tg, fac = fields(shape, uniform)
    box33 = (1, 34, 1, ny - 1, 1, nz - 1)
    want = twin(shape, T, iCp, [box33], fast)
    got = run(shape, Tg, fac, [box33], tuning(fast, uniform, xface=32))
    assert same_bits(got.cpu(), want)
    # a face box and a wide box in one launch; then faces of every lanes-per-row
    # class with a wide box between them
    for boxes in ([(1, 16, 1, ny - 1, 1, nz - 1), (16, nx - 1, 1, ny - 1, 1, nz - 1)],
                  [(1, 4, 1, ny - 1, 1, nz - 1), (4, 40, 2, ny - 1, 1, nz - 2),
                   (40, 53, 1, ny - 2, 2, nz - 1), (53, nx - 1, 1, ny - 1, 1, nz - 1)]):
        want = twin(shape, T, iCp, boxes, fast)
        for xf in (16, 32):
            got = run(shape, Tg, fac, boxes, tuning(fast, uniform, xface=xf))
            assert same_bits(got.cpu(), want), (boxes, xf)
            assert outside_kept(got.cpu(), boxes)


def test_xface_33_is_refused_before_any_launch():
    from rocm_mpi_amd._native import native

    shape = SHAPES[1]
    nz, ny, nx = shape
    T, iCp, Tg, fac = fields(shape, False)
    T2 = torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")
    box = [ops.interior_box(nx, ny, nz)]
    for bad in (33, -1):
        with pytest.raises(ValueError, match="xface"):
            ops.stencil3d_step(T2, Tg, fac, COEF, box, ops.Stencil3DTuning(xface=bad))
        with pytest.raises(RuntimeError, match="invalid argument"):
            native().stencil3d_boxes(T2.data_ptr(), Tg.data_ptr(), fac.data_ptr(), nx, ny, nz, box,
                                     tuple(COEF), xface=bad)
    torch.cuda.synchronize()
    assert bool((T2 == SENTINEL).all())
    # CPU tensors accept and ignore it
    a = torch.full(shape, SENTINEL, dtype=torch.float64)
    ops.stencil3d_step(a, T, iCp, COEF, box, ops.Stencil3DTuning(xface=16))
    assert same_bits(a, twin(shape, T, iCp, box, False))


def guarded(src, margin):
    """src inside a larger device buffer with canary margins on both sides."""
    n = src.numel()
    base = torch.full((n + 2 * margin,), CANARY, dtype=torch.float64, device="cuda")
    v = base[margin:margin + n].view(src.shape)
    v.copy_(src)
    return base, v


def margins_intact(base, margin):
    return bool((base[:margin] == CANARY).all()) and bool((base[-margin:] == CANARY).all())


@pytest.mark.parametrize("shape", SHAPES + [(6, 9, 131)], ids=["37x13x70", "5x3x35", "6x9x131"])
def test_guard_bands_around_the_face_path(shape):
    """Canary bands around every field; faces in the first and last rows, planes
    and columns of the interior, where a clamp that is off by one leaves the array."""
    nz, ny, nx = shape
    margin = (ny * nx + 1) // 2 * 2 + 2 * nx  # more than a plane
    bl = [(1, 2, 1, ny - 1, 1, nz - 1), (2, 11, 1, ny - 1, 1, nz - 1),
          (nx - 33, nx - 1, 1, ny - 1, 1, nz - 1), (12, 28, 1, ny - 1, 1, nz - 1)]
    for fast, uniform in itertools.product((False, True), repeat=2):
        T, iCp, _, _ = fields(shape, uniform)
        fac = torch.full_like(T, float("nan")) if uniform else iCp
        want = twin(shape, T, iCp, bl, fast)
        bT, vT = guarded(T, margin)
        bI, vI = guarded(fac, margin)
        b2, v2 = guarded(torch.full(shape, SENTINEL, dtype=torch.float64), margin)
        ops.stencil3d_step(v2, vT, vI, COEF, bl, tuning(fast, uniform, xface=32))
        torch.cuda.synchronize()
        assert margins_intact(b2, margin) and margins_intact(bT, margin), (fast, uniform)
        assert margins_intact(bI, margin), (fast, uniform)
        assert same_bits(vT.cpu(), T) and same_bits(vI.cpu(), fac)  # inputs unchanged
        got = v2.cpu()
        assert outside_kept(got, bl), (fast, uniform)
        assert same_bits(got, want), (fast, uniform)
