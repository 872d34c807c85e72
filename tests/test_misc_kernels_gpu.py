"""The HIP utility kernels of csrc/kernels/misc.hip against the independent
oracles of tests/misc_oracles.py, at sizes that run their grid-stride loops.

Each launcher caps its grid and walks the rest of the data in a stride loop.
The constants the sizes below were computed from (csrc/kernels/misc.hip):

  reduce       :142 kRedBlock = 256, :143 kRedMaxBlocks = 1024, :498 one block per
               256 * 8 cells: beyond 1024 * 2048 cells every thread strides;
  field_stats  :144 kStatsBlocks = 2048, :512 one block per 256 * 4 16-byte elements
               (2 cells each): S = 2048 * 256 elements per sweep of the grid;
  init_*, fill :366-368 grid_stride_blocks caps at 256 * 16 = 4096 blocks of 256
               threads; fill (:394) asks for n / 2 + 1 threads (16-byte stores);
  plane copies :119 kCopyBlock = 256, :435 min(blocks, 256 * 8 = 2048) in x;
  stream_*     the caller gives the block count; 256 threads, 4 x 16 bytes in flight.

A retuned launcher shows here which cases no longer cross its cap. Nothing in
this file provokes a fault: the refusal cases are argument checks that throw
before any launch."""
import dataclasses
import struct

import numpy as np
import pytest
import torch

import misc_oracles as mo
from rocm_mpi_amd import ops
from rocm_mpi_amd._native import native

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LO, HI = -3.5, 2.25
G = 512  # canary cells on each side of a guarded buffer (even: keeps 16-byte alignment)
CANARY = -1.2345678901234567e300


def tile_geometry(g):
    return ops.TileGeometry(**dataclasses.asdict(g))


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------- init_random --------------------------------
# (1025, 1031) = 1 056 775 cells > 4096 * 256 = 1 048 576 threads: the stride loop runs
@pytest.mark.parametrize("per", mo.PERIODS, ids=str)
@pytest.mark.parametrize("ny,nx", mo.TILES)
def test_init_random_bitwise(ny, nx, per):
    assert mo.TILES[-1][0] * mo.TILES[-1][1] > 4096 * 256
    A = torch.empty((ny, nx), dtype=torch.float64, device=DEV)
    for g in mo.init_geoms(ny, nx, per):
        for seed in mo.SEEDS:
            ops.init_random_(A, tile_geometry(g), seed=seed, lo=LO, hi=HI)
            want = mo.uniform_field(nx, ny, g, seed, LO, HI)
            assert np.array_equal(mo.bits(A.cpu().numpy()), mo.bits(want)), (g, seed)


@pytest.mark.parametrize("per", mo.PERIODS[1:], ids=str)
def test_init_random_periodic_tiles_are_images_of_the_full_field(per):
    """Decomposition invariance across the wrap: the ghost column / row of a
    periodic tile is the image of the far edge of the full (open) field."""
    nx, ny = 41, 37
    for g in mo.init_geoms(ny, nx, per):
        full = torch.empty((g.nyg, g.nxg), dtype=torch.float64, device=DEV)
        ops.init_random_(full, ops.TileGeometry(0, 0, g.nxg, g.nyg, g.dx, g.dy), seed=7)
        part = torch.empty((ny, nx), dtype=torch.float64, device=DEV)
        ops.init_random_(part, tile_geometry(g), seed=7)
        cols = torch.from_numpy(mo.global_index_1d(g.gx0, nx, g.nxg, g.periodx)).to(DEV)
        rows = torch.from_numpy(mo.global_index_1d(g.gy0, ny, g.nyg, g.periody)).to(DEV)
        assert torch.equal(part, full[rows][:, cols])


# ------------------------------ init_gaussian -------------------------------
def check_gaussian(ny, nx, g, lx, ly):
    T = torch.empty((ny, nx), dtype=torch.float64, device=DEV)
    ops.init_gaussian_(T, tile_geometry(g), lx, ly)
    twin = torch.empty((ny, nx), dtype=torch.float64)
    ops.init_gaussian_(twin, tile_geometry(g), lx, ly)
    want = mo.gaussian_field(nx, ny, g, lx, ly)
    dev, tol = mo.max_rel_dev(T.cpu().numpy(), want), mo.gaussian_tolerance(nx, ny, g, lx, ly)
    print(f"init_gaussian {ny}x{nx} {g}: max rel dev gpu {dev:.3e}, "
          f"cpu twin {mo.max_rel_dev(twin.numpy(), want):.3e}, bound {tol:.3e}")
    assert dev <= tol, (g, dev, tol)
    torch.testing.assert_close(T.cpu(), twin, rtol=4e-16, atol=1e-300)


@pytest.mark.parametrize("per", mo.PERIODS, ids=str)
@pytest.mark.parametrize("ny,nx", mo.TILES)
def test_init_gaussian_within_derived_bound(ny, nx, per):
    """Anisotropic (dx != dy), plain and staggered, every placement of
    ``init_geoms``; the large tile (grid-stride loop) at its far placement."""
    geoms = mo.init_geoms(ny, nx, per, stagger=ny * nx <= 128 * 128)
    if ny * nx > 128 * 128:
        geoms = geoms[-1:]  # a million exact rationals per placement
    for g in geoms:
        check_gaussian(ny, nx, g, mo.LX, mo.LY)


def test_init_gaussian_mid_grid_tile():
    check_gaussian(128, 128, mo.Geom(gx0=126, gy0=0, nxg=254, nyg=254, dx=10 / 254, dy=10 / 254),
                   10.0, 10.0)


# --------------------------------- reduce -----------------------------------
RED_CAP = 1024 * 8 * 256  # kRedMaxBlocks blocks x 8 cells per thread x kRedBlock threads
RED_SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, RED_CAP + 1, 5 * RED_CAP + 12345]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", RED_SIZES)
def test_reduce(n, offset):
    """All five ops: exact integer sums, all-ones, all-NaN, NaN / inf semantics
    and a +-7 planted at wave, block, grid-stride and end positions."""
    blocks = min(max(-(-n // (8 * 256)), 1), 1024)
    mo.check_reduce(ops.reduce, DEV, n, offset, blocks * 256, seed=n + offset)


# ------------------------------- field_stats --------------------------------
S = 2048 * 256  # kStatsBlocks * kRedBlock: 16-byte elements per sweep of a full grid
STATS_SIZES = [2 * (1 * 4 * S + 12345) + 1,  # unrolled loop, remainder loop, odd tail
               2 * (2 * 4 * S + 1) + 1,  # two unrolled rounds, one element of remainder, tail
               2 * 3 * S,  # remainder loop only, three rounds
               1, 2, 3, 2047, 2049]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", STATS_SIZES)
def test_field_stats(n, offset):
    """Aligned (16-byte loads) and on a view 8 bytes off (scalar loop)."""
    blocks = min(max(-(-(n // 2) // (4 * 256)), 1), 2048)
    sweep = blocks * 256  # threads: cells per sweep on the scalar path, half of them on the other
    extra = [sweep - 1, sweep, 2 * sweep - 1, 2 * sweep, 8 * sweep - 1, 8 * sweep, 2 * (n // 2) - 1]
    mo.check_field_stats(ops.field_stats, DEV, n, offset, 2 * sweep, seed=n + offset,
                         extra=extra)


# ----------------------------------- fill -----------------------------------
NAN = float("nan")


# 2 * 4096 * 256 + 3 cells: more 16-byte stores than the capped grid has threads, odd tail
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 4097, 2 * 4096 * 256 + 3])
def test_fill_bitwise_between_canaries(n, offset):
    """Aligned (16-byte stores + odd tail) and 8 bytes off (scalar kernel): the
    cells hold the value's bit pattern, the canary bands and the element before
    an offset view are untouched."""
    for v in (0.25, -0.0, float("inf"), NAN):
        buf = torch.full((G + offset + n + G,), CANARY, dtype=torch.float64, device=DEV)
        ops.fill_(buf[G + offset:G + offset + n], v)
        want = np.full(buf.numel(), CANARY)
        want[G + offset:G + offset + n] = v
        vbits = struct.unpack("<q", struct.pack("<d", v))[0]
        assert mo.bits(want)[G + offset] == vbits
        assert np.array_equal(mo.bits(buf.cpu().numpy()), mo.bits(want)), (n, offset, v)


# -------------------------------- plane copies ------------------------------
@pytest.mark.parametrize("name", mo.COPY_CASES)
def test_copy_planes(name):
    mo.check_copy_case(ops.copy_planes, name, DEV)


@pytest.mark.parametrize("name", ["narrow_8B_beyond_cap", "narrow_16B_beyond_cap",
                                  "wide_8B_beyond_cap", "complex128_narrow", "float16_wide"])
def test_copy_plane(name):
    mo.check_copy_case(lambda pairs: [ops.copy_plane(d, s) for d, s in pairs], name, DEV)


# ------------------------------ roofline probes -----------------------------
def probe_sizes(blocks):
    # 2 * (4 * blocks * 256 * 2 + 77) cells: two rounds of the 4x-unrolled loop, then 77
    # 16-byte elements of remainder (flat form, blocks = 0: 77 elements in one block)
    return [2, 510, 512, 514, 2 * (4 * blocks * 256 * 2 + 77)]


def guarded_vec(n, seed=None):
    """(buffer, 16-byte aligned view of n cells) with canaries before and after."""
    buf = torch.full((2 + n + 64,), CANARY, dtype=torch.float64, device=DEV)
    v = buf[2:2 + n]
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        v.copy_(torch.rand(n, generator=g, dtype=torch.float64) * 4 - 2)
    return buf, v


def canaries_intact(buf, n):
    edge = torch.cat([buf[:2], buf[2 + n:]])
    return bool((edge.view(torch.int64) == torch.full_like(edge, CANARY).view(torch.int64)).all())


@pytest.mark.parametrize("blocks", [0, 1, 3, 256, 4096])
@pytest.mark.parametrize("nt", [0, 1])
def test_stream_copy_bitwise(nt, blocks):
    for n in probe_sizes(blocks):
        (ba, a), (bb, b) = guarded_vec(n, 1), guarded_vec(n)
        a0 = a.clone()
        native().stream_copy(b.data_ptr(), a.data_ptr(), n, stream(), nt, blocks)
        torch.cuda.synchronize()
        assert torch.equal(b.view(torch.int64), a0.view(torch.int64)), (n, nt, blocks)
        assert torch.equal(a.view(torch.int64), a0.view(torch.int64))
        assert canaries_intact(ba, n) and canaries_intact(bb, n), (n, nt, blocks)


@pytest.mark.parametrize("blocks", [0, 1, 3, 256, 4096])
@pytest.mark.parametrize("nt", [0, 1])
def test_stream_triad_bitwise(nt, blocks):
    """c = a + s * b: a multiply, then an add (the build has no contraction)."""
    s = 1.0 / 3.0
    for n in probe_sizes(blocks):
        (ba, a), (bb, b), (bc, c) = guarded_vec(n, 1), guarded_vec(n, 2), guarded_vec(n)
        want = a + s * b  # torch: two kernels, two roundings
        native().stream_triad(c.data_ptr(), a.data_ptr(), b.data_ptr(), s, n, stream(), nt, blocks)
        torch.cuda.synchronize()
        assert torch.equal(c.view(torch.int64), want.view(torch.int64)), (n, nt, blocks)
        assert canaries_intact(ba, n) and canaries_intact(bb, n) and canaries_intact(bc, n)


@pytest.mark.parametrize("blocks", [0, 3])
def test_stream_probes_refuse_odd_or_unaligned(blocks):
    """Odd n or a pointer 8 bytes off a 16-byte boundary raises before any launch."""
    n = 512
    (ba, a), (bb, b) = guarded_vec(n, 1), guarded_vec(n, 2)
    (bc, c), (bo, o) = guarded_vec(n), guarded_vec(n)  # outputs: all canary
    off = 8  # bytes
    for nt in (0, 1):
        for args in ((o.data_ptr(), a.data_ptr(), n - 1), (o.data_ptr() + off, a.data_ptr(), n - 2),
                     (o.data_ptr(), a.data_ptr() + off, n - 2)):
            with pytest.raises(RuntimeError):
                native().stream_copy(*args, stream(), nt, blocks)
        for args in ((c.data_ptr(), a.data_ptr(), b.data_ptr(), 2.0, n - 1),
                     (c.data_ptr() + off, a.data_ptr(), b.data_ptr(), 2.0, n - 2),
                     (c.data_ptr(), a.data_ptr() + off, b.data_ptr(), 2.0, n - 2),
                     (c.data_ptr(), a.data_ptr(), b.data_ptr() + off, 2.0, n - 2)):
            with pytest.raises(RuntimeError):
                native().stream_triad(*args, stream(), nt, blocks)
    torch.cuda.synchronize()
    assert bool((o == CANARY).all()) and bool((c == CANARY).all())  # nothing was launched
