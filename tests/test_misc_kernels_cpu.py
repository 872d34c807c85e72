"""The oracles of tests/misc_oracles.py against the C++ CPU twins of the utility
kernels (init_random, init_gaussian, reduce, field_stats, plane copies) and
against the torch fallbacks of ``rocm_mpi_amd.ops``: proves the oracles on a
machine without a GPU, before tests/test_misc_kernels_gpu.py holds the HIP
kernels to them. The twins share wrap_index / global_coord / uniform01 with the
device code, so only an oracle that shares nothing with them can tell a wrong
wrap or hash from a right one."""
import dataclasses
import math
import random

import numpy as np
import pytest
import torch

import misc_oracles as mo
from rocm_mpi_amd import ops

LO, HI = -3.5, 2.25


def tile_geometry(g):
    return ops.TileGeometry(**dataclasses.asdict(g))


def no_native(monkeypatch):
    """Route the CPU ops to their pure-torch ``else`` branches."""
    monkeypatch.setattr("rocm_mpi_amd.ops.stencil.has_native", lambda: False)


# ------------------------------- init_random --------------------------------
def test_uniform_field_equals_its_integer_twin():
    """The vectorised oracle against plain Python integers on ~200 seeded cells
    of a tile that straddles both periodic wraps, its four corners and its
    ghost row / column among them."""
    r = random.Random(5)
    for per in mo.PERIODS:
        for g in mo.init_geoms(37, 41, per):
            for seed in mo.SEEDS:
                f = mo.uniform_field(41, 37, g, seed, LO, HI)
                cells = [(0, 0), (40, 0), (0, 36), (40, 36), (3, 3), (4, 4)]
                cells += [(r.randrange(41), r.randrange(37)) for _ in range(3)]
                for ix, iy in cells:
                    assert f[iy, ix] == mo.uniform_cell(ix, iy, g, seed, LO, HI)
    assert 4 * 2 * 4 * 9 >= 200


def test_uniform_cell_first_values():
    """The generator's definition, worked by hand for idx = 0, seed = 0: the
    splitmix64 finaliser of the golden-ratio increment is the first output of
    the published splitmix64 stream, 0xE220A8397B1DCDAF."""
    g = mo.Geom(0, 0, 8, 8, 1.0, 1.0)
    assert mo.uniform_cell(0, 0, g, 0, 0.0, 1.0) == (0xE220A8397B1DCDAF >> 11) * 2.0**-53
    gp = mo.Geom(0, 0, 8, 8, 1.0, 1.0, periodx=1, periody=1)  # ghost corner -> global (7, 7)
    assert mo.uniform_cell(0, 0, gp, 9, LO, HI) == mo.uniform_cell(7, 7, g, 9, LO, HI)
    assert mo.uniform_cell(1, 1, gp, 9, LO, HI) == mo.uniform_cell(0, 0, g, 9, LO, HI)


@pytest.mark.parametrize("per", mo.PERIODS, ids=str)
@pytest.mark.parametrize("ny,nx", mo.TILES)
def test_init_random_cpu_bitwise(ny, nx, per):
    A = torch.empty((ny, nx), dtype=torch.float64)
    for g in mo.init_geoms(ny, nx, per):
        for seed in mo.SEEDS:
            ops.init_random_(A, tile_geometry(g), seed=seed, lo=LO, hi=HI)
            want = mo.uniform_field(nx, ny, g, seed, LO, HI)
            assert np.array_equal(mo.bits(A.numpy()), mo.bits(want)), (g, seed)
            assert LO <= want.min() and want.max() < HI


@pytest.mark.parametrize("per", mo.PERIODS[1:], ids=str)
def test_init_random_cpu_periodic_tiles_are_images_of_the_full_field(per):
    """Decomposition invariance across the wrap: the ghost column / row of a
    periodic tile is the image of the far edge of the full (open) field."""
    nx, ny = 41, 37
    for g in mo.init_geoms(ny, nx, per):
        full = torch.empty((g.nyg, g.nxg), dtype=torch.float64)
        ops.init_random_(full, ops.TileGeometry(0, 0, g.nxg, g.nyg, g.dx, g.dy), seed=7)
        part = torch.empty((ny, nx), dtype=torch.float64)
        ops.init_random_(part, tile_geometry(g), seed=7)
        cols = mo.global_index_1d(g.gx0, nx, g.nxg, g.periodx)
        rows = mo.global_index_1d(g.gy0, ny, g.nyg, g.periody)
        if g.gx0 == 0 and g.periodx:
            assert cols[0] == g.nxg - 1 and cols[1] == 0
        assert torch.equal(part, full[torch.from_numpy(rows)][:, torch.from_numpy(cols)])


# ------------------------------ init_gaussian -------------------------------
def gaussian_dev(fn, ny, nx, g):
    """Largest relative deviation of ``fn``'s field from the exact oracle, and the bound."""
    T = torch.empty((ny, nx), dtype=torch.float64)
    fn(T, tile_geometry(g), mo.LX, mo.LY)
    return (mo.max_rel_dev(T.numpy(), mo.gaussian_field(nx, ny, g, mo.LX, mo.LY)),
            mo.gaussian_tolerance(nx, ny, g, mo.LX, mo.LY))


@pytest.mark.parametrize("per", mo.PERIODS, ids=str)
@pytest.mark.parametrize("ny,nx", mo.TILES)
def test_init_gaussian_cpu_within_derived_bound(ny, nx, per):
    geoms = mo.init_geoms(ny, nx, per, stagger=ny * nx <= 128 * 128)
    if ny * nx > 128 * 128:
        geoms = geoms[-1:]  # the large tile: the far placement only (a million rationals each)
    for g in geoms:
        dev, tol = gaussian_dev(ops.init_gaussian_, ny, nx, g)
        print(f"init_gaussian_cpu {ny}x{nx} {g}: max rel dev {dev:.3e}, bound {tol:.3e}")
        assert dev <= tol, (g, dev, tol)


def test_init_gaussian_cpu_mid_grid_tile():
    """A tile in the middle of a multi-rank grid (tests/test_kernels_gpu.py's)."""
    g = mo.Geom(gx0=126, gy0=0, nxg=254, nyg=254, dx=10 / 254, dy=10 / 254)
    T = torch.empty((128, 128), dtype=torch.float64)
    ops.init_gaussian_(T, tile_geometry(g), 10.0, 10.0)
    tol = mo.gaussian_tolerance(128, 128, g, 10.0, 10.0)
    assert 1.0e-13 < tol < 1.1e-13  # the number in the oracle's docstring
    assert mo.max_rel_dev(T.numpy(), mo.gaussian_field(128, 128, g, 10.0, 10.0)) <= tol


def test_gaussian_oracle_tells_a_wrong_wrap():
    """Sensitivity of the bound: the exact field of a tile shifted by one cell,
    or taken as open where it is periodic, is orders of magnitude outside it."""
    g = mo.init_geoms(128, 128, (1, 1))[1]
    want = mo.gaussian_field(128, 128, g, mo.LX, mo.LY)
    tol = mo.gaussian_tolerance(128, 128, g, mo.LX, mo.LY)
    shifted = dataclasses.replace(g, gx0=g.gx0 + 1)
    unwrapped = dataclasses.replace(g, periodx=0)
    for wrong in (shifted, unwrapped):
        dev = np.abs(mo.gaussian_field(128, 128, wrong, mo.LX, mo.LY) - want) / want
        assert dev.max() > 1e6 * tol
    # a one-cell shift shows on every column but the one whose neighbour is its mirror
    # image about the centre (here across the wrap: the grid is exactly LX long)
    dev = np.abs(mo.gaussian_field(128, 128, shifted, mo.LX, mo.LY) - want) / want
    assert ((dev > 1e3 * tol).sum(axis=1) >= 127).all()


# --------------------------- reduce / field_stats ---------------------------
RED_SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2**16 + 3]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", RED_SIZES)
def test_reduce_cpu(n, offset):
    mo.check_reduce(ops.reduce, "cpu", n, offset, 256, seed=n + offset)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", RED_SIZES)
def test_field_stats_cpu(n, offset):
    mo.check_field_stats(ops.field_stats, "cpu", n, offset, 512, seed=n + offset)


@pytest.mark.parametrize("n", [1, 2, 3, 257, 2049])
def test_torch_fallbacks_have_the_native_semantics(n, monkeypatch):
    """The ``else`` branches of ops.reduce and ops.field_stats (no extension)
    against the same oracles, special values included: max / min / maxabs
    ignore NaN there too."""
    no_native(monkeypatch)
    assert not ops.stencil._use_native_cpu()
    mo.check_reduce(ops.reduce, "cpu", n, 0, 64, seed=n)
    mo.check_field_stats(ops.field_stats, "cpu", n, 0, 64, seed=n)


def test_torch_fallback_agrees_with_native_on_special_fields(monkeypatch):
    fields = [a for n in (1, 5, 300) for _, a in mo._special_fields(n, n, list(range(n)))]
    native_res = [[float(ops.reduce(torch.from_numpy(a), op)) for op in mo.reduce_expected(a)]
                  + list(ops.field_stats(torch.from_numpy(a))) for a in fields]
    no_native(monkeypatch)
    for a, want in zip(fields, native_res):
        got = [float(ops.reduce(torch.from_numpy(a), op)) for op in mo.reduce_expected(a)]
        got += list(ops.field_stats(torch.from_numpy(a)))
        finite_sum = math.isfinite(want[0])  # the order of a finite float sum is free
        assert all(mo.same(g, w) for g, w in list(zip(got, want))[1 if finite_sum else 0:]), (got, want)
        if finite_sum:
            assert got[0] == pytest.approx(want[0], rel=1e-13, abs=1e-13)


@pytest.mark.parametrize("per", mo.PERIODS, ids=str)
def test_init_gaussian_torch_fallback(per, monkeypatch):
    """ops.init_gaussian_ without the extension: within the derived bound of the
    exact oracle, and within two ulps (one per exp: 2 * 2**-52) of the native CPU twin."""
    ny, nx = 37, 41
    for g in mo.init_geoms(ny, nx, per, stagger=True):
        nat = torch.empty((ny, nx), dtype=torch.float64)
        ops.init_gaussian_(nat, tile_geometry(g), mo.LX, mo.LY)
        with monkeypatch.context() as m:
            no_native(m)
            dev, tol = gaussian_dev(ops.init_gaussian_, ny, nx, g)
            fb = torch.empty((ny, nx), dtype=torch.float64)
            ops.init_gaussian_(fb, tile_geometry(g), mo.LX, mo.LY)
        assert dev <= tol, (g, dev, tol)
        torch.testing.assert_close(fb, nat, rtol=2.0**-51, atol=0.0)


# -------------------------------- plane copies ------------------------------
@pytest.mark.parametrize("name", mo.COPY_CASES)
def test_copy_planes_cpu(name):
    mo.check_copy_case(ops.copy_planes, name, "cpu")


@pytest.mark.parametrize("name", ["narrow_8B_beyond_cap", "edge_129", "complex128_narrow",
                                  "float16_wide"])
def test_copy_plane_cpu(name):
    mo.check_copy_case(lambda pairs: [ops.copy_plane(d, s) for d, s in pairs], name, "cpu")
