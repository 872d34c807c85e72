"""Diffusion3D on one MI355X: against the NumPy golden model, and multi-rank
(rank threads over the device loopback transport, 3D halos through the native
halo engine) against the single-rank run of the same global grid, bitwise."""
from types import SimpleNamespace

import numpy as np
import pytest

import golden3d
from helpers import run_loopback
from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig
from rocm_mpi_amd.parallel import implicit_grid as gg

pytestmark = pytest.mark.gpu
SEED = 1234


def spmd3(rank, hub, variant, n, nt, dims, periods):
    gg.init_global_grid(*n, dimx=dims[0], dimy=dims[1], dimz=dims[2], periodx=periods[0],
                        periody=periods[1], periodz=periods[2], quiet=True, loopback=(hub, rank))
    g = gg.global_grid()
    assert g.device.type == "cuda" and g.halo is not None  # the native halo engine
    m = Diffusion3D(Diffusion3DConfig(variant=variant, nx=n[0], ny=n[1], nz=n[2], nt=nt,
                                      init="random", seed=SEED, dims=dims, periods=periods,
                                      quiet=True))
    m.step(nt)
    Tv = m.gather_interior()
    out = None if Tv is None else Tv.numpy().copy()
    m.close()
    gg.finalize_global_grid()
    return out


@pytest.mark.parametrize("variant", ["perf", "ap"])
def test_one_gpu_equals_golden_bitwise(variant):
    nx, ny, nz, nt = 34, 21, 18, 30
    Tv = run_loopback(1, spmd3, variant, (nx, ny, nz), nt, (1, 1, 1), (0, 0, 0), timeout=60)[0]
    geom = SimpleNamespace(gx0=0, gy0=0, gz0=0, nxg=nx, nyg=ny, nzg=nz, periodx=0, periody=0,
                           periodz=0)
    G = golden3d.run3(nx, ny, nz, nt, T0=golden3d.random_field3(nx, ny, nz, geom, SEED))
    assert np.array_equal(Tv.view(np.int64),
                          np.ascontiguousarray(G[1:-1, 1:-1, 1:-1]).view(np.int64))


@pytest.mark.parametrize("dims,periods", [((2, 2, 2), (0, 0, 0)), ((1, 1, 2), (0, 0, 1))])
def test_rank_threads_equal_the_single_rank_run_bitwise(dims, periods):
    n, nt = (34, 12, 10), 24
    P = dims[0] * dims[1] * dims[2]
    Tv = run_loopback(P, spmd3, "perf", n, nt, dims, periods, timeout=120)[0]
    one = tuple(d * (k - 2) + 2 for d, k in zip(dims, n))
    ref = run_loopback(1, spmd3, "perf", one, nt, (1, 1, 1), periods, timeout=120)[0]
    assert Tv.shape == ref.shape
    assert np.array_equal(Tv.view(np.int64), ref.view(np.int64))
