"""Diffusion3D with two-step passes (temporal=2) on CPU loopback rank threads
against the NumPy golden model of the global grid of the overlap-4
decomposition (bitwise), the single-rank equivalence and the refusals."""
from types import SimpleNamespace

import numpy as np
import pytest

import golden3d
from helpers import run_loopback
from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig
from rocm_mpi_amd.parallel import implicit_grid as gg

NX, NY, NZ, NT, SEED, K = 14, 13, 12, 25, 1234, 2  # 25 steps: 12 passes and a remainder


def spmd3(rank, hub, temporal, dims, periods, n=(NX, NY, NZ), nt=NT, device="cpu"):
    """The model creates the grid (overlap 2K, halo width K for temporal=K)."""
    m = Diffusion3D(Diffusion3DConfig(nx=n[0], ny=n[1], nz=n[2], nt=nt, init="random", seed=SEED,
                                      dims=dims, periods=periods, quiet=True, temporal=temporal,
                                      device=device),
                    grid_kwargs=dict(loopback=(hub, rank)))
    g = m.g
    if temporal > 1:
        assert tuple(g.overlaps) == (2 * K,) * 3 and tuple(g.halowidths) == (K,) * 3
        assert m.plan(nt) == [K] * (nt // K) + [1] * (nt % K)
    m.step(nt)
    assert m.steps_done == nt
    Tv = m.gather_interior()
    out = (None if Tv is None else Tv.numpy().copy(), tuple(g.nxyz_g))
    m.close()
    return out


def golden_global(dims, periods, overlap, n=(NX, NY, NZ), nt=NT, seed=SEED):
    """golden3d.run3 on the global array of the decomposition with this overlap:
    dims*(n-overlap)+overlap cells on an open dimension; on a periodic one
    dims*(n-overlap) distinct cells and the golden model's two ghost cells."""
    ng = [d * (k - overlap) + (0 if p else overlap) for d, k, p in zip(dims, n, periods)]
    arr = [g + 2 if p else g for g, p in zip(ng, periods)]
    geom = SimpleNamespace(gx0=0, gy0=0, gz0=0, nxg=ng[0], nyg=ng[1], nzg=ng[2],
                           periodx=periods[0], periody=periods[1], periodz=periods[2])
    T0 = golden3d.random_field3(arr[0], arr[1], arr[2], geom, seed)
    return golden3d.run3(arr[0], arr[1], arr[2], nt, T0=T0, periods=periods), ng


CASES = [((2, 1, 1), (0, 0, 0)), ((1, 2, 1), (0, 0, 0)), ((1, 1, 2), (0, 0, 0)),
         ((2, 2, 2), (0, 0, 0)), ((1, 1, 2), (0, 0, 1))]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("dims,periods", CASES)
def test_loopback_ranks_with_two_step_passes_equal_golden_bitwise(dims, periods):
    P = dims[0] * dims[1] * dims[2]
    Tv, nxyz_g = run_loopback(P, spmd3, K, dims, periods, timeout=60)[0]
    G, ng = golden_global(dims, periods, 2 * K)
    assert list(nxyz_g) == ng
    inner = G[1:-1, 1:-1, 1:-1]
    assert Tv.shape == inner.shape  # every global cell once
    assert np.array_equal(bits(Tv), bits(inner))
    before = golden_global(dims, periods, 2 * K, nt=NT - 1)[0][1:-1, 1:-1, 1:-1]
    assert not np.array_equal(Tv, before)


def test_single_rank_two_step_passes_equal_one_step_passes_bitwise():
    a = run_loopback(1, spmd3, 2, (1, 1, 1), (0, 0, 0), timeout=60)[0]
    b = run_loopback(1, spmd3, 1, (1, 1, 1), (0, 0, 0), timeout=60)[0]
    assert a[1] == b[1] == (NX, NY, NZ)
    assert a[0].shape == (NZ - 2, NY - 2, NX - 2)
    assert np.array_equal(bits(a[0]), bits(b[0]))


def existing_grid(rank, hub, dims, overlaps, halowidths):
    gg.init_global_grid(NX, NY, NZ, dimx=dims[0], dimy=dims[1], dimz=dims[2], quiet=True,
                        loopback=(hub, rank), device="cpu", overlaps=overlaps,
                        halowidths=halowidths)
    try:
        Diffusion3D(Diffusion3DConfig(nx=NX, ny=NY, nz=NZ, quiet=True, temporal=2)).close()
        return "accepted"
    except ValueError as e:
        return str(e)
    finally:
        gg.finalize_global_grid()


def test_refusals():
    # overlap 2 with a neighbour in z
    out = run_loopback(2, existing_grid, (1, 1, 2), (2, 2, 2), (1, 1, 1), timeout=60)
    assert all("needs grid overlaps >= 4" in o for o in out), out
    # overlap 2 where no dimension has a neighbour, and overlap 4 where one has
    assert run_loopback(1, existing_grid, (1, 1, 1), (2, 2, 2), (1, 1, 1), timeout=60) == ["accepted"]
    assert run_loopback(2, existing_grid, (1, 1, 2), (2, 2, 4), (1, 1, 2),
                        timeout=60) == ["accepted"] * 2
    with pytest.raises(ValueError, match="perf variant"):
        Diffusion3DConfig(variant="ap", temporal=2).validate()
    with pytest.raises(ValueError, match="temporal must be one of"):
        Diffusion3DConfig(temporal=3).validate()
    Diffusion3DConfig(temporal=2).validate()
