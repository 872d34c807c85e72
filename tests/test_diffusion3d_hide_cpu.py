"""Diffusion3D ``variant="perf_hide"`` on CPU loopback rank threads (the boxes of
the frame / interior split run in sequence: frame, exchange, interior): bitwise
the ``perf`` run of the same grid and the NumPy golden model of the global grid,
for one- and two-step passes; fast7 against the fast7 ``perf`` run; refusals."""
import numpy as np
import pytest

from helpers import run_loopback
from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig
from test_diffusion3d_tb_cpu import CASES, NT, NX, NY, NZ, SEED, bits, golden_global

B_WIDTH = (3, 2, 2)  # an interior box remains on the 14 x 13 x 12 tile, overlap 2 and 4


def spmd_hide(rank, hub, variant, temporal, dims, periods, fast_math=False, b_width=B_WIDTH,
              n=(NX, NY, NZ), nt=NT, device="cpu", expect_inner=None):
    m = Diffusion3D(Diffusion3DConfig(variant=variant, nx=n[0], ny=n[1], nz=n[2], nt=nt,
                                      init="random", seed=SEED, dims=dims, periods=periods,
                                      quiet=True, temporal=temporal, fast_math=fast_math,
                                      b_width=b_width, device=device),
                    grid_kwargs=dict(loopback=(hub, rank)))
    assert m.plan(nt) == [temporal] * (nt // temporal) + [1] * (nt % temporal)  # as perf's
    if variant == "perf_hide" and expect_inner is not None:
        frame, inner = m.hide_boxes(temporal)
        assert (inner is not None) == expect_inner and len(frame) <= 6
    m.step(nt)
    assert m.steps_done == nt
    Tv = m.gather_interior()
    out = None if Tv is None else Tv.numpy().copy()
    m.close()
    return out


@pytest.mark.parametrize("temporal", [1, 2])
@pytest.mark.parametrize("dims,periods", CASES)
def test_perf_hide_equals_perf_and_golden_bitwise(dims, periods, temporal):
    P = dims[0] * dims[1] * dims[2]
    hide = run_loopback(P, spmd_hide, "perf_hide", temporal, dims, periods, expect_inner=True,
                        timeout=60)[0]
    perf = run_loopback(P, spmd_hide, "perf", temporal, dims, periods, timeout=60)[0]
    assert hide.shape == perf.shape
    assert np.array_equal(bits(hide), bits(perf))
    G, _ = golden_global(dims, periods, 2 * temporal)
    inner = G[1:-1, 1:-1, 1:-1]
    assert hide.shape == inner.shape
    assert np.array_equal(bits(hide), bits(inner))


@pytest.mark.parametrize("temporal", [1, 2])
def test_default_b_width_leaves_no_interior_on_a_small_tile(temporal):
    """b_width (16, 2, 2) on 14 cells in x: every pass is the one perf launch."""
    dims, periods = (2, 2, 2), (0, 0, 0)
    hide = run_loopback(8, spmd_hide, "perf_hide", temporal, dims, periods, b_width=(16, 2, 2),
                        expect_inner=False, timeout=60)[0]
    perf = run_loopback(8, spmd_hide, "perf", temporal, dims, periods, timeout=60)[0]
    assert np.array_equal(bits(hide), bits(perf))


@pytest.mark.parametrize("temporal", [1, 2])
def test_fast_math_equals_the_fast7_perf_run_bitwise(temporal):
    dims, periods = (1, 1, 2), (0, 0, 1)
    hide = run_loopback(2, spmd_hide, "perf_hide", temporal, dims, periods, fast_math=True,
                        expect_inner=True, timeout=60)[0]
    perf = run_loopback(2, spmd_hide, "perf", temporal, dims, periods, fast_math=True,
                        timeout=60)[0]
    canon = run_loopback(2, spmd_hide, "perf", temporal, dims, periods, timeout=60)[0]
    assert np.array_equal(bits(hide), bits(perf))
    assert not np.array_equal(bits(hide), bits(canon))  # fast7 ran: rounding-close only


def test_one_rank_without_a_neighbour_runs_the_perf_pass():
    hide = run_loopback(1, spmd_hide, "perf_hide", 1, (1, 1, 1), (0, 0, 0), timeout=60)[0]
    perf = run_loopback(1, spmd_hide, "perf", 1, (1, 1, 1), (0, 0, 0), timeout=60)[0]
    assert np.array_equal(bits(hide), bits(perf))


def test_config_refusals():
    from rocm_mpi_amd.models.diffusion3d import VARIANTS3D

    assert "perf_hide" in VARIANTS3D
    assert Diffusion3DConfig().b_width == (16, 2, 2) and Diffusion3DConfig().variant == "perf"
    Diffusion3DConfig(variant="perf_hide").validate()
    Diffusion3DConfig(variant="perf_hide", temporal=2, fast_math=True).validate()
    for bw in [(0, 2, 2), (16, 2), (16, 2, 2.5), (1, 1, -1)]:
        with pytest.raises(ValueError, match="b_width"):
            Diffusion3DConfig(variant="perf_hide", b_width=bw).validate()
    for xf in (-1, 33):
        with pytest.raises(ValueError, match="xface"):
            Diffusion3DConfig(variant="perf_hide", xface=xf).validate()
    Diffusion3DConfig(variant="perf_hide", xface=None).validate()
    with pytest.raises(ValueError, match="perf variant"):
        Diffusion3DConfig(variant="ap", temporal=2).validate()
    with pytest.raises(ValueError, match="perf variant"):
        Diffusion3DConfig(variant="ap", fast_math=True).validate()
    with pytest.raises(ValueError, match="variant must be one of"):
        Diffusion3DConfig(variant="hide").validate()
