"""Executor passes at six cells per lane (uniform 1/Cp, K = 17 / 20 / 21 / 24;
csrc/runtime/executor.cpp pass_tuning, geometry): the frame and task geometry
follows the 384-column strip step. By default only the 288 GB tile class runs
them; ``RMA_DIAG=pipe_cells=6`` runs them on every tile, which is how these
small tiles reach them. Tiles with nx % 6 != 0, plans that mix six-cell and
four-cell depths, one rank and 2 x 2 loopback rank threads with neighbours;
bitwise equal to the same run with ``RMA_DIAG=pipe_cells=4`` and to the field
path (``RMA_DIAG=uniform_factor=off``)."""
import pytest
import torch

from rocm_mpi_amd._native import native
from rocm_mpi_amd.models import Diffusion2D, DiffusionConfig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_one(nx, ny, K, nt):
    m = Diffusion2D(DiffusionConfig(variant="perf_hide", nx=nx, ny=ny, nt=nt, device=DEV,
                                    quiet=True, init="random", executor="native", temporal=K,
                                    fast_math=True))
    assert m.executor is not None
    plan = list(m.executor.plan(nt))
    m.step(nt)
    out = (m.field.cpu().clone(), bool(m.executor.uniform_factor), plan,
           int(m.executor.geometry(plan[0])["task_w"]))
    m.close()
    return out


@pytest.mark.parametrize("nx,ny,K,nt,plan", [(1300, 211, 24, 37, [24, 13]),
                                              (1102, 300, 21, 21, [21]),
                                              (890, 150, 20, 37, [20, 17])])
def test_one_rank_six_cells_equal_four_cells_and_field_path(monkeypatch, nx, ny, K, nt, plan):
    assert nx % 6 != 0
    monkeypatch.setenv("RMA_DIAG", "pipe_cells=6")
    a, ua, pa, wa = run_one(nx, ny, K, nt)
    assert ua and pa == plan
    assert wa == (384 - 2 * K) // 6 * 6  # the six-cell strip step
    monkeypatch.setenv("RMA_DIAG", "pipe_cells=4")
    b, ub, _, wb = run_one(nx, ny, K, nt)
    monkeypatch.delenv("RMA_DIAG")
    d, ud, _, wd = run_one(nx, ny, K, nt)  # a small tile keeps four cells by default
    v = native().pipe_vec(K, 0, 13 if K == 24 else 3, nx, 4, True)  # 2 where nx % 4 = 2
    assert wb == wd == (64 * v - 2 * K) // v * v and ud
    monkeypatch.setenv("RMA_DIAG", "uniform_factor=off,pipe_cells=6")
    c, uc, _, wc = run_one(nx, ny, K, nt)
    assert ub and not uc and wc == wb
    assert torch.equal(a, d)
    assert torch.equal(a, b) and torch.equal(a, c)


def spmd_hide(rank, hub, nx, ny, nt, K):
    from rocm_mpi_amd.parallel import implicit_grid as gg

    gg.init_global_grid(nx, ny, 1, dimx=2, dimy=2, overlaps=(2 * K, 2 * K, 2),
                        halowidths=(K, K, 1), quiet=True, loopback=(hub, rank))
    m = Diffusion2D(DiffusionConfig(variant="perf_hide", nx=nx, ny=ny, nt=nt, init="random",
                                    quiet=True, dims=(2, 2, 0), temporal=K, fast_math=True))
    assert m.executor is not None
    m.step(nt)
    out = (m.field.cpu().clone(), bool(m.executor.uniform_factor), int(m.executor.fused_passes),
           int(m.executor.geometry(K)["task_w"]))
    m.close()
    gg.finalize_global_grid()
    return out


@pytest.mark.parametrize("fused", ["0", "1"])
def test_four_ranks_six_cells_equal_four_cells_and_field_path(monkeypatch, fused):
    """2 x 2 ranks, 1100 x 1100 tiles (1100 % 6 = 2, aligned frames), passes of 24
    and 13 steps: the split launches and the frame-first fused launch."""
    from helpers import run_loopback

    monkeypatch.setenv("RMA_EXEC_FUSED", fused)
    monkeypatch.setenv("RMA_DIAG", "pipe_cells=6")
    a = run_loopback(4, spmd_hide, 1100, 1100, 37, 24, timeout=120)
    monkeypatch.setenv("RMA_DIAG", "pipe_cells=4")
    b = run_loopback(4, spmd_hide, 1100, 1100, 37, 24, timeout=120)
    monkeypatch.setenv("RMA_DIAG", "uniform_factor=off")
    c = run_loopback(4, spmd_hide, 1100, 1100, 37, 24, timeout=120)
    for (fa, ua, na, wa), (fb, ub, nb, wb), (fc, uc, nc, wc) in zip(a, b, c):
        assert ua and ub and not uc
        # ranks with neighbours did resolve to six cells (1100 % 4 == 0: four otherwise)
        assert wa == (384 - 48) // 6 * 6 and wb == wc == (256 - 48) // 4 * 4
        assert (na > 0) == (fused == "1")
        assert torch.equal(fa, fb) and torch.equal(fa, fc)
