"""Graded task rows through the executor (csrc/runtime/executor.cpp
launch_region): ``RMA_DIAG=task_rows=96/32/8`` forces three row bands on a
770 x 203 tile (three six-cell strips, one partial; seams between the bands, a
partial last task, bands of 3 blocks). Six cells at K = 24 and 17, four cells
at K = 20, the field path (non-uniform 1/Cp) at K = 12; 2K + 5 steps, the depth
K made the planner's cheapest (``pass_costs``) so the plan is K, K, 5. The field
is bitwise equal to the run with ``task_rows=uniform`` and to the CPU twin; one
case runs the ``perf`` variant, whose one launch per pass is graded too. A
64-row tile is too short for the bands and keeps the single band.

Any task mapping computes the same cells, so the bitwise checks cannot tell
whether the bands reached the device. ``graded_passes`` and ``row_bands`` are
host-side; ``native().pipe_last_launch()`` reports the grid and the band count
that the last pipelined launch handed to its kernel, and the mapping that the
kernel then runs is the function ``tests/test_task_map_cpu.py`` checks."""
import pytest
import torch

from rocm_mpi_amd import ops
from rocm_mpi_amd._native import native
from rocm_mpi_amd.models import Diffusion2D, DiffusionConfig

pytestmark = pytest.mark.gpu
NX, NY = 770, 203
ICP_SEED = 4321


def run_one(K, ny, icp, device, variant="perf_hide"):
    gpu = device != "cpu"
    nt = 2 * K + 5
    m = Diffusion2D(DiffusionConfig(variant=variant, nx=NX, ny=ny, nt=nt, device=device,
                                    quiet=True, init="random", temporal=K, fast_math=True,
                                    executor="native" if gpu else "auto"))
    assert (m.executor is not None) == gpu
    if icp == "random":  # below 1/Cp0 = 1: dt stays stable
        ops.init_random_(m.iCp, m.geometry(), seed=ICP_SEED, lo=0.5, hi=1.0)
        if gpu:  # a write torch does not see
            m.executor.rescan_factor()
    info = None
    if gpu:
        assert bool(m.executor.uniform_factor) == (icp == "uniform")
        plan = list(m.executor.plan(nt))
        assert plan == [K, K, 5]
        info = dict(bands=[m.executor.row_bands(k, (1, NX - 1, 1, ny - 1)) for k in plan],
                    task_w=int(m.executor.geometry(K)["task_w"]), plan=plan)
    m.step(nt)
    if gpu:
        info["graded"] = int(m.executor.graded_passes)
        # the last launch: the 5-step pass (fast-math ring kernel, arithmetic 0)
        info["launch"] = tuple(native().pipe_last_launch())
        v = native().pipe_vec_uniform(5, 0, 0, NX, 4, True, icp == "uniform")
        info["strips5"] = native().pipe_strip_count(1, NX - 1, 5, v)
    out = m.field.cpu().clone()
    m.close()
    return out, info


@pytest.fixture(scope="module")
def twin():
    """The CPU twin's field per (K, ny, 1/Cp), computed once."""
    cache = {}

    def get(K, ny, icp):
        if (K, ny, icp) not in cache:
            cache[(K, ny, icp)] = run_one(K, ny, icp, "cpu")[0]
        return cache[(K, ny, icp)]

    return get


@pytest.mark.parametrize("K,cells,icp,variant", [(24, 6, "uniform", "perf_hide"),
                                                 (17, 6, "uniform", "perf_hide"),
                                                 (20, 4, "uniform", "perf_hide"),
                                                 (12, 4, "random", "perf_hide"),
                                                 (24, 6, "uniform", "perf")])
def test_graded_bands_equal_uniform_rows_and_the_cpu_twin(monkeypatch, twin, K, cells, icp,
                                                          variant):
    monkeypatch.setenv("RMA_DIAG", f"pipe_cells={cells},pass_costs={K}:0.5,task_rows=96/32/8")
    a, ia = run_one(K, NY, icp, "cuda:0", variant)
    # 201 rows: one task of 96, one of 32, ten of 8 rows (the last a single row),
    # in every pass of the plan; three strips at six cells: bands of 3 blocks
    assert all(b == [(1, 97, 96), (97, 129, 32), (129, NY - 1, 8)] for b in ia["bands"])
    assert ia["graded"] == len(ia["plan"])
    # the launcher got the bands: 1 + 1 + 10 chunk rows of every strip, three bands
    assert ia["launch"] == (12 * ia["strips5"], 3)
    if cells == 6:
        assert ia["task_w"] == (384 - 2 * K) // 6 * 6 and -(-(NX - 2) // ia["task_w"]) == 3
    monkeypatch.setenv("RMA_DIAG", f"pipe_cells={cells},pass_costs={K}:0.5,task_rows=uniform")
    b, ib = run_one(K, NY, icp, "cuda:0", variant)
    assert ib["graded"] == 0 and all(len(x) == 1 for x in ib["bands"])
    rows5 = ib["bands"][-1][0][2]  # uniform rows per task of the 5-step pass
    assert ib["launch"] == (-(-(NY - 2) // rows5) * ib["strips5"], 0)
    assert ib["task_w"] == ia["task_w"]
    assert torch.equal(a, b)
    assert torch.equal(a, twin(K, NY, icp))


def test_a_short_tile_keeps_the_single_band(monkeypatch, twin):
    # (K = 17: a tile of 64 rows holds passes of at most 21 steps)
    monkeypatch.setenv("RMA_DIAG", "pipe_cells=6,pass_costs=17:0.5,task_rows=96/32/8")
    a, ia = run_one(17, 64, "uniform", "cuda:0")
    assert ia["graded"] == 0 and ia["launch"][1] == 0
    assert all(len(b) == 1 and b[0][:2] == (1, 63) for b in ia["bands"])
    monkeypatch.setenv("RMA_DIAG", "pipe_cells=6,pass_costs=17:0.5,task_rows=uniform")
    b, ib = run_one(17, 64, "uniform", "cuda:0")
    assert ib["bands"] == ia["bands"]  # today's rows per task
    assert torch.equal(a, b) and torch.equal(a, twin(17, 64, "uniform"))


def test_default_tiles_below_the_288_gb_class_stay_uniform(monkeypatch):
    monkeypatch.setenv("RMA_DIAG", "pass_costs=24:0.5")
    _, info = run_one(24, NY, "uniform", "cuda:0")
    assert info["graded"] == 0 and all(len(b) == 1 for b in info["bands"])
