"""Diffusion3D ``variant="perf_hide"`` on one MI355X: the frame and the halo
exchange on a high-priority stream next to the interior on a low-priority one.
Bitwise the ``perf`` field and the NumPy golden model, one- and two-step passes,
one rank that is its own periodic neighbour and rank threads over the device
loopback transport; a case whose interior outlasts the frame (a missing wait
between the streams shows there); stream hygiene of ``step``."""
import numpy as np
import pytest
import torch

from helpers import run_loopback
from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig
from test_diffusion3d_tb_cpu import SEED, bits, golden_global

pytestmark = pytest.mark.gpu
_ref: dict = {}


def spmd(rank, hub, variant, temporal, n, nt, dims, periods, b_width=(16, 2, 2), fast_math=False,
         xface=0, expect_inner=None):
    m = Diffusion3D(Diffusion3DConfig(variant=variant, nx=n[0], ny=n[1], nz=n[2], nt=nt,
                                      init="random", seed=SEED, dims=dims, periods=periods,
                                      quiet=True, temporal=temporal, fast_math=fast_math,
                                      b_width=b_width, xface=xface),
                    grid_kwargs=dict(loopback=(hub, rank)))
    assert m.device.type == "cuda" and m.g.halo is not None  # the native halo engine
    if variant == "perf_hide" and expect_inner is not None:
        assert (m.hide_boxes(temporal)[1] is not None) == expect_inner
    m.step(nt)
    Tv = m.gather_interior()
    out = None if Tv is None else Tv.numpy().copy()
    m.close()
    return out


def perf_run(*key, **kw):
    """The perf field of a case, computed once and left unchanged."""
    k = (key, tuple(sorted(kw.items())))
    if k not in _ref:
        temporal, n, nt, dims, periods = key
        P = dims[0] * dims[1] * dims[2]
        _ref[k] = run_loopback(P, spmd, "perf", temporal, n, nt, dims, periods, timeout=120,
                               **kw)[0]
    return _ref[k]


@pytest.mark.parametrize("xface", [0, None], ids=["march", "xface"])
@pytest.mark.parametrize("b_width,inner", [((16, 2, 2), True), ((17, 2, 2), False)])
@pytest.mark.parametrize("temporal", [1, 2])
def test_one_rank_its_own_neighbour_equals_perf_and_golden(temporal, b_width, inner, xface):
    n, nt, dims, periods = (34, 12, 10), 24, (1, 1, 1), (1, 1, 1)
    hide = run_loopback(1, spmd, "perf_hide", temporal, n, nt, dims, periods, b_width=b_width,
                        xface=xface, expect_inner=inner, timeout=120)[0]
    perf = perf_run(temporal, n, nt, dims, periods)
    assert np.array_equal(bits(hide), bits(perf))
    G, _ = golden_global(dims, periods, 2 * temporal, n=n, nt=nt)
    assert np.array_equal(bits(hide), bits(G[1:-1, 1:-1, 1:-1]))


@pytest.mark.parametrize("fast_math", [False, True], ids=["canonical", "fast7"])
@pytest.mark.parametrize("temporal", [1, 2])
@pytest.mark.parametrize("dims,periods", [((2, 2, 2), (0, 0, 0)), ((1, 1, 2), (0, 0, 1))])
def test_rank_threads_equal_the_single_rank_run_bitwise(dims, periods, temporal, fast_math):
    n, nt, ol = (34, 12, 10), 24, 2 * temporal
    P = dims[0] * dims[1] * dims[2]
    hide = run_loopback(P, spmd, "perf_hide", temporal, n, nt, dims, periods, b_width=(3, 2, 2),
                        fast_math=fast_math, xface=None, expect_inner=True, timeout=120)[0]
    # the single-rank perf run of the same global grid (overlap 2 * temporal)
    one = tuple(d * (k - ol) + ol for d, k in zip(dims, n))
    ref = perf_run(temporal, one, nt, (1, 1, 1), periods, fast_math=fast_math)
    assert hide.shape == ref.shape
    assert np.array_equal(bits(hide), bits(ref))


def test_interior_outlasts_the_frame_two_step_passes():
    """130 x 66 x 40, periodic on every side, two-step passes: the interior kernel
    runs longer than the frame, so a frame or an interior of the next pass that
    did not wait for it would read or overwrite cells still in use."""
    n, nt, dims, periods = (130, 66, 40), 12, (1, 1, 1), (1, 1, 1)
    hide = run_loopback(1, spmd, "perf_hide", 2, n, nt, dims, periods, expect_inner=True,
                        timeout=120)[0]
    assert np.array_equal(bits(hide), bits(perf_run(2, n, nt, dims, periods)))


def test_step_leaves_the_field_ordered_on_the_current_stream():
    """No device synchronise between step(n) and the clone on the current stream."""
    from rocm_mpi_amd.parallel import implicit_grid as gg

    n, nt = (130, 66, 40), 12
    out = {}
    for variant in ("perf", "perf_hide"):
        m = Diffusion3D(Diffusion3DConfig(variant=variant, nx=n[0], ny=n[1], nz=n[2], nt=nt,
                                          init="random", seed=SEED, periods=(1, 1, 1),
                                          quiet=True))
        assert m.device.type == "cuda"
        m.step(nt)
        snap = m.field.clone()  # current stream, right behind step
        m.synchronize()
        assert torch.equal(snap.view(torch.int64), m.field.view(torch.int64))
        m.step(1)  # a second call re-uses the streams and events
        out[variant] = m.field.clone()
        m.close()
        assert not gg.grid_is_initialized()
    assert torch.equal(out["perf"].view(torch.int64), out["perf_hide"].view(torch.int64))
