"""Frame-first single-launch passes of 3D perf_hide on one MI355X: the signalling
form of the one- and two-step kernels against the unsignalled launch (bitwise,
flag and counter, re-arm), ``Diffusion3D(perf_hide, fused=True)`` in the Python
and the native loop against ``perf`` and the golden model, rank threads over the
device loopback, an interior that outlasts the frame, stream hygiene and the C
ABI. Every wait of a fused pass here gives up after 10 s: the kernels at these
sizes run for microseconds, so a miscounted signal fails a test in seconds."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import run_loopback
from rocm_mpi_amd import ops
from rocm_mpi_amd._native import native
from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig
from test_diffusion3d_tb_cpu import SEED, bits, golden_global

pytestmark = pytest.mark.gpu
TIMEOUT_S = 10.0
COEF = ops.StencilCoef3(-1.0, 25.8, 13.0, 7.0, 2.4e-4)
_ref: dict = {}


def eq(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


# ---------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------
def frame_and_interior(K, n, b_width):
    """The boxes of a pass of a rank with a neighbour on all six sides."""
    own = []
    for d in range(3):
        own += [K, n[d] - K]
    frame, inner = ops.hide_boxes3d(n, tuple(own), [(True, True)] * 3, (2 * K,) * 3, b_width)
    assert len(frame) == 6 and inner is not None
    return frame, inner


@pytest.mark.parametrize("fast", [False, True], ids=["canonical", "fast7"])
@pytest.mark.parametrize("uniform", [False, True], ids=["field", "uniform"])
@pytest.mark.parametrize("n,chunk", [((130, 23, 13), 4), ((131, 23, 13), 0)],
                         ids=["130x23x13-chunk4", "131x23x13-V1"])
@pytest.mark.parametrize("K", [1, 2])
def test_signalling_launch_equals_the_unsignalled_one_and_rearms(K, n, chunk, uniform, fast):
    nx, ny, nz = n
    g = torch.Generator().manual_seed(11)
    T = torch.rand((nz, ny, nx), generator=g, dtype=torch.float64).cuda()
    iCp = (torch.full((nz, ny, nx), 0.75, dtype=torch.float64) if uniform else
           0.5 + torch.rand((nz, ny, nx), generator=g, dtype=torch.float64)).cuda()
    base = dict(chunk_z=chunk, tb_chunk_z=chunk, fast_math=fast, uniform=uniform,
                uniform_value=0.75 if uniform else None)
    sig = torch.zeros(2, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for b_width in ((16, 2, 2), (3, 2, 2)):  # x slabs on the strip march / thin at K = 1
        frame, inner = frame_and_interior(K, n, b_width)
        boxes = list(frame) + [inner]
        plan = ops.stencil3d_fused_plan(K, (nz, ny, nx), boxes, len(frame),
                                        ops.Stencil3DTuning(**base))
        assert plan.prefix_blocks > 1 and plan.blocks - plan.prefix_blocks >= 1
        if K == 1 and b_width[0] == 3:
            paths = [p for _, p, _ in ops.stencil3d_dispatch(K, (nz, ny, nx), boxes)]
            assert "thin" in paths and "march" in paths
        want = torch.full_like(T, -3.0)
        ops.stencil3dk_step(K, want, T, iCp, COEF, boxes, tuning=ops.Stencil3DTuning(**base))
        tn = ops.Stencil3DTuning(signal=sig.data_ptr(), signal_boxes=len(frame), **base)
        for again in range(2):  # the second launch reuses the words: the re-arm
            got = torch.full_like(T, -3.0)
            ops.stencil3dk_step(K, got, T, iCp, COEF, boxes, tuning=tn)
            # a wait behind the launch on its stream: a flag that never comes costs
            # TIMEOUT_S and sets err instead of passing for a flag read too early
            native().flag_wait(sig.data_ptr() + 8, 1, TIMEOUT_S, err.data_ptr(), 1, s)
            torch.cuda.current_stream().synchronize()
            assert err.item() == 0
            assert sig.tolist() == [0, 1], (b_width, again)  # counter re-armed, flag up
            assert eq(got, want), (b_width, again)
            native().flag_write(sig.data_ptr() + 8, 0, s)
            torch.cuda.current_stream().synchronize()
            assert sig.tolist() == [0, 0]


def test_launcher_refusals_before_any_work():
    n = (130, 23, 13)
    nx, ny, nz = n
    T = torch.rand((nz, ny, nx), dtype=torch.float64).cuda()
    T2 = torch.full_like(T, 7.25)
    iCp = torch.ones_like(T)
    sig = torch.zeros(2, dtype=torch.int64, device="cuda")
    for K in (1, 2):
        frame, inner = frame_and_interior(K, n, (16, 2, 2))
        boxes = list(frame) + [inner]
        cases = [(dict(signal=sig.data_ptr(), signal_boxes=0), "signal_boxes"),
                 (dict(signal=sig.data_ptr(), signal_boxes=len(boxes)), "signal_boxes"),
                 (dict(signal=0, signal_boxes=2), "signal is null"),
                 (dict(signal=sig.data_ptr(), signal_boxes=2, rows=2, tb_rows=2), "signal: ")]
        for kw, msg in cases:
            with pytest.raises(RuntimeError, match=msg):
                ops.stencil3dk_step(K, T2, T, iCp, COEF, boxes, tuning=ops.Stencil3DTuning(**kw))
    torch.cuda.synchronize()
    assert bool((T2 == 7.25).all()) and sig.tolist() == [0, 0]


# ---------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------
def spmd(rank, hub, variant, temporal, n, nt, dims, periods, b_width=(16, 2, 2), fast_math=False,
         fused=False, native_loop=False, expect_fused=None, extra_step=False):
    m = Diffusion3D(Diffusion3DConfig(variant=variant, nx=n[0], ny=n[1], nz=n[2], nt=nt,
                                      init="random", seed=SEED, dims=dims, periods=periods,
                                      quiet=True, temporal=temporal, fast_math=fast_math,
                                      b_width=b_width, fused=fused, fused_timeout_s=TIMEOUT_S,
                                      native=native_loop),
                    grid_kwargs=dict(loopback=(hub, rank)))
    assert m.device.type == "cuda" and m.g.halo is not None
    assert m.native_loop == native_loop
    m.step(nt)
    if extra_step:
        m.step(1)  # reuses the streams, the events and the signal words
    Tv = m.gather_interior()
    m.synchronize()  # raises if a wait timed out
    if expect_fused is not None:
        assert (m.fused_passes > 0) == expect_fused, m.fused_passes
        if expect_fused:
            assert m.fused_passes == len(m.plan(nt)) + (1 if extra_step else 0)
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


@pytest.mark.parametrize("native_loop", [False, True], ids=["python", "native"])
@pytest.mark.parametrize("b_width,inner", [((16, 2, 2), True), ((17, 2, 2), False)])
@pytest.mark.parametrize("temporal", [1, 2])
def test_one_rank_its_own_neighbour_equals_perf_and_golden(temporal, b_width, inner, native_loop):
    n, nt, dims, periods = (34, 12, 10), 24, (1, 1, 1), (1, 1, 1)
    hide = run_loopback(1, spmd, "perf_hide", temporal, n, nt, dims, periods, b_width=b_width,
                        fused=True, native_loop=native_loop, expect_fused=inner, timeout=120)[0]
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
                        fast_math=fast_math, fused=True, expect_fused=True, timeout=120)[0]
    one = tuple(d * (k - ol) + ol for d, k in zip(dims, n))
    ref = perf_run(temporal, one, nt, (1, 1, 1), periods, fast_math=fast_math)
    assert hide.shape == ref.shape
    assert np.array_equal(bits(hide), bits(ref))


@pytest.mark.parametrize("native_loop", [False, True], ids=["python", "native"])
def test_interior_outlasts_the_frame_two_step_passes(native_loop):
    """130 x 66 x 40, periodic on every side, two-step passes: the interior blocks
    run long after the frame's flag, so an exchange or a next launch that did not
    wait for what it needs would read or overwrite cells still in use."""
    n, nt, dims, periods = (130, 66, 40), 12, (1, 1, 1), (1, 1, 1)
    hide = run_loopback(1, spmd, "perf_hide", 2, n, nt, dims, periods, fused=True,
                        native_loop=native_loop, expect_fused=True, extra_step=True,
                        timeout=120)[0]
    ref = perf_run(2, n, nt, dims, periods, extra_step=True)
    assert np.array_equal(bits(hide), bits(ref))


def test_step_leaves_the_field_ordered_on_the_current_stream():
    """No device synchronise between step(n) and the clone on the current stream."""
    n, nt = (130, 66, 40), 12
    out = {}
    for variant, fused in (("perf", False), ("perf_hide", True)):
        m = Diffusion3D(Diffusion3DConfig(variant=variant, nx=n[0], ny=n[1], nz=n[2], nt=nt,
                                          init="random", seed=SEED, periods=(1, 1, 1), quiet=True,
                                          fused=fused, fused_timeout_s=TIMEOUT_S))
        assert m.device.type == "cuda"
        m.step(nt)
        snap = m.field.clone()  # current stream, right behind step
        m.synchronize()
        assert eq(snap, m.field)
        assert m.fused_passes == (nt if fused else 0)
        out[variant] = snap
        m.close()
    assert eq(out["perf"], out["perf_hide"])


# ---------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------
def test_capi_create_f_fused_equals_split_and_refuses_other_values(monkeypatch):
    import test_capi3d_gpu as capi

    monkeypatch.setenv("RMA_EXEC_FUSED_TIMEOUT", str(TIMEOUT_S))
    L = capi.lib()
    L.rma_executor3d_fused_passes.restype = ctypes.c_int64
    P, I64, DBL = capi.P, capi.I64, capi.DBL
    n, nt, K = (130, 13, 9), 7, 2
    g0 = torch.Generator().manual_seed(3)
    T0 = torch.rand((n[2], n[1], n[0]), generator=g0, dtype=torch.float64).cuda()
    iCp = torch.ones_like(T0)
    got = {}
    for fused in (0, 1):
        g = capi.grid(L, n, K, periods=(1, 1, 1))
        T, T2 = T0.clone(), T0.clone()
        torch.cuda.synchronize()
        ex = ctypes.c_void_p()
        capi.ck(L, L.rma_executor3d_create_f(
            g, 1, P(T.data_ptr()), P(T2.data_ptr()), P(iCp.data_ptr()), I64(n[0]), I64(n[1]),
            I64(n[2]), (DBL * 5)(*COEF), (I64 * 3)(16, 2, 2), K, 0, 0, fused, ctypes.byref(ex)))
        capi.ck(L, L.rma_executor3d_run(ex, I64(nt), capi.stream()))
        torch.cuda.synchronize()
        capi.ck(L, L.rma_executor3d_check(ex))
        assert L.rma_executor3d_fused_passes(ex) == (nt // K + nt % K if fused else 0)
        got[fused] = (T, T2)[L.rma_executor3d_parity(ex)].clone()
        capi.ck(L, L.rma_executor3d_destroy(ex))
        capi.ck(L, L.rma_finalize_global_grid(g))
    assert eq(got[0], got[1])
    g = capi.grid(L, n, K, periods=(1, 1, 1))
    T, T2 = T0.clone(), torch.full_like(T0, 7.25)
    ex = ctypes.c_void_p()
    rc = L.rma_executor3d_create_f(
        g, 1, P(T.data_ptr()), P(T2.data_ptr()), P(iCp.data_ptr()), I64(n[0]), I64(n[1]),
        I64(n[2]), (DBL * 5)(*COEF), (I64 * 3)(16, 2, 2), K, 0, 0, 2, ctypes.byref(ex))
    assert rc != 0 and b"fused 2" in L.rma_last_error()
    torch.cuda.synchronize()
    assert bool((T2 == 7.25).all())
    capi.ck(L, L.rma_finalize_global_grid(g))
