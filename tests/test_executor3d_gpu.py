"""The native 3D time loop (csrc/runtime/executor3d.cpp): ``_C.Executor3D`` and
``Diffusion3D(native=True)`` against the Python-issued ``Diffusion3D`` loop from
the same random initial field, bitwise, on one MI355X. Five steps: an odd count
gives two-step plans a remainder pass and every plan an odd parity.

Shapes (nz, ny, nx): (9, 13, 130) has the two-step kernel's strip seam at column
126 and, with b_width (16, 2, 2) at overlap 4, an interior box of one plane;
(9, 13, 20) has no room for an interior, so perf_hide falls back to the perf pass."""
import numpy as np
import pytest
import torch

from helpers import run_loopback
from rocm_mpi_amd._native import native
from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig
from test_diffusion3d_tb_cpu import SEED, bits

pytestmark = pytest.mark.gpu
NT = 5
SHAPES = {"seam": (130, 13, 9), "nointerior": (20, 13, 9)}  # (nx, ny, nz)


def eq(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def model(variant, K, fast, periodic, n, native_loop, icp="uniform", xface=0, **kw):
    p = (1, 1, 1) if periodic else (0, 0, 0)
    m = Diffusion3D(Diffusion3DConfig(variant=variant, nx=n[0], ny=n[1], nz=n[2], nt=NT,
                                      init="random", seed=SEED, periods=p, quiet=True,
                                      temporal=K, fast_math=fast, xface=xface,
                                      native=native_loop, **kw))
    assert m.device.type == "cuda" and m.g.halo is not None
    assert m.native_loop == native_loop
    if icp == "random":  # an in-place torch edit: step() rescans by itself
        g = torch.Generator().manual_seed(SEED + 1)
        m.iCp.copy_((0.5 + torch.rand(m.iCp.shape, generator=g, dtype=torch.float64)))
    return m


def raw_executor(m, T, T2, **over):
    """_C.Executor3D on the model's grid and coefficients."""
    cfg, g = m.cfg, m.g
    kw = dict(overlaps=list(g.overlaps), halowidths=list(g.halowidths),
              steps_per_pass=cfg.temporal, fast_math=cfg.fast_math, b_width=list(cfg.b_width),
              xface=-1 if cfg.xface is None else cfg.xface)
    coef = over.pop("coef", tuple(m.coef))
    iCp = over.pop("iCp", m.iCp.data_ptr())
    mode = over.pop("mode", 1 if cfg.variant == "perf_hide" else 0)
    kw.update(over)
    return native().Executor3D(T if isinstance(T, int) else T.data_ptr(),
                               T2 if isinstance(T2, int) else T2.data_ptr(), iCp,
                               cfg.nx, cfg.ny, cfg.nz, mode, coef, g.halo, **kw)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "open"])
@pytest.mark.parametrize("icp", ["uniform", "random"])
@pytest.mark.parametrize("fast", [False, True], ids=["canonical", "fast7"])
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("variant", ["perf", "perf_hide"])
def test_native_loop_equals_the_python_loop_bitwise(variant, K, fast, icp, periodic, shape):
    n = SHAPES[shape]
    ref = model(variant, K, fast, periodic, n, False, icp)
    T0 = ref.field.clone()
    ref.step(NT)
    want = ref.field.clone()
    ref.close()

    m = model(variant, K, fast, periodic, n, True, icp)
    if variant == "perf_hide" and periodic:  # the split the shape is there for
        assert (m.hide_boxes(K)[1] is not None) == (shape == "seam")
    assert eq(m.field, T0)
    # the raw executor on buffers of its own, next to the model's
    T, T2 = T0.clone(), T0.clone()
    torch.cuda.synchronize()
    ex = raw_executor(m, T, T2)
    assert ex.plan(NT) == m.plan(NT)
    ex.run(NT, torch.cuda.current_stream().cuda_stream)
    m.step(NT)
    assert m.steps_done == NT and ex.steps_done == NT
    assert ex.parity == 1 and ex.uniform == (icp == "uniform")
    assert m.uniform_factor == (icp == "uniform")
    torch.cuda.synchronize()
    assert eq((T, T2)[ex.parity], want)
    assert eq(m.field, want)
    assert m.field.data_ptr() == m._bufs[m._exec.parity].data_ptr()
    del ex
    m.close()


def test_xface_default_width_on_the_frame_of_one_step_passes():
    n = SHAPES["seam"]
    ref = model("perf_hide", 1, False, True, n, False, xface=None)
    ref.step(NT)
    want = ref.field.clone()
    ref.close()
    m = model("perf_hide", 1, False, True, n, True, xface=None)
    assert m._exec.frame_xface == m.frame_xface() == 16
    m.step(NT)
    assert eq(m.field, want)
    m.close()


@pytest.mark.parametrize("K", [1, 2])
def test_two_runs_back_to_back_on_a_side_stream_without_a_synchronisation(K):
    """130 x 66 x 40: the interior kernel outlasts the frame, so a wait missing
    between the streams, or between the two runs, shows in the field."""
    n = (130, 66, 40)
    out = {}
    for nat in (False, True):
        m = model("perf_hide", K, False, True, n, nat)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.step(3)
            m.step(2)
            snap = m.field.clone()  # on s, right behind the second run
        s.synchronize()
        assert eq(snap, m.field)
        out[nat] = snap
        m.close()
    assert eq(out[True], out[False])


@pytest.mark.parametrize("variant", ["perf", "perf_hide"])
def test_an_edit_of_iCp_then_rescan_factor_changes_uniform_and_the_field_matches(variant):
    n = SHAPES["seam"]
    out = {}
    for nat in (False, True):
        m = model(variant, 2, False, True, n, nat)
        m.step(2)
        assert m.uniform_factor
        m.iCp[4, 6, 50] = 1.25
        assert m.rescan_factor() is False and not m.uniform_factor
        if nat:
            assert not m._exec.uniform
        m.step(3)
        m.iCp[4, 6, 50] = 1.0
        assert m.rescan_factor() is True and m.uniform_value == 1.0
        m.step(1)
        out[nat] = m.field.clone()
        m.close()
    assert eq(out[True], out[False])


def test_uniform_factor_switch_and_diag_off(monkeypatch):
    n = SHAPES["nointerior"]
    m = model("perf", 1, False, True, n, True, uniform_factor=False)
    assert not m._exec.uniform and not m.uniform_factor
    m.close()
    monkeypatch.setenv("RMA_DIAG", "uniform_factor=off")
    m = model("perf", 1, False, True, n, True)
    assert not m._exec.uniform and not m.uniform_factor
    m.close()


def test_app_native_flag_runs_the_native_loop_and_says_so(capsys):
    from rocm_mpi_amd.apps import diffusion_3D_perf as app

    args = ["--nx", "40", "--ny", "12", "--nz", "9", "--nt", "12", "--periods", "1,1,1",
            "--variant", "perf_hide", "--json"]
    teff = {}
    for flag in ([], ["--native"]):
        assert app.main(args + flag) == 0
        lines = capsys.readouterr().out.splitlines()
        loop = [ln for ln in lines if ln.startswith("[loop]")]
        assert len(loop) == 1 and loop[0].startswith("[loop] native" if flag else "[loop] python")
        teff[bool(flag)] = [ln for ln in lines if ln.startswith("Executed 12 steps")]
    assert teff[True] and teff[False]


REFUSALS = {
    "K3": (dict(steps_per_pass=3), "steps_per_pass"),
    "K0": (dict(steps_per_pass=0), "steps_per_pass"),
    "overlap_below_2K": (dict(steps_per_pass=2, overlaps=[2, 2, 2], halowidths=[1, 1, 1]),
                         "overlap"),
    "halo_width_not_K": (dict(steps_per_pass=2, overlaps=[4, 4, 4], halowidths=[1, 1, 1]),
                         "halo width"),
    "fast7_not_ok": (dict(fast_math=True, coef=(0.0, 1.0, 1.0, 1.0, 0.1)), "fast_math"),
    "b_width_zero": (dict(b_width=[16, 0, 2]), "b_width"),
    "xface_out_of_range": (dict(xface=33), "xface"),
    "mode": (dict(mode=2), "mode"),
    "null_iCp": (dict(iCp=0), "NULL"),
}


@pytest.mark.parametrize("case", list(REFUSALS) + ["null_T", "T2_is_T", "T2_overlaps_T"])
def test_refusals_come_before_any_launch(case):
    m = model("perf_hide", 1, False, True, SHAPES["seam"], False)
    T = m.field.clone()
    T2 = torch.full_like(T, 7.25)  # the sentinel
    big = torch.full((T.numel() + 8,), 7.25, dtype=torch.float64, device=T.device)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError) as e:
        if case == "null_T":
            raw_executor(m, 0, T2)
        elif case == "T2_is_T":
            raw_executor(m, T2, T2)
        elif case == "T2_overlaps_T":
            raw_executor(m, big[:T.numel()].view_as(T), big[8:].view_as(T))
        else:
            raw_executor(m, T, T2, **dict(REFUSALS[case][0]))
    want = {"null_T": "NULL", "T2_is_T": "alias", "T2_overlaps_T": "alias"}.get(
        case) or REFUSALS[case][1]
    assert want in str(e.value) and "invalid argument" in str(e.value)
    torch.cuda.synchronize()
    assert bool((T2 == 7.25).all()) and bool((big == 7.25).all())
    m.close()


def spmd(rank, hub, variant, K, n, dims, periods, nat, fast=False):
    m = Diffusion3D(Diffusion3DConfig(variant=variant, nx=n[0], ny=n[1], nz=n[2], nt=NT,
                                      init="random", seed=SEED, dims=dims, periods=periods,
                                      quiet=True, temporal=K, fast_math=fast, b_width=(3, 2, 2),
                                      xface=None, native=nat),
                    grid_kwargs=dict(loopback=(hub, rank)))
    assert m.device.type == "cuda" and m.g.halo is not None and m.native_loop == nat
    if nat and variant == "perf_hide":
        assert m.hide_boxes(K)[1] is not None
    m.step(NT)
    Tv = m.gather_interior()
    out = None if Tv is None else Tv.numpy().copy()
    m.close()
    return out


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("variant", ["perf", "perf_hide"])
@pytest.mark.parametrize("dims,periods", [((2, 1, 1), (0, 0, 0)), ((1, 2, 2), (0, 1, 0))])
def test_rank_threads_over_loopback_equal_one_rank_bitwise(dims, periods, variant, K):
    n, ol = (34, 12, 10), 2 * K
    P = dims[0] * dims[1] * dims[2]
    got = run_loopback(P, spmd, variant, K, n, dims, periods, True, timeout=120)[0]
    one = tuple(d * (k - ol) + ol for d, k in zip(dims, n))
    ref = run_loopback(1, spmd, "perf", K, one, (1, 1, 1), periods, False, timeout=120)[0]
    assert got.shape == ref.shape
    assert np.array_equal(bits(got), bits(ref))
