"""Uniform-factor variant of the register-factor pipelined kernels
(csrc/kernels/stencil_pipe.h, template flag ``Uni``): with 1/Cp bit-for-bit one
value the kernel takes it as an argument and reads no 1/Cp array. Everything
here is compared bitwise with the CPU twin ``stencilk5_rects_cpu`` fed the
ARRAY (``ops.stencilk_step`` on CPU tensors), at the kernel level and through
the executor, whose verdict (one device scan of 1/Cp) decides which path runs.
Guard values (-5) catch writes outside the rects."""
import pytest
import torch

from rocm_mpi_amd import ops
from rocm_mpi_amd.models import Diffusion2D, DiffusionConfig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# H = 3, 5, 5, 6, 6 levels per stage; 10..21 piper, 24 piper_nosb (the executor's kernels)
DEPTHS = [10, 17, 20, 21, 24]


def kernel_of(K):
    return "piper_nosb" if K == 24 else "piper"


def rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64)


def coef():
    # dx != dy (ry != 1), stable explicit step for 1/Cp <= 1
    return ops.StencilCoef(-1.3, 1 / 0.037, 1 / 0.041, 0.00031)


_T = {}


def field(nx, ny):
    """One random field per shape, shared (and never written) by the cases."""
    if (nx, ny) not in _T:
        _T[(nx, ny)] = rand((ny, nx), 7 + nx)
    return _T[(nx, ny)]


def twin(K, T, iCp, rects):
    out = torch.full_like(T, -5.0)
    ops.stencilk_step(K, out, T, iCp, coef(), rects, ops.StencilTuning(kernel="pipe"))
    return out


def gpu(K, T, iCp, rects, chunk, vec=4, uniform=True):
    out = torch.full(T.shape, -5.0, dtype=torch.float64, device=DEV)
    tn = ops.StencilTuning(kernel=kernel_of(K), xcd_remap=1, chunk_rows=chunk, vec=vec,
                           uniform=uniform)
    ops.stencilk_step(K, out, T.to(DEV), iCp.to(DEV), coef(), rects, tn)
    return out.cpu()


# nx x ny, rows per task: two strips whose windows both touch an x edge and
# chunks shorter than K; interior windows beside edge windows over several
# chunks; nx % 4 = 2 (2 cells per lane); odd nx (1 cell per lane: field path)
TILES = [(520, 131, 16), (1300, 211, 37), (1026, 97, 37), (1025, 97, 37)]


@pytest.mark.parametrize("c0", [1.0, 0.37])
@pytest.mark.parametrize("nx,ny,chunk", TILES)
@pytest.mark.parametrize("K", DEPTHS)
def test_uniform_variant_bitwise_vs_cpu_twin_on_the_array(K, nx, ny, chunk, c0):
    T = field(nx, ny)
    iCp = torch.full((ny, nx), c0, dtype=torch.float64)
    rects = [ops.interior_rect(nx, ny)]
    assert torch.equal(gpu(K, T, iCp, rects, chunk), twin(K, T, iCp, rects))


@pytest.mark.parametrize("K", DEPTHS)
def test_uniform_variant_on_a_frame_rect_list(K):
    """A frame of four rects around an inset interior (plan.cpp's layout), the
    frame at 2 cells per lane and short tasks, the interior at 4."""
    nx, ny = 1300, 211
    T = field(nx, ny)
    iCp = torch.full((ny, nx), 0.37, dtype=torch.float64)
    w = K + 1
    frame = [(K, nx - K, K, K + w), (K, nx - K, ny - K - w, ny - K), (K, K + w, K + w, ny - K - w),
             (nx - K - w, nx - K, K + w, ny - K - w)]
    interior = (K + w, nx - K - w, K + w, ny - K - w)
    ref = twin(K, T, iCp, frame + [interior])
    out = torch.full((ny, nx), -5.0, dtype=torch.float64, device=DEV)
    Td, iCpd = T.to(DEV), iCp.to(DEV)
    kn = kernel_of(K)
    ops.stencilk_step(K, out, Td, iCpd, coef(), frame,
                      ops.StencilTuning(kernel=kn, chunk_rows=16, vec=2, xcd_remap=1, uniform=True))
    ops.stencilk_step(K, out, Td, iCpd, coef(), [interior],
                      ops.StencilTuning(kernel=kn, chunk_rows=64, vec=4, xcd_remap=1, uniform=True))
    assert torch.equal(out.cpu(), ref)


# ------------------------------ executor level ------------------------------
def model(nx=1300, ny=211, K=24, **kw):
    m = Diffusion2D(DiffusionConfig(variant="perf", nx=nx, ny=ny, nt=K, device=DEV, quiet=True,
                                    init="random", executor="native", temporal=K,
                                    fast_math=True, **kw))
    assert m.executor is not None
    return m


def model_twin(m, T0, K):
    """K steps of the CPU twin from T0 with the model's coefficients and 1/Cp array."""
    iCp = m.iCp.cpu()
    ny, nx = T0.shape
    out = T0.clone()  # the boundary cells keep their values
    ops.stencilk_step(K, out, T0, iCp, m.coef, [ops.interior_rect(nx, ny)],
                      ops.StencilTuning(kernel="pipe"))
    return out


def test_executor_uses_the_variant_only_for_a_uniform_array(monkeypatch):
    m = model()
    assert m.executor.uniform_factor
    T0 = m.field.cpu().clone()
    assert list(m.executor.plan(24)) == [24]
    m.step(24)
    assert torch.equal(m.field.cpu(), model_twin(m, T0, 24))
    m.close()
    monkeypatch.setenv("RMA_DIAG", "uniform_factor=off")
    m = model()
    assert not m.executor.uniform_factor
    m.close()


def test_executor_one_differing_cell_takes_the_field_path():
    m = model()
    m.iCp.view(-1)[-1] = 0.5  # the last cell of the array
    T0 = m.field.cpu().clone()
    m.step(24)  # rescans: the array's version changed
    assert not m.executor.uniform_factor
    assert torch.equal(m.field.cpu(), model_twin(m, T0, 24))
    m.close()


def run_two_passes(edit):
    m = model()
    m.step(24)
    m.step(13)
    assert m.executor.passes_done == 2
    if edit:
        m.iCp[5, 7] = 2.0
        m.step(24)
    f = m.field.cpu().clone()
    uni = m.executor.uniform_factor
    m.close()
    return f, uni


@pytest.mark.parametrize("edit", [False, True])
def test_executor_default_equals_field_path(monkeypatch, edit):
    """K = 24 then K = 13 on 1300 x 211; then an in-place edit of 1/Cp followed
    by step(): the model rescans, so the edit can never run stale."""
    a, uni = run_two_passes(edit)
    assert uni == (not edit)
    monkeypatch.setenv("RMA_DIAG", "uniform_factor=off")
    b, uni = run_two_passes(edit)
    assert not uni
    assert torch.equal(a, b)


def spmd_hide(rank, hub, nx, ny, nt, K):
    from rocm_mpi_amd.parallel import implicit_grid as gg

    gg.init_global_grid(nx, ny, 1, dimx=2, dimy=1, overlaps=(2 * K, 2 * K, 2),
                        halowidths=(K, K, 1), quiet=True, loopback=(hub, rank))
    m = Diffusion2D(DiffusionConfig(variant="perf_hide", nx=nx, ny=ny, nt=nt, init="random",
                                    quiet=True, dims=(2, 1, 0), temporal=K, fast_math=True))
    assert m.executor is not None
    m.step(nt)
    out = (m.field.cpu().clone(), bool(m.executor.uniform_factor), int(m.executor.fused_passes))
    m.close()
    gg.finalize_global_grid()
    return out


@pytest.mark.parametrize("fused", ["0", "1"])
def test_two_ranks_default_equals_field_path(monkeypatch, fused):
    """2 x 1 ranks, perf_hide: the split frame / interior launches and the
    frame-first fused launch, with the variant against the field path."""
    from helpers import run_loopback

    # 1100 x 1100 tiles: large enough for the aligned frame layout, which the
    # fused launch needs (tests/test_multirank_gpu.py, aligned frames)
    monkeypatch.setenv("RMA_EXEC_FUSED", fused)
    a = run_loopback(2, spmd_hide, 1100, 1100, 37, 24, timeout=120)
    monkeypatch.setenv("RMA_DIAG", "uniform_factor=off")
    b = run_loopback(2, spmd_hide, 1100, 1100, 37, 24, timeout=120)
    for (fa, ua, na), (fb, ub, nb) in zip(a, b):
        assert ua and not ub
        assert (na > 0) == (fused == "1") and na == nb
        assert torch.equal(fa, fb)
