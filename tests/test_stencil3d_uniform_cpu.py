"""``ops.count_differing`` (the uniform-1/Cp verdict: a bit compare with cell 0)
on CPU tensors, and the ``uniform`` fields of ``ops.Stencil3DTuning``, which CPU
tensors accept and ignore (the twins always read the array)."""
import pytest
import torch

from rocm_mpi_amd import ops
from test_misc_kernels_cpu import RED_SIZES, no_native

COEF = ops.StencilCoef3.from_physics(1.3, 0.11, 0.07, 0.05, 3.1e-4)
# 1, 2, 4099, the largest size of the CPU reductions' tests, and one beyond the
# 2048 blocks x 8 cells x 256 threads at which the GPU launcher caps its grid
# (the same list runs on the GPU in tests/test_stencil3d_uniform_gpu.py)
SIZES = [1, 2, 4099, max(RED_SIZES), 2048 * 8 * 256 + 1]


def planted(n):
    return sorted({p for p in (1, n // 2, n - 1) if 0 < p < n})


@pytest.mark.parametrize("native_twin", [True, False], ids=["native", "torch"])
@pytest.mark.parametrize("n", SIZES)
def test_count_differing(n, native_twin, monkeypatch):
    if not native_twin:
        no_native(monkeypatch)
        assert not ops.stencil._use_native_cpu()
    A = torch.full((n,), 0.75, dtype=torch.float64)
    assert ops.count_differing(A) == 0
    for i, p in enumerate(planted(n)):  # index 1, the middle, the last index
        A[p] = 1.5
        assert ops.count_differing(A) == i + 1
    if n > 1:
        A[0] = 1.5  # the reference cell itself: now the planted cells are the uniform ones
        assert ops.count_differing(A) == n - 1 - len(planted(n))


@pytest.mark.parametrize("native_twin", [True, False], ids=["native", "torch"])
def test_count_differing_compares_bit_patterns(native_twin, monkeypatch):
    if not native_twin:
        no_native(monkeypatch)
    Z = torch.zeros((3, 5, 7), dtype=torch.float64)
    assert ops.count_differing(Z) == 0
    Z[2, 4, 6] = -0.0
    assert bool((Z == 0.0).all()) and ops.count_differing(Z) == 1
    M = torch.full((3, 5, 7), -0.0, dtype=torch.float64)
    M[1, 2, 3] = 0.0
    assert ops.count_differing(M) == 1
    N = torch.full((4099,), float("nan"), dtype=torch.float64)
    assert ops.count_differing(N) == 0
    N.view(torch.int64)[17] += 1  # a NaN with another payload
    N.view(torch.int64)[4098] ^= 1 << 63  # and one with the other sign
    assert bool(torch.isnan(N).all()) and ops.count_differing(N) == 2


def test_count_differing_refusals():
    with pytest.raises(TypeError, match="float64"):
        ops.count_differing(torch.zeros(4, dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        ops.count_differing(torch.zeros((4, 4), dtype=torch.float64)[:, ::2])
    with pytest.raises(ValueError, match="empty"):
        ops.count_differing(torch.zeros(0, dtype=torch.float64))


@pytest.mark.parametrize("K", ops.TEMPORAL_3D)
def test_cpu_tensors_accept_and_ignore_the_uniform_fields(K):
    """The CPU twin reads the array whatever ``uniform`` says: a wrong
    ``uniform_value`` changes nothing, and iCp is still validated."""
    g = torch.Generator().manual_seed(3)
    T = torch.rand((6, 7, 9), dtype=torch.float64, generator=g)
    iCp = torch.rand((6, 7, 9), dtype=torch.float64, generator=g) + 0.5
    want = torch.full_like(T, -7.25)
    ops.stencil3dk_step(K, want, T, iCp, COEF)
    for tn in (ops.Stencil3DTuning(uniform=True, uniform_value=123.0),
               ops.Stencil3DTuning(uniform=True)):
        got = torch.full_like(T, -7.25)
        ops.stencil3dk_step(K, got, T, iCp, COEF, tuning=tn)
        assert torch.equal(got.view(torch.int64), want.view(torch.int64))
        with pytest.raises(ValueError, match="iCp has shape"):
            ops.stencil3dk_step(K, got, T, iCp[:, :, :8].contiguous(), COEF, tuning=tn)
        with pytest.raises(TypeError, match="iCp must be float64"):
            ops.stencil3dk_step(K, got, T, iCp.float(), COEF, tuning=tn)
    tn = ops.Stencil3DTuning()
    assert tn.uniform is False and tn.uniform_value is None
