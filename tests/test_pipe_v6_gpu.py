"""Six cells per lane of the uniform-factor pipelined kernels
(csrc/kernels/stencil_pipe.h, ``pipe_kernel<K, 4, 6, Ar, 1, false, true>``, K =
17..24): 384-column windows whose loads are clamped per 16-byte pair, so any
even nx runs them. Through ``ops.stencilk_step`` with ``StencilTuning(vec=6,
uniform=True)``, everything bitwise against the CPU twin ``stencilk5_rects_cpu``
fed the array and against the four-cell uniform kernel. Guard values (-5) catch
writes outside the rects."""
import pytest
import torch

from rocm_mpi_amd import ops
from rocm_mpi_amd._native import native

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# every instantiated depth: H = 5 (HL = 2..5) and H = 6 (HL = 3..6) levels per
# stage; 24 is piper_nosb
DEPTHS = [17, 18, 19, 20, 21, 22, 23, 24]
C0 = 0.37


def kernel_of(K):
    return "piper_nosb" if K == 24 else "piper"


def step_of(K):
    return (384 - 2 * K) // 6 * 6  # output columns per strip (Geo::kStep)


def seam_of(K):
    """First column of the second strip of a rect that starts at x = 1."""
    xa = (1 - K) // 6 * 6
    return xa + K + step_of(K)


def widths(K):
    """Even nx: one strip; two strips whose second one holds one / two interior
    columns, and the widest single strip; three strips with nx % 6 = 0, 2, 4."""
    e = seam_of(K)
    one = 300
    assert one <= 384 - 2 * K + 2
    last = e + e % 2  # even
    three = (2 * step_of(K) + 200) // 6 * 6
    return [one, last, last + 2, three, three + 2, three + 4]


def coef():
    return ops.StencilCoef(-1.3, 1 / 0.037, 1 / 0.041, 0.00031)


_T, _REF = {}, {}


def field(nx, ny):
    if (nx, ny) not in _T:
        g = torch.Generator().manual_seed(11 + nx + 7 * ny)
        _T[(nx, ny)] = torch.rand((ny, nx), generator=g, dtype=torch.float64)
    return _T[(nx, ny)]


def twin(K, nx, ny, rects):
    key = (K, nx, ny, tuple(rects))
    if key not in _REF:
        T = field(nx, ny)
        out = torch.full_like(T, -5.0)
        ops.stencilk_step(K, out, T, torch.full_like(T, C0), coef(), list(rects),
                          ops.StencilTuning(kernel="pipe"))
        _REF[key] = out
    return _REF[key]


def gpu(K, Td, rects, chunk, vec):
    out = torch.full(Td.shape, -5.0, dtype=torch.float64, device=DEV)
    iCp = torch.full(Td.shape, C0, dtype=torch.float64, device=DEV)
    tn = ops.StencilTuning(kernel=kernel_of(K), xcd_remap=1, chunk_rows=chunk, vec=vec,
                           uniform=True)
    ops.stencilk_step(K, out, Td, iCp, coef(), list(rects), tn)
    return out.cpu()


def check(K, nx, ny, rects, chunk, want_vec=6):
    ar = 13 if K == 24 else 3
    assert native().pipe_vec_uniform(K, 0, ar, nx, 6, True, True) == want_vec
    Td = field(nx, ny).to(DEV)
    six = gpu(K, Td, rects, chunk, 6)
    assert torch.equal(six, twin(K, nx, ny, rects))
    assert torch.equal(six, gpu(K, Td, rects, chunk, 4))


@pytest.mark.parametrize("wi", range(6))
@pytest.mark.parametrize("K", DEPTHS)
def test_six_cells_bitwise_over_strip_counts_and_nx_mod_6(K, wi):
    nx = widths(K)[wi]
    # a few chunks of 16 rows with a shorter last one (148 = 9 * 16 + 4)
    check(K, nx, 150, [ops.interior_rect(nx, 150)], 16)


def test_widths_cover_every_residue_and_strip_count():
    for K in DEPTHS:
        w = widths(K)
        assert {n % 6 for n in w} == {0, 2, 4} and all(n % 2 == 0 for n in w)
        strips = [-(-(n - 1 - (seam_of(K) - step_of(K))) // step_of(K)) for n in w]
        assert strips == [1, 1, 2, 3, 3, 3] or strips == [1, 2, 2, 3, 3, 3], strips


@pytest.mark.parametrize("ny,chunk", [(13, 16), (150, 64), (211, 37)])
@pytest.mark.parametrize("K", DEPTHS)
def test_six_cells_heights_and_chunks(K, ny, chunk):
    """ny < K; two 64-row chunks and a 20-row one; chunks that are no multiple of 3."""
    nx = widths(K)[4]
    check(K, nx, ny, [ops.interior_rect(nx, ny)], chunk)


@pytest.mark.parametrize("K", DEPTHS)
def test_six_cells_rect_edges_and_rect_lists(K):
    """Rect edges off the lane and pair boundaries, several rects in one launch, a
    rect narrower than one lane: nothing outside the rects is written."""
    nx, ny = widths(K)[5], 90
    for x0 in (1, 2, 3, 7):
        for x1 in (nx - 1, nx - 2, nx - 5):
            check(K, nx, ny, [(x0, x1, 3, ny - 4)], 64)
    rects = [(1, nx - 1, 1, 9), (7, 10, 20, 61), (401, nx - 2, 30, 89), (2, 399, 64, 70)]
    check(K, nx, ny, rects, 16)


@pytest.mark.parametrize("K", [20, 24])
def test_odd_nx_and_misaligned_arrays_fall_back_with_the_same_bits(K):
    ar = 13 if K == 24 else 3
    N = native()
    nx, ny = 1025, 60
    check(K, nx, ny, [ops.interior_rect(nx, ny)], 16, want_vec=1)
    assert N.pipe_vec_uniform(K, 0, ar, 1026, 6, True, False) == 2   # not uniform: as pipe_vec
    assert N.pipe_vec_uniform(K, 0, ar, 1028, 6, True, False) == 4
    assert N.pipe_vec_uniform(16, 0, 3, 1026, 6, True, True) == 2     # no six-cell K = 16
    assert N.pipe_vec_uniform(K, 0, ar, 1026, 6, False, True) == 1
    # T at an address that is 8 mod 16: one cell per lane, the same field
    nx = 1026
    T = field(nx, ny)
    flat = torch.empty(nx * ny + 1, dtype=torch.float64, device=DEV)
    Td = flat[1:].view(ny, nx)
    Td.copy_(T)
    assert Td.data_ptr() % 16 == 8
    rects = [ops.interior_rect(nx, ny)]
    assert torch.equal(gpu(K, Td, rects, 16, 6), twin(K, nx, ny, rects))
