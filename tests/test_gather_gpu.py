"""The strided block-copy kernel (csrc/kernels/blocks.hip) and the IGG-style
gather of the C ABI (rma_gather_igg) on one GPU.

``ops.copy_blocks`` runs between canary guard bands (the idiom of
test_guard_bands_gpu.py) and must equal its CPU twin bitwise over the WHOLE
destination allocation, so a write outside the block shows as well;
``ops.assemble_blocks`` is compared with a torch reshape / permute; the C ABI
is driven through ctypes on a 1-rank grid the way a C or Julia host would."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import ROOT
from rocm_mpi_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 4096  # guard elements on each side (keeps the field 16-byte aligned)
CANARY = -1.2345678901234567e30


def guarded(shape, dtype, seed):
    n = int(np.prod(shape))
    buf = torch.full((G + n + G,), CANARY, dtype=dtype, device=DEV)
    f = buf[G:G + n].view(shape)
    g = torch.Generator().manual_seed(seed)
    f.copy_(torch.rand(shape, generator=g, dtype=torch.float64).to(dtype))
    return buf, f


def guards_intact(buf):
    torch.cuda.synchronize()
    c = torch.tensor(CANARY, dtype=buf.dtype, device=DEV)
    return bool((buf[:G] == c).all()) and bool((buf[-G:] == c).all())


def sl(*ranges):
    return tuple(slice(a, b) for a, b in ranges)


# (id, dtype, source field shape, source slices): the destination is a dense
# field of the block's shape, then the block goes back into a strided view
F64, F32 = torch.float64, torch.float32
CASES = [
    ("nx1_single_column_rows", F64, (5, 8), sl((0, 5), (3, 4))),
    ("nx2_fp64_one_vector_per_row", F64, (6, 8), sl((0, 6), (2, 4))),
    ("nx7_odd_row_element_path", F64, (5, 12), sl((0, 5), (2, 9))),
    ("nx66_wave_plus_vector_tail", F64, (5, 70), sl((0, 5), (2, 68))),
    ("nx520_wider_than_a_block_of_vectors", F64, (3, 524), sl((0, 3), (2, 522))),
    ("nx2100_several_column_groups_element_path", F64, (3, 2102), sl((0, 3), (1, 2101))),
    ("nx4200_several_column_groups_vector_path", F64, (2, 4204), sl((0, 2), (2, 4202))),
    ("ny1_nz3_plane_pitch_is_not_ny_times_row_pitch", F64, (3, 4, 10), sl((0, 3), (1, 2), (2, 8))),
    ("interior_3d", F64, (4, 5, 12), sl((1, 3), (1, 4), (2, 10))),
    ("rows_of_one_block_span_planes", F64, (40, 5, 8), sl((0, 40), (1, 4), (1, 6))),
    ("source_offset_by_one_element_misaligned_base", F64, (6, 16), sl((0, 6), (1, 9))),
    ("fp32_odd_nx_element_path", F32, (5, 11), sl((0, 5), (1, 8))),
    ("fp32_vector_path", F32, (5, 16), sl((0, 5), (4, 12))),
    ("more_wide_rows_than_blocks", F64, (2500, 132), sl((0, 2500), (1, 131))),
    ("more_wide_rows_than_blocks_3d", F64, (1000, 3, 132), sl((0, 1000), (0, 3), (1, 131))),
    ("more_narrow_rows_than_blocks", F64, (200000, 4), sl((0, 200000), (0, 3))),
]


@pytest.mark.parametrize("name,dtype,shape,src", CASES, ids=[c[0] for c in CASES])
def test_copy_blocks_equals_the_cpu_twin_between_guard_bands(name, dtype, shape, src):
    bS, S = guarded(shape, dtype, 1)
    block = tuple(S[src].shape)
    bD, D = guarded(block, dtype, 2)       # pack: strided -> dense
    bB, B = guarded(shape, dtype, 3)       # place: dense -> strided
    hS, hD, hB = S.cpu(), D.cpu().clone(), B.cpu().clone()
    ops.copy_blocks([(D, S[src])])
    ops.copy_blocks([(B[src], D)])
    ops.copy_blocks([(hD, hS[src])])
    ops.copy_blocks([(hB[src], hD)])
    assert guards_intact(bS) and guards_intact(bD) and guards_intact(bB)
    assert torch.equal(hD, hS[src]) and torch.equal(hB[src], hS[src])  # the twin is right
    assert torch.equal(D.cpu(), hD)
    assert torch.equal(B.cpu(), hB), "a write outside the destination block"
    assert torch.equal(S.cpu(), hS)


def test_copy_blocks_36_blocks_split_into_several_launches():
    dims = (6, 6, 1)
    bS, staging = guarded((36, 2, 3), F64, 4)
    bG, A = guarded((12, 18), F64, 5)
    hS, hA = staging.cpu(), A.cpu().clone()
    ops.assemble_blocks(staging, A, dims)
    ops.assemble_blocks(hS, hA, dims)
    assert guards_intact(bS) and guards_intact(bG)
    assert torch.equal(A.cpu(), hA)
    assert torch.equal(hA, hS.view(6, 6, 2, 3).permute(1, 2, 0, 3).reshape(12, 18))


def test_copy_blocks_mixed_paths_in_one_call():
    """Vector-path and element-path blocks in one call: split by path, in order."""
    bS, S = guarded((9, 40), F64, 6)
    bD, D = guarded((9, 40), F64, 7)
    views = [sl((0, 9), (0, 8)), sl((0, 9), (9, 16)), sl((0, 9), (16, 24)), sl((0, 9), (25, 40))]
    hS, hD = S.cpu(), D.cpu().clone()
    ops.copy_blocks([(D[v], S[v]) for v in views])
    ops.copy_blocks([(hD[v], hS[v]) for v in views])
    assert guards_intact(bS) and guards_intact(bD)
    assert torch.equal(D.cpu(), hD)
    for v in views:
        assert torch.equal(hD[v], hS[v])


def test_copy_blocks_refuses_before_launch():
    A = torch.zeros((8, 10), dtype=F64, device=DEV)
    with pytest.raises(ValueError, match="unit-stride"):
        ops.copy_blocks([(torch.zeros((8, 5), dtype=F64, device=DEV), A[:, ::2])])
    with pytest.raises(ValueError, match="element size 2"):
        h = torch.zeros((8, 10), dtype=torch.float16, device=DEV)
        ops.copy_blocks([(h.clone(), h)])
    with pytest.raises(RuntimeError, match="row pitch"):
        ops.copy_blocks([(torch.zeros((8, 10), dtype=F64, device=DEV), A[0:1].expand(8, 10))])
    with pytest.raises(ValueError, match="device"):
        ops.copy_blocks([(torch.zeros((8, 10), dtype=F64), A)])
    torch.cuda.synchronize()
    assert not A.any()


def assembled_by_torch(staging, dims):
    P, nz, ny, nx = staging.shape
    d0, d1, d2 = dims
    return (staging.view(d0, d1, d2, nz, ny, nx).permute(2, 3, 1, 4, 0, 5)
            .reshape(d2 * nz, d1 * ny, d0 * nx))


@pytest.mark.parametrize("block", [(5, 3, 1), (8, 4, 2)], ids=["5x3x1", "8x4x2"])
@pytest.mark.parametrize("dims", [(2, 2, 1), (1, 4, 1), (2, 1, 2)])
def test_assemble_blocks_matches_a_torch_permute(dims, block):
    nx, ny, nz = block
    bS, staging = guarded((4, nz, ny, nx), F64, 8)
    bG, A = guarded((dims[2] * nz, dims[1] * ny, dims[0] * nx), F64, 9)
    ops.assemble_blocks(staging, A, dims)
    assert guards_intact(bS) and guards_intact(bG)
    assert torch.equal(A, assembled_by_torch(staging, dims))


# ---- the C ABI on a 1-rank grid, through ctypes ----
I64P = ctypes.POINTER(ctypes.c_int64)


def lib():
    L = ctypes.CDLL(os.path.join(ROOT, "rocm_mpi_amd", "librma_core.so"))
    L.rma_last_error.restype = ctypes.c_char_p
    L.rma_gather_igg.argtypes = [ctypes.c_void_p, ctypes.c_void_p, I64P, I64P, ctypes.c_int,
                                 ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.rma_gather_igg.restype = ctypes.c_int
    return L


def grid(L, nx, ny):
    g = ctypes.c_void_p()
    rc = L.rma_init_global_grid(nx, ny, 1, None, None, None, None, 1, 0, None, 0,
                                ctypes.byref(g), None, None, None)
    assert rc == 0, L.rma_last_error().decode()
    return g


def i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def gather(L, g, A, size, pitch, eb, out, root=0):
    s = torch.cuda.current_stream().cuda_stream
    return L.rma_gather_igg(g, A, i64(*size), i64(*pitch) if pitch else None, eb, out, root, s)


def test_capi_gather_igg_on_one_rank_host_and_device():
    L = lib()
    NX, NY = 67, 130
    g = grid(L, NX, NY)
    rng = np.random.default_rng(5)
    # host -> host (numpy arrays: pointers the HIP runtime has never seen)
    hA = rng.random((NY, NX))
    hG = np.full((NY, NX), -1.0)
    assert gather(L, g, hA.ctypes.data, (NX, NY, 1), None, 8, hG.ctypes.data) == 0, \
        L.rma_last_error().decode()
    assert np.array_equal(hG, hA)
    # the classification's failed query left no sticky HIP error behind
    dA = torch.from_numpy(hA).to(DEV)
    torch.cuda.synchronize()
    # device -> device
    dG = torch.full_like(dA, -1.0)
    assert gather(L, g, dA.data_ptr(), (NX, NY, 1), None, 8, dG.data_ptr()) == 0, \
        L.rma_last_error().decode()
    assert torch.equal(dG, dA)  # blocking: no synchronize needed, torch.equal reads after it
    # device with pitch_A (the interior of the field) -> host == A[1:-1, 1:-1]
    hI = np.full((NY - 2, NX - 2), -1.0)
    interior = dA[1:-1, 1:-1]
    assert gather(L, g, interior.data_ptr(), (NX - 2, NY - 2, 1), (NX, NX * NY), 8,
                  hI.ctypes.data) == 0, L.rma_last_error().decode()
    assert np.array_equal(hI, hA[1:-1, 1:-1])
    # host with pitch_A -> device, float32
    hA32 = rng.random((NY, NX)).astype(np.float32)
    dI = torch.full((NY - 2, NX - 2), -1.0, dtype=F32, device=DEV)
    assert gather(L, g, hA32[1:-1, 1:-1].ctypes.data, (NX - 2, NY - 2, 1), (NX, NX * NY), 4,
                  dI.data_ptr()) == 0, L.rma_last_error().decode()
    assert np.array_equal(dI.cpu().numpy(), hA32[1:-1, 1:-1])
    assert L.rma_finalize_global_grid(g) == 0


def test_capi_gather_igg_refusals_name_the_argument(monkeypatch):
    L = lib()
    NX, NY = 16, 12
    g = grid(L, NX, NY)
    A = torch.arange(NX * NY, dtype=F64, device=DEV).view(NY, NX)
    out = torch.full_like(A, -1.0)
    a, o = A.data_ptr(), out.data_ptr()

    def refused(word, *args, **kw):
        assert gather(L, g, *args, **kw) != 0
        assert word in L.rma_last_error().decode(), L.rma_last_error().decode()

    refused("A_global", a, (NX, NY, 1), None, 8, None)
    refused("elem_bytes", a, (NX, NY, 1), None, 2, o)
    refused("size_A", a, (NX, 0, 1), None, 8, o)
    refused("size_A", a, (NX, NY, -1), None, 8, o)
    refused("pitch_A", a, (NX, NY, 1), (NX - 1, NX * NY), 8, o)
    refused("pitch_A", a, (NX - 2, NY - 2, 2), (NX, NX), 8, o)
    refused("root", a, (NX, NY, 1), None, 8, o, root=1)
    refused("root", a, (NX, NY, 1), None, 8, o, root=-1)
    monkeypatch.setenv("RMA_GATHER_MAX_BYTES", str(NX * NY * 8 - 1))
    refused("RMA_GATHER_MAX_BYTES", a, (NX, NY, 1), None, 8, o)
    monkeypatch.setenv("RMA_GATHER_MAX_BYTES", str(NX * NY * 8))
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())  # nothing was written by a refused call
    assert gather(L, g, a, (NX, NY, 1), None, 8, o) == 0, L.rma_last_error().decode()
    assert torch.equal(out, A)
    assert L.rma_finalize_global_grid(g) == 0
