"""The host side of the IGG-style gather of the C ABI (rma_gather_igg): the
gather plan (csrc/runtime/gather.cpp) against the Python ``gather_`` over
loopback ranks and against a brute-force contiguity test, the CPU twin of the
strided block-copy kernel (``ops.copy_blocks`` / ``ops.assemble_blocks`` on CPU
tensors) against torch slicing, and the timers' barrier timeout."""
import itertools
import os
import re

import pytest
import torch

from helpers import ROOT, run_loopback
from rocm_mpi_amd import ops
from rocm_mpi_amd._native import native
from rocm_mpi_amd.parallel import implicit_grid as gg
from rocm_mpi_amd.parallel.halo import gather_


def spmd_gather(rank, hub, dims, block):
    """Every rank's block holds rank * block_elems + the cell's local index."""
    nz_grid = 4 if dims[2] > 1 else 1
    gg.init_global_grid(6, 5, nz_grid, dimx=dims[0], dimy=dims[1], dimz=dims[2], quiet=True,
                        loopback=(hub, rank), select_device=False)
    n = 1
    for s in block:
        n *= s
    A = (torch.arange(n, dtype=torch.float64) + rank * n).view(block)
    out = gather_(A)
    gg.finalize_global_grid()
    return out


@pytest.mark.parametrize("dims", [(2, 2, 1), (4, 1, 1), (1, 4, 1), (2, 1, 2), (3, 2, 1)])
def test_plan_places_blocks_where_gather_does(dims):
    P = dims[0] * dims[1] * dims[2]
    block = (2, 3, 5) if dims[2] > 1 else (3, 5)  # torch order: ([nz,] ny, nx)
    G = run_loopback(P, spmd_gather, dims, block)[0]
    size = tuple(block[::-1]) + (1,) * (3 - len(block))  # nx, ny, nz
    plan = native().gather_plan(dims, size, 8)
    nx, ny, nz = size
    assert plan["nprocs"] == P
    assert tuple(plan["size_g"][:len(block)][::-1]) == tuple(G.shape)
    assert plan["row_pitch_g"] == dims[0] * nx
    assert plan["plane_pitch_g"] == dims[0] * nx * dims[1] * ny
    assert plan["block_elems"] == nx * ny * nz
    flat = G.reshape(-1)
    n = nx * ny * nz
    for r in range(P):
        got = torch.as_strided(flat, (nz, ny, nx), (plan["plane_pitch_g"], plan["row_pitch_g"], 1),
                               plan["offsets"][r])
        want = (torch.arange(n, dtype=torch.float64) + r * n).view(nz, ny, nx)
        assert torch.equal(got, want), (dims, r, plan["coords"][r])


def _contiguous_brute_force(dims, size):
    """Is every block's set of element offsets in A_global one unbroken range?"""
    nx, ny, nz = size
    row, plane = dims[0] * nx, dims[0] * nx * dims[1] * ny
    for c0, c1, c2 in itertools.product(*(range(d) for d in dims)):
        offs = sorted((c2 * nz + z) * plane + (c1 * ny + y) * row + c0 * nx + x
                      for z in range(nz) for y in range(ny) for x in range(nx))
        if offs[-1] - offs[0] + 1 != len(offs):
            return False
    return True


def test_contiguous_in_global_is_exact():
    plan = native().gather_plan
    for dims in itertools.product((1, 2, 3), repeat=3):
        for size in itertools.product((1, 2, 3), repeat=3):
            assert plan(dims, size, 8)["contiguous_in_global"] == \
                _contiguous_brute_force(dims, size), (dims, size)
    for P in (2, 4):
        assert plan((1, 1, 1), (5, 3, 2), 8)["contiguous_in_global"]
        assert plan((1, P, 1), (5, 3, 1), 4)["contiguous_in_global"]
        assert plan((1, 1, P), (5, 3, 1), 8)["contiguous_in_global"]
        assert plan((1, 1, P), (5, 3, 2), 8)["contiguous_in_global"]
        # blocks of several planes stacked along y leave gaps between their planes
        assert not plan((1, P, 1), (5, 3, 2), 8)["contiguous_in_global"]
        assert not plan((P, 1, 1), (5, 3, 1), 8)["contiguous_in_global"]
        assert not plan((P, P, 1), (5, 3, 1), 8)["contiguous_in_global"]


def test_plan_refuses_bad_arguments():
    with pytest.raises(RuntimeError, match="elem_bytes"):
        native().gather_plan((2, 2, 1), (5, 3, 1), 2)
    with pytest.raises(RuntimeError, match="size_A"):
        native().gather_plan((2, 2, 1), (5, 0, 1), 8)


def _field(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_copy_blocks_cpu_crops_like_torch_slicing(dtype):
    A = _field((9, 14), dtype, 1)
    out = torch.full((7, 12), -1.0, dtype=dtype)
    ops.copy_blocks([(out, A[1:-1, 1:-1])])
    assert torch.equal(out, A[1:-1, 1:-1])
    B = _field((6, 9, 14), dtype, 2)
    out3 = torch.full((4, 7, 12), -1.0, dtype=dtype)
    ops.copy_blocks([(out3, B[1:-1, 1:-1, 1:-1])])
    assert torch.equal(out3, B[1:-1, 1:-1, 1:-1])
    # strided on the destination side, and only the destination block changes
    C = torch.full((6, 9, 14), -2.0, dtype=dtype)
    ops.copy_blocks([(C[1:-1, 1:-1, 1:-1], out3)])
    want = torch.full((6, 9, 14), -2.0, dtype=dtype)
    want[1:-1, 1:-1, 1:-1] = out3
    assert torch.equal(C, want)


def assembled_by_torch(staging, dims):
    """rank = (c0 * d1 + c1) * d2 + c2 holds the block at (c0, c1, c2), x last."""
    P, nz, ny, nx = staging.shape
    d0, d1, d2 = dims
    return (staging.view(d0, d1, d2, nz, ny, nx).permute(2, 3, 1, 4, 0, 5)
            .reshape(d2 * nz, d1 * ny, d0 * nx))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 2, 1), (6, 6, 1)])
def test_assemble_blocks_cpu_places_1_4_and_36_blocks(dims, dtype):
    P = dims[0] * dims[1] * dims[2]
    assert P in (1, 4, 36) and (P <= native().copy_blocks_max()) == (P < 36)
    staging = _field((P, 2, 3), dtype, 3)  # 36 blocks of 3 x 2: more than one launch's descriptors
    G = torch.full((dims[1] * 2, dims[0] * 3), -1.0, dtype=dtype)
    assert ops.assemble_blocks(staging, G, dims) is G
    assert torch.equal(G, assembled_by_torch(staging.view(P, 1, 2, 3), dims)[0])


def test_assemble_blocks_cpu_3d():
    dims = (2, 1, 2)
    staging = _field((4, 2, 4, 8), torch.float64, 4)
    G = torch.empty((4, 4, 16), dtype=torch.float64)
    ops.assemble_blocks(staging, G, dims)
    assert torch.equal(G, assembled_by_torch(staging, dims))


def test_copy_blocks_refuses_bad_views():
    A = torch.zeros((8, 10), dtype=torch.float64)
    with pytest.raises(ValueError, match="shapes"):
        ops.copy_blocks([(torch.zeros((6, 7), dtype=torch.float64), A[1:-1, 1:-1])])
    with pytest.raises(ValueError, match="unit-stride"):
        ops.copy_blocks([(torch.zeros((8, 5), dtype=torch.float64), A[:, ::2])])
    with pytest.raises(ValueError, match="unit-stride"):
        ops.copy_blocks([(torch.zeros((10, 8), dtype=torch.float64), A.t())])
    with pytest.raises(ValueError, match="dtype"):
        ops.copy_blocks([(torch.zeros((8, 10), dtype=torch.float32), A)])
    h = torch.zeros((8, 10), dtype=torch.float16)
    with pytest.raises(ValueError, match="element size 2"):
        ops.copy_blocks([(h.clone(), h)])
    with pytest.raises(ValueError):
        ops.copy_blocks([(torch.zeros((1, 1, 8, 10), dtype=torch.float64), A.view(1, 1, 8, 10))])
    # the native launcher's own checks: element size, and rows that overlap
    d = (A.data_ptr(), A.data_ptr(), 10, 80, 10, 80, 10, 8, 1)
    with pytest.raises(RuntimeError, match="elem_bytes 2"):
        native().copy_blocks([d], 2, 0, False)
    with pytest.raises(RuntimeError, match="row pitch"):
        ops.copy_blocks([(torch.zeros((8, 10), dtype=torch.float64), A[0:1].expand(8, 10))])
    assert not A.any()


def test_timers_use_the_grid_timeout_not_a_literal():
    src = open(os.path.join(ROOT, "csrc", "runtime", "capi.cpp")).read()
    src = re.sub(r"//[^\n]*", "", src)
    calls = re.findall(r"barrier\(([^)]*)\)", src)
    assert len(calls) >= 2
    for args in calls:
        timeout = args.split(",")[-1].strip()
        assert not re.match(r"^[0-9.]", timeout), f"literal barrier timeout: barrier({args})"
    # RMA_COMM_TIMEOUT is read once, at init
    assert src.count('getenv("RMA_COMM_TIMEOUT")') == 1
