"""Strided block copies on torch tensors: the native ``copy_blocks`` kernel.

``copy_blocks([(dst, src), ...])`` copies each (possibly strided) ``src`` view
into its ``dst`` view: views of up to 3 dimensions with a unit-stride inner
dimension, equal shapes, one dtype (4 or 8 bytes per element) and one device
for the whole call. Any number of pairs: the native launcher splits them into
launches. On CUDA tensors this is the HIP kernel of ``csrc/kernels/blocks.hip``
on the current stream, on CPU tensors its bitwise twin. It is the device crop
of the reference scripts (``Array(T[2:end-1,2:end-1])``)::

    out = torch.empty((ny - 2, nx - 2), dtype=T.dtype, device=T.device)
    ops.copy_blocks([(out, T[1:-1, 1:-1])])

``assemble_blocks(staging, A_global, dims)`` is the placement pass of the C
ABI's ``rma_gather_igg`` on one device: ``staging[r]`` is rank r's block
(rank-major), ``dims`` the process grid ``(dimx, dimy, dimz)``; block r goes to
its Cartesian position in ``A_global`` (shape ``dims .* block`` with torch's
row-major order, x last), with the ordering of the native gather plan.
"""
from __future__ import annotations

import torch

from .._native import native
from .stencil import stream_handle


def _desc(dst: torch.Tensor, src: torch.Tensor):
    for name, t in (("dst", dst), ("src", src)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"copy_blocks: {name} must be a torch.Tensor, got {type(t).__name__}")
    if dst.shape != src.shape:
        raise ValueError(f"copy_blocks: shapes differ: dst {tuple(dst.shape)}, src {tuple(src.shape)}")
    if not 1 <= dst.dim() <= 3:
        raise ValueError(f"copy_blocks: views of 1 to 3 dimensions, got {dst.dim()}")
    if dst.dtype != src.dtype or dst.device != src.device:
        raise ValueError("copy_blocks: dtype/device mismatch between dst and src")
    if dst.numel() == 0:
        raise ValueError("copy_blocks: empty view")
    if dst.stride(-1) != 1 or src.stride(-1) != 1:
        raise ValueError("copy_blocks: inner dimension must be unit-stride")
    pad = 3 - dst.dim()
    shape = (1,) * pad + tuple(dst.shape)
    ds = (0,) * pad + tuple(dst.stride())
    ss = (0,) * pad + tuple(src.stride())
    nz, ny, nx = shape
    # strides along extents of 1 are never used; the native launcher refuses
    # used ones that do not hold their extent (expanded or transposed views)
    return (dst.data_ptr(), src.data_ptr(), ds[1], ds[0], ss[1], ss[0], nx, ny, nz)


def copy_blocks(pairs) -> None:
    """Copy every ``src`` view into its ``dst`` view (see the module docstring)."""
    pairs = list(pairs)
    if not pairs:
        return
    d0 = pairs[0][0]
    descs = []
    for dst, src in pairs:
        descs.append(_desc(dst, src))
        if dst.dtype != d0.dtype or dst.device != d0.device:
            raise ValueError("copy_blocks: one dtype and device per call")
    if d0.element_size() not in (4, 8):
        raise ValueError(f"copy_blocks: element size {d0.element_size()} bytes ({d0.dtype}); 4 or 8")
    native().copy_blocks(descs, d0.element_size(), stream_handle(d0), d0.is_cuda)


def assemble_blocks(staging: torch.Tensor, A_global: torch.Tensor, dims) -> torch.Tensor:
    """Place rank-major ``staging[r]`` blocks at their Cartesian positions in ``A_global``."""
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError(f"assemble_blocks: dims must be three positive integers, got {dims}")
    if not 2 <= staging.dim() <= 4:
        raise ValueError("assemble_blocks: staging is (nprocs, [nz, [ny,]] nx)")
    if not staging.is_contiguous():
        raise ValueError("assemble_blocks: staging must be contiguous (rank-major)")
    block = tuple(staging.shape[1:])
    nd = len(block)
    size = tuple(block[::-1]) + (1,) * (3 - nd)  # nx, ny, nz
    if any(d != 1 for d in dims[nd:]):
        raise ValueError(f"assemble_blocks: {nd}-D blocks on a process grid {dims}")
    plan = native().gather_plan(dims, size, staging.element_size())
    if staging.shape[0] != plan["nprocs"]:
        raise ValueError(f"assemble_blocks: {staging.shape[0]} blocks for {plan['nprocs']} ranks")
    want = tuple(dims[d] * size[d] for d in reversed(range(nd)))
    if tuple(A_global.shape) != want:
        raise ValueError(f"assemble_blocks: A_global has shape {tuple(A_global.shape)}, expected {want}")
    if not A_global.is_contiguous():
        raise ValueError("assemble_blocks: A_global must be contiguous")
    pairs = []
    for r, c in enumerate(plan["coords"]):
        idx = tuple(slice(c[d] * size[d], (c[d] + 1) * size[d]) for d in reversed(range(nd)))
        pairs.append((A_global[idx], staging[r]))
    copy_blocks(pairs)
    return A_global
