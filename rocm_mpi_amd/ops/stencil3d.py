"""Tensor-level entry points of the 3D (7-point) diffusion kernels.

Fields are ``(nz, ny, nx)`` float64 tensors, contiguous, x fastest. As in
``ops.stencil`` every op validates on the host before any launch and then
dispatches: GPU tensors to ``csrc/kernels/stencil3d.hip`` / ``misc.hip`` on
the current torch stream (the extension is mandatory there), CPU tensors to
the bit-identical C++ twins, or to a pure-torch formulation with the same
operation order when the extension is absent.

The canonical per-cell update (``StencilCoef3`` in csrc/include/rma/common.h) is
the 2D expression with the z flux difference subtracted last::

    T2 = c + dt*( iCp*( ((-(qxR-qxL))*rdx - (qyU-qyD)*rdy) - (qzF-qzB)*rdz ) )
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Iterable, NamedTuple, Sequence

import torch

from .._native import has_native, native
from .stencil import _ptr, check_field, stream_handle

Box = tuple  # (x0, x1, y0, y1, z0, z1), half-open, 0-based cell indices
MAX_BOXES = 8


class StencilCoef3(NamedTuple):
    """Coefficients of the canonical 3D update (csrc/include/rma/common.h)."""

    mlam: float  # -lam
    rdx: float  # 1/dx
    rdy: float  # 1/dy
    rdz: float  # 1/dz
    dt: float

    @classmethod
    def from_physics(cls, lam: float, dx: float, dy: float, dz: float,
                     dt: float) -> "StencilCoef3":
        return cls(-lam, 1.0 / dx, 1.0 / dy, 1.0 / dz, dt)


@dataclass
class Stencil3DTuning:
    """Knobs of the z-march kernel (defaults: profiles/diffusion3d.md): rows of
    the y-band a wave keeps in registers (2, 4, 8), planes per march iteration
    (1 or 2; 1 with 8 rows), cells per lane (2: 16-byte accesses, 1: scalar),
    non-temporal bitmask (1: T2 stores, 2: 1/Cp loads), planes per wave task
    (0: the measured default, 32) and the per-XCD block order. The K-step kernel
    (``stencil3dk_step``, csrc/kernels/stencil3d_tb.hip) shares vec and xcd_remap
    and has its own output rows per wave (``tb_rows``: 2, 4), output planes per
    wave task (``tb_chunk_z``) and non-temporal bitmask (``tb_nontemporal``); 0 is
    the measured default of each (4 rows, 32 planes, plain accesses:
    profiles/diffusion3d_temporal.md).

    ``uniform``: the caller vouches that every cell of ``iCp`` has the bit pattern
    of ``uniform_value`` (``Diffusion3D`` decides this with ``ops.count_differing``);
    both GPU kernels then run their uniform-factor variant, which takes the value
    as an argument and never reads the array (16 instead of 24 bytes per cell and
    pass), bitwise equal to the field path. The 1/Cp-load bit (2) of the
    non-temporal masks has nothing to act on there. CPU tensors accept and ignore both fields: the twins
    always read the array.

    ``fast_math``: the fast7 arithmetic (``fast7_ok``; the 7-point sum with the
    constants folded into one per-cell factor, 8 fp64 operations per update instead
    of about 30) in both kernels, field and uniform paths alike. Rounding-close to
    the canonical update, not bitwise equal to it. CPU tensors honour it: they run
    the fast7 C++ twin, bitwise equal to the GPU kernels. It needs the native
    extension and a coefficient set that passes ``fast7_ok``.

    ``xface`` (0..32, default 0 = today's dispatch): the widest box in x that runs
    an x-face path instead of the thin-box path (one-step, widths up to 8) or the
    128-cell strip march. One-step kernel (csrc/kernels/stencil3d.hip): a wave of
    64/LX rows of LX = 8, 16 or 32 lanes marching along z. Two-step kernel
    (csrc/kernels/stencil3d_tb.hip): a wave of 64/LX groups of LX lanes, each the
    two-step march of one LX-column segment; a box of width W needs W + 2 <= LX,
    so boxes wider than ``min(xface, 30)`` keep the strip march. Bitwise the same
    result. ``stencil3d_dispatch`` tells which box takes which path. CPU tensors
    accept and ignore it.

    ``signal`` / ``signal_boxes`` (frame-first fused passes): ``signal`` is the
    address of two device ``uint64`` words, a counter that is zero and a flag. The
    blocks of the first ``signal_boxes`` non-empty boxes then dispatch first (never
    XCD-remapped), every one of their waves counts itself in ``signal[0]`` after its
    last store, and the last one resets the counter and stores 1 into ``signal[1]``
    with a system-scope release: a ``flag_wait`` on another stream orders work after
    those boxes without waiting for the rest of the launch. It needs
    ``1 <= signal_boxes <`` the number of non-empty boxes and the shipped tuning
    (``rows=4, unroll=2``; ``tb_rows`` 0 or 4). The x-face kernels do not signal: in
    a signalling launch every box runs the march or thin path and ``xface`` is not
    applied (``stencil3d_dispatch`` says so). ``stencil3d_fused_plan`` returns the
    block counts of such a launch. Bitwise the unsignalled result; CPU tensors
    accept and ignore both fields."""

    rows: int = 4
    unroll: int = 2
    vec: int = 2
    nontemporal: int = 3
    chunk_z: int = 0
    xcd_remap: int = 1
    tb_rows: int = 0
    tb_chunk_z: int = 0
    tb_nontemporal: int = 0
    uniform: bool = False
    uniform_value: float | None = None  # None: read iCp[0, 0, 0] (synchronises the device)
    fast_math: bool = False
    xface: int = 0
    signal: int = 0  # address of the two signal words (0: no signal)
    signal_boxes: int = 0


XFACE_MAX = 32  # widest box the x-face path takes (Stencil3DTuning.xface)
# every (rows, unroll) the launcher instantiates
TUNINGS_3D = ((2, 1), (2, 2), (4, 1), (4, 2), (8, 1))
# steps per pass stencil3dk_step runs (csrc/kernels/stencil3d_tb.hip stencil3dk_has)
# and the output rows per wave its launcher instantiates
TEMPORAL_3D = (1, 2)
TB_ROWS_3D = (2, 4)


@dataclass
class TileGeometry3:
    """Placement of a local (nz, ny, nx) tile in the implicit global grid."""

    gx0: int
    gy0: int
    gz0: int
    nxg: int
    nyg: int
    nzg: int
    dx: float
    dy: float
    dz: float
    xoff: float = 0.0
    yoff: float = 0.0
    zoff: float = 0.0
    periodx: int = 0
    periody: int = 0
    periodz: int = 0

    def as_tuple(self):
        return (int(self.gx0), int(self.gy0), int(self.gz0), int(self.nxg), int(self.nyg),
                int(self.nzg), float(self.dx), float(self.dy), float(self.dz), float(self.xoff),
                float(self.yoff), float(self.zoff), int(self.periodx), int(self.periody),
                int(self.periodz))


def interior_box(nx: int, ny: int, nz: int) -> Box:
    return (1, nx - 1, 1, ny - 1, 1, nz - 1)


def validate_boxes(boxes: Sequence[Box], nx: int, ny: int, nz: int) -> list[Box]:
    if len(boxes) > MAX_BOXES:
        raise ValueError(f"at most {MAX_BOXES} boxes per launch, got {len(boxes)}")
    out = []
    for b in boxes:
        x0, x1, y0, y1, z0, z1 = (int(v) for v in b)
        if x1 <= x0 or y1 <= y0 or z1 <= z0:
            continue
        if x0 < 1 or y0 < 1 or z0 < 1 or x1 > nx - 1 or y1 > ny - 1 or z1 > nz - 1:
            raise ValueError(f"box {tuple(b)} outside the interior "
                             f"[1,{nx - 1})x[1,{ny - 1})x[1,{nz - 1})")
        out.append((x0, x1, y0, y1, z0, z1))
    return out


def hide_boxes3d(n: Sequence[int], owned: Box, sides: Sequence[Sequence[bool]],
                 overlaps: Sequence[int], b_width: Sequence[int]):
    """Frame / interior split of the cells a pass writes (``@hide_communication``):
    ``(frame_boxes, inner_box | None)``.

    ``n = (nx, ny, nz)``; ``owned`` is ``Diffusion3D.owned_box(k)``;
    ``sides[d] = (has_low_neighbour, has_high_neighbour)`` (a rank that is its own
    periodic neighbour has one); ``b_width[d] >= 1`` is the boundary width in cells
    from the array edge. On a side with a neighbour the inner box starts
    ``max(b_width[d], overlaps[d])`` cells from the array edge, so the send planes
    ``[ol-hw, ol)`` and ``[n-ol, n-ol+hw)`` lie in the frame; a side without one has
    no frame slab and the inner box reaches the owned bound. The frame is ``owned``
    minus the inner box as at most six disjoint slabs: z slabs over the full owned
    x-y extent, y slabs over the inner z range, x slabs over the inner y and z
    range; empty slabs are dropped. An inner box empty in some dimension gives
    ``([owned], None)``, no neighbour at all ``([], owned)``."""
    n = tuple(int(v) for v in n)
    bw = tuple(int(v) for v in b_width)
    ol = tuple(int(v) for v in overlaps)
    if len(n) != 3 or len(bw) != 3 or len(ol) != 3 or len(sides) != 3 or len(owned) != 6:
        raise ValueError("hide_boxes3d takes three dimensions: n, sides, overlaps, b_width of "
                         "length 3 and a box of 6 bounds")
    if min(bw) < 1:
        raise ValueError(f"b_width >= 1 required, got {bw}")
    own = tuple(int(v) for v in owned)
    if not any(bool(s) for d in range(3) for s in sides[d]):
        return [], own
    inner = []
    for d in range(3):
        lo, hi = own[2 * d], own[2 * d + 1]
        m = max(bw[d], ol[d])
        if sides[d][0]:
            lo = max(lo, m)
        if sides[d][1]:
            hi = min(hi, n[d] - m)
        if hi <= lo:
            return [own], None
        inner += [lo, hi]
    ox0, ox1, oy0, oy1, oz0, oz1 = own
    ix0, ix1, iy0, iy1, iz0, iz1 = inner
    slabs = [(ox0, ox1, oy0, oy1, oz0, iz0), (ox0, ox1, oy0, oy1, iz1, oz1),
             (ox0, ox1, oy0, iy0, iz0, iz1), (ox0, ox1, iy1, oy1, iz0, iz1),
             (ox0, ix0, iy0, iy1, iz0, iz1), (ix1, ox1, iy0, iy1, iz0, iz1)]
    frame = [b for b in slabs if b[1] > b[0] and b[3] > b[2] and b[5] > b[4]]
    return frame, tuple(inner)


def stencil3d_torch(T2: torch.Tensor, T: torch.Tensor, iCp: torch.Tensor, c: StencilCoef3,
                    boxes: Iterable[Box]) -> None:
    """Pure-torch twin of the fused 3D kernel (same operation order, bitwise)."""
    for x0, x1, y0, y1, z0, z1 in boxes:
        cu = T[z0:z1, y0:y1, x0:x1]
        qxR = (c.mlam * (T[z0:z1, y0:y1, x0 + 1:x1 + 1] - cu)) * c.rdx
        qxL = (c.mlam * (cu - T[z0:z1, y0:y1, x0 - 1:x1 - 1])) * c.rdx
        qyU = (c.mlam * (T[z0:z1, y0 + 1:y1 + 1, x0:x1] - cu)) * c.rdy
        qyD = (c.mlam * (cu - T[z0:z1, y0 - 1:y1 - 1, x0:x1])) * c.rdy
        qzF = (c.mlam * (T[z0 + 1:z1 + 1, y0:y1, x0:x1] - cu)) * c.rdz
        qzB = (c.mlam * (cu - T[z0 - 1:z1 - 1, y0:y1, x0:x1])) * c.rdz
        d = iCp[z0:z1, y0:y1, x0:x1] * (((-(qxR - qxL)) * c.rdx - (qyU - qyD) * c.rdy)
                                        - (qzF - qzB) * c.rdz)
        T2[z0:z1, y0:y1, x0:x1] = cu + c.dt * d


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def fast7_ok(coef: StencilCoef3) -> bool:
    """Mirror of rma::fast7_ok: fast7 divides by lam/dx^2, so it needs lam != 0
    and finite folded constants (ay/ax, az/ax, dt*ax)."""
    c = StencilCoef3(*coef)
    ax, ay, az = ((-c.mlam) * r * r for r in (c.rdx, c.rdy, c.rdz))
    if ax == 0.0 or not all(math.isfinite(v) for v in (ax, ay, az)):
        return False
    return all(math.isfinite(v) for v in (ay / ax, az / ax, c.dt * ax))


def _fast_math(tn: "Stencil3DTuning | None", coef: StencilCoef3) -> bool:
    """tuning.fast_math, refused before any work where it cannot run."""
    if tn is None or not tn.fast_math:
        return False
    if not fast7_ok(coef):
        raise ValueError("fast_math: the fast7 arithmetic needs lam != 0 and finite "
                         f"coefficients, got {tuple(coef)}")
    if not has_native():
        raise RuntimeError("fast_math needs the native extension (python -m rocm_mpi_amd._build): "
                           "there is no torch formulation of the fast7 arithmetic")
    return True


def _uniform_args(tn: Stencil3DTuning, iCp: torch.Tensor) -> tuple[bool, float]:
    if not tn.uniform:
        return False, 0.0
    return True, float(iCp[0, 0, 0]) if tn.uniform_value is None else float(tn.uniform_value)


def stencil3d_step(T2: torch.Tensor, T: torch.Tensor, iCp: torch.Tensor, coef: StencilCoef3,
                   boxes: Sequence[Box] | None = None,
                   tuning: Stencil3DTuning | None = None) -> None:
    """One explicit 3D diffusion step on every box (default: the interior):
    T2[b] = T[b] + dt*iCp*(div q)[b]. Cells outside the boxes keep T2's values.
    ``tuning.uniform`` runs the GPU kernel's uniform-factor variant (the array is
    validated but not read); on CPU tensors it is accepted and ignored.
    ``tuning.fast_math`` runs the fast7 arithmetic, on GPU and CPU tensors alike.
    ``tuning.xface`` sends boxes at most that wide in x through the GPU kernel's
    x-face path (bitwise the same cells); CPU tensors accept and ignore it."""
    xface = int(tuning.xface) if tuning is not None else 0
    if not 0 <= xface <= XFACE_MAX:
        raise ValueError(f"xface={xface} (0: off, or the widest face box, up to {XFACE_MAX})")
    check_field("T", T)
    if T.dim() != 3:
        raise ValueError(f"T must be a (nz, ny, nx) field, got shape {tuple(T.shape)}")
    nz, ny, nx = T.shape
    if min(nx, ny, nz) < 3:
        raise ValueError(f"nx, ny, nz >= 3 required, got (nz, ny, nx) = {tuple(T.shape)}")
    check_field("T2", T2, (nz, ny, nx), T.device)
    check_field("iCp", iCp, (nz, ny, nx), T.device)
    if _overlap(T2, T):
        raise ValueError("T2 must not alias T (double buffering)")
    boxes = validate_boxes(boxes if boxes is not None else [interior_box(nx, ny, nz)],
                           nx, ny, nz)
    if not boxes:
        return
    coef = StencilCoef3(*coef)
    fast = _fast_math(tuning, coef)
    if T.is_cuda:
        tn = tuning or Stencil3DTuning()
        native().stencil3d_boxes(_ptr(T2), _ptr(T), _ptr(iCp), nx, ny, nz, boxes, tuple(coef),
                                 int(tn.rows), int(tn.unroll), int(tn.vec), int(tn.nontemporal),
                                 int(tn.chunk_z), int(tn.xcd_remap), stream_handle(T), True,
                                 *_uniform_args(tn, iCp), fast_math=fast, xface=xface,
                                 signal=int(tn.signal), signal_boxes=int(tn.signal_boxes))
    elif has_native():
        native().stencil3d_boxes(_ptr(T2), _ptr(T), _ptr(iCp), nx, ny, nz, boxes, tuple(coef),
                                 4, 1, 2, 0, 0, 0, 0, False, fast_math=fast)
    else:
        stencil3d_torch(T2, T, iCp, coef, boxes)


def stencil3dk_step(K: int, T2: torch.Tensor, T: torch.Tensor, iCp: torch.Tensor,
                    coef: StencilCoef3, boxes: Sequence[Box] | None = None,
                    tuning: Stencil3DTuning | None = None) -> None:
    """K explicit 3D diffusion steps in one pass: T2[b] = f^K(T)[b] on every box
    (default: the interior), the intermediate levels being f on the interior and
    T on the six faces. Bitwise equal to K full-interior ``stencil3d_step`` calls
    cropped to the boxes; cells outside the boxes keep T2's values.
    ``tuning.uniform`` as in ``stencil3d_step``: the GPU kernel does not read
    ``iCp`` then; accepted and ignored on CPU tensors. ``tuning.fast_math``: every
    level in the fast7 arithmetic (K = 1 included), on GPU and CPU tensors alike.
    ``tuning.xface`` sends boxes at most ``min(xface, 30)`` wide in x through the
    two-step kernel's x-face path (bitwise the same cells; ``stencil3d_dispatch``);
    CPU tensors accept and ignore it."""
    K = int(K)
    if K not in TEMPORAL_3D:
        raise ValueError(f"K={K} steps per pass is not instantiated (one of {TEMPORAL_3D})")
    if K == 1:
        stencil3d_step(T2, T, iCp, coef, boxes, tuning)
        return
    xface = int(tuning.xface) if tuning is not None else 0
    if not 0 <= xface <= XFACE_MAX:
        raise ValueError(f"xface={xface} (0: off, or the widest face box, up to {XFACE_MAX})")
    check_field("T", T)
    if T.dim() != 3:
        raise ValueError(f"T must be a (nz, ny, nx) field, got shape {tuple(T.shape)}")
    nz, ny, nx = T.shape
    if min(nx, ny, nz) < 3:
        raise ValueError(f"nx, ny, nz >= 3 required, got (nz, ny, nx) = {tuple(T.shape)}")
    check_field("T2", T2, (nz, ny, nx), T.device)
    check_field("iCp", iCp, (nz, ny, nx), T.device)
    if _overlap(T2, T):
        raise ValueError("T2 must not alias T (double buffering)")
    boxes = validate_boxes(boxes if boxes is not None else [interior_box(nx, ny, nz)],
                           nx, ny, nz)
    if not boxes:
        return
    coef = StencilCoef3(*coef)
    fast = _fast_math(tuning, coef)
    if T.is_cuda:
        tn = tuning or Stencil3DTuning()
        native().stencil3dk_boxes(K, _ptr(T2), _ptr(T), _ptr(iCp), nx, ny, nz, boxes,
                                  tuple(coef), int(tn.rows), int(tn.unroll), int(tn.vec),
                                  int(tn.nontemporal), int(tn.chunk_z), int(tn.xcd_remap),
                                  int(tn.tb_rows), int(tn.tb_chunk_z), int(tn.tb_nontemporal),
                                  stream_handle(T), True, *_uniform_args(tn, iCp),
                                  fast_math=fast, xface=xface, signal=int(tn.signal),
                                  signal_boxes=int(tn.signal_boxes))
    elif has_native():
        native().stencil3dk_boxes(K, _ptr(T2), _ptr(T), _ptr(iCp), nx, ny, nz, boxes,
                                  tuple(coef), 4, 1, 2, 0, 0, 0, 0, 0, 0, 0, False,
                                  fast_math=fast)
    else:
        stencil3dk_torch(K, T2, T, iCp, coef, boxes)


def stencil3d_dispatch(K: int, shape: Sequence[int], boxes: Sequence[Box],
                       tuning: Stencil3DTuning | None = None) -> list:
    """The kernel path each non-empty box of a K-step GPU launch on a
    ``(nz, ny, nx)`` field takes: ``[(box, path, lanes), ...]`` in the order of
    ``boxes``, ``path`` one of ``"march"`` (the strip march, 64 lanes a strip),
    ``"thin"`` (one-step boxes at most 8 wide, one thread per row, ``lanes`` 1)
    and ``"xface"`` (``tuning.xface``: ``lanes`` = 8, 16 or 32 per row). It is the
    host function both launchers run (``plan_dispatch3d``, csrc/kernels/
    kernel_select.cpp), so it needs the native extension and no GPU. With
    ``tuning.signal`` set (a frame-first fused launch) ``xface`` is not applied: no
    box takes the ``"xface"`` path."""
    K = int(K)
    if K not in TEMPORAL_3D:
        raise ValueError(f"K={K} steps per pass is not instantiated (one of {TEMPORAL_3D})")
    xface = int(tuning.xface) if tuning is not None else 0
    if not 0 <= xface <= XFACE_MAX:
        raise ValueError(f"xface={xface} (0: off, or the widest face box, up to {XFACE_MAX})")
    nz, ny, nx = (int(v) for v in shape)
    boxes = validate_boxes(boxes, nx, ny, nz)
    if tuning is not None and tuning.signal:
        xface = 0  # the x-face kernels do not signal
    got = native().stencil3d_dispatch(K, boxes, xface)
    return [(b, path, int(lanes)) for b, (path, lanes) in zip(boxes, got)]


class FusedPlan3D(NamedTuple):
    """``stencil3d_fused_plan``'s answer."""

    blocks: int  # blocks of the march launch
    prefix_blocks: int  # blocks of the signal prefix: the first ones, in dispatch order
    signalling_waves: int  # waves that count in signal[0]: 4 per prefix block
    boxes: list  # the boxes of the launch, in launch order
    block_map: list  # per block: (index into boxes, block inside that box)


def stencil3d_fused_plan(K: int, shape: Sequence[int], boxes: Sequence[Box], signal_boxes: int,
                         tuning: Stencil3DTuning | None = None) -> FusedPlan3D:
    """The march launch of a K-step GPU pass on a ``(nz, ny, nx)`` field whose first
    ``signal_boxes`` non-empty boxes are the signal prefix (``Stencil3DTuning.signal``):
    its block counts and the ``(box, block inside the box)`` every block works on,
    computed on the host by the functions the launchers and the kernels run
    (``stencil3d_fused_plan``, csrc/kernels/stencil3d.hip): the native extension, no
    GPU. Every refusal of a signalling launch is raised here too. ``signal_boxes=0``
    plans the unsignalled launch (``tuning.xface`` applies; boxes on the x-face path
    are not part of the march launch). Cells per lane are ``tuning.vec`` for even
    ``nx`` (16-byte aligned arrays assumed), else 1."""
    K = int(K)
    if K not in TEMPORAL_3D:
        raise ValueError(f"K={K} steps per pass is not instantiated (one of {TEMPORAL_3D})")
    tn = tuning or Stencil3DTuning()
    nz, ny, nx = (int(v) for v in shape)
    boxes = validate_boxes(boxes, nx, ny, nz)
    V = int(tn.vec) if nx % 2 == 0 else 1
    blocks, prefix, waves, _, pairs = native().stencil3d_fused_plan(
        K, V, boxes, int(signal_boxes), rows=int(tn.rows), unroll=int(tn.unroll),
        chunk_z=int(tn.chunk_z), xcd_remap=int(tn.xcd_remap), tb_rows=int(tn.tb_rows),
        tb_chunk_z=int(tn.tb_chunk_z), xface=int(tn.xface))
    if int(signal_boxes) > 0:
        used = boxes
    else:
        used = [b for b, path, _ in stencil3d_dispatch(K, shape, boxes, tn) if path != "xface"]
    return FusedPlan3D(int(blocks), int(prefix), int(waves), used,
                       [(int(a), int(b)) for a, b in pairs])


def stencil3dk_torch(K: int, T2: torch.Tensor, T: torch.Tensor, iCp: torch.Tensor,
                     c: StencilCoef3, boxes: Iterable[Box]) -> None:
    """Pure-torch twin of the K-step pass: K - 1 full-interior steps through two
    clones of T (the faces keep T), then the last step on the boxes."""
    nz, ny, nx = T.shape
    a, b = T.clone(), T.clone()
    for _ in range(K - 1):
        stencil3d_torch(b, a, iCp, c, [interior_box(nx, ny, nz)])
        a, b = b, a
    stencil3d_torch(T2, a, iCp, c, boxes)


def _check3(name: str, t: torch.Tensor):
    check_field(name, t)
    if t.dim() != 3:
        raise ValueError(f"{name} must be a (nz, ny, nx) field, got shape {tuple(t.shape)}")
    return t.shape


def init_gaussian3d_(T: torch.Tensor, geom: TileGeometry3, lx: float, ly: float,
                     lz: float) -> torch.Tensor:
    """T = exp(-(x_g+dx/2-lx/2)^2 - (y_g+dy/2-ly/2)^2 - (z_g+dz/2-lz/2)^2)."""
    nz, ny, nx = _check3("T", T)
    if T.is_cuda or has_native():
        native().init_gaussian3d(_ptr(T), nx, ny, nz, geom.as_tuple(), lx, ly, lz,
                                 stream_handle(T), T.is_cuda)
    else:
        from ..parallel.geometry import coords_1d

        x = coords_1d(geom.gx0, nx, geom.dx, geom.xoff, geom.nxg, geom.periodx)
        y = coords_1d(geom.gy0, ny, geom.dy, geom.yoff, geom.nyg, geom.periody)
        z = coords_1d(geom.gz0, nz, geom.dz, geom.zoff, geom.nzg, geom.periodz)
        a = (x + geom.dx / 2) - lx / 2
        b = (y + geom.dy / 2) - ly / 2
        c = (z + geom.dz / 2) - lz / 2
        T.copy_(torch.exp(-(a * a)[None, None, :] - (b * b)[None, :, None]
                          - (c * c)[:, None, None]))
    return T


def init_random3d_(A: torch.Tensor, geom: TileGeometry3, seed: int = 0, lo: float = 0.0,
                   hi: float = 1.0) -> torch.Tensor:
    """Counter-based uniform field keyed by the global cell index
    ``(gz*nyg + gy)*nxg + gx``: the same field for every decomposition."""
    nz, ny, nx = _check3("A", A)
    native().init_random3d(_ptr(A), nx, ny, nz, geom.as_tuple(), int(seed) & (2**64 - 1), lo, hi,
                           stream_handle(A), A.is_cuda)
    return A
