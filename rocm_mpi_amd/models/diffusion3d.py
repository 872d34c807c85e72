"""3D heat diffusion (explicit Euler, 7-point stencil, fp64) on the global grid.

ImplicitGlobalGrid's flagship example, with the physics of the 2D scripts
carried to three dimensions: ``lx=ly=lz=10, lam=1, Cp0=1``, ``dx=lx/nx_g()``
(likewise y, z) and ``dt=min(dx^2,dy^2,dz^2)*Cp0/lam/6.1`` (the explicit 3D
limit is 1/6; the reference takes 4.1 against the 2D limit of 4), initial
Gaussian on cell centres or the counter-based random field.

``perf``  one fused kernel on the interior (csrc/kernels/stencil3d.hip, or its
          CPU twin), swap, then ``update_halo_(T)`` -- serial, as the
          reference's ``diffusion_2D_perf.jl:47-52``.
``ap``    the same update as torch tensor expressions.
``perf_hide``  the perf pass split into a boundary frame and an interior box
          (``ops.hide_boxes3d``, ImplicitGlobalGrid's ``@hide_communication``
          with boundary width ``b_width``): the frame runs on a high-priority
          stream with ``update_halo_`` right behind it, the interior on a
          low-priority stream next to both. Bitwise the ``perf`` field.

All compute the canonical per-cell expression (``ops.StencilCoef3``), so their
fields agree bitwise, with each other and across decompositions.

``temporal=2`` (perf only) runs two steps per kernel pass (temporal blocking,
csrc/kernels/stencil3d_tb.hip): bitwise the same field, half the passes and
halo exchanges. As in 2D, K-step passes need width-K halos, i.e. grid overlap
2K, which changes ``nx_g``, ``dx`` and ``dt`` on a multi-rank grid.

Uniform 1/Cp (``uniform_factor``, on by default): the model scans ``iCp`` once
(``ops.count_differing``, a bit compare with cell 0) and, when every cell holds
one value, the perf passes on a GPU run the kernels' uniform-factor variants:
the value travels as a kernel argument, the array is not read, and a pass moves
16 instead of 24 bytes per cell -- bitwise the same field (the CPU twins always
read the array). An in-place torch edit of ``iCp`` is seen through the tensor's
version counter before the next step; after a write torch cannot see (a raw
pointer, ``ops.fill_``) call ``rescan_factor()``. The verdict is per rank: the
paths are bitwise equal, so ranks need not agree. ``T_eff`` keeps the
reference's ``3*nx*ny*nz*8`` bytes per step by definition, whichever path runs.

``fast_math`` (perf only, off by default): every pass of ``plan(n)``, the
one-step remainder passes included, runs the fast7 arithmetic (``ops.fast7_ok``;
the 7-point sum with the constants folded into one per-cell factor, 8 fp64
operations per update instead of about 30). The field is then independent of
the plan, of the decomposition, of the uniform-factor path and of the device
(the C++ twin is bitwise equal to the kernels), and rounding-close to the
canonical field, not bitwise equal to it. It combines with ``temporal`` and with
the uniform-factor scan unchanged.

``perf_hide`` in detail. ``b_width[d]`` (default ``(16, 2, 2)``, the reference's
3D example) counts cells from the array edge; on a side with a neighbour the
interior box starts ``max(b_width[d], overlap[d])`` cells in, a side without a
neighbour has no frame slab. Per pass of ``plan(n)`` on a GPU, enqueued in this
order so that a transport whose exchange blocks the host still overlaps:

1. the frame boxes, one ``ops`` launch on the high-priority stream H;
2. the interior box on the low-priority stream L;
3. ``update_halo_(T2)`` on H; then the buffers swap.

Streams and events are created once per model; ordering is by events only, no
host synchronisation. At the start of ``step`` H and L wait for the caller's
current stream, at its end the current stream waits for both, so ``step`` stays
asynchronous and ``field``, ``check_finite`` and ``gather_interior`` stay correct
on the current stream. Between passes the light protocol ships (not the full
join): with X the buffer pass p writes and Y the one it reads,

* H's frame of pass p+1 waits for L's interior of pass p: it reads interior
  cells of X and overwrites frame cells of Y, which that interior read. The
  exchange of pass p precedes it on H in stream order.
* L's interior of pass p+1 waits for H's frame kernel of pass p, not for the
  exchange of pass p: it reads X at least ``overlap - K >= halo width`` cells
  from the array edge, so never a halo cell, the only cells the exchange
  writes, and it writes interior cells of Y, which the exchange (it reads send
  planes of X, all in the frame, and writes halo cells of X) does not touch.

With no neighbour at all, or an interior box empty in some dimension, a pass is
one launch on the current stream followed by the exchange, as ``perf``. CPU
tensors run the same boxes in sequence: frame, exchange, interior.
``temporal``, ``fast_math`` and the uniform-factor scan apply as for ``perf``.
``xface`` (default 0, decided by profiles/diffusion3d_hide.md): the width up to
which the frame's boxes run the kernels' x-face paths
(``Stencil3DTuning.xface``); ``None`` takes ``min(max(b_width[0], overlap), 32)``.
It applies to the frame launch of one- and two-step passes alike; in a two-step
pass a box needs two more columns than its width, so boxes wider than 30 keep
the strip march (``ops.stencil3d_dispatch`` tells which box runs where).

``fused`` (perf_hide only; the default is decided by profiles/diffusion3d_fused.md):
frame-first single-launch passes. A pass that splits is ONE launch on L, the
frame boxes as its signal prefix and the interior box after them
(``Stencil3DTuning.signal``): the frame blocks dispatch first and the last frame
wave raises a device flag. Per pass, enqueued in this order:

1. L waits for the event of H's previous exchange (the frame blocks read the halo);
2. the launch on L;
3. on H ``flag_wait(signal + 1, 1)``, ``flag_write(signal + 1, 0)``,
   ``update_halo_(T2)``, its event; then the buffers swap.

The launch is always enqueued before the wait on it. No box of such a launch takes
the x-face path. Passes that do not split stay the perf pass, ordered as above;
CPU tensors run frame, exchange, interior in sequence as without ``fused``. The
wait is bounded (``fused_timeout_s``, ``RMA_EXEC_FUSED_TIMEOUT``): ``synchronize()``
raises if one timed out, since the halos of that pass are wrong. ``fused_passes``
counts the fused passes. Bitwise the ``perf`` field.

``native`` (off by default; perf and perf_hide on a GPU whose grid has a native
halo engine: the self, rccl, ipc and loopback transports): ``step(n)`` is one call
into the C++ time loop (csrc/runtime/executor3d.cpp), which enqueues on the
current stream exactly what is described above, so the field is bitwise the same;
``T`` / ``T2`` follow its parity and ``rescan_factor()`` is forwarded to it. CPU
tensors, ``ap`` and the other transports keep the Python-issued loop
(``native_loop`` says which one runs). profiles/diffusion3d_native.md has the host
cost of both loops.

Out of scope here (the 2D model has them): passes deeper than two steps, a pass
planner, hipGraph replay, checkpointing, direct-store halos and the x-face path
inside a fused launch.
"""
from __future__ import annotations

import dataclasses
import os
from dataclasses import dataclass

import torch

from .. import ops
from ..config import diag_value
from ..parallel import implicit_grid as gg
from ..parallel.halo import gather_, update_halo_
from ..utils import metrics

VARIANTS3D = ("perf", "ap", "perf_hide")
_KERNEL_VARIANTS = ("perf", "perf_hide")  # the fused kernels on double buffers
# steps per pass whose uniform-factor kernel the model runs when 1/Cp is one value
# (profiles/diffusion3d_uniform.md); the others keep the field path
UNIFORM_PASSES_3D = (1, 2)


def _factor_diag_off() -> bool:
    """RMA_DIAG=uniform_factor=off (the 2D executor's switch)."""
    v = diag_value("uniform_factor")
    if v not in ("", "off"):
        raise ValueError(f"RMA_DIAG uniform_factor={v} (off)")
    return v == "off"


@dataclass
class Diffusion3DConfig:
    variant: str = "perf"
    nx: int = 64
    ny: int = 64
    nz: int = 64
    nt: int = 100
    lx: float = 10.0
    ly: float = 10.0
    lz: float = 10.0
    lam: float = 1.0
    Cp0: float = 1.0
    init: str = "gaussian"  # gaussian | random
    seed: int = 1234
    dims: tuple = (0, 0, 0)
    periods: tuple = (0, 0, 0)
    transport: str = "auto"
    device: str | None = None
    check_every: int = 0  # NaN/Inf guard period (0 = off)
    quiet: bool = False
    tuning: ops.Stencil3DTuning | None = None
    temporal: int = 1  # steps per kernel pass (ops.TEMPORAL_3D), perf only
    uniform_factor: bool = True  # uniform-1/Cp kernel variants where 1/Cp is one value
    fast_math: bool = False  # the fast7 arithmetic in every pass, perf / perf_hide only
    b_width: tuple = (16, 2, 2)  # perf_hide boundary width per dimension, from the array edge
    # perf_hide: widest frame box on the x-face path of the one- and two-step kernels
    # (0: off, None: min(max(b_width[0], overlap), 32)); profiles/diffusion3d_hide.md
    xface: int | None = 0
    # perf / perf_hide on a GPU with a native halo engine: step(n) is enqueued by the
    # C++ time loop (_C.Executor3D, csrc/runtime/executor3d.cpp) instead of pass by
    # pass from Python; bitwise the same field (profiles/diffusion3d_native.md)
    native: bool = False
    # perf_hide: frame-first single-launch passes (module docstring); off by the rule
    # of profiles/diffusion3d_fused.md. The wait of the exchange stream for the
    # frame flag gives up after fused_timeout_s (RMA_EXEC_FUSED_TIMEOUT replaces it)
    fused: bool = False
    fused_timeout_s: float = 60.0

    def validate(self) -> None:
        if self.variant not in VARIANTS3D:
            raise ValueError(f"variant must be one of {VARIANTS3D}")
        if self.init not in ("gaussian", "random"):
            raise ValueError("init must be gaussian or random")
        if min(self.nx, self.ny, self.nz) < 3:
            raise ValueError("nx, ny, nz >= 3 required")
        if self.nt < 1:
            raise ValueError("nt >= 1 required")
        if self.temporal not in ops.TEMPORAL_3D:
            raise ValueError(f"temporal must be one of {ops.TEMPORAL_3D}")
        if self.temporal > 1 and self.variant not in _KERNEL_VARIANTS:
            raise ValueError("temporal blocking applies to the perf variant (and perf_hide)")
        if self.fast_math and self.variant not in _KERNEL_VARIANTS:
            raise ValueError("fast_math applies to the perf variant (and perf_hide)")
        if self.fused not in (False, True, 0, 1):
            raise ValueError(f"fused must be False or True, got {self.fused!r}")
        if self.fused and self.variant != "perf_hide":
            raise ValueError(f"fused=True applies to the perf_hide variant, got {self.variant!r}")
        if self.fused and not float(self.fused_timeout_s) > 0.0:
            raise ValueError(f"fused_timeout_s > 0 required, got {self.fused_timeout_s}")
        if self.variant == "perf_hide":
            bw = tuple(self.b_width)
            if len(bw) != 3 or any(int(b) != b or b < 1 for b in bw):
                raise ValueError(f"b_width must be three integers >= 1, got {self.b_width}")
            if self.xface is not None and not 0 <= int(self.xface) <= ops.XFACE_MAX:
                raise ValueError(f"xface must be None or 0..{ops.XFACE_MAX}, got {self.xface}")


class Diffusion3D:
    """One rank's share of the distributed 3D diffusion problem. Uses the
    current global grid, or creates (and then owns) one from the config."""

    def __init__(self, cfg: Diffusion3DConfig, grid_kwargs: dict | None = None):
        cfg.validate()
        _factor_diag_off()  # a bad value is refused before the grid exists
        self.cfg = cfg
        if not gg.grid_is_initialized():
            kw = dict(grid_kwargs or {})
            kw.setdefault("quiet", cfg.quiet)
            if cfg.temporal > 1:  # width-K halos need overlap 2K (IGG: ol >= 2*hw)
                K = cfg.temporal
                kw.setdefault("overlaps", (2 * K, 2 * K, 2 * K))
                kw.setdefault("halowidths", (K, K, K))
            gg.init_global_grid(cfg.nx, cfg.ny, cfg.nz, dimx=cfg.dims[0], dimy=cfg.dims[1],
                                dimz=cfg.dims[2], periodx=cfg.periods[0], periody=cfg.periods[1],
                                periodz=cfg.periods[2], transport=cfg.transport,
                                device=cfg.device, **kw)
            self._owns_grid = True
        else:
            self._owns_grid = False
        g = self.g = gg.global_grid()
        if tuple(g.nxyz) != (cfg.nx, cfg.ny, cfg.nz):
            raise ValueError(f"global grid local size {g.nxyz} != config "
                             f"{(cfg.nx, cfg.ny, cfg.nz)}")
        if cfg.temporal > 1:
            K = cfg.temporal
            if any(max(g.neighbors[d]) >= 0 and g.overlaps[d] < 2 * K for d in (0, 1, 2)):
                raise ValueError(f"temporal={K} needs grid overlaps >= {2 * K} "
                                 f"(init_global_grid(overlaps=({2 * K},{2 * K},{2 * K}), "
                                 f"halowidths=({K},{K},{K})))")
        self.device = g.device
        nx, ny, nz = cfg.nx, cfg.ny, cfg.nz
        self.dx, self.dy, self.dz = cfg.lx / gg.nx_g(), cfg.ly / gg.ny_g(), cfg.lz / gg.nz_g()
        self.dt = min(self.dx * self.dx, self.dy * self.dy, self.dz * self.dz) \
            * cfg.Cp0 / cfg.lam / 6.1
        self.coef = ops.StencilCoef3.from_physics(cfg.lam, self.dx, self.dy, self.dz, self.dt)
        if cfg.fast_math and not ops.fast7_ok(self.coef):
            self.close()
            raise ValueError("fast_math: the fast7 arithmetic needs lam != 0 and finite "
                             f"coefficients, got {tuple(self.coef)}")
        f64 = dict(dtype=torch.float64, device=self.device)
        self.iCp = torch.empty((nz, ny, nx), **f64)
        ops.fill_(self.iCp, 1.0 / cfg.Cp0)
        self.rescan_factor()
        self.T = torch.empty((nz, ny, nx), **f64)
        self.init_field(self.T)
        self.T2 = self.T.clone() if cfg.variant in _KERNEL_VARIANTS else None
        self._hide = None  # perf_hide on a GPU: (H, L, events), created at the first step
        self._fused = None  # cfg.fused on a GPU: (signal words, error word), with _hide
        self._fused_passes = 0
        if cfg.variant == "ap":  # flux arrays of the interior rows, preallocated
            self.qx = torch.empty((nz - 2, ny - 2, nx - 1), **f64)
            self.qy = torch.empty((nz - 2, ny - 1, nx - 2), **f64)
            self.qz = torch.empty((nz - 1, ny - 2, nx - 2), **f64)
            self.dTdt = torch.empty((nz - 2, ny - 2, nx - 2), **f64)
            self._tmp = torch.empty((nz - 2, ny - 2, nx - 2), **f64)
        self.steps_done = 0
        self._exec = None  # the native time loop (cfg.native), with the two buffers it holds
        if self.native_loop:
            try:
                self._make_executor()
            except Exception:
                self.close()
                raise

    # ------------------------------------------------------------------
    @property
    def native_loop(self) -> bool:
        """step(n) goes to the C++ time loop: cfg.native, a kernel variant, GPU
        tensors and a native halo engine (the self, rccl, ipc and loopback
        transports). Everything else keeps the Python-issued loop."""
        return bool(self.cfg.native and self.cfg.variant in _KERNEL_VARIANTS
                    and self.device.type == "cuda" and self.g.halo is not None)

    def _make_executor(self) -> None:
        from .._native import native

        cfg, g = self.cfg, self.g
        tn = cfg.tuning or ops.Stencil3DTuning()
        if tn.uniform or tn.fast_math or tn.xface or tn.signal or tn.signal_boxes:
            raise ValueError("native=True sets uniform, fast_math, xface and the signal per launch "
                             "from the config (uniform_factor, fast_math, xface, fused), not from "
                             "cfg.tuning")
        self._bufs = (self.T, self.T2)
        self._exec = native().Executor3D(
            self.T.data_ptr(), self.T2.data_ptr(), self.iCp.data_ptr(), cfg.nx, cfg.ny, cfg.nz,
            1 if cfg.variant == "perf_hide" else 0, tuple(self.coef), g.halo,
            overlaps=[int(o) for o in g.overlaps], halowidths=[int(h) for h in g.halowidths],
            steps_per_pass=int(cfg.temporal), fast_math=bool(cfg.fast_math),
            b_width=[int(b) for b in cfg.b_width],
            xface=-1 if cfg.xface is None else int(cfg.xface),
            uniform_factor=bool(cfg.uniform_factor), rows=int(tn.rows), unroll=int(tn.unroll),
            vec=int(tn.vec), nontemporal=int(tn.nontemporal), chunk_z=int(tn.chunk_z),
            xcd_remap=int(tn.xcd_remap), tb_rows=int(tn.tb_rows), tb_chunk_z=int(tn.tb_chunk_z),
            tb_nontemporal=int(tn.tb_nontemporal), fused=1 if cfg.fused else 0,
            fused_timeout_s=float(cfg.fused_timeout_s))
        self._adopt_verdict()

    def _adopt_verdict(self) -> None:
        """The executor's scan of 1/Cp is the model's."""
        self._iCp_scanned = self.iCp._version
        self._uniform = bool(self._exec.uniform)
        self._factor = float(self._exec.uniform_value) if self._uniform else 0.0

    def _step_native(self, n: int) -> None:
        self._exec.run(int(n), torch.cuda.current_stream(self.device).cuda_stream)
        p = self._exec.parity
        self.T, self.T2 = self._bufs[p], self._bufs[1 - p]
        self.steps_done += int(n)

    # ------------------------------------------------------------------
    def geometry(self) -> ops.TileGeometry3:
        g = self.g
        return ops.TileGeometry3(
            gx0=g.coords[0] * (g.nx - g.overlaps[0]), gy0=g.coords[1] * (g.ny - g.overlaps[1]),
            gz0=g.coords[2] * (g.nz - g.overlaps[2]), nxg=g.nxyz_g[0], nyg=g.nxyz_g[1],
            nzg=g.nxyz_g[2], dx=self.dx, dy=self.dy, dz=self.dz, periodx=g.periods[0],
            periody=g.periods[1], periodz=g.periods[2])

    def init_field(self, T: torch.Tensor) -> None:
        cfg = self.cfg
        if cfg.init == "random":
            ops.init_random3d_(T, self.geometry(), seed=cfg.seed)
        else:
            ops.init_gaussian3d_(T, self.geometry(), cfg.lx, cfg.ly, cfg.lz)

    @property
    def field(self) -> torch.Tensor:
        """The current temperature field (after the last completed step)."""
        return self.T

    # ------------------------------------------------------------------
    def owned_box(self, k: int) -> tuple:
        """Cells a k-step pass writes: next to a neighbour the k cells [0,k) are
        halo (refreshed by the exchange), elsewhere the boundary cell 0 stays."""
        nb, n = self.g.neighbors, (self.cfg.nx, self.cfg.ny, self.cfg.nz)
        box = []
        for d in (0, 1, 2):
            box += [k if nb[d][0] >= 0 else 1, n[d] - (k if nb[d][1] >= 0 else 1)]
        return tuple(box)

    @property
    def uniform_factor(self) -> bool:
        """The verdict of the last scan of 1/Cp: every cell holds one bit pattern
        (the perf passes on a GPU then do not read the array). False when the
        config or RMA_DIAG=uniform_factor=off disables the variant."""
        return self._uniform

    def rescan_factor(self) -> bool:
        """Examine 1/Cp again (one pass over the array, synchronises) and return
        the verdict. step() does this by itself after an in-place torch edit;
        call it after a write torch's version counter does not see."""
        off = _factor_diag_off()
        if getattr(self, "_exec", None) is not None:  # the native loop scans for both
            self._exec.rescan_factor()
            self._adopt_verdict()
            return self._uniform
        self._iCp_scanned = self.iCp._version
        self._uniform, self._factor = False, 0.0
        if self.cfg.uniform_factor and not off and ops.count_differing(self.iCp) == 0:
            self._uniform, self._factor = True, float(self.iCp[0, 0, 0])
        return self._uniform

    @property
    def uniform_value(self) -> float:
        """The one value of 1/Cp found by the last scan (0.0 without a verdict)."""
        return self._factor

    def uniform_passes(self) -> tuple:
        """Steps per pass whose kernel runs its uniform-factor variant now: the
        perf passes on a GPU, after a scan that found one value."""
        if not (self._uniform and self.cfg.variant in _KERNEL_VARIANTS
                and self.device.type == "cuda"):
            return ()
        return tuple(k for k in sorted({1, self.cfg.temporal}) if k in UNIFORM_PASSES_3D)

    def _tuning(self, k: int) -> ops.Stencil3DTuning | None:
        """cfg.tuning, with cfg.fast_math and the uniform-factor variant of a
        k-step GPU pass on top where the last scan allows it."""
        tn = self.cfg.tuning
        if self.cfg.fast_math:
            tn = dataclasses.replace(tn or ops.Stencil3DTuning(), fast_math=True)
        if k not in self.uniform_passes():
            return tn
        return dataclasses.replace(tn or ops.Stencil3DTuning(), uniform=True,
                                   uniform_value=self._factor)

    def plan(self, n: int) -> list:
        """Passes step(n) runs: n // K passes of K steps, the rest one step each."""
        K = self.cfg.temporal
        return [K] * (int(n) // K) + [1] * (int(n) % K)

    def step(self, n: int = 1) -> None:
        """Advance n time steps (asynchronous on a GPU)."""
        # uniform-factor passes do not read 1/Cp: an in-place edit since the last
        # scan must be seen before they run
        if self.iCp._version != self._iCp_scanned:
            self.rescan_factor()
        if self._exec is not None:
            self._step_native(n)
            return
        if self.cfg.variant == "ap":
            for _ in range(int(n)):
                self._step_ap()
                self.steps_done += 1
            return
        if self.cfg.variant == "perf_hide":
            self._step_hide(n)
            return
        for k in self.plan(n):
            if k == 1:
                ops.stencil3d_step(self.T2, self.T, self.iCp, self.coef, tuning=self._tuning(1))
            else:
                ops.stencil3dk_step(k, self.T2, self.T, self.iCp, self.coef, [self.owned_box(k)],
                                    tuning=self._tuning(k))
            self.T, self.T2 = self.T2, self.T
            update_halo_(self.T)
            self.steps_done += k

    # ------------------------------------------------------------------
    def hide_boxes(self, k: int) -> tuple:
        """(frame boxes, interior box | None) of a k-step perf_hide pass."""
        g = self.g
        sides = [(g.neighbors[d][0] >= 0, g.neighbors[d][1] >= 0) for d in (0, 1, 2)]
        return ops.hide_boxes3d((self.cfg.nx, self.cfg.ny, self.cfg.nz), self.owned_box(k),
                                sides, g.overlaps, self.cfg.b_width)

    def frame_xface(self, k: int = 1) -> int:
        """Stencil3DTuning.xface of the frame launch of a k-step perf_hide pass:
        cfg.xface, or with None ``min(max(b_width[0], overlap), 32)``. The value
        does not depend on k; what it does per box does (``ops.stencil3d_dispatch``:
        a two-step pass keeps boxes wider than 30 on the strip march)."""
        if int(k) not in ops.TEMPORAL_3D:
            raise ValueError(f"k={k} steps per pass (one of {ops.TEMPORAL_3D})")
        xf = self.cfg.xface
        if xf is None:
            xf = min(max(int(self.cfg.b_width[0]), int(self.g.overlaps[0])), ops.XFACE_MAX)
        return int(xf)

    @property
    def fused_passes(self) -> int:
        """Passes enqueued as one frame-first launch so far (cfg.fused on a GPU)."""
        if self._exec is not None:
            return int(self._exec.fused_passes)
        return self._fused_passes

    def fused_timeout(self) -> float:
        """Bound of the exchange stream's wait for the frame flag, seconds:
        RMA_EXEC_FUSED_TIMEOUT where set (as the native loops read it), else
        cfg.fused_timeout_s."""
        v = os.environ.get("RMA_EXEC_FUSED_TIMEOUT")
        if v is None:
            return float(self.cfg.fused_timeout_s)
        try:
            t = float(v)
        except ValueError:
            t = float("nan")
        if not 1e-9 <= t <= 1e6:
            raise ValueError(f"RMA_EXEC_FUSED_TIMEOUT={v!r} (a number of seconds in [1e-9, 1e6])")
        return t

    def _launch(self, k: int, boxes, frame: bool = False, signal_boxes: int = 0) -> None:
        """One k-step launch T -> T2 on the boxes, on the current stream; with
        signal_boxes the first boxes are the signal prefix of a fused pass."""
        tn = self._tuning(k)
        if frame and self.frame_xface(k):
            tn = dataclasses.replace(tn or ops.Stencil3DTuning(), xface=self.frame_xface(k))
        if signal_boxes:
            tn = dataclasses.replace(tn or ops.Stencil3DTuning(), xface=0,
                                     signal=self._fused[0].data_ptr(),
                                     signal_boxes=int(signal_boxes))
        if k == 1:
            ops.stencil3d_step(self.T2, self.T, self.iCp, self.coef, boxes, tuning=tn)
        else:
            ops.stencil3dk_step(k, self.T2, self.T, self.iCp, self.coef, boxes, tuning=tn)

    def _step_hide(self, n: int) -> None:
        """The passes of plan(n), frame / exchange overlapped with the interior
        (module docstring: streams, events and the read / write sets)."""
        plan = self.plan(n)
        split = {k: self.hide_boxes(k) for k in set(plan)}
        gpu = self.device.type == "cuda"
        overlapped = gpu and any(fr and inner is not None for fr, inner in split.values())
        if overlapped:
            if self._hide is None:
                # torch: a lower number is a higher priority, 0 the default one
                self._hide = (torch.cuda.Stream(self.device, priority=-1),
                              torch.cuda.Stream(self.device, priority=0),
                              [torch.cuda.Event() for _ in range(4)])
            H, L, (ev_in, ev_frame, ev_inner, ev_halo) = self._hide
            if self.cfg.fused and self._fused is None:
                # [frame wave counter, frame flag] and the error word of the bounded
                # wait, zeroed on L, where the signalling launches run, and waited for
                with torch.cuda.stream(L):
                    self._fused = (torch.zeros(2, dtype=torch.int64, device=self.device),
                                   torch.zeros(1, dtype=torch.int32, device=self.device))
                L.synchronize()
                self._fused_timeout = self.fused_timeout()
            cur = torch.cuda.current_stream(self.device)
            ev_in.record(cur)
            H.wait_event(ev_in)
            L.wait_event(ev_in)
            # the first pass waits on these as on "the pass before"
            ev_inner.record(L)
            ev_frame.record(H)
        for k in plan:
            frame, inner = split[k]
            if not frame or inner is None:  # nothing to overlap: the perf pass
                if overlapped:  # (another k of this plan overlaps) stay ordered on H
                    H.wait_event(ev_inner)
                    with torch.cuda.stream(H):
                        self._launch(k, frame or [inner])
                        self.T, self.T2 = self.T2, self.T
                        update_halo_(self.T)
                    ev_frame.record(H)
                    L.wait_event(ev_frame)
                    ev_inner.record(L)
                else:
                    self._launch(k, frame or [inner])
                    self.T, self.T2 = self.T2, self.T
                    update_halo_(self.T)
            elif not gpu:  # the same boxes in sequence: frame, exchange, interior
                self._launch(k, frame, frame=True)
                update_halo_(self.T2)
                self._launch(k, [inner])
                self.T, self.T2 = self.T2, self.T
            elif self.cfg.fused:
                from .._native import native

                # frame-first single launch (module docstring); ev_frame is the event
                # of H's previous exchange here
                sig, err = self._fused
                L.wait_event(ev_frame)
                with torch.cuda.stream(L):
                    self._launch(k, list(frame) + [inner], signal_boxes=len(frame))
                ev_inner.record(L)
                native().flag_wait(sig.data_ptr() + 8, 1, self._fused_timeout, err.data_ptr(), 1,
                                   H.cuda_stream)
                native().flag_write(sig.data_ptr() + 8, 0, H.cuda_stream)
                with torch.cuda.stream(H):
                    update_halo_(self.T2)
                ev_frame.record(H)
                self.T, self.T2 = self.T2, self.T
                self._fused_passes += 1
            else:
                H.wait_event(ev_inner)  # interior of the pass before: reads / writes above
                with torch.cuda.stream(H):
                    self._launch(k, frame, frame=True)
                L.wait_event(ev_frame)  # frame kernel of the pass before, not its exchange
                ev_frame.record(H)
                with torch.cuda.stream(L):
                    self._launch(k, [inner])
                ev_inner.record(L)
                with torch.cuda.stream(H):
                    update_halo_(self.T2)
                self.T, self.T2 = self.T2, self.T
            self.steps_done += k
        if overlapped:
            cur = torch.cuda.current_stream(self.device)
            ev_halo.record(H)
            cur.wait_event(ev_halo)
            cur.wait_event(ev_inner)

    def _step_ap(self) -> None:
        """The canonical update as torch expressions (same operation order)."""
        c = self.coef
        T, qx, qy, qz, d, tmp = self.T, self.qx, self.qy, self.qz, self.dTdt, self._tmp
        torch.sub(T[1:-1, 1:-1, 1:], T[1:-1, 1:-1, :-1], out=qx)
        qx.mul_(c.mlam).mul_(c.rdx)
        torch.sub(T[1:-1, 1:, 1:-1], T[1:-1, :-1, 1:-1], out=qy)
        qy.mul_(c.mlam).mul_(c.rdy)
        torch.sub(T[1:, 1:-1, 1:-1], T[:-1, 1:-1, 1:-1], out=qz)
        qz.mul_(c.mlam).mul_(c.rdz)
        torch.sub(qx[:, :, 1:], qx[:, :, :-1], out=d)
        d.neg_().mul_(c.rdx)  # (-(qxR-qxL))*rdx
        torch.sub(qy[:, 1:, :], qy[:, :-1, :], out=tmp)
        d.sub_(tmp.mul_(c.rdy))  # - (qyU-qyD)*rdy
        torch.sub(qz[1:, :, :], qz[:-1, :, :], out=tmp)
        d.sub_(tmp.mul_(c.rdz))  # - (qzF-qzB)*rdz
        d.mul_(self.iCp[1:-1, 1:-1, 1:-1]).mul_(c.dt)
        T[1:-1, 1:-1, 1:-1].add_(d)
        update_halo_(T)

    def synchronize(self) -> None:
        """Wait for the device; raises if a fused pass's wait for the frame flag
        timed out (the halos of that pass are wrong)."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
            if self._exec is not None:
                self._exec.check()
            elif self._fused is not None and int(self._fused[1].item()) != 0:
                raise RuntimeError("frame-first fused pass: the exchange stream's wait for the "
                                   f"frame flag timed out after {self._fused_timeout} s "
                                   "(RMA_EXEC_FUSED_TIMEOUT); the halos of that pass are wrong")

    def check_finite(self) -> None:
        bad = float(ops.reduce(self.field, "nonfinite"))
        if bad:
            raise FloatingPointError(
                f"rank {self.g.me}: {int(bad)} non-finite cells after step {self.steps_done}")

    def _advance(self, n: int) -> None:
        k = self.cfg.check_every
        if k <= 0:
            self.step(n)
            return
        done = 0
        while done < n:
            m = min(k, n - done)
            self.step(m)
            done += m
            self.check_finite()

    def run(self, nt: int | None = None, warmup: int = 10) -> metrics.RunResult:
        """The reference protocol: nt steps, the timer starts after ``warmup``
        of them; wall time through tic/toc and T_eff of the local tile."""
        cfg, g = self.cfg, self.g
        nt = cfg.nt if nt is None else int(nt)
        warm = min(int(warmup), nt - 1) if nt > 1 else 0
        timed = nt - warm
        if warm:
            self._advance(warm)
        self.synchronize()
        gg.tic()
        self._advance(timed)
        self.synchronize()
        wtime = gg.toc()
        teff = metrics.t_eff(cfg.nx, cfg.ny, wtime, timed, nz=cfg.nz)
        res = metrics.RunResult(
            variant=cfg.variant + "3d", nprocs=g.nprocs, dims=g.dims, nx=cfg.nx, ny=cfg.ny,
            nxg=g.nxyz_g[0], nyg=g.nxyz_g[1], nt=nt, timed_steps=timed, wtime=wtime,
            t_it=wtime / timed, teff=teff, teff_min=g.comm.allreduce(teff, "min"),
            teff_max=g.comm.allreduce(teff, "max"), teff_total=g.comm.allreduce(teff, "sum"),
            transport=g.transport, device=str(self.device))
        res.extra["nz"] = cfg.nz
        res.extra["nzg"] = g.nxyz_g[2]
        res.extra["fast_math"] = bool(cfg.fast_math)
        if cfg.variant == "perf_hide":
            res.extra["b_width"] = [int(b) for b in cfg.b_width]
        if g.me == 0 and not cfg.quiet:
            print(metrics.reference_line(nt, wtime, teff), flush=True)
        return res

    def gather_interior(self, root: int = 0):
        """The global field without its boundary cells assembled on root (None
        elsewhere): every rank contributes the cells it owns, each global cell
        once whatever the overlap."""
        g = self.g
        if all(o == 2 for o in g.overlaps):  # equal shares: the reference's gather!
            return gather_(self.field[1:-1, 1:-1, 1:-1].contiguous(), None, root)
        parts = g.comm.gather(self.field.contiguous(), root)
        if g.me != root:
            return None
        n = (self.cfg.nx, self.cfg.ny, self.cfg.nz)

        def owned(c: int, d: int) -> tuple:
            """Local [lo, hi) of the cells the rank at coordinate c owns along d."""
            ol = g.overlaps[d]
            if g.periods[d]:  # n - ol distinct cells per rank, the grid's first is a ghost
                return 1, 1 + n[d] - ol
            # the overlap is split between the two neighbours; a physical face loses 1 cell
            return (ol // 2 if c > 0 else 1), n[d] - ((ol - ol // 2) if c < g.dims[d] - 1 else 1)

        size = [sum(hi - lo for lo, hi in (owned(c, d) for c in range(g.dims[d])))
                for d in (0, 1, 2)]
        out = torch.empty(size[::-1], dtype=self.field.dtype)
        for r, part in enumerate(parts):
            c = g.topo.coords(r)
            src, dst = [], []
            for d in (2, 1, 0):
                lo, hi = owned(c[d], d)
                start = sum(b - a for a, b in (owned(cc, d) for cc in range(c[d])))
                src.append(slice(lo, hi))
                dst.append(slice(start, start + hi - lo))
            out[tuple(dst)] = part[tuple(src)].to(out.device)
        return out

    def close(self) -> None:
        self.synchronize()
        self._exec = None  # its streams and events go before the grid's halo engine
        if self._owns_grid:
            gg.finalize_global_grid()
            self._owns_grid = False
