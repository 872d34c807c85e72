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

Both compute the canonical per-cell expression (``ops.StencilCoef3``), so their
fields agree bitwise, with each other and across decompositions.

Out of scope here (the 2D model has them): overlap of the boundary update with
the interior, K-step passes, the native executor (every step is issued from
Python), checkpointing and direct-store halos.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import ops
from ..parallel import implicit_grid as gg
from ..parallel.halo import gather_, update_halo_
from ..utils import metrics

VARIANTS3D = ("perf", "ap")


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

    def validate(self) -> None:
        if self.variant not in VARIANTS3D:
            raise ValueError(f"variant must be one of {VARIANTS3D}")
        if self.init not in ("gaussian", "random"):
            raise ValueError("init must be gaussian or random")
        if min(self.nx, self.ny, self.nz) < 3:
            raise ValueError("nx, ny, nz >= 3 required")
        if self.nt < 1:
            raise ValueError("nt >= 1 required")


class Diffusion3D:
    """One rank's share of the distributed 3D diffusion problem. Uses the
    current global grid, or creates (and then owns) one from the config."""

    def __init__(self, cfg: Diffusion3DConfig, grid_kwargs: dict | None = None):
        cfg.validate()
        self.cfg = cfg
        if not gg.grid_is_initialized():
            kw = dict(grid_kwargs or {})
            kw.setdefault("quiet", cfg.quiet)
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
        self.device = g.device
        nx, ny, nz = cfg.nx, cfg.ny, cfg.nz
        self.dx, self.dy, self.dz = cfg.lx / gg.nx_g(), cfg.ly / gg.ny_g(), cfg.lz / gg.nz_g()
        self.dt = min(self.dx * self.dx, self.dy * self.dy, self.dz * self.dz) \
            * cfg.Cp0 / cfg.lam / 6.1
        self.coef = ops.StencilCoef3.from_physics(cfg.lam, self.dx, self.dy, self.dz, self.dt)
        f64 = dict(dtype=torch.float64, device=self.device)
        self.iCp = torch.empty((nz, ny, nx), **f64)
        ops.fill_(self.iCp, 1.0 / cfg.Cp0)
        self.T = torch.empty((nz, ny, nx), **f64)
        self.init_field(self.T)
        self.T2 = self.T.clone() if cfg.variant == "perf" else None
        if cfg.variant == "ap":  # flux arrays of the interior rows, preallocated
            self.qx = torch.empty((nz - 2, ny - 2, nx - 1), **f64)
            self.qy = torch.empty((nz - 2, ny - 1, nx - 2), **f64)
            self.qz = torch.empty((nz - 1, ny - 2, nx - 2), **f64)
            self.dTdt = torch.empty((nz - 2, ny - 2, nx - 2), **f64)
            self._tmp = torch.empty((nz - 2, ny - 2, nx - 2), **f64)
        self.steps_done = 0

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
    def step(self, n: int = 1) -> None:
        """Advance n time steps (asynchronous on a GPU)."""
        for _ in range(int(n)):
            if self.cfg.variant == "perf":
                ops.stencil3d_step(self.T2, self.T, self.iCp, self.coef, tuning=self.cfg.tuning)
                self.T, self.T2 = self.T2, self.T
                update_halo_(self.T)
            else:
                self._step_ap()
            self.steps_done += 1

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
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

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
        if g.me == 0 and not cfg.quiet:
            print(metrics.reference_line(nt, wtime, teff), flush=True)
        return res

    def gather_interior(self, root: int = 0):
        """The halo-stripped fields of all ranks assembled on root (None elsewhere)."""
        return gather_(self.field[1:-1, 1:-1, 1:-1].contiguous(), None, root)

    def close(self) -> None:
        self.synchronize()
        if self._owns_grid:
            gg.finalize_global_grid()
            self._owns_grid = False
