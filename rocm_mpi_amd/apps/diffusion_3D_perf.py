"""3D heat diffusion with one fused kernel per step (ImplicitGlobalGrid's
flagship example in the naming scheme of the reference's 2D scripts).

    python -m rocm_mpi_amd.apps.diffusion_3D_perf [--help]
    python -m rocm_mpi_amd.launch -n 8 -m rocm_mpi_amd.apps.diffusion_3D_perf --dims 2,2,2
"""
from __future__ import annotations

import argparse
import os
import sys


def _triple(s: str) -> tuple:
    v = tuple(int(x) for x in s.split(","))
    if len(v) != 3:
        raise argparse.ArgumentTypeError(f"expected three integers a,b,c, got {s!r}")
    return v


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(
        prog="diffusion_3D_perf",
        description="3D heat diffusion (explicit Euler, 7-point stencil, fp64) on MI355X")
    ap.add_argument("--nx", type=int, default=256, help="local grid points in x (halo incl.)")
    ap.add_argument("--ny", type=int, default=256)
    ap.add_argument("--nz", type=int, default=256)
    ap.add_argument("--nt", type=int, default=1000, help="time steps (first 10 untimed)")
    ap.add_argument("--dims", type=_triple, default=(0, 0, 0), help="process grid a,b,c")
    ap.add_argument("--periods", type=_triple, default=(0, 0, 0))
    ap.add_argument("--init", choices=["gaussian", "random"], default="gaussian")
    ap.add_argument("--variant", choices=["perf", "ap", "perf_hide"], default="perf",
                    help="perf_hide: boundary frame and halo exchange on a high-priority stream "
                         "next to the interior update (bitwise the perf field)")
    ap.add_argument("--b-width", dest="b_width", type=_triple, default=(16, 2, 2),
                    help="perf_hide boundary width a,b,c in cells from the array edge")
    ap.add_argument("--xface", type=int, default=0,
                    help="perf_hide: widest frame box on the kernels' x-face path, one- and "
                         "two-step passes (0: off, -1: the x boundary width)")
    ap.add_argument("--fused", action="store_true",
                    help="perf_hide: frame-first single-launch passes (the frame boxes dispatch "
                         "first in one launch with the interior; a device flag starts the "
                         "exchange); bitwise the same field")
    ap.add_argument("--device", default=None, help="cpu, cuda, cuda:N (default: one GPU per rank)")
    ap.add_argument("--transport", default=os.environ.get("RMA_TRANSPORT", "auto"),
                    choices=["auto", "rccl", "ipc", "staged", "gloo", "self"])
    ap.add_argument("--vis", action="store_true",
                    help="write the gathered mid-z plane as a heatmap PNG under output/")
    ap.add_argument("--json", action="store_true", help="print the run record as JSON (rank 0)")
    ap.add_argument("--check-every", type=int, default=0, help="NaN/Inf guard period")
    ap.add_argument("--temporal", type=int, default=1, choices=[1, 2],
                    help="steps per kernel pass (2: temporal blocking, grid overlap 4, perf only)")
    ap.add_argument("--no-uniform-factor", dest="uniform_factor", action="store_false",
                    help="read the 1/Cp array in every pass also where it holds one value")
    ap.add_argument("--fast-math", dest="fast_math", action="store_true",
                    help="every pass in the fast7 arithmetic (7-point sum, one folded per-cell "
                         "factor; rounding-level difference from canonical, perf only)")
    ap.add_argument("--native", action="store_true",
                    help="perf / perf_hide on a GPU: issue the time loop from C++ "
                         "(_C.Executor3D) instead of pass by pass from Python; the same field")
    return ap


def loop_line(model) -> str:
    """Who issues the passes of step(n)."""
    if model.native_loop:
        return "[loop] native (the C++ time loop, csrc/runtime/executor3d.cpp)"
    if not model.cfg.native:
        return "[loop] python (every pass issued from Python; --native: from C++)"
    why = ("variant ap has no kernel passes" if model.cfg.variant == "ap" else
           "CPU tensors" if model.device.type != "cuda" else
           f"transport {model.g.transport} has no native halo engine")
    return f"[loop] python (--native does not apply: {why})"


def factor_line(model) -> str:
    """Which 1/Cp path the kernel passes run and its model traffic (rank 0's
    verdict: the paths are bitwise equal, so ranks need not agree)."""
    depths = model.uniform_passes()
    if depths:
        return (f"[factor] 1/Cp is one value ({model.uniform_value!r}): uniform-factor kernels in "
                f"the {'/'.join(str(k) for k in depths)}-step passes, 16 B per cell and pass "
                f"(read T, write T2; the array is not read)")
    if model.uniform_factor:
        why = "1/Cp is one value, but only the perf passes on a GPU have the uniform variant"
    elif not model.cfg.uniform_factor:
        why = "--no-uniform-factor"
    else:
        why = "1/Cp varies, or RMA_DIAG=uniform_factor=off"
    return (f"[factor] 1/Cp field path, 24 B per cell and pass (read T, read 1/Cp, write T2): "
            f"{why}")


def face_path_text(model, k: int, frame) -> str:
    """Which frame boxes of a k-step pass run the x-face path, as the launcher
    decides it (ops.stencil3d_dispatch): their widths and lanes per row, and for
    the x slabs that stay on the strip march, why."""
    from .. import ops
    from .._native import has_native

    xf = model.frame_xface(k)
    if not xf:
        return "no box on the x-face path (--xface 0)"
    if not has_native():
        return f"x-face width {xf} (the native extension decides per box; it is not built)"
    cfg = model.cfg
    plan = ops.stencil3d_dispatch(k, (cfg.nz, cfg.ny, cfg.nx), frame,
                                  ops.Stencil3DTuning(xface=xf))
    faced = [(b[1] - b[0], lanes) for b, path, lanes in plan if path == "xface"]
    if faced:
        boxes = ", ".join(f"width {w} on {lanes} lanes per row" for w, lanes in sorted(set(faced)))
        text = f"x-face path for {len(faced)} of {len(frame)} frame boxes ({boxes}; width <= {xf})"
    else:
        text = f"no box on the x-face path (width <= {xf})"
    cap = ops.XFACE_MAX - 2 * (k - 1)  # a k-step segment needs width + 2(k-1) <= 32 columns
    # the x slabs are the frame boxes that do not span the owned x range
    own = model.owned_box(k)
    kept = [b[1] - b[0] for b, path, _ in plan
            if path != "xface" and (b[0], b[1]) != (own[0], own[1])]
    if kept:
        why = [f"width {w} > " + (f"--xface {xf}" if w > xf else
                                  f"{cap}, the widest box of the {k}-step face path")
               for w in sorted(set(kept))]
        text += f"; x slabs on the march: {', '.join(why)}"
    return text


def hide_line(model) -> str:
    """The frame / interior split of the perf_hide passes (rank 0's boxes)."""
    cfg = model.cfg
    parts = []
    for k in sorted({1, cfg.temporal}, reverse=True):
        frame, inner = model.hide_boxes(k)
        own = model.owned_box(k)
        vol = lambda b: (b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4])  # noqa: E731
        share = sum(vol(b) for b in frame) / max(1, vol(own))
        splits = bool(frame) and inner is not None and model.device.type == "cuda"
        # a fused launch has no box on the x-face path (the face kernels do not signal)
        path = ("no box on the x-face path (fused launch)" if splits and cfg.fused
                else face_path_text(model, k, frame))
        overlap = ("fused: one launch, frame blocks first, the exchange behind their flag"
                   if splits and cfg.fused else
                   "split: frame + exchange overlap the interior, two launches" if splits else
                   "boxes in sequence: frame, exchange, interior" if frame and inner is not None
                   else "no overlap: one launch, then the exchange")
        parts.append(f"{k}-step passes: frame {frame}, inner {inner}, {100.0 * share:.1f} % of "
                     f"the cells in the frame, {path}, {overlap}")
    return f"[hide] b_width {tuple(cfg.b_width)}; " + "; ".join(parts)


def grid_line(model) -> str | None:
    """The loud note when the solved global grid is not the reference's
    (overlap 2K of K-step passes on a multi-rank grid); None when equal."""
    from ..parallel import geometry as geo

    g, cfg = model.g, model.cfg
    run = tuple(g.nxyz_g)
    ref = tuple(geo.n_global(n, g.dims[d], 2, int(g.periods[d]))
                for d, n in enumerate((cfg.nx, cfg.ny, cfg.nz)))
    if run == ref:
        return None
    dx_ref, dy_ref, dz_ref = cfg.lx / ref[0], cfg.ly / ref[1], cfg.lz / ref[2]
    dt_ref = min(dx_ref * dx_ref, dy_ref * dy_ref, dz_ref * dz_ref) * cfg.Cp0 / cfg.lam / 6.1
    return (f"[grid] global grid {run[0]}x{run[1]}x{run[2]} (overlap {g.overlaps[0]} for "
            f"{cfg.temporal}-step passes), dx = {model.dx:.6e}, dt = {model.dt:.6e}; the "
            f"reference's overlap 2 gives {ref[0]}x{ref[1]}x{ref[2]}, dx = {dx_ref:.6e}, dt = "
            f"{dt_ref:.6e} (run with --temporal 1 to solve the reference's problem)")


def plan_line(model, steps: int) -> str:
    """What the timed loop runs (printed next to the reference's T_eff line)."""
    import collections

    plan = model.plan(steps)
    passes = ", ".join(f"{n} x {k}" for k, n in sorted(collections.Counter(plan).items(),
                                                         reverse=True))
    arith = ("fast-math (fast7: 7-point sum, folded factor; rounding-level vs canonical)"
             if model.cfg.fast_math else "canonical (bitwise = one-step updates)")
    return (f"[plan] {steps} timed steps in passes of {passes} step(s); {arith}; max "
            f"{model.cfg.temporal} steps per pass (--temporal)")


def visualise(model, outdir: str = "output") -> dict | None:
    """Gather the de-haloed field and write its middle z plane on rank 0."""
    from ..utils import vis

    T_v = model.gather_interior()
    if T_v is None:
        return None
    g = model.g
    path = os.path.join(outdir, f"Temp_3D_{g.nprocs}_{g.nxyz_g[0]}_{g.nxyz_g[1]}_"
                                f"{g.nxyz_g[2]}.png")
    return vis.heatmap_png(T_v[T_v.shape[0] // 2], path)


def main(argv=None) -> int:
    from ..models import Diffusion3D, Diffusion3DConfig

    a = build_parser().parse_args(argv)
    cfg = Diffusion3DConfig(variant=a.variant, nx=a.nx, ny=a.ny, nz=a.nz, nt=a.nt, init=a.init,
                            dims=a.dims, periods=a.periods, transport=a.transport,
                            device=a.device, check_every=a.check_every, temporal=a.temporal,
                            uniform_factor=a.uniform_factor, fast_math=a.fast_math,
                            b_width=a.b_width, xface=None if a.xface < 0 else a.xface,
                            native=a.native, fused=a.fused)
    model = Diffusion3D(cfg)
    if model.g.me == 0:
        print(loop_line(model), flush=True)
        print(factor_line(model), flush=True)
        if a.variant == "perf_hide":
            print(hide_line(model), flush=True)
    gline = grid_line(model) if a.temporal > 1 else None
    if gline and model.g.me == 0:
        print(gline, flush=True)
    res = model.run()
    if (a.temporal > 1 or a.fast_math) and model.g.me == 0:
        print(plan_line(model, res.timed_steps), flush=True)
    if a.temporal > 1:
        res.extra["temporal"] = cfg.temporal
        res.extra["overlaps"] = list(model.g.overlaps)
    res.extra["uniform_factor"] = model.uniform_factor
    res.extra["uniform_passes"] = list(model.uniform_passes())
    if a.vis:
        info = visualise(model)
        if info is not None:
            res.extra["vis"] = info
            print(f"maximum(T_v) = {info['max']}", flush=True)
    if a.json and model.g.me == 0:
        print(res.to_json(), flush=True)
    model.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
