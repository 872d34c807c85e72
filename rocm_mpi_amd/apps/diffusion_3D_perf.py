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
    ap.add_argument("--variant", choices=["perf", "ap"], default="perf")
    ap.add_argument("--device", default=None, help="cpu, cuda, cuda:N (default: one GPU per rank)")
    ap.add_argument("--transport", default=os.environ.get("RMA_TRANSPORT", "auto"),
                    choices=["auto", "rccl", "ipc", "staged", "gloo", "self"])
    ap.add_argument("--vis", action="store_true",
                    help="write the gathered mid-z plane as a heatmap PNG under output/")
    ap.add_argument("--json", action="store_true", help="print the run record as JSON (rank 0)")
    ap.add_argument("--check-every", type=int, default=0, help="NaN/Inf guard period")
    return ap


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
                            device=a.device, check_every=a.check_every)
    model = Diffusion3D(cfg)
    res = model.run()
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
