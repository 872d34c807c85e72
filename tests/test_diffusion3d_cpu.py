"""Diffusion3D on CPU loopback rank threads against the NumPy golden model of the
global grid (bitwise), and the diffusion_3D_perf entry point."""
import json
import math
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import golden3d
from helpers import ROOT, run_loopback
from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig
from rocm_mpi_amd.parallel import implicit_grid as gg

NX, NY, NZ, NT, SEED = 10, 9, 8, 25, 1234


def spmd3(rank, hub, variant, dims, periods, device="cpu"):
    gg.init_global_grid(NX, NY, NZ, dimx=dims[0], dimy=dims[1], dimz=dims[2],
                        periodx=periods[0], periody=periods[1], periodz=periods[2], quiet=True,
                        loopback=(hub, rank), device=device)
    m = Diffusion3D(Diffusion3DConfig(variant=variant, nx=NX, ny=NY, nz=NZ, nt=NT, init="random",
                                      seed=SEED, dims=dims, periods=periods, quiet=True))
    m.step(NT)
    Tv = m.gather_interior()
    out = (None if Tv is None else Tv.numpy().copy(), tuple(m.g.nxyz_g))
    m.close()
    gg.finalize_global_grid()
    return out


def golden_global(dims, periods, n=(NX, NY, NZ), nt=NT, seed=SEED):
    """golden3d.run3 on the global array dims*(n-2)+2 from the random field of the
    package's global cell numbering, written in Python integers."""
    arr = [d * (k - 2) + 2 for d, k in zip(dims, n)]
    ng = [a - 2 if p else a for a, p in zip(arr, periods)]
    geom = SimpleNamespace(gx0=0, gy0=0, gz0=0, nxg=ng[0], nyg=ng[1], nzg=ng[2],
                           periodx=periods[0], periody=periods[1], periodz=periods[2])
    T0 = golden3d.random_field3(arr[0], arr[1], arr[2], geom, seed)
    return golden3d.run3(arr[0], arr[1], arr[2], nt, T0=T0, periods=periods), ng


CASES = [((2, 1, 1), (0, 0, 0)), ((1, 2, 1), (0, 0, 0)), ((1, 1, 2), (0, 0, 0)),
         ((2, 2, 2), (0, 0, 0)), ((1, 1, 2), (0, 0, 1))]


@pytest.mark.parametrize("variant", ["perf", "ap"])
@pytest.mark.parametrize("dims,periods", CASES)
def test_loopback_ranks_equal_golden_bitwise(variant, dims, periods):
    P = dims[0] * dims[1] * dims[2]
    Tv, nxyz_g = run_loopback(P, spmd3, variant, dims, periods, timeout=60)[0]
    G, ng = golden_global(dims, periods)
    assert list(nxyz_g) == ng
    assert Tv.shape == G[1:-1, 1:-1, 1:-1].shape
    assert np.array_equal(Tv.view(np.int64), np.ascontiguousarray(G[1:-1, 1:-1, 1:-1]).view(np.int64))
    assert not np.array_equal(Tv, golden_global(dims, periods, nt=NT - 1)[0][1:-1, 1:-1, 1:-1])


def test_run_reports_t_eff_with_nz_and_nan_guard():
    m = Diffusion3D(Diffusion3DConfig(nx=12, ny=11, nz=10, nt=14, device="cpu", quiet=True,
                                      check_every=3))
    res = m.run(14, warmup=4)
    assert res.timed_steps == 10 and m.steps_done == 14
    assert res.teff == pytest.approx(3 * 12 * 11 * 10 * 8 / 1e9 / (res.wtime / 10))
    m.T[2, 3, 4] = float("nan")
    with pytest.raises(FloatingPointError, match="non-finite"):
        m.run(3, warmup=0)
    m.close()


def test_app_smoke(tmp_path):
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "rocm_mpi_amd.apps.diffusion_3D_perf", "--device",
                        "cpu", "--nx", "16", "--ny", "16", "--nz", "16", "--nt", "20", "--json"],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Executed ")]
    assert len(lines) == 1
    assert re.fullmatch(r"Executed 20 steps in = \d\.\d{3}e[-+]\d{2} sec "
                        r"\(@ T_eff = \d+\.\d{2} GB/s\) ?", lines[0])
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["timed_steps"] == 10 and rec["extra"]["nz"] == 16
    assert math.isfinite(rec["teff"]) and rec["teff"] > 0
