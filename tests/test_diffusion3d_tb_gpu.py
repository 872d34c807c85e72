"""Diffusion3D with two-step passes on one MI355X: rank threads over the device
loopback transport (width-2 halos through the native halo engine) against the
NumPy golden model of the overlap-4 global grid, bitwise, and the app."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT, run_loopback
from test_diffusion3d_tb_cpu import K, NT, bits, golden_global, spmd3

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dims,periods", [((2, 2, 2), (0, 0, 0)), ((1, 1, 2), (0, 0, 1))])
def test_rank_threads_with_two_step_passes_equal_golden_bitwise(dims, periods):
    n = (34, 13, 12)
    P = dims[0] * dims[1] * dims[2]
    Tv, nxyz_g = run_loopback(P, spmd3, K, dims, periods, n, NT, None, timeout=120)[0]
    G, ng = golden_global(dims, periods, 2 * K, n=n)
    assert list(nxyz_g) == ng
    inner = G[1:-1, 1:-1, 1:-1]
    assert Tv.shape == inner.shape
    assert np.array_equal(bits(Tv), bits(inner))
    before = golden_global(dims, periods, 2 * K, n=n, nt=NT - 1)[0][1:-1, 1:-1, 1:-1]
    assert not np.array_equal(Tv, before)


def test_app_with_two_step_passes(tmp_path):
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "rocm_mpi_amd.apps.diffusion_3D_perf", "--nx", "64",
                        "--ny", "64", "--nz", "64", "--nt", "21", "--temporal", "2", "--json"],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len([ln for ln in lines if ln.startswith("Executed 21 steps in = ")]) == 1
    plan = [ln for ln in lines if ln.startswith("[plan]")]
    assert len(plan) == 1
    assert re.fullmatch(r"\[plan\] 11 timed steps in passes of 5 x 2, 1 x 1 step\(s\); canonical "
                        r"\(bitwise = one-step updates\); max 2 steps per pass \(--temporal\)",
                        plan[0]), plan[0]
    assert not [ln for ln in lines if ln.startswith("[grid]")]  # one rank: the reference's grid
    rec = json.loads([ln for ln in lines if ln.startswith("{")][-1])
    assert rec["timed_steps"] == 11 and rec["extra"]["temporal"] == 2
    assert "cuda" in rec["device"]
