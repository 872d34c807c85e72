"""Diffusion3D on one MI355X with the uniform-1/Cp kernel variants (on by
default): rank threads over the device loopback against the NumPy golden model
(bitwise), the in-place edit sequence of tests/test_diffusion3d_uniform_cpu.py
against a field-path model given the same edits, and the app's report."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT, run_loopback
from rocm_mpi_amd import ops
from test_diffusion3d_tb_cpu import NT, bits, golden_global, spmd3
from test_diffusion3d_uniform_cpu import model

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("temporal", [1, 2])
@pytest.mark.parametrize("dims,periods", [((2, 2, 2), (0, 0, 0)), ((1, 1, 2), (0, 0, 1))])
def test_rank_threads_on_the_uniform_path_equal_golden_bitwise(dims, periods, temporal):
    n = (34, 13, 12)
    P = dims[0] * dims[1] * dims[2]
    Tv, nxyz_g = run_loopback(P, spmd3, temporal, dims, periods, n, NT, "cuda", timeout=120)[0]
    G, ng = golden_global(dims, periods, 2 * temporal, n=n)
    assert list(nxyz_g) == ng
    inner = G[1:-1, 1:-1, 1:-1]
    assert Tv.shape == inner.shape
    assert np.array_equal(bits(Tv), bits(inner))
    before = golden_global(dims, periods, 2 * temporal, n=n, nt=NT - 1)[0][1:-1, 1:-1, 1:-1]
    assert not np.array_equal(Tv, before)


def same(a, b):
    return torch.equal(a.field.view(torch.int64), b.field.view(torch.int64))


@pytest.mark.parametrize("temporal", [1, 2])
def test_edit_sequence_equals_the_field_path_bitwise(temporal):
    m = model(temporal, device="cuda")
    f = model(temporal, device="cuda", uniform_factor=False)  # shares m's grid
    want_passes = tuple(sorted({1, temporal}))
    assert m.uniform_factor is True and m.uniform_passes() == want_passes
    assert f.uniform_factor is False and f.uniform_passes() == ()
    tn = m._tuning(temporal)
    assert tn.uniform is True and tn.uniform_value == 1.0 and f._tuning(temporal) is None

    def both(fn):
        fn(m)
        fn(f)

    both(lambda x: x.step(3))
    assert m.uniform_factor is True and same(m, f)

    def edit(x, v):
        x.iCp[5, 6, 7] = v

    both(lambda x: edit(x, 2.0))
    both(lambda x: x.step())
    assert m.uniform_factor is False and m.uniform_passes() == () and same(m, f)
    both(lambda x: x.step(4))
    assert same(m, f)
    both(lambda x: edit(x, 1.0))
    both(lambda x: x.step())
    assert m.uniform_factor is True and m.uniform_passes() == want_passes and same(m, f)
    # a raw-pointer write: torch's version counter does not move
    v = m.iCp._version
    both(lambda x: ops.fill_(x.iCp, 0.5))
    assert m.iCp._version == v
    assert m.rescan_factor() is True and m.uniform_value == 0.5
    both(lambda x: x.step(3))
    assert same(m, f)
    got, done = m.field.cpu(), m.steps_done
    m.close()  # owns the grid
    f.close()
    # and the CPU twin, which reads the array, given the same edits from the start
    c = model(temporal)
    assert c.device.type == "cpu"
    c.step(3)
    edit(c, 2.0)
    c.step(5)
    edit(c, 1.0)
    c.step()
    ops.fill_(c.iCp, 0.5)
    c.step(3)
    assert done == c.steps_done == 12
    assert torch.equal(got.view(torch.int64), c.field.view(torch.int64))
    c.close()


def run_app(tmp_path, *extra):
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "rocm_mpi_amd.apps.diffusion_3D_perf", "--nx", "64",
                        "--ny", "64", "--nz", "64", "--nt", "21", "--temporal", "2", "--json",
                        *extra], capture_output=True, text=True, timeout=300, cwd=str(tmp_path),
                       env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    fac = [ln for ln in lines if ln.startswith("[factor]")]
    assert len(fac) == 1, lines
    rec = json.loads([ln for ln in lines if ln.startswith("{")][-1])
    assert "cuda" in rec["device"]
    return fac[0], rec


def test_app_reports_the_factor_path(tmp_path):
    line, rec = run_app(tmp_path)
    assert rec["extra"]["uniform_factor"] is True and rec["extra"]["uniform_passes"] == [1, 2]
    assert "16 B per cell and pass" in line and "1.0" in line
    line, rec = run_app(tmp_path, "--no-uniform-factor")
    assert rec["extra"]["uniform_factor"] is False and rec["extra"]["uniform_passes"] == []
    assert "24 B per cell and pass" in line and "--no-uniform-factor" in line
