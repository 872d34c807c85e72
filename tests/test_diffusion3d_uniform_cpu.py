"""Diffusion3D's uniform-1/Cp verdict on CPU: the scan at construction, the
rescan after in-place edits (torch's version counter) and after writes torch
does not see (``rescan_factor``), the switches that disable it; the field stays
bitwise the NumPy golden model's (tests/golden3d.py) with the edited 1/Cp."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import golden3d
from rocm_mpi_amd import ops
from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig

N = (34, 13, 12)  # nx, ny, nz
SEED = 1234


def model(temporal, device="cpu", **kw):
    return Diffusion3D(Diffusion3DConfig(nx=N[0], ny=N[1], nz=N[2], nt=10, init="random",
                                         seed=SEED, quiet=True, temporal=temporal, device=device,
                                         **kw))


class Golden:
    """golden3d.step3 on one rank's array with an editable 1/Cp."""

    def __init__(self):
        nx, ny, nz = N
        geom = SimpleNamespace(gx0=0, gy0=0, gz0=0, nxg=nx, nyg=ny, nzg=nz, periodx=0, periody=0,
                               periodz=0)
        self.T = golden3d.random_field3(nx, ny, nz, geom, SEED)
        self.iCp = np.full_like(self.T, 1.0)
        dx, dy, dz, self.dt = golden3d.params3(nx, ny, nz)
        self.k = (-1.0, 1.0 / dx, 1.0 / dy, 1.0 / dz)

    def step(self, n=1):
        for _ in range(n):
            self.T = golden3d.step3(self.T, self.iCp, *self.k, self.dt)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(m, G):
    return np.array_equal(bits(m.field.cpu().numpy()), bits(G.T))


@pytest.mark.parametrize("temporal", [1, 2])
def test_verdict_follows_in_place_edits_and_the_field_stays_golden(temporal):
    m, G = model(temporal), Golden()
    assert m.uniform_factor is True and m.uniform_value == 1.0
    assert m.uniform_passes() == ()  # the CPU twins read the array
    assert same(m, G)
    m.step(3)
    G.step(3)
    assert m.uniform_factor is True and same(m, G)
    m.iCp[5, 6, 7] = 2.0
    G.iCp[5, 6, 7] = 2.0
    m.step()
    G.step()
    assert m.uniform_factor is False and same(m, G)
    m.step(4)  # two-step passes with the edited cell
    G.step(4)
    assert m.uniform_factor is False and same(m, G)
    m.iCp[5, 6, 7] = 1.0
    G.iCp[5, 6, 7] = 1.0
    m.step()
    G.step()
    assert m.uniform_factor is True and same(m, G)
    m.step(3)
    G.step(3)
    assert same(m, G) and m.steps_done == 12
    m.close()


@pytest.mark.parametrize("temporal", [1, 2])
def test_rescan_factor_picks_up_writes_torch_does_not_see(temporal):
    m, G = model(temporal), Golden()
    ops.fill_(m.iCp, 0.5)
    G.iCp[:] = 0.5
    assert m.rescan_factor() is True
    assert m.uniform_factor is True and m.uniform_value == 0.5
    m.step(3)
    G.step(3)
    assert same(m, G)
    v = m.iCp._version
    m.iCp.numpy()[1, 2, 3] = 3.0  # through the buffer: no version bump
    G.iCp[1, 2, 3] = 3.0
    assert m.iCp._version == v and m.uniform_factor is True  # the stale verdict
    assert m.rescan_factor() is False and m.uniform_factor is False
    m.step(3)
    G.step(3)
    assert same(m, G)
    m.iCp.numpy()[1, 2, 3] = 0.5
    assert m.rescan_factor() is True
    m.close()


def test_switches(monkeypatch):
    m = model(1, uniform_factor=False)
    assert m.uniform_factor is False and m.rescan_factor() is False
    m.step(2)
    assert m.uniform_factor is False
    m.close()
    monkeypatch.setenv("RMA_DIAG", "uniform_factor=off")
    m = model(2)
    assert m.uniform_factor is False and m.uniform_passes() == ()
    m.close()
    monkeypatch.setenv("RMA_DIAG", "uniform_factor=on")
    with pytest.raises(ValueError, match="uniform_factor=on"):
        model(1)
    monkeypatch.delenv("RMA_DIAG")
    from rocm_mpi_amd.parallel import implicit_grid as gg

    assert not gg.grid_is_initialized()  # refused before the grid was created
    assert Diffusion3DConfig().uniform_factor is True
    m = model(1, variant="ap")  # ap reads the array too; the verdict is still reported
    m.iCp[1, 1, 1] = 4.0
    m.step()
    assert m.uniform_factor is False
    m.close()


def test_app_prints_the_factor_line_on_cpu(tmp_path):
    import json
    import os
    import subprocess
    import sys

    from helpers import ROOT

    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "rocm_mpi_amd.apps.diffusion_3D_perf", "--device",
                        "cpu", "--nx", "16", "--ny", "16", "--nz", "16", "--nt", "12", "--json"],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    fac = [ln for ln in lines if ln.startswith("[factor]")]
    assert len(fac) == 1 and "24 B per cell and pass" in fac[0], fac
    rec = json.loads([ln for ln in lines if ln.startswith("{")][-1])
    assert rec["extra"]["uniform_factor"] is True and rec["extra"]["uniform_passes"] == []
