"""Diffusion3D(fast_math=True) on CPU tensors (the fast7 C++ twin): loopback rank
threads against the one-rank run of the same global grid (bitwise), independence
of the plan and of the uniform-factor switch, the distance from the canonical
field, the config refusals and the app's report."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT, run_loopback
from rocm_mpi_amd import ops
from rocm_mpi_amd.models import Diffusion3D, Diffusion3DConfig
from rocm_mpi_amd.parallel import implicit_grid as gg

N = (34, 13, 12)  # local tile nx, ny, nz
NT, SEED = 7, 1234  # odd: three two-step passes and a one-step remainder
CASES = [((2, 2, 2), (0, 0, 0)), ((1, 1, 2), (0, 0, 1))]


def spmd(rank, hub, temporal, dims, periods, n, device, nt=NT, **kw):
    """One rank of a fast-math run: (gathered interior on rank 0, global size)."""
    m = Diffusion3D(Diffusion3DConfig(nx=n[0], ny=n[1], nz=n[2], nt=nt, init="random", seed=SEED,
                                      dims=dims, periods=periods, quiet=True, temporal=temporal,
                                      device=device, fast_math=kw.pop("fast_math", True), **kw),
                    grid_kwargs=dict(loopback=(hub, rank)))
    assert m.plan(nt) == [temporal] * (nt // temporal) + [1] * (nt % temporal)
    tn = m._tuning(temporal)
    assert (tn is not None and tn.fast_math is True) == m.cfg.fast_math
    m.step(nt)
    Tv = m.gather_interior()
    out = (None if Tv is None else Tv.numpy().copy(), tuple(m.g.nxyz_g))
    m.close()
    return out


def one_rank_size(ng, periods):
    """Local size of the one-rank grid (overlap 2) with the global size ng."""
    return tuple(g + 2 if p else g for g, p in zip(ng, periods))


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def rank_threads_equal_one_rank(dims, periods, temporal, device):
    P = dims[0] * dims[1] * dims[2]
    Tv, ng = run_loopback(P, spmd, temporal, dims, periods, N, device, timeout=120)[0]
    ol = 2 * temporal
    assert list(ng) == [d * (k - ol) + (0 if p else ol) for d, k, p in zip(dims, N, periods)]
    # the same global grid on one rank, one-step passes (the field does not depend on the plan)
    one, ng1 = run_loopback(1, spmd, 1, (1, 1, 1), periods, one_rank_size(ng, periods), device,
                            timeout=120)[0]
    assert ng1 == ng and Tv.shape == one.shape  # every global cell once
    assert np.array_equal(bits(Tv), bits(one))
    before = run_loopback(1, spmd, 1, (1, 1, 1), periods, one_rank_size(ng, periods), device,
                          nt=NT - 1, timeout=120)[0][0]
    assert not np.array_equal(Tv, before)
    return Tv, ng


@pytest.mark.parametrize("temporal", [1, 2])
@pytest.mark.parametrize("dims,periods", CASES)
def test_loopback_ranks_equal_the_one_rank_run_bitwise(dims, periods, temporal):
    rank_threads_equal_one_rank(dims, periods, temporal, "cpu")


def single(device, temporal=1, nt=NT, **kw):
    return run_loopback(1, spmd, temporal, (1, 1, 1), (0, 0, 0), N, device, nt=nt, timeout=120,
                        **kw)[0][0]


def plan_and_factor_independence(device):
    a = single(device, temporal=2)  # odd nt: 2, 2, 2, 1
    b = single(device, temporal=1)
    assert np.array_equal(bits(a), bits(b))
    c = single(device, temporal=2, uniform_factor=False)
    assert np.array_equal(bits(a), bits(c))
    return a


def test_field_is_independent_of_the_plan_and_of_the_uniform_switch():
    a = plan_and_factor_independence("cpu")
    canon = single("cpu", temporal=2, fast_math=False)
    diff = np.abs(a - canon)
    assert not np.array_equal(a, canon) and float(diff.max()) < 1e-14  # another arithmetic


def test_config_refusals():
    assert Diffusion3DConfig().fast_math is False
    Diffusion3DConfig(fast_math=True, temporal=2).validate()
    with pytest.raises(ValueError, match="fast_math applies to the perf variant"):
        Diffusion3DConfig(variant="ap", fast_math=True).validate()
    # fast7_ok is false (lam = inf: infinite folded constants): refused at construction
    cfg = Diffusion3DConfig(nx=8, ny=8, nz=8, quiet=True, device="cpu", fast_math=True,
                            lam=float("inf"))
    with pytest.raises(ValueError, match="fast7"):
        Diffusion3D(cfg)
    assert not gg.grid_is_initialized()  # the grid the model created is gone again
    cfg.fast_math = False
    m = Diffusion3D(cfg)  # the canonical model does not mind
    assert not ops.fast7_ok(m.coef)
    m.close()


def run_app(tmp_path, *args):
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "rocm_mpi_amd.apps.diffusion_3D_perf", "--nx", "16",
                        "--ny", "16", "--nz", "16", "--nt", "13", "--json", *args],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    rec = json.loads([ln for ln in lines if ln.startswith("{")][-1])
    return [ln for ln in lines if ln.startswith("[plan]")], rec


def test_app_reports_the_arithmetic_on_cpu(tmp_path):
    plan, rec = run_app(tmp_path, "--device", "cpu", "--fast-math", "--temporal", "2")
    assert rec["extra"]["fast_math"] is True and rec["extra"]["temporal"] == 2
    assert len(plan) == 1 and "3 timed steps in passes of 1 x 2, 1 x 1 step(s); fast-math (fast7" \
        in plan[0], plan
    plan, rec = run_app(tmp_path, "--device", "cpu")
    assert rec["extra"]["fast_math"] is False and plan == []
