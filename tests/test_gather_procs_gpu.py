"""rma_gather_igg between SEPARATE processes: the reference's call site
``gather!(T_nh, T_v)`` (scripts/diffusion_2D_ap.jl:45-46) done in one call of
the C ABI. Four processes on cuda:0 (RCCL told that each rank is its own host,
as test_rccl_between_processes_sharing_the_gpu does) drive only the C ABI;
every rank fills its block with its cells' global linear indices, so the
assembled array must equal ``arange`` bitwise: any block at a wrong position
(the rank-major layout on a 2x2 grid, for one) shows.

The four cases run as four grids in ONE set of four processes (one process
start and one torch import per rank instead of four); each test then checks
its case's array."""
import numpy as np
import pytest

import mp_gather_targets as T
from helpers import run_procs

pytestmark = pytest.mark.gpu

ENV = {"RMA_TRANSPORT": "rccl", "RMA_RCCL_SHARED_GPU": "1", "RMA_COMM_TIMEOUT": "60"}


@pytest.fixture(scope="module")
def gathered(tmp_path_factory):
    out = tmp_path_factory.mktemp("gather_igg")
    err = None
    try:
        run_procs(4, "mp_gather_targets:igg_gather", str(out), list(T.CASES), env=ENV, timeout=240)
    except AssertionError as e:  # every case then reports it (cases before the failure still check)
        err = e
    return out, err


@pytest.mark.parametrize("name", list(T.CASES))
def test_gather_igg_between_processes(gathered, name):
    out, err = gathered
    path = out / f"A_global_{name}.npy"
    assert path.exists(), f"the root wrote no A_global for {name}: {err}"
    A = np.load(path)
    want = T.expected(name)
    assert A.dtype == want.dtype and A.shape == want.shape
    assert np.array_equal(A, want)
    assert err is None, err
