"""Randomised ``update_halo_`` on device fields through the native ``HaloExchanger``
(rank threads over the device loopback transport on cuda:0) against the NumPy
oracles of ``fuzz_halo_cases``: the plane rule on cell-unique data (tier A, every cell
and guard element of every rank, bitwise) and the cut of one global array (tier B).
The 2-D cases with x AND y neighbours run on the merged plan and again on the
per-dimension plan (RMA_DIAG=no_halo_merged); the first single-rank periodic cases
also run over transport="rccl", their planes sent to the rank itself through RCCL
and copied locally. Seeds run in groups of 8 to 12; a failure names its seed.

Measured on one MI355X: the slowest loopback group (seeds 0-11, the first to touch
the device) takes 1.0 s, every other group under 0.3 s; an RCCL test (two
communicators) 1.2 to 1.4 s, 4.8 s for the one that loads RCCL first; the file 17 s.
"""
import pytest

import fuzz_halo_cases as H
from fuzz_halo_cases import GROUP, N_GPU, N_GPU_TRUTH, N_RCCL

pytestmark = pytest.mark.gpu

MERGED = [s for s in range(N_GPU) if H.merged_eligible(H.halo_case(s))]
SINGLE = [s for s in range(N_GPU) if H.nranks(H.halo_case(s)) == 1][:N_RCCL]


def _groups(seeds, k):
    seeds = list(seeds)
    return [seeds[i:i + k] for i in range(0, len(seeds), k)]


def _ids(g):
    return f"{g[0]}-{g[-1]}"


def _each(seeds, check, *args, **kw):
    for seed in seeds:
        try:
            check(seed, *args, **kw)
        except Exception as e:  # noqa: BLE001
            raise AssertionError(f"halo_case({seed}): {e}") from e


@pytest.mark.parametrize("seeds", _groups(range(N_GPU), GROUP), ids=_ids)
def test_random_exchanges_match_the_plane_rule(seeds, monkeypatch):
    monkeypatch.setenv("RMA_DIAG", "")  # the merged plan wherever it is eligible
    _each(seeds, H.spec_check, "cuda:0")


@pytest.mark.parametrize("seeds", _groups(MERGED, 8), ids=_ids)
def test_merged_eligible_cases_on_the_per_dimension_plan(seeds, monkeypatch):
    monkeypatch.setenv("RMA_DIAG", "no_halo_merged")
    _each(seeds, H.spec_check, "cuda:0")


@pytest.mark.parametrize("seeds", _groups(range(N_GPU_TRUTH), 8), ids=_ids)
def test_random_exchanges_restore_the_global_cut(seeds, monkeypatch):
    monkeypatch.setenv("RMA_DIAG", "")
    _each(seeds, H.truth_check, "cuda:0")


@pytest.mark.parametrize("seed", SINGLE)
def test_single_rank_periodic_cases_over_rccl(seed, monkeypatch):
    """transport="rccl" on one rank: the planes sent to the rank itself through RCCL
    send/recv, then copied locally, both against the oracle's field."""
    monkeypatch.setenv("RMA_DIAG", "")
    assert len(SINGLE) == N_RCCL
    for via in (True, False):
        _each([seed], H.spec_check, "cuda:0", single=True,
              grid_kw={"transport": "rccl", "self_via_transport": via})
