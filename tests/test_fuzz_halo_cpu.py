"""Randomised ``update_halo_`` on CPU tensors over loopback rank threads (the Python
plane algebra of ``parallel/halo.py``) against the two NumPy oracles of
``fuzz_halo_cases``: the plane rule on unrelated, cell-unique data (tier A, every
cell and guard element of every rank, bitwise) and the cut of one global array
(tier B, unstaggered fields). Also here, without a call into the package: the
generator reaches what it claims, the tier-A oracle restores the global cut, and
the checker reports planted differences."""
import numpy as np
import pytest

import fuzz_halo_cases as H
from fuzz_halo_cases import N_CPU, N_CPU_TRUTH, N_GPU, N_RCCL

# floors of the CPU seed range; the GPU range asserts them scaled by N_GPU / N_CPU
FLOORS = {"nd1": 25, "nd2": 25, "nd3": 25, "merged": 20, "periodic2": 15, "periodic3": 15,
          "self": 15, "narrow_hw": 15, "big_sets": 40, "big_cases": N_CPU // 4, "mixed_sets": 30,
          "wide": 30, "not_wide": 30, "no_halo": 15, "partial_mask": 20, "dtype": 10}


def _counts(n):
    cases = [H.halo_case(s) for s in range(n)]
    cv = H.coverage(cases)
    got = {k: cv[k] for k in FLOORS if k in cv and k != "dtype"}
    got.update({f"nd{k}": v for k, v in cv["nd"].items()})
    got["dtype"] = min(cv["dtype"].values())
    got["big_cases"] = sum(any(H.max_phase_copies(c, fs) > H.COPY_BATCH for fs in c.sets)
                           for c in cases)
    return cases, cv, got


def _assert_valid(c):
    """What the generator promises of every case (nothing is filtered at run time)."""
    P = H.nranks(c)
    assert c.dims in H.DIMS_POOL and 1 <= c.nd <= 3 and P <= 8
    assert P > 1 or any(c.periods)
    for d in range(3):
        if d >= c.nd:
            assert (c.n[d], c.dims[d], c.periods[d]) == (1, 1, 0)
            continue
        assert c.hw[d] in H.HW_POOL and c.ol[d] >= 2 * c.hw[d] and c.n[d] >= c.ol[d] + c.hw[d] + 1
    assert (c.halowidths is not None) == any(c.hw[d] != c.ol[d] // 2 for d in range(c.nd))
    assert c.mask and set(c.mask) <= {0, 1, 2}
    assert 1 <= len(c.sets) <= 3 and (len(c.sets) < 3 or c.sets[2] is c.sets[0])
    for fs in c.sets:
        assert 1 <= len(fs) <= 6
        for f in fs:
            assert int(np.prod(f.shape)) <= H.MAX_CELLS and f.odd in (0, 1)
            assert all(s in (-1, 0, 1) for s in f.stagger) and f.dtype in H.DTYPES
            assert any(H.field_has_halo(c, f, d) for d in range(c.nd))
        assert any(H.field_has_halo(c, f, d) for f in fs for d in c.mask if H.active(c, d))


def test_the_cpu_seed_range_reaches_what_it_claims():
    cases, cv, got = _counts(N_CPU)
    for c in cases:
        _assert_valid(c)
    assert vars(H.halo_case(7)) == vars(H.halo_case(7))  # a seed replays its case
    short = {k: (got[k], FLOORS[k]) for k in FLOORS if got[k] < FLOORS[k]}
    assert not short, short


def test_the_gpu_seed_range_reaches_what_it_claims():
    cases, cv, got = _counts(N_GPU)
    short = {k: (got[k], FLOORS[k] * N_GPU // N_CPU) for k in FLOORS
             if got[k] < FLOORS[k] * N_GPU // N_CPU}
    assert not short, short
    assert len(cv["single_periodic"]) >= N_RCCL
    # the single-rank seeds cover the merged plan, 3-D fields and a narrow halowidth
    first = [H.halo_case(s) for s in cv["single_periodic"][:N_RCCL]]
    assert any(H.merged_eligible(c) for c in first) and {c.nd for c in first} >= {2, 3}


@pytest.mark.parametrize("seed", range(N_CPU))
def test_random_exchanges_match_the_plane_rule(seed):
    H.spec_check(seed, None)


@pytest.mark.parametrize("seed", range(N_CPU_TRUTH))
def test_random_exchanges_restore_the_global_cut(seed):
    H.truth_check(seed, None)


@pytest.mark.parametrize("seed", range(N_CPU_TRUTH))
def test_the_plane_rule_restores_the_global_cut(seed):
    """Ties the tier-A oracle to an independent fact, without the package: applied to
    the corrupted cuts of one global array it gives the cuts back."""
    c = H.truth_case(seed)
    for xchg, fs in enumerate(c.sets):
        pairs = [H.truth_buffers(c, xchg, rank) for rank in range(H.nranks(c))]
        assert any(not np.array_equal(H._uint(b), H._uint(w))
                   for bad, good in pairs for b, w in zip(bad, good))  # something was corrupted
        got = H.spec_exchange(c, fs, [bad for bad, _ in pairs])
        H.compare_buffers(c, xchg, got, [good for _, good in pairs], what="spec_exchange")


def _mutation_case():
    # 2 x 2 ranks, two float64 fields and one complex128: small enough to read
    for seed in range(N_CPU):
        c = H.halo_case(seed)
        if c.nd == 2 and H.nranks(c) == 4 and c.sets[0][0].dtype == "float64":
            return c
    raise AssertionError("no 2-D four-rank case in the seed range")


def test_the_checker_reports_planted_differences():
    c = _mutation_case()
    want = H.expected(c, 0, "A")
    f = c.sets[0][0]
    k = int(np.prod(f.shape))

    def mutated(rank):
        got = [[b.copy() for b in bufs] for bufs in want]
        return got, H._interior(got[rank][0], f)

    H.compare_buffers(c, 0, mutated(0)[0], want)  # the unmutated copy passes
    # two interior planes (rows) swapped on rank 2
    got, A = mutated(2)
    y = c.hw[1] + 1
    A[[y, y + 1]] = A[[y + 1, y]]
    with pytest.raises(AssertionError, match=rf"seed {c.seed} exchange 0 rank 2 field 0 .*"
                                             rf"first differing cell \({y}, 0\)"):
        H.compare_buffers(c, 0, got, want)
    # the last halo corner cell of rank 1 off by one ulp
    got, A = mutated(1)
    A[-1, -1] = np.nextafter(A[-1, -1], np.inf)
    with pytest.raises(AssertionError, match=rf"rank 1 field 0 .*first differing cell "
                                             rf"\({f.shape[0] - 1}, {f.shape[1] - 1}\).*1 cells"):
        H.compare_buffers(c, 0, got, want)
    # a guard element changed, in front of and behind the field of rank 3
    for e, name in ((H.GUARD + f.odd - 1, r"-1 \(front\)"), (H.GUARD + f.odd + k, r"\+0 \(back\)")):
        got, _ = mutated(3)
        got[3][0][e] += 1
        with pytest.raises(AssertionError, match=rf"rank 3 field 0 .*guard element {name}"):
            H.compare_buffers(c, 0, got, want)
