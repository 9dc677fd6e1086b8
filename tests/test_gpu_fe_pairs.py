"""GPU parity of the level-1 pair stage of the TPKE batched check (lcb_set_fe_pair_min; k_tpke.hip "level-1 pair
stage"): one final exponentiation per pair of level-1 groups, a second pass over one member of each failed pair, the
other member's value as the quotient gamma_pair * conj(gamma_first).

10 decryptors (F = 3), 7 ciphertexts, 70 shares: seven level-1 groups, so three pairs and one solo entry.  The stage is
forced with set_fe_pair_min(2).  Every case runs with set_coop_max(0) (the one-lane final-exponentiation kernel in
both passes) and with the default (the nine-lane kernel); every decision must equal the oracle's per-share decision and
the decisions of the same call with the stage off, and the counters must show that the stage ran.  The level-1 list is
built with atomic appends, so the tests do not assume which groups share a pair: the number of failed pairs is checked
against the bounds every pairing of the failing groups satisfies (they are tight: each is reached by some pairing), and
pass 2 must have run exactly one exponentiation per failed pair and one per job that holds an exact single.  The cases
in which every group fails do not depend on the pairing: every pair fails, so the second member of every pair is
searched (one error, two errors) or split into singles (three errors) from its quotient.  The suspect-key case puts
exact singles (desc.w == 1) beside randomized groups, the jobs that never form a product."""
import copy
import os

import numpy as np
import pytest

import oracle as o
from helpers import R
from test_gpu_batched import Batch, off_subgroup_g2, run_dev

pytestmark = pytest.mark.gpu
N, F, C = 10, 3, 7


@pytest.fixture(scope="module")
def nat():
    from helpers import gpu_native
    return gpu_native()


@pytest.fixture(scope="module")
def tdev():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def batch():
    return Batch(b"gpu-fe-pairs", N, F, C)


@pytest.fixture(params=["one_lane", "default"])
def fe_kernel(nat, request):
    """both final-exponentiation kernels under the pair stage; the settings are restored afterwards"""
    if request.param == "one_lane":
        nat.set_coop_max(0)
    yield request.param
    nat.set_coop_max(32768)
    nat.set_coop_miller_max(65536)
    nat.set_fe_pair_min(None)


CT = np.repeat(np.arange(C, dtype=np.uint32), N)
DEC = np.tile(np.arange(N, dtype=np.uint32), C)


def check(nat, tdev, b, bad, failing_groups, entries=C):
    """bad: the (ciphertext, position) pairs whose share is replaced by a wrong point; failing_groups: the randomized
    groups whose own check fails; entries: the level-1 entries (C groups unless a census splits suspect keys out).
    Returns (pairs failed, jobs holding an exact single)"""
    shares = [(b.bad if (int(c), int(j)) in bad else b.good)[c][j] for c, j in zip(CT, DEC)]
    expect = np.array([b.expect(int(c), int(j), s) for c, j, s in zip(CT, DEC, shares)], dtype=np.uint8)
    try:
        nat.set_fe_pair_min(2)
        got = run_dev(nat, tdev, b, CT, DEC, shares)
        levels, _ = nat.tpke_batched_stats()
        formed, failed, pass1, pass2 = nat.tpke_fe_pair_stats()
        nat.set_fe_pair_min(0)
        off = run_dev(nat, tdev, b, CT, DEC, shares)
        levels_off, _ = nat.tpke_batched_stats()
        stats_off = nat.tpke_fe_pair_stats()
    finally:
        nat.set_fe_pair_min(None)
    assert np.array_equal(got, expect), (got.tolist(), expect.tolist())
    assert np.array_equal(got, off)
    assert levels == levels_off and levels[0] == entries     # levels count groups, not exponentiations
    assert stats_off == [0, 0, 0, 0]
    assert pass1 == (entries + 1) // 2                       # one slot per two entries
    singles = pass1 - formed - entries % 2                   # jobs with an exact single: no product, both passes
    assert pass2 == failed + singles                         # one more exponentiation per failed pair and such job
    if entries == C:
        assert formed == 3 and singles == 0                  # three products and the solo entry
    nb = len(failing_groups)
    # any pairing of nb failing groups among `formed` pairs, the others alone
    assert max(0, nb - (entries - 2 * formed) + 1) // 2 <= failed <= min(formed, nb), (failed, nb, formed)
    return failed, singles


CASES = {
    "all_valid": [],
    "first_member": [(0, 4)],
    "second_member": [(1, 7)],                     # the one-error search runs on the quotient
    "both_members": [(2, 0), (3, 9)],
    "two_in_second": [(3, 2), (3, 6)],             # the two-error search runs on the quotient
    "three_in_second": [(5, 1), (5, 4), (5, 8)],   # singles
    "solo_group": [(6, 3)],
    "every_group_one": [(c, (3 * c) % N) for c in range(C)],        # every second member: the one-error search
    "every_group_two": [(c, (3 * c + d) % N) for c in range(C) for d in (0, 4)],      # ... the two-error search
    "every_group_three": [(c, (3 * c + d) % N) for c in range(C) for d in (0, 4, 5)],   # ... singles
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fe_pairs_cases(nat, tdev, batch, fe_kernel, case):
    bad = set(CASES[case])
    failed, _ = check(nat, tdev, batch, bad, {c for c, _ in bad})
    if case == "all_valid":
        assert failed == 0
    if case.startswith("every_group"):
        assert failed == 3


@pytest.mark.parametrize("density", [0.3, 1.0])
def test_fe_pairs_corruption_density(nat, tdev, batch, fe_kernel, density):
    rng = np.random.default_rng(int(density * 100) + 7)
    bad = {(int(c), int(j)) for c, j in zip(CT, DEC) if rng.random() < density}
    check(nat, tdev, batch, bad, {c for c, _ in bad})


@pytest.mark.parametrize("which", [2, 3])
def test_fe_pairs_undecodable_ciphertext(nat, tdev, batch, fe_kernel, which):
    """a ciphertext whose W does not decode: its group checks two points at infinity (and passes), its shares are
    rejected; the other groups, whichever shares its pair, are decided as without pairing"""
    b = copy.copy(batch)
    b.cts = list(batch.cts)
    u, v, w = b.cts[which]
    b.cts[which] = (u, v, w[::-1])
    check(nat, tdev, b, {(2, 5), (3, 5)}, {2, 3} - {which})
    check(nat, tdev, b, set(), set())


@pytest.mark.parametrize("which", [4, 5])
def test_fe_pairs_w_outside_g2(nat, tdev, batch, fe_kernel, which):
    """a ciphertext whose W is outside G2: its shares get exact singles whatever its pair's exponentiation gives, the
    other groups are decided as without pairing"""
    b = copy.copy(batch)
    b.cts = list(batch.cts)
    q = off_subgroup_g2(b.d)
    t2 = o.g2_add(o.g2_mul(q, o.fr(R - 1)), q)
    u, v, w = b.cts[which]
    w2 = o.g2_add(w, t2)
    assert o.g2_valid(w2) and not o.g2_in_subgroup(w2)
    b.cts[which] = (u, v, w2)
    check(nat, tdev, b, {(4, 1), (5, 1), (5, 2)}, {4, 5} - {which})


def test_fe_pairs_fixed_and_fresh_keys(nat, tdev, batch, fe_kernel):
    """the default exponent key (getrandom) and a fixed one"""
    bad = {(0, 1), (1, 2), (4, 0), (4, 9), (6, 6)}
    check(nat, tdev, batch, bad, {0, 1, 4, 6})
    os.environ["LCB_ALLOW_FIXED_BATCH_SEED"] = "1"
    try:
        nat.set_batch_seed(bytes(range(32)))
        check(nat, tdev, batch, bad, {0, 1, 4, 6})
    finally:
        nat.set_batch_seed(None)
        del os.environ["LCB_ALLOW_FIXED_BATCH_SEED"]


def test_fe_pairs_suspect_key_singles(nat, tdev, batch, fe_kernel):
    """a Byzantine validator: decryptor 2's share is wrong in every ciphertext.  With a census (the first 17 shares,
    where both of its sampled shares fail) its key is suspect, so level 1 holds the six remaining groups and, beside
    them, its five other shares as exact singles (desc.w == 1): 11 entries.  A job with a single forms no product: one
    member is exponentiated in each pass.  One more bad share fails a randomized group."""
    bad = {(c, 2) for c in range(C)} | {(4, 7)}
    nat.set_batch_census(64)
    try:
        failed, singles = check(nat, tdev, batch, bad, {4}, entries=11)
        census = nat.batched_census()
    finally:
        nat.set_batch_census(16384)
    assert census == [17, 1, 6, 11], census
    assert singles >= 1                  # five singles among 11 entries: at most three pairs of two groups
