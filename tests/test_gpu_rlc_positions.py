"""GPU parity of the TPKE batch check's position exponents (k_batch.hip header): a share's exponent is
t[ct_idx & 3][pos], pos = its place in its level-1 group, the randomisation's lanes are sorted by that bin, and the
key side comes from the table P[bin][key].

Every case compares every decision with the oracle's exact per-share result, under the two knobs in all four
combinations (lcb_set_rlc_share_exponents x lcb_set_rlc_lane_permutation); the two combinations with position
exponents run once with the key table P forced (lcb_set_rlc_pos_table_min(0): these batches are far below the size at
which it repays itself) and once without it (the per-share table additions).  The oracle's decisions are computed
once per case and shared by the modes.  The batches hold 60-200 shares of N = 4 or 22 decryptors."""
import copy

import numpy as np
import pytest

import oracle as o
from helpers import R
from test_gpu_batched import Batch, off_subgroup_g2, run_dev

pytestmark = pytest.mark.gpu

# (per-share exponents, lane permutation, P forced)
MODES = {
    "pos_perm_table": (0, 1, True),
    "pos_perm": (0, 1, False),
    "pos_table": (0, 0, True),
    "pos": (0, 0, False),
    "share_perm": (1, 1, False),
    "share": (1, 0, False),              # the behaviour before the position exponents
}


@pytest.fixture(scope="module")
def nat():
    from helpers import gpu_native
    return gpu_native()


@pytest.fixture(scope="module")
def tdev():
    import torch
    return torch, torch.device("cuda", 0)


def set_mode(nat, name):
    share, perm, table = MODES[name]
    nat.set_rlc_share_exponents(share)
    nat.set_rlc_lane_permutation(perm)
    nat.set_rlc_pos_table_min(0 if table else 512)


@pytest.fixture(params=sorted(MODES))
def mode(nat, request):
    set_mode(nat, request.param)
    yield request.param
    set_mode(nat, "pos_perm")            # the defaults
    nat.set_fe_pair_min(None)
    nat.set_batch_census(16384)


_cases = {}


def case(name, build):
    """(batch, ct, dec, shares, expect) of a case, built once"""
    if name not in _cases:
        b, ct, dec, shares = build()
        ct = np.asarray(ct, dtype=np.uint32)
        dec = np.asarray(dec, dtype=np.uint32)
        expect = np.array([int(b.expect(int(c), int(j), s)) for c, j, s in zip(ct, dec, shares)], dtype=np.uint8)
        expect.setflags(write=False)
        _cases[name] = (b, ct, dec, shares, expect)
    return _cases[name]


def decide(nat, tdev, name, build, fused=False):
    b, ct, dec, shares, expect = case(name, build)
    got = run_dev(nat, tdev, b, ct, dec, shares, fused=fused)
    assert np.array_equal(got, expect), (np.nonzero(got != expect)[0].tolist(), got.tolist())
    return expect


def runs(b, spec, bad=()):
    """spec: (ciphertext, run length) in batch order; share k of a run belongs to decryptor k mod N.  bad: indices in
    the batch whose share is the wrong point"""
    ct = [c for c, ln in spec for _ in range(ln)]
    dec = [k % b.n for _, ln in spec for k in range(ln)]
    shares = [(b.bad if i in bad else b.good)[c][j] for i, (c, j) in enumerate(zip(ct, dec))]
    return ct, dec, shares


NEG_G = o.g1_mul(o.g1_gen(), o.fr(R - 1))


def build_cancelling():
    """one group holds (c, d, S + G) and (c, d, S - G) beside good shares: under one exponent per decryptor the two
    errors would cancel; positions never repeat in a group, so both are rejected.  15 ciphertexts of N = 4, 62 shares"""
    b = Batch(b"gpu-rlc-pos-cancel", 4, 1, 15)
    ct, dec, shares = runs(b, [(c, 4) for c in range(15)])
    s = b.good[5][1]
    at = 5 * 4 + 1
    shares[at] = o.g1_add(s, o.g1_gen())
    ct.insert(at + 1, 5)
    dec.insert(at + 1, 1)
    shares.insert(at + 1, o.g1_add(s, NEG_G))
    ct.insert(0, 7)                      # and a wrong share of ciphertext 7 ahead of the batch: a group of one
    dec.insert(0, 2)
    shares.insert(0, o.g1_add(b.good[7][2], NEG_G))
    return b, ct, dec, shares


def test_cancelling_duplicates(nat, tdev, mode):
    expect = decide(nat, tdev, "cancel", build_cancelling)
    assert expect.tolist().count(0) == 3 and expect[22] == 0 and expect[23] == 0


def build_run_lengths():
    """runs of 1, 22, 33 and 40 shares of one ciphertext (the cap of 32 splits the last two), ciphertext 1 in two
    separate runs, 129 shares (not a multiple of 64), wrong shares at a run's first place, at places 31 and 32 of a
    split run and in the one-share run"""
    b = Batch(b"gpu-rlc-pos-runs", 22, 7, 5)
    spec = [(0, 1), (1, 22), (2, 33), (3, 40), (1, 11), (4, 22)]
    first = np.cumsum([0] + [ln for _, ln in spec])
    bad = {0, int(first[1]), int(first[2]) + 31, int(first[2]) + 32, int(first[3]) + 39, int(first[4]) + 3}
    return (b,) + runs(b, spec, bad)


def test_run_lengths(nat, tdev, mode):
    expect = decide(nat, tdev, "runs", build_run_lengths)
    assert len(expect) == 129 and expect.tolist().count(0) == 6 and expect[0] == 0


def build_scattered():
    """the shares of 22 x 5 in random order: level-1 groups of one or two shares; 107 of them"""
    b, ct, dec, shares, _ = case("runs", build_run_lengths)
    rng = np.random.default_rng(5)
    p = rng.permutation(len(shares))[:107]
    return b, ct[p], dec[p], [shares[i] for i in p]


def test_scattered_order(nat, tdev, mode):
    decide(nat, tdev, "scattered", build_scattered)


def build_census():
    """50 ciphertext slots of N = 4, 200 shares; decryptor 2 is wrong everywhere (suspect after the census of the
    first 50 shares), decryptor 1 once"""
    b = Batch(b"gpu-rlc-pos-census", 4, 1, 5)
    bb = copy.copy(b)
    bb.c = 50
    bb.cts = [b.cts[c % 5] for c in range(50)]
    bb.good = [b.good[c % 5] for c in range(50)]
    bb.bad = [b.bad[c % 5] for c in range(50)]
    ct, dec, shares = runs(bb, [(c, 4) for c in range(50)], {4 * c + 2 for c in range(50)} | {4 * 30 + 1})
    return bb, ct, dec, shares


@pytest.mark.parametrize("fused", [False, True])
def test_census_prefix_and_suspect_key(nat, tdev, mode, fused):
    nat.set_batch_census(64)
    decide(nat, tdev, "census", build_census, fused=fused)
    m, suspects, groups, entries = nat.batched_census()
    assert m == 50 and suspects == 1                  # shares [0, 50) by the census, the rest behind it (i0 = 50)
    assert groups == 38 and entries > groups          # 37 ciphertexts and the split one; decryptor 2's singles


def build_small_order_key():
    """decryptor 2's key has order 3: its fixed-base table is unusable (the ladder forms its multiples), the pairing
    kills it, so its shares pass exactly when e(U, H) = 1; 16 ciphertexts of N = 4"""
    b = Batch(b"gpu-rlc-pos-order3", 4, 1, 16)
    k3 = bytearray(48)
    k3[47] |= 0x80
    k3 = bytes(k3)
    assert o.g1_valid(k3) and o.g1_mul(k3, o.fr(3)) == bytes(48)
    b.yi[2] = k3
    ct, dec, shares = runs(b, [(c, 4) for c in range(16)], {4 * 9 + 3})
    shares[2] = k3
    shares[4 + 2] = bytes(48)
    return b, ct, dec, shares


def test_small_order_key(nat, tdev, mode):
    expect = decide(nat, tdev, "order3", build_small_order_key)
    assert expect[2] == 1 and expect[6] == 1 and expect[10] == 0 and expect[39] == 0


def build_undecodable_and_w():
    """a share that does not decode, and a ciphertext whose W lies outside G2 (exact checks for its shares, one of
    them wrong); 16 ciphertexts of N = 4, one share dropped (63 shares)"""
    b = Batch(b"gpu-rlc-pos-w", 4, 1, 16)
    q = off_subgroup_g2(b.d)
    t2 = o.g2_add(o.g2_mul(q, o.fr(R - 1)), q)
    u, v, w = b.cts[6]
    w2 = o.g2_add(w, t2)
    assert o.g2_valid(w2) and not o.g2_in_subgroup(w2)
    b.cts[6] = (u, v, w2)
    ct, dec, shares = runs(b, [(c, 4) for c in range(16)], {4 * 6 + 1, 4 * 11})
    s = bytearray(shares[4 * 3 + 2])
    while o.g1_valid(bytes(s)):
        s[0] = (s[0] + 1) & 0xFF
    shares[4 * 3 + 2] = bytes(s)
    return b, ct[:-1], dec[:-1], shares[:-1]


def test_undecodable_share_and_w_outside_g2(nat, tdev, mode):
    expect = decide(nat, tdev, "w", build_undecodable_and_w)
    assert len(expect) == 63 and expect[14] == 0 and expect[25] == 0 and expect[44] == 0


def build_pairs(second):
    """validator 1 is wrong in two neighbouring ciphertexts, 0 and `second`; 16 ciphertexts of N = 4 in the order
    0, second, then the others"""
    def build():
        b = Batch(b"gpu-rlc-pos-pairs", 4, 1, 16)
        order = [0, second] + [c for c in range(1, 16) if c != second]
        ct, dec, shares = runs(b, [(c, 4) for c in order], {1, 5})
        return b, ct, dec, shares
    return build


@pytest.mark.parametrize("second", [1, 4])
def test_pair_stage_sets(nat, tdev, mode, second):
    """the pair stage forced on: groups of different sets (ciphertexts 0, 1) form a product, groups of one set
    (0, 4) keep an exponentiation each; the decisions are the oracle's both times"""
    nat.set_fe_pair_min(2)
    decide(nat, tdev, "pairs%d" % second, build_pairs(second))
    formed, failed, pass1, pass2 = nat.tpke_fe_pair_stats()
    assert pass1 == 8 and formed >= 1


def build_one_set():
    b = Batch(b"gpu-rlc-pos-oneset", 4, 1, 61)
    ct, dec, shares = runs(b, [(c, 4) for c in range(0, 61, 4)], {1, 5, 22})
    return b, ct, dec, shares


def test_pair_stage_one_set_forms_no_pair(nat, tdev, mode):
    """every ciphertext index is 0 mod 4: with position exponents no two groups may share an exponentiation"""
    nat.set_fe_pair_min(2)
    decide(nat, tdev, "oneset", build_one_set)
    formed, failed, pass1, pass2 = nat.tpke_fe_pair_stats()
    assert pass1 == 8
    if MODES[mode][0]:
        assert formed == 8                # per-share exponents: every neighbouring pair
    else:
        assert formed == 0 and failed == 0 and pass2 == 8


def build_levels(k):
    def build():
        b = Batch(b"gpu-rlc-pos-levels", 22, 7, 3)
        ct, dec, shares = runs(b, [(c, 22) for c in range(3)], set([22 + 4, 22 + 17, 22 + 9][:k]))
        return b, ct, dec, shares
    return build


@pytest.mark.parametrize("k", [2, 3])
def test_levels_unchanged(nat, tdev, mode, k):
    """two bad shares in one group: located at level 2 (one-error search, then the two-error search); three: the
    group's other shares go to singles.  The levels are those of per-share exponents in batch order"""
    decide(nat, tdev, "levels%d" % k, build_levels(k))
    levels, _ = nat.tpke_batched_stats()
    set_mode(nat, "share")
    decide(nat, tdev, "levels%d" % k, build_levels(k))
    today, _ = nat.tpke_batched_stats()
    assert levels == today
    assert levels[:3] == [3, 1, 1] and len(levels) == (3 if k == 2 else 4)
