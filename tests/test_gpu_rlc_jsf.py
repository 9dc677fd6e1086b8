"""GPU parity of the signed-digit (Joint Sparse Form) ladder of the TPKE batch check's randomisation
(rlc_common.hpp g1_mul_ab_jsf, lcb_set_rlc_signed_digits; the recoding itself: tests/test_rlc_jsf.py).

A wave of k_tpke_rlc_points whose lanes hold one exponent walks the exponent's signed digits; every other wave keeps
the per-lane binary ladder.  The batches of tests/test_gpu_rlc_positions.py and tests/test_gpu_rlc_exponents.py never
fill a wave with one bin, so the shapes here are the smallest that do:

  n4x256   N = 4, 256 ciphertexts: 16 bins of exactly 64 shares, every wave uniform;
  n4x260   N = 4, 260 ciphertexts: bins of 65 — a uniform wave, straddling waves and a short (uniform) last wave;
  n22x88   N = 22, 88 ciphertexts: bins of 22, every wave mixed (the per-lane ladder, reached through the new code).

Each shape runs six cases (all valid; one wrong share in a full-wave bin; two wrong shares in one group; an undecodable
share; the order-3 point (0, -2) as a share, whose x = 0 sends its wave to the binary ladder; a ciphertext whose W lies
outside G2), with the knob at 0 and at 1, with the key table P forced and without it.  Every run's decisions are
compared with the oracle's exact per-share result and the two knob settings with each other.  Under a fixed ChaCha20
key the stored records s_i U_i of every share are also equal between the two settings, and those of three shares per
case (four with the order-3 share) equal the oracle's multiplication by the model's exponent (tests/pyref/rlc.py).

The ciphertexts of a shape repeat a few distinct ones, and the oracle's decisions are cached per (key, ciphertext,
share), so a case costs the oracle a handful of pairings beyond the shape's first."""
import copy
import os

import numpy as np
import pytest

import oracle as o
from helpers import R, gpu_native
from pyref import rlc as M
from test_gpu_batched import Batch, off_subgroup_g2
from test_gpu_rlc_exponents import INF1, K3, SEED, g1_ab, run_tpke

pytestmark = pytest.mark.gpu

SHAPES = {"n4x256": (4, 1, 8, 256), "n4x260": (4, 1, 8, 260), "n22x88": (22, 7, 4, 88)}     # N, F, distinct cts, cts
CASES = ["valid", "one_bad", "two_bad", "undecodable", "order3", "w_outside_g2"]


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


@pytest.fixture(scope="module")
def tdev():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture
def env(nat):
    """the record hook and the fixed key; afterwards neither, and the knobs at their defaults"""
    os.environ["LCB_ALLOW_TEST_HOOKS"] = "1"
    os.environ["LCB_ALLOW_FIXED_BATCH_SEED"] = "1"
    nat.set_batch_seed(SEED)
    yield
    nat.set_batch_seed(None)
    del os.environ["LCB_ALLOW_FIXED_BATCH_SEED"]
    del os.environ["LCB_ALLOW_TEST_HOOKS"]
    nat.set_rlc_signed_digits(1)
    nat.set_rlc_pos_table_min(512)


_batches, _expect = {}, {}


def batch(shape):
    """the shape's batch: `distinct` ciphertexts repeated (every ciphertext index keeps its own set c & 3)"""
    if shape not in _batches:
        n, f, distinct, c = SHAPES[shape]
        key = (n, f, distinct)
        if key not in _batches:
            _batches[key] = Batch(b"gpu-rlc-jsf-%d" % n, n, f, distinct)
        b = _batches[key]
        bb = copy.copy(b)
        bb.c = c
        bb.cts = [b.cts[k % distinct] for k in range(c)]
        bb.good = [b.good[k % distinct] for k in range(c)]
        bb.bad = [b.bad[k % distinct] for k in range(c)]
        _batches[shape] = bb
    return _batches[shape]


def expect_of(b, ct, dec, shares):
    out = []
    for c, j, s in zip(ct, dec, shares):
        key = (b.yi[j], b.cts[c], s)
        if key not in _expect:
            _expect[key] = int(b.expect(c, j, s))
        out.append(_expect[key])
    return np.array(out, dtype=np.uint8)


def build(shape, case):
    """(batch, ct, dec, shares, special): ciphertext-major, share j of a ciphertext belongs to decryptor j; special:
    the index of the case's share whose record is compared as well (None: none)"""
    b = batch(shape)
    n = b.n
    ct = [c for c in range(b.c) for _ in range(n)]
    dec = [j for _ in range(b.c) for j in range(n)]
    shares = [b.good[c][j] for c, j in zip(ct, dec)]
    special = None
    if case == "one_bad":                        # ciphertext 8, place 0: bin 0, the first (full) wave of the N = 4 shapes
        special = 8 * n
        shares[special] = b.bad[8][0]
    elif case == "two_bad":
        for j in ((0, 2) if n == 4 else (4, 17)):
            special = 20 * n + j
            shares[special] = b.bad[20][j]
    elif case == "undecodable":
        special = 30 * n + 2
        s = bytearray(shares[special])
        while o.g1_valid(bytes(s)):
            s[0] = (s[0] + 1) & 0xFF
        shares[special] = bytes(s)
    elif case == "order3":
        special = 40 * n + 3
        assert o.g1_valid(K3) and o.g1_mul(K3, o.fr(3)) == INF1
        shares[special] = K3
    elif case == "w_outside_g2":
        q = off_subgroup_g2(b.d)
        t2 = o.g2_add(o.g2_mul(q, o.fr(R - 1)), q)
        u, v, w = b.cts[6]
        w2 = o.g2_add(w, t2)
        assert o.g2_valid(w2) and not o.g2_in_subgroup(w2)
        b = copy.copy(b)
        b.cts = list(b.cts)
        b.cts[6] = (u, v, w2)
        shares[6 * n + 1] = b.bad[6][1]
        special = 6 * n + 1
    return b, ct, dec, shares, special


@pytest.mark.parametrize("table", [False, True], ids=["no_table", "table"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_signed_digits_decisions_and_records(nat, tdev, env, shape, case, table):
    b, ct, dec, shares, special = build(shape, case)
    n = len(shares)
    expect = expect_of(b, ct, dec, shares)
    if case == "valid":
        assert expect.all()
    elif case != "order3":
        assert not expect[special]
    bins = M.tpke_bins(ct, b.c)
    picks = sorted({0, n // 2, n - 1} | ({special} if special is not None else set()))
    nat.set_rlc_pos_table_min(0 if table else 512)
    runs = []
    for knob in (0, 1):
        nat.set_rlc_signed_digits(knob)
        with nat.Context() as ctx:
            got = run_tpke(nat, tdev, ctx, b, ct, dec, shares)
            ra, rb, nonce, kind = nat.debug_rlc_records(n, ctx)
        assert (nonce, kind) == (1, 0)
        assert np.array_equal(got, expect), (knob, np.nonzero(got != expect)[0].tolist())
        for i in picks:
            if not o.g1_valid(shares[i]):
                want = INF1
            else:
                want = g1_ab(shares[i], *M.rlc_scalar(SEED, 1, bins[i], M.DOM_POS))
            assert ra[i] == want, (knob, i)
        runs.append((got, ra, rb))
    assert np.array_equal(runs[0][0], runs[1][0])
    diff = [i for i in range(n) if runs[0][1][i] != runs[1][1][i] or runs[0][2][i] != runs[1][2][i]]
    assert not diff, diff[:8]
