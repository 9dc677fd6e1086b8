"""The random exponents of the randomized batch check (k_batch.hip, k_rlc_rand.hip, rlc_common.hpp, ts_rlc.hpp,
lcb_batch.cpp) against the plain-Python model tests/pyref/rlc.py, bit for bit.

The batch check's soundness is the small-exponent test: a group check wrongly accepts with probability <= 2^-64
because share i is raised to s_i = a + b lambda, (a, b) = words 0 and 1 of a ChaCha20 block keyed by 32 fresh getrandom
bytes and indexed by (counter, domain, the call's nonce).  The decisions of a batched call do not change under almost
any defect of these exponents, so they are pinned here directly, through two test hooks:

  a. lcb_debug_rlc_scalars: the device routine that draws (a, b) equals the RFC 8439 block function;
  b. lcb_debug_rlc_records after a TPKE call: every share's stored s_i U_i and s_i Y_d equal the model's points, in all
     six modes of tests/test_gpu_rlc_positions.py (per position / per share, lanes sorted by bin or not, P table or not),
     with the nonce advancing per call;
  c. the same after a threshold-signature call: s_i PK and s_i sig_i (G2);
  d. without a fixed key the records follow no known key, and the fixed key needs its opt-in;
  e. end to end: shares forged with knowledge of the key, nonce and bins pass the batched call under exactly that key and
     nonce and are rejected under every other — what a known key buys an attacker.

Not covered: the (0, 0) -> (1, 0) rule (no key that reaches it can be found: only the model carries it,
tests/test_rlc_model.py), and any statistical property of ChaCha20 beyond equality with the RFC function.

Every test sets and restores the environment switches it needs.  The batches hold at most 90 shares (no census); the
model points of a case are computed once per (exponent kind, nonce) and shared by the modes."""
import ctypes
import functools
import os

import numpy as np
import pytest

import oracle as o
from helpers import R, gpu_native
from pyref import bls12_381 as B
from pyref import rlc as M
from test_gpu_batched import Batch, off_subgroup_g1, up
from test_gpu_batched_ts import Rounds, off_subgroup_g2
from test_gpu_rlc_positions import MODES, set_mode
from test_rlc_model import RFC_BLOCK, RFC_KEY, RFC_WORDS

pytestmark = pytest.mark.gpu

SEED = bytes(range(32))
SEED2 = bytes(32)
INF1, INF2 = bytes(48), bytes(96)


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


@pytest.fixture(scope="module")
def tdev():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture
def hooks():
    os.environ["LCB_ALLOW_TEST_HOOKS"] = "1"
    yield
    del os.environ["LCB_ALLOW_TEST_HOOKS"]


@pytest.fixture
def fixed_seed(nat):
    """LCB_ALLOW_FIXED_BATCH_SEED=1 and the key SEED; afterwards no seed and no opt-in"""
    os.environ["LCB_ALLOW_FIXED_BATCH_SEED"] = "1"
    nat.set_batch_seed(SEED)
    yield SEED
    nat.set_batch_seed(None)
    del os.environ["LCB_ALLOW_FIXED_BATCH_SEED"]


@pytest.fixture
def defaults(nat):
    set_mode(nat, "pos_perm")
    yield
    set_mode(nat, "pos_perm")


# ------------------------------------------------------------------------------------------------ model points
@functools.lru_cache(maxsize=None)
def _g1_sub(p):
    return p != INF1 and o.g1_in_subgroup(p)


@functools.lru_cache(maxsize=None)
def g1_ab(p, a, b):
    """the model's a P + b phi(P) as wire bytes: the oracle's multiplication by the exponent for a point of G1 (the
    two are equal there, tests/test_rlc_model.py), the model's own sum for any other point"""
    if _g1_sub(p):
        return o.g1_mul(p, o.fr(M.exponent(a, b) % R))
    return B.g1_to_bytes(M.g1_ab(B.g1_from_bytes(p), a, b))


def g2_ab(s, a, b):
    if s != INF2 and o.g2_in_subgroup(s):
        return o.g2_mul(s, o.fr(M.exponent(a, b) % R))
    return B.g2_to_bytes(M.g2_ab(B.g2_from_bytes(s), a, b))


# ------------------------------------------------------------------------------------------------ a. the scalars
def test_scalars_rfc_vector(nat, hooks):
    nonce = RFC_WORDS[2] | (RFC_WORDS[3] << 32)
    got = nat.debug_rlc_scalars([(RFC_KEY, nonce, RFC_WORDS[0], RFC_WORDS[1])])
    assert got == [(0xE4E7F110, 0x15593BD1)] == [(RFC_BLOCK[0], RFC_BLOCK[1])]


def test_scalars_equal_the_model(nat, hooks):
    """4096 items (16 blocks of lanes): random keys, nonces, counters and domains, and every combination of the edge
    values: the zero key, all-ones key words, counters 0, 1, 127, 128, 2^32 - 1 (the bins end at 127), domains 0, 1,
    2^32 - 1, nonces 0, 1, 2^32 (the high word alone) and 2^64 - 1"""
    rng = np.random.default_rng(8439)
    keys = [bytes(32), b"\xff" * 32, b"\xff" * 4 + bytes(28), bytes(28) + b"\xff" * 4, SEED]
    ctrs = [0, 1, 127, 128, 2 ** 32 - 1]
    doms = [0, 1, 2 ** 32 - 1]
    nonces = [0, 1, 2 ** 32, 2 ** 64 - 1]
    items = [(k, n, c, d) for k in keys for n in nonces for c in ctrs for d in doms]
    assert len(items) == 300
    while len(items) < 4096:
        items.append((rng.bytes(32), int(rng.integers(0, 2 ** 64, dtype=np.uint64)),
                      int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))))
    got = nat.debug_rlc_scalars(items)
    want = [M.rlc_scalar(*it) for it in items]
    bad = [i for i in range(len(items)) if got[i] != want[i]]
    assert not bad, (bad[:8], [(got[i], want[i]) for i in bad[:3]])


# ------------------------------------------------------------------------------------------------ b. TPKE records
SPEC = [(0, 1), (1, 4), (2, 33), (3, 40), (4, 4), (5, 4), (1, 3)]       # (ciphertext, run length): sets 0 1 2 3 0 1, 1
K3 = bytes(47) + b"\x80"                                                # (0, -2): order 3
_tpke = {}


def tpke_case():
    """N = 4 decryptors, 6 ciphertexts, 90 shares in runs of 1, 4, 33, 40, 4, 4 shares, a second run of ciphertext 1
    and a last share whose ciphertext index is out of range (it reads as ciphertext 0: a run of its own); share k of a
    run belongs to decryptor k mod 4.  Decryptor 2's key is the order-3 point: no fixed-base table, the ladder forms
    its multiples.  Shares of other kinds: wrong points at places 31 and 32 of the 33-share run (the bins wrap), an
    off-subgroup point and the point at infinity in the 40-share run, an undecodable encoding, an out-of-range
    decryptor, and K3 itself as a share of decryptor 2"""
    if not _tpke:
        b = Batch(b"gpu-rlc-exponents-tpke", 4, 1, 6)
        assert o.g1_valid(K3) and o.g1_mul(K3, o.fr(3)) == INF1
        b.yi[2] = K3
        ct = [c for c, ln in SPEC for _ in range(ln)] + [99]
        dec = [k % 4 for _, ln in SPEC for k in range(ln)] + [0]
        shares = [b.good[min(c, 5)][j] for c, j in zip(ct[:-1], dec[:-1])] + [b.good[0][0]]
        first = np.cumsum([0] + [ln for _, ln in SPEC]).tolist()
        shares[first[1] + 2] = K3
        shares[first[2] + 31] = b.bad[2][31 % 4]
        shares[first[2] + 32] = b.bad[2][32 % 4]
        shares[first[3] + 5] = off_subgroup_g1(b.d)
        shares[first[3] + 33] = INF1
        u = bytearray(shares[first[4] + 1])
        while o.g1_valid(bytes(u)):
            u[0] = (u[0] + 1) & 0xFF
        shares[first[4] + 1] = bytes(u)
        dec[first[5] + 3] = 9
        n = len(shares)
        assert n == 90
        live = [c < b.c and j < b.n and o.g1_valid(s) for c, j, s in zip(ct, dec, shares)]
        assert live.count(False) == 3
        expect = np.array([int(live[i] and b.expect(ct[i], dec[i], shares[i])) for i in range(n)], dtype=np.uint8)
        assert expect[first[1] + 2] == 1 and expect[first[2] + 31] == 0 and 20 < expect.sum() < n
        _tpke.update(b=b, ct=ct, dec=dec, shares=shares, live=live, expect=expect, first=first,
                     bins=M.tpke_bins(ct, b.c), models={})
    return _tpke


def tpke_model(pos, nonce, seed=SEED):
    """(rec_a, rec_b) of the case under `seed` and `nonce`: exponents per position (pos) or per share"""
    t = tpke_case()
    key = (pos, nonce, seed)
    if key not in t["models"]:
        ra, rb = [], []
        for i in range(len(t["shares"])):
            if not t["live"][i]:
                ra.append(INF1)
                rb.append(INF1)
                continue
            a, b = M.rlc_scalar(seed, nonce, t["bins"][i], M.DOM_POS) if pos else M.rlc_scalar(seed, nonce, i, M.DOM_SHARE)
            ra.append(INF1 if t["shares"][i] == INF1 else g1_ab(t["shares"][i], a, b))
            rb.append(g1_ab(t["b"].yi[t["dec"][i]], a, b))
        t["models"][key] = (ra, rb)
    return t["models"][key]


def run_tpke(nat, tdev, ctx, b, ct, dec, shares):
    """the fused batched call on the explicit context -> the decisions"""
    torch, dev = tdev
    sh = torch.cuda.current_stream(dev).cuda_stream
    n = len(shares)
    d_y = up(torch, dev, b"".join(b.yi))
    d_u = up(torch, dev, b"".join(c[0] for c in b.cts))
    d_w = up(torch, dev, b"".join(c[2] for c in b.cts))
    d_v = up(torch, dev, b"".join(c[1] for c in b.cts))
    d_voff = up(torch, dev, np.arange(0, 32 * (b.c + 1), 32, dtype=np.uint32))
    d_ct = up(torch, dev, np.asarray(ct, dtype=np.uint32))
    d_dec = up(torch, dev, np.asarray(dec, dtype=np.uint32))
    d_sh = up(torch, dev, b"".join(shares))
    d_acc = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    rc = nat.lib().lcb_ctx_tpke_verify_shares_batched_dev(
        ctx.ptr, d_acc.data_ptr(), n, d_y.data_ptr(), b.n, d_u.data_ptr(), d_w.data_ptr(), d_v.data_ptr(),
        d_voff.data_ptr(), b.c, d_ct.data_ptr(), d_dec.data_ptr(), d_sh.data_ptr(), sh)
    assert rc == 0, nat.last_error()
    torch.cuda.synchronize(dev)
    return d_acc.cpu().numpy()


def mismatches(got, want):
    return [i for i in range(len(want)) if got[i] != want[i]]


@pytest.fixture(params=sorted(MODES))
def mode(nat, request):
    set_mode(nat, request.param)
    yield request.param
    set_mode(nat, "pos_perm")


def test_tpke_records_equal_the_model(nat, tdev, hooks, fixed_seed, mode):
    """under the fixed key, every stored record of both calls of a fresh context equals the model's point: position
    modes draw (a, b) from (bin, domain 1), per-share modes from (index, domain 0); the 90 shares fill one wave that
    holds whole bins and one that straddles them (permuted modes), the P table is forced in two modes.  Shares the
    kernel leaves out (undecodable, an index out of range) store two points at infinity; the share at infinity stores
    infinity and its key's multiple"""
    t = tpke_case()
    pos = not MODES[mode][0]
    n = len(t["shares"])
    with nat.Context() as ctx:
        recs = []
        for nonce in (1, 2):
            got = run_tpke(nat, tdev, ctx, t["b"], t["ct"], t["dec"], t["shares"])
            ra, rb, got_nonce, kind = nat.debug_rlc_records(n, ctx)
            assert (got_nonce, kind) == (nonce, 0)
            wa, wb = tpke_model(pos, nonce)
            assert not mismatches(ra, wa), ("share side", nonce, mismatches(ra, wa))
            assert not mismatches(rb, wb), ("key side", nonce, mismatches(rb, wb))
            assert np.array_equal(got, t["expect"]), np.nonzero(got != t["expect"])[0].tolist()
            recs.append((ra, rb))
        dead = [i for i in range(n) if not t["live"][i]]
        assert all(recs[0][0][i] == INF1 and recs[0][1][i] == INF1 for i in dead)
        inf_share = t["first"][3] + 33
        assert recs[0][0][inf_share] == INF1 and recs[0][1][inf_share] != INF1
        # the second call's exponents are new ones: no record repeats (but the order-3 key's, which has three multiples)
        for i in range(n):
            if t["live"][i] and t["dec"][i] != 2:
                assert recs[0][1][i] != recs[1][1][i], i
                assert i == inf_share or recs[0][0][i] != recs[1][0][i], i


def test_model_modes_differ():
    """the two kinds of exponents give different points for the same share (so a mode that drew the other kind would
    fail above), and positions repeat across groups of one set while share indices do not"""
    t = tpke_case()
    pa, _ = tpke_model(True, 1)
    sa, _ = tpke_model(False, 1)
    live = [i for i in range(90) if t["live"][i] and t["shares"][i] != INF1]
    assert all(pa[i] != sa[i] for i in live)
    assert t["bins"][t["first"][1]] == t["bins"][t["first"][6]] == 32       # both runs of ciphertext 1 start at bin 32
    assert t["bins"][0] == t["bins"][t["first"][4]] == t["bins"][89] == 0   # sets 0 (ciphertexts 0, 4, out of range)


# ------------------------------------------------------------------------------------------------ c. TS records
_ts = {}


def ts_case():
    """7 signers, 3 messages, 21 shares message-major: a wrong signer's share, a share outside G2, an undecodable one"""
    if not _ts:
        b = Rounds(b"gpu-rlc-exponents-ts", 7, 3)
        midx = [r for r in range(3) for _ in range(7)]
        pidx = [i for _ in range(3) for i in range(7)]
        sigs = [b.good[r][i] for r, i in zip(midx, pidx)]
        sigs[3] = b.bad[0][3]
        sigs[7 + 2] = off_subgroup_g2(b.d)
        s = bytearray(sigs[14 + 5])
        while o.g2_valid(bytes(s)):
            s[0] = (s[0] + 1) & 0xFF
        sigs[14 + 5] = bytes(s)
        _ts.update(b=b, midx=midx, pidx=pidx, sigs=sigs)
    return _ts


def ts_model(b, pidx, sigs, nonce, seed=SEED):
    """k_ts_rlc_points' rule: a share that does not decode, or whose point lies outside G2 (it gets an exact single
    check instead), stores two points at infinity; every other share i stores (a, b)(i, domain 0) times its key and
    its signature"""
    ra, rb = [], []
    for i, (k, s) in enumerate(zip(pidx, sigs)):
        if not o.g2_valid(s) or not o.g2_in_subgroup(s):
            ra.append(INF1)
            rb.append(INF2)
            continue
        a, bb = M.rlc_scalar(seed, nonce, i, M.DOM_SHARE)
        ra.append(g1_ab(b.pks[k], a, bb))
        rb.append(g2_ab(s, a, bb))
    return ra, rb


def run_ts(nat, tdev, ctx, b, midx, pidx, sigs):
    torch, dev = tdev
    sh = torch.cuda.current_stream(dev).cuda_stream
    n = len(sigs)
    d_pk = up(torch, dev, b"".join(b.pks))
    d_m = up(torch, dev, b"".join(b.msgs))
    d_mo = up(torch, dev, np.arange(0, 24 * (b.m + 1), 24, dtype=np.uint32))
    d_mi = up(torch, dev, np.asarray(midx, dtype=np.uint32))
    d_pi = up(torch, dev, np.asarray(pidx, dtype=np.uint32))
    d_s = up(torch, dev, b"".join(sigs))
    d_acc = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    rc = nat.lib().lcb_ctx_ts_verify_shares_batched_dev(
        ctx.ptr, d_acc.data_ptr(), n, d_pk.data_ptr(), b.n, d_s.data_ptr(), d_m.data_ptr(), d_mo.data_ptr(), b.m,
        d_mi.data_ptr(), d_pi.data_ptr(), sh)
    assert rc == 0, nat.last_error()
    torch.cuda.synchronize(dev)
    return d_acc.cpu().numpy()


@pytest.mark.parametrize("order", ["message_major", "shuffled"])
def test_ts_records_equal_the_model(nat, tdev, hooks, fixed_seed, order):
    """rec_a[i] = a PK + b phi(PK), rec_b[i] = a sig_i + b psi^4(sig_i) with (a, b) from (i, domain 0) and the call's
    nonce, for two calls of a fresh context.  The excluded shares follow k_ts_rlc_points: the undecodable share and the
    share outside G2 both store two points at infinity (the latter is decided by an exact single check)"""
    t = ts_case()
    b = t["b"]
    p = list(range(21)) if order == "message_major" else np.random.default_rng(21).permutation(21).tolist()
    midx, pidx, sigs = ([t[k][i] for i in p] for k in ("midx", "pidx", "sigs"))
    expect = [int(b.expect(r, i, s)) for r, i, s in zip(midx, pidx, sigs)]
    assert expect.count(0) == 3
    with nat.Context() as ctx:
        for nonce in (1, 2):
            got = run_ts(nat, tdev, ctx, b, midx, pidx, sigs)
            ra, rb, got_nonce, kind = nat.debug_rlc_records(21, ctx)
            assert (got_nonce, kind) == (nonce, 1)
            wa, wb = ts_model(b, pidx, sigs, nonce)
            assert wa.count(INF1) == 2 and wb.count(INF2) == 2
            assert not mismatches(ra, wa), ("key side", nonce, mismatches(ra, wa))
            assert not mismatches(rb, wb), ("signature side", nonce, mismatches(rb, wb))
            assert got.tolist() == expect


def test_nonce_counts_the_contexts_batched_calls(nat, tdev, hooks, fixed_seed, defaults):
    """the nonce is the context's call counter across both kinds of calls: a TPKE call (1), then a threshold-signature
    call (2) whose records are the model's at nonce 2; the hook refuses a context without a batched call and a share
    count that is not the last call's"""
    t, s = tpke_case(), ts_case()
    with nat.Context() as ctx:
        with pytest.raises(RuntimeError, match="no batched call"):
            nat.debug_rlc_records(90, ctx)
        run_tpke(nat, tdev, ctx, t["b"], t["ct"], t["dec"], t["shares"])
        ra, rb, nonce, kind = nat.debug_rlc_records(90, ctx)
        assert (nonce, kind) == (1, 0) and (ra, rb) == tpke_model(True, 1)
        with pytest.raises(RuntimeError, match="share count"):
            nat.debug_rlc_records(89, ctx)
        run_ts(nat, tdev, ctx, s["b"], s["midx"], s["pidx"], s["sigs"])
        ra, rb, nonce, kind = nat.debug_rlc_records(21, ctx)
        assert (nonce, kind) == (2, 1) and (ra, rb) == ts_model(s["b"], s["pidx"], s["sigs"], 2)
        with pytest.raises(RuntimeError, match="share count"):
            nat.debug_rlc_records(90, ctx)


# ------------------------------------------------------------------------------------------------ d. the key is live
def test_exponents_follow_no_known_key_without_the_opt_in(nat, tdev, hooks, defaults):
    """without a seed every call draws its own key: a valid share's records differ between two fresh contexts and from
    the model under the zero key and under SEED; lcb_set_batch_seed without LCB_ALLOW_FIXED_BATCH_SEED=1 changes
    nothing of that"""
    t = tpke_case()
    i = t["first"][2] + 1                          # a good share of decryptor 1
    assert t["expect"][i] == 1
    known = [(m[0][i], m[1][i]) for m in (tpke_model(True, 1, SEED), tpke_model(True, 1, SEED2))]
    assert os.environ.get("LCB_ALLOW_FIXED_BATCH_SEED") is None
    seen = []
    try:
        for seeded in (False, False, True):
            nat.set_batch_seed(SEED if seeded else None)      # (ignored: no opt-in)
            with nat.Context() as ctx:
                got = run_tpke(nat, tdev, ctx, t["b"], t["ct"], t["dec"], t["shares"])
                ra, rb, nonce, kind = nat.debug_rlc_records(90, ctx)
            assert np.array_equal(got, t["expect"]) and (nonce, kind) == (1, 0)
            assert (ra[i], rb[i]) not in known and (ra[i], rb[i]) not in seen
            assert ra[i] != INF1 and rb[i] != INF1 and o.g1_valid(ra[i]) and o.g1_valid(rb[i])
            seen.append((ra[i], rb[i]))
    finally:
        nat.set_batch_seed(None)


def test_hooks_need_their_opt_in(nat, tdev):
    assert os.environ.get("LCB_ALLOW_TEST_HOOKS") is None
    t = tpke_case()
    with pytest.raises(RuntimeError, match="LCB_ALLOW_TEST_HOOKS"):
        nat.debug_rlc_scalars([(SEED, 1, 0, 0)])
    with nat.Context() as ctx:
        run_tpke(nat, tdev, ctx, t["b"], t["ct"], t["dec"], t["shares"])
        with pytest.raises(RuntimeError, match="LCB_ALLOW_TEST_HOOKS"):
            nat.debug_rlc_records(90, ctx)
        ra, rb = ctypes.create_string_buffer(48 * 90), ctypes.create_string_buffer(48 * 90)
        assert nat.lib().lcb_debug_rlc_records(ctx.ptr, ra, rb, 90, None, None) == -1
        assert ra.raw == bytes(48 * 90) and rb.raw == bytes(48 * 90)            # nothing was written
    ab = (ctypes.c_uint32 * 2)()
    key10, zero = (ctypes.c_uint32 * 10)(), (ctypes.c_uint32 * 1)()
    assert nat.lib().lcb_debug_rlc_scalars(key10, zero, zero, 1, ab) == -1 and list(ab) == [0, 0]


# ------------------------------------------------------------------------------------------------ e. forged pairs
def forged_tpke_case(share_exp, seed, nonce):
    """3 ciphertexts of N = 4 in ciphertext-major order; shares 5 and 7 (places 1 and 3 of ciphertext 1's group) are
    replaced by S1 + [t2] G and S2 - [t1] G, t_k the exponents the call under (seed, nonce) gives them"""
    b = Batch(b"gpu-rlc-exponents-forged", 4, 1, 3)
    ct = [c for c in range(3) for _ in range(4)]
    dec = [j for _ in range(3) for j in range(4)]
    shares = [b.good[c][j] for c, j in zip(ct, dec)]
    i1, i2 = 5, 7
    bins = M.tpke_bins(ct, b.c)
    assert (bins[i1], bins[i2]) == (32 + 1, 32 + 3)
    if share_exp:
        t1, t2 = (M.exponent(*M.rlc_scalar(seed, nonce, i, M.DOM_SHARE)) % R for i in (i1, i2))
    else:
        t1, t2 = (M.exponent(*M.rlc_scalar(seed, nonce, bins[i], M.DOM_POS)) % R for i in (i1, i2))
    g = o.g1_gen()
    shares[i1] = o.g1_add(shares[i1], o.g1_mul(g, o.fr(t2)))
    shares[i2] = o.g1_add(shares[i2], o.g1_mul(g, o.fr(R - t1)))
    expect = [int(b.expect(c, j, s)) for c, j, s in zip(ct, dec, shares)]
    assert expect == [1] * 5 + [0, 1, 0] + [1] * 4           # the oracle rejects both
    return b, ct, dec, shares, expect, (i1, i2)


@pytest.mark.parametrize("share_exp", [0, 1])
def test_forged_pair_passes_only_under_the_known_key_and_nonce(nat, tdev, fixed_seed, defaults, share_exp):
    """WHAT A KNOWN KEY BUYS AN ATTACKER, and why lcb_set_batch_seed needs LCB_ALLOW_FIXED_BATCH_SEED=1: whoever knows
    the ChaCha20 key, the call's nonce and the shares' places can make two wrong shares whose errors cancel in
    sum t_i S_i; the batched call then accepts both in one level while the exact check rejects both.  The same two
    shares are rejected on the context's next call (nonce 2), under another fixed key and under a fresh key — so the
    device's exponents are exactly the model's at (key, nonce, counter, domain): with any other exponent on either
    share the errors would not cancel.  Position exponents (counter = bin, domain 1) and per-share exponents
    (counter = index, domain 0)"""
    nat.set_rlc_share_exponents(share_exp)
    b, ct, dec, shares, expect, (i1, i2) = forged_tpke_case(share_exp, SEED, 1)
    with nat.Context() as ctx:
        got = run_tpke(nat, tdev, ctx, b, ct, dec, shares)
        levels, _ = nat.tpke_batched_stats()
        assert got.tolist() == [1] * 12 and levels == [3], (got.tolist(), levels)     # forged shares accepted
        got = run_tpke(nat, tdev, ctx, b, ct, dec, shares)                            # nonce 2
        levels, _ = nat.tpke_batched_stats()
        assert got.tolist() == expect and len(levels) > 1
    nat.set_batch_seed(SEED2)
    with nat.Context() as ctx:
        assert run_tpke(nat, tdev, ctx, b, ct, dec, shares).tolist() == expect
    nat.set_batch_seed(None)
    with nat.Context() as ctx:
        assert run_tpke(nat, tdev, ctx, b, ct, dec, shares).tolist() == expect


def test_forged_pair_of_signature_shares(nat, tdev, fixed_seed):
    """the same for threshold signatures: shares 2 and 5 of message 0 become sig1 + [s2] H and sig2 - [s1] H for a G2
    point H (the shares stay in G2, so no exact single check sees them), s_k the exponents of (index, domain 0) under
    SEED at nonce 1"""
    b = Rounds(b"gpu-rlc-exponents-forged-ts", 7, 2)
    midx = [r for r in range(2) for _ in range(7)]
    pidx = [i for _ in range(2) for i in range(7)]
    sigs = [b.good[r][i] for r, i in zip(midx, pidx)]
    i1, i2 = 2, 5
    s1, s2 = (M.exponent(*M.rlc_scalar(SEED, 1, i, M.DOM_SHARE)) % R for i in (i1, i2))
    h = o.g2_mul(o.g2_gen(), o.fr(0x5EED))
    sigs[i1] = o.g2_add(sigs[i1], o.g2_mul(h, o.fr(s2)))
    sigs[i2] = o.g2_add(sigs[i2], o.g2_mul(h, o.fr(R - s1)))
    assert o.g2_in_subgroup(sigs[i1]) and o.g2_in_subgroup(sigs[i2])
    expect = [int(b.expect(r, i, s)) for r, i, s in zip(midx, pidx, sigs)]
    assert expect == [1, 1, 0, 1, 1, 0, 1] + [1] * 7
    with nat.Context() as ctx:
        got = run_ts(nat, tdev, ctx, b, midx, pidx, sigs)
        levels, _ = nat.tpke_batched_stats()
        assert got.tolist() == [1] * 14 and levels == [2], (got.tolist(), levels)
        got = run_ts(nat, tdev, ctx, b, midx, pidx, sigs)                             # nonce 2
        levels, _ = nat.tpke_batched_stats()
        assert got.tolist() == expect and len(levels) > 1
    nat.set_batch_seed(SEED2)
    with nat.Context() as ctx:
        assert run_ts(nat, tdev, ctx, b, midx, pidx, sigs).tolist() == expect
    nat.set_batch_seed(None)
    with nat.Context() as ctx:
        assert run_ts(nat, tdev, ctx, b, midx, pidx, sigs).tolist() == expect
