"""GPU receipt verification (lcb_receipts_verify_batch, lcb_block_txs_verify_batch and their device forms; the mirror
in lachain_amd/transactions.py) against the plain-Python restatement (tests/pyref/txhash.py) plus the oracle's
o.ecdsa_recover / o.ecdsa_verify_hashed and tests/pyref/rbc_merkle.py's root.  64 receipts under 8 keys are signed on
the device; every way VerifyTransactionImmediately (TransactionVerifier.cs:109-143) can turn a receipt down is injected
once, and every accept and detail byte of the batch is compared, none skipped."""
import random

import pytest

import oracle as o
from helpers import gpu_native
from pyref import rbc_merkle as R
from pyref import txhash as T

pytestmark = pytest.mark.gpu

N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
CHAIN = {False: 25, True: 225}
_batches = {}


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


@pytest.fixture(scope="module")
def tx(nat):
    from lachain_amd import transactions as m
    if m.TransactionUtils.ChainId(False) == 0:
        m.TransactionUtils.SetChainId(CHAIN[False], CHAIN[True])
    return m


def fields(t):
    return (t.Nonce, t.GasPrice, t.GasLimit, t.To, t.Value, t.Invocation)


def high_s(sig: bytes, new: bool) -> bytes:
    """s -> n - s with the other recovery id: the same key recovers (there is no low-s rule on recovery)"""
    s = N_ORDER - int.from_bytes(sig[32:64], "big")
    v = int.from_bytes(sig[64:], "big")
    rid = v - 2 * CHAIN[new] - 35
    assert rid in (0, 1)
    return sig[:32] + s.to_bytes(32, "big") + (v - rid + (1 - rid)).to_bytes(len(sig) - 64, "big")


def signed_batch(tx, new):
    """64 receipts under 8 keys, signed on the device by the mirror; computed once per signature width"""
    if new in _batches:
        return _batches[new]
    rng = random.Random(64 + new)
    privs = [rng.randrange(1, N_ORDER).to_bytes(32, "big") for _ in range(8)]
    addrs = [T.address_of(o.ecdsa_pubkey(p)[0]) for p in privs]
    txs = []
    for i in range(64):
        to = rng.randbytes(20) if i % 5 else b""
        txs.append(tx.Transaction(To=to, Value=rng.randrange(2 ** 70).to_bytes(32, "big"), From=addrs[i % 8], Nonce=i // 8,
                                  GasPrice=rng.randrange(3), GasLimit=rng.randrange(10 ** 9),
                                  Invocation=rng.randbytes([0, 36, 68, 200][i % 4])))
    receipts = tx.Signer.SignBatch(txs, [privs[i % 8] for i in range(64)],
                                   [rng.randrange(1, N_ORDER).to_bytes(32, "big") for _ in range(64)], new)
    _batches[new] = (receipts, privs, addrs)
    return _batches[new]


def flat(nat, receipts):
    return (b"".join(r.Transaction.record() for r in receipts), [r.Transaction.Invocation for r in receipts],
            b"".join(r.Signature for r in receipts), b"".join(r.Hash for r in receipts))


def want_of(receipts, new):
    res = [T.verify_receipt(fields(r.Transaction), r.Signature, r.Hash, r.Transaction.From, new, CHAIN[new]) for r in receipts]
    return bytes(a for a, _ in res), bytes(d for _, d in res)


def injected(tx, receipts, new):
    """the 64 receipts with each rejection case once; (receipts, {index: expected (accept, detail)})"""
    rs = list(receipts)
    size = 66 if new else 65

    def resign(i, sig):
        t = rs[i].Transaction
        rs[i] = tx.TransactionReceipt(t, T.full_hash(*fields(t), sig), sig)

    h = bytearray(rs[3].Hash)
    h[17] ^= 0x04
    rs[3] = rs[3]._replace(Hash=bytes(h))                                                    # claimed hash, one bit
    frm = bytearray(rs[7].Transaction.From)
    frm[0] ^= 0x80
    rs[7] = rs[7]._replace(Transaction=rs[7].Transaction._replace(From=bytes(frm)))          # From flipped
    resign(11, high_s(rs[11].Signature, new))                                                # high s: still accepted
    resign(15, bytes(32) + rs[15].Signature[32:])                                            # r = 0
    resign(19, rs[19].Signature[:64] + b"\xff" * (size - 64))                                # v out of range
    resign(23, bytes(size))                                                                  # the zero signature
    return rs, {3: (0, 6), 7: (0, 3), 11: (1, 7), 15: (0, 1), 19: (0, 1), 23: (0, 1)}


@pytest.mark.parametrize("new", [False, True])
def test_signed_receipts_match_the_restatement(nat, tx, new):
    receipts, _, _ = signed_batch(tx, new)
    for r in receipts[:8]:
        t = r.Transaction
        assert tx.TransactionUtils.Rlp(t, new) == T.rlp(*fields(t), CHAIN[new])
        assert tx.TransactionUtils.RlpWithSignature(t, r.Signature, new) == T.rlp_with_signature(*fields(t), r.Signature)
    assert [r.Hash for r in receipts] == [T.full_hash(*fields(r.Transaction), r.Signature) for r in receipts]
    assert tx.TransactionUtils.RawHashes([r.Transaction for r in receipts], new) == \
        [T.raw_hash(*fields(r.Transaction), CHAIN[new]) for r in receipts]


@pytest.mark.parametrize("new", [False, True])
def test_receipts_verify_every_rejection_case(nat, tx, new):
    receipts, _, _ = signed_batch(tx, new)
    rs, pinned = injected(tx, receipts, new)
    want_acc, want_det = want_of(rs, new)
    for i, (a, d) in pinned.items():
        assert (want_acc[i], want_det[i]) == (a, d), i
    assert want_acc.count(1) == 64 - 5
    recs, invs, sigs, hashes = flat(nat, rs)
    acc, det = nat.receipts_verify_batch(recs, invs, sigs, 66 if new else 65, hashes, new, CHAIN[new])
    assert det == want_det
    assert acc == want_acc
    ver = tx.TransactionVerifier()
    assert ver.VerifyTransactions(rs, new, False) == [bool(a) for a in want_acc]
    assert ver.VerifyTransactionImmediately(rs[11], new, False) and not ver.VerifyTransactionImmediately(rs[23], new, False)


def block_case(tx, new):
    receipts, _, _ = signed_batch(tx, new)
    rs, _ = injected(tx, receipts, new)
    rs = rs[:14]                                      # blocks of 0, 1, 2, 3 and 8 receipts; receipts 3, 7, 11 are special
    tx_off = [0, 0, 1, 3, 6, 14]
    roots = []
    for b in range(5):
        root = R.compute_root([r.Hash for r in rs[tx_off[b]:tx_off[b + 1]]])
        roots.append(root if root is not None else bytes(32))
    roots[3] = bytes([roots[3][0] ^ 1]) + roots[3][1:]                                       # one wrong expected root
    return rs, tx_off, roots


def test_block_form(nat, tx):
    new = False
    rs, tx_off, roots = block_case(tx, new)
    want_acc, want_det = want_of(rs, new)
    recs, invs, sigs, hashes = flat(nat, rs)
    acc, det, root_ok = nat.block_txs_verify_batch(recs, invs, sigs, 65, hashes, tx_off, b"".join(roots), new, CHAIN[new])
    assert (acc, det) == (want_acc, want_det)
    assert root_ok == bytes([1, 1, 1, 0, 1])
    # an empty block's root is zero: any other expectation fails it
    acc, det, root_ok = nat.block_txs_verify_batch(recs, invs, sigs, 65, hashes, tx_off, b"\x01" + bytes(31) + b"".join(roots[1:]),
                                                   new, CHAIN[new])
    assert (acc, det, root_ok) == (want_acc, want_det, bytes([0, 1, 1, 0, 1]))
    # blocks only, no receipts at all
    acc, det, root_ok = nat.block_txs_verify_batch(b"", [], b"", 65, b"", [0, 0, 0], bytes(32) + b"\x02" + bytes(31), new,
                                                   CHAIN[new])
    assert (acc, det, root_ok) == (b"", b"", bytes([1, 0]))


def test_device_forms(nat, tx):
    import torch
    new = True
    rs, tx_off, roots = block_case(tx, new)
    want_acc, want_det = want_of(rs, new)
    recs, invs, sigs, hashes = flat(nat, rs)
    n = len(rs)
    off = [0]
    for i in invs:
        off.append(off[-1] + len(i))
    dev = torch.device("cuda:0")

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    d_rec, d_inv, d_sig, d_hash, d_exp = up(recs), up(b"".join(invs)), up(sigs), up(hashes), up(b"".join(roots))
    d_off = torch.tensor(off, dtype=torch.int64, device=dev)
    d_toff = torch.tensor(tx_off, dtype=torch.int64, device=dev)
    lib = nat.lib()
    st = torch.cuda.current_stream().cuda_stream
    with nat.Context() as ctx:
        for c in (None, ctx.ptr):
            pre = (c,) if c else ()
            acc = torch.full((n,), 9, dtype=torch.uint8, device=dev)
            det = torch.full((n,), 9, dtype=torch.uint8, device=dev)
            fn = lib.lcb_ctx_receipts_verify_dev if c else lib.lcb_receipts_verify_dev
            assert fn(*pre, acc.data_ptr(), det.data_ptr(), d_rec.data_ptr(), d_inv.data_ptr(), d_off.data_ptr(),
                      d_sig.data_ptr(), 66, d_hash.data_ptr(), n, 1, CHAIN[new], st) == 0, lib.lcb_last_error()
            torch.cuda.synchronize()
            assert (bytes(acc.cpu().numpy()), bytes(det.cpu().numpy())) == (want_acc, want_det)
            acc.fill_(9)
            rok = torch.full((5,), 9, dtype=torch.uint8, device=dev)
            fn = lib.lcb_ctx_block_txs_verify_dev if c else lib.lcb_block_txs_verify_dev
            assert fn(*pre, acc.data_ptr(), None, rok.data_ptr(), d_rec.data_ptr(), d_inv.data_ptr(), d_off.data_ptr(),
                      d_sig.data_ptr(), 66, d_hash.data_ptr(), n, d_toff.data_ptr(), d_exp.data_ptr(), 5, 1, CHAIN[new],
                      st) == 0, lib.lcb_last_error()
            torch.cuda.synchronize()
            assert bytes(acc.cpu().numpy()) == want_acc and bytes(rok.cpu().numpy()) == bytes([1, 1, 1, 0, 1])
    ms = nat.tx_phase_ms()                             # the default context's last call: the block form above
    assert len(ms) == 3 and all(m > 0 for m in ms), ms
    # a signature width that does not go with the chain id fails the call
    assert lib.lcb_receipts_verify_dev(acc.data_ptr(), None, d_rec.data_ptr(), d_inv.data_ptr(), d_off.data_ptr(),
                                       d_sig.data_ptr(), 65, d_hash.data_ptr(), n, 1, CHAIN[new], st) == -1


def sequential_reference(receipts, new):
    """the reference's loop with the cache on, from the restatement and the oracle"""
    cache, out = {}, []
    for r in receipts:
        t = fields(r.Transaction)
        if T.full_hash(*t, r.Signature) != r.Hash:
            out.append(False)
            continue
        raw = T.raw_hash(*t, CHAIN[new])
        frm = r.Transaction.From
        if frm in cache:
            out.append(bool(o.ecdsa_verify_hashed(raw, r.Signature, cache[frm], new, CHAIN[new])))
            continue
        rec = T.rec_id(r.Signature, CHAIN[new], new)
        pk = o.ecdsa_recover(raw, r.Signature[:64], rec) if rec is not None else None
        if pk is None or T.address_of(pk) != frm:
            out.append(False)
            continue
        cache[frm] = pk
        out.append(True)
    return out


@pytest.mark.parametrize("new", [False, True])
def test_cached_walk_equals_the_sequential_loop(nat, tx, new):
    receipts, _, _ = signed_batch(tx, new)
    a = [r for i, r in enumerate(receipts) if i % 8 == 0]          # one sender's receipts
    b = [r for i, r in enumerate(receipts) if i % 8 == 1]

    def with_high_s(r):
        sig = high_s(r.Signature, new)
        return tx.TransactionReceipt(r.Transaction, T.full_hash(*fields(r.Transaction), sig), sig)

    bad = a[0]._replace(Hash=bytes(32))
    # sender a: a bad first receipt (not cached), a high s before the key is cached (recovered: accepted, and cached),
    # a good one (cached branch), a high s after (cached branch: low s enforced, rejected); sender b in between
    seq = [bad, with_high_s(a[1]), a[2], with_high_s(a[3]), b[0], a[4], with_high_s(b[1]), b[2]]
    want = sequential_reference(seq, new)
    assert want == [False, True, True, False, True, True, False, True]
    ver = tx.TransactionVerifier()
    assert ver.VerifyTransactions(seq, new, True) == want
    # a second call starts with both senders cached: every receipt takes the cached branch
    assert ver.VerifyTransactions(seq, new, True) == [False, False, True, False, True, True, False, True]
    # receipt by receipt, as the reference's worker does
    one = tx.TransactionVerifier()
    assert [one.VerifyTransactionImmediately(r, new, True) for r in seq] == want
