"""GPU raw-transaction ingress (lcb_raw_txs_ingest_batch and its device forms; the mirror in
lachain_amd/transactions.py) against the plain-Python restatement (tests/pyref/rawtx.py) over the oracle.  The cases
are the ones tests/test_rawtx_emul.py has already run through the lane on the CPU under the sanitizer
(tests/rawtx_cases.py): the reference's six strings, the sweep's round trip and the hostile items, cut into calls of 1,
63, 64, 65 and 257 items.  Every byte of every output is compared, none skipped, and every buffer handed to the library
carries a guard pattern on both sides that must be intact afterwards."""
import ctypes
import os
import random
import struct
import sys

import pytest

import oracle as o
from helpers import gpu_native

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rawtx_cases as C  # noqa: E402
from pyref import rawtx as W  # noqa: E402
from pyref import txhash as T  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xa5
PAD = bytes([PATTERN]) * GUARD
SIZES = [1, 63, 64, 65, 257]
N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
CHAIN = {False: 25, True: 225}
_expected = {}


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


@pytest.fixture(scope="module")
def tx(nat):
    from lachain_amd import transactions as m
    if m.TransactionUtils.ChainId(False) == 0:
        m.TransactionUtils.SetChainId(CHAIN[False], CHAIN[True])
    return m


def guarded(data: bytes):
    """(buffer, pointer to the data inside it)"""
    buf = (ctypes.c_uint8 * (2 * GUARD + len(data))).from_buffer_copy(PAD + data + PAD)
    return buf, ctypes.cast(ctypes.byref(buf, GUARD), ctypes.POINTER(ctypes.c_uint8))


def inner(buf) -> bytes:
    raw = bytes(buf)
    assert raw[:GUARD] == PAD and raw[-GUARD:] == PAD, "guard overwritten"
    return raw[GUARD:-GUARD]


def sizes_of(n, L):
    """the outputs in the ABI's order: accept, status, detail, records, spans, signatures, raw hashes, full hashes"""
    return [n, n, n, 104 * n, 16 * n, L * n, 32 * n, 32 * n]


def unpack(outs, n, L):
    acc, st, det, recs, spans, sigs, raw32, full32 = outs
    sp = struct.unpack("<%dQ" % (2 * n), spans)
    return [W.Ingested(acc[i], st[i], det[i], recs[104 * i:104 * i + 104], (sp[2 * i], sp[2 * i + 1]),
                       sigs[L * i:L * i + L], raw32[32 * i:32 * i + 32], full32[32 * i:32 * i + 32]) for i in range(n)]


def host_call(nat, raw, off, new, chain, recover=True):
    """one lcb_raw_txs_ingest_batch over raw[off[0] .. off[-1]), the offsets as they are (not rebased by the test)"""
    n, L = len(off) - 1, 66 if new else 65
    b_raw, p_raw = guarded(raw)
    outs = [guarded(bytes([0x5a]) * s) for s in sizes_of(n, L)]
    ptr = [p for _, p in outs]
    ptr[4] = ctypes.cast(ptr[4], ctypes.POINTER(ctypes.c_uint64))
    if not recover:
        ptr[0] = None
    offs = (ctypes.c_uint64 * (n + 1))(*off)
    rc = nat.lib().lcb_raw_txs_ingest_batch(*ptr, p_raw, offs, n, int(new), chain)
    assert rc == 0, nat.last_error()
    assert inner(b_raw) == raw
    got = [inner(b) for b, _ in outs]
    if not recover:
        assert got[0] == bytes([0x5a]) * n                 # accept == NULL: nothing written there
        got[0] = bytes(n)
    return unpack(got, n, L)


def sliced(off):
    """(first item, one past the last) of successive calls of 1, 63, 64, 65, 257, 1, ... items"""
    out, i, k = [], 0, 0
    while i < len(off) - 1:
        j = min(len(off) - 1, i + SIZES[k % len(SIZES)])
        out.append((i, j))
        i, k = j, k + 1
    return out


def cases_of(new):
    """(raw, off, items, expectation with the recovery) of one width: computed once, shared by every test here"""
    if new not in _expected:
        cases, chain = C.hostile(new)
        assert chain == CHAIN[new]
        cases = [C.Case(w, "kat") for w, n_, c, _, _ in C.kats() if (n_, c) == (new, chain)] + cases + C.roundtrip(new, chain)
        aligned = {i for i, c in enumerate(cases) if c.note in ("kat", "base", "invocation", "truncated", "10 elements")}
        raw, off, items = C.pack(cases, aligned)
        _expected[new] = (raw, off, items, C.expected(items, off, new, chain, recover=True))
    return _expected[new]


def differences(got, want, items, first=0):
    return [(first + i, items[first + i].note, [f for f in W.Ingested._fields if getattr(got[i], f) != getattr(want[first + i], f)])
            for i in range(len(got)) if got[i] != want[first + i]]


def test_six_vectors_end_to_end(nat):
    for k, (wire, new, chain, frm, pinned) in enumerate(C.kats()):
        got, = host_call(nat, wire, [0, len(wire)], new, chain)
        assert got == W.ingest(wire, 0, new, chain), k
        assert (got.accept, got.status, got.detail, got.record[76:96]) == (1, 0, 7, frm), k
        assert got.full32 == o.keccak256(wire) and (pinned is None or got.full32 == pinned), k


@pytest.mark.parametrize("new", [False, True])
def test_cases_host_form(nat, new):
    raw, off, items, want = cases_of(new)
    assert {w.status for w in want} == {0, 1, 2, 3, 4, 5} and {w.detail for w in want} >= {0, 1, 3, 5, 6, 7}
    bad = []
    for i, j in sliced(off):
        # the whole buffer goes in with the call's own offsets: spans are offsets into raw, not into the call's items
        bad += differences(host_call(nat, raw, off[i:j + 1], new, CHAIN[new]), want, items, i)
    assert not bad, bad[:10]


@pytest.mark.parametrize("new", [False, True])
def test_cases_device_form(nat, new):
    import torch
    raw, off, items, want = cases_of(new)
    L = 66 if new else 65
    dev = torch.device("cuda:0")
    lib = nat.lib()
    d_raw = torch.frombuffer(bytearray(PAD + raw + PAD), dtype=torch.uint8).to(dev)
    d_off = torch.tensor(off, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    bad = []
    with nat.Context() as ctx:
        for k, (i, j) in enumerate(sliced(off)):
            n = j - i
            c = ctx.ptr if k % 2 else None
            outs = [torch.frombuffer(bytearray(PAD + bytes([0x5a]) * s + PAD), dtype=torch.uint8).to(dev) for s in sizes_of(n, L)]
            fn = lib.lcb_ctx_raw_txs_ingest_dev if c else lib.lcb_raw_txs_ingest_dev
            assert fn(*((c,) if c else ()), *[t.data_ptr() + GUARD for t in outs], d_raw.data_ptr() + GUARD,
                      d_off.data_ptr() + 8 * i, n, int(new), CHAIN[new], st) == 0, lib.lcb_last_error()
            torch.cuda.synchronize()
            got = []
            for t in outs:
                b = bytes(t.cpu().numpy())
                assert b[:GUARD] == PAD and b[-GUARD:] == PAD, "guard overwritten"
                got.append(b[GUARD:-GUARD])
            bad += differences(unpack(got, n, L), want, items, i)
    assert bytes(d_raw.cpu().numpy()) == PAD + raw + PAD
    assert not bad, bad[:10]
    ms = nat.rawtx_phase_ms()
    assert len(ms) == 3 and all(m >= 0 for m in ms), ms


def test_decode_and_hash_form(nat):
    """accept == NULL: no recovery, detail carries bits 0 and 1 only, From stays zero"""
    raw, off, items, _ = cases_of(True)
    i, j = sliced(off)[4]
    want = C.expected(items[i:j], off[i:j], True, CHAIN[True], recover=False)
    got = host_call(nat, raw, off[i:j + 1], True, CHAIN[True], recover=False)
    assert not differences(got, want, items[i:j])
    assert any(w.detail == 3 for w in want) and all(w.detail < 4 and w.record[76:96] == bytes(20) for w in want)


def signed_wires(tx, new):
    """64 transactions under 8 keys signed on the device (lcb_tx_hash_batch's raw hashes, lcb_ecdsa_sign_hashed_batch), on
    the wire, with each rejection injected once: {index: (status, detail)}"""
    rng = random.Random(640 + new)
    privs = [rng.randrange(1, N_ORDER).to_bytes(32, "big") for _ in range(8)]
    addrs = [T.address_of(o.ecdsa_pubkey(p)[0]) for p in privs]
    txs = [tx.Transaction(To=rng.randbytes(20) if i % 5 else b"", Value=rng.randrange(2 ** 70).to_bytes(32, "big"),
                          From=addrs[i % 8], Nonce=i // 8 + 1, GasPrice=rng.randrange(1, 3), GasLimit=rng.randrange(1, 10 ** 9),
                          Invocation=rng.randbytes([0, 36, 68, 1100][i % 4])) for i in range(64)]
    receipts = tx.Signer.SignBatch(txs, [privs[i % 8] for i in range(64)],
                                   [rng.randrange(1, N_ORDER).to_bytes(32, "big") for _ in range(64)], new)
    wires = [T.rlp_with_signature(r.Transaction.Nonce, r.Transaction.GasPrice, r.Transaction.GasLimit, r.Transaction.To,
                                  r.Transaction.Value, r.Transaction.Invocation, r.Signature) for r in receipts]
    chain = CHAIN[new]

    def rebuilt(i, k, body):
        e = C.elements(wires[i], new, chain)
        e[k] = body
        return C.build(e)

    e3 = C.elements(wires[3], new, chain)
    wires[3] = rebuilt(3, 0, b"\x00" + e3[0])                                          # the nonce with a leading zero byte
    v7 = int.from_bytes(C.elements(wires[7], new, chain)[6], "big")
    wires[7] = rebuilt(7, 6, (v7 + 2).to_bytes(2 if new else 1, "big"))                # another chain's v
    wires[11] = rebuilt(11, 7, b"")                                                    # r = 0: does not recover
    wires[15] = rebuilt(15, 8, (N_ORDER).to_bytes(32, "big"))                          # s = n: does not recover
    wires[19] = wires[19][:-1]                                                         # truncated
    wires[23] = rebuilt(23, 3, rng.randbytes(19))                                      # To of 19 bytes
    wires[27] = wires[27] + b"\x80"                                                    # a trailing byte
    wires[31] = b""                                                                    # nothing
    pinned = {3: (0, 6), 7: (0, 5), 11: (0, 3), 15: (0, 3), 19: (2, 0), 23: (5, 0), 27: (2, 0), 31: (1, 0)}
    return wires, addrs, pinned


@pytest.mark.parametrize("new", [False, True])
def test_device_signed_transactions_and_the_receipt_path(nat, tx, new):
    wires, addrs, pinned = signed_wires(tx, new)
    chain, L = CHAIN[new], 66 if new else 65
    raw = b"".join(wires)
    off = [0]
    for w in wires:
        off.append(off[-1] + len(w))
    want = [W.ingest(w, off[i], new, chain) for i, w in enumerate(wires)]
    for i, (st, det) in pinned.items():
        assert (want[i].status, want[i].detail, want[i].accept) == (st, det, 0), i
    got = host_call(nat, raw, off, new, chain)
    assert got == want
    for i in range(64):
        if i not in pinned:
            assert (got[i].accept, got[i].record[76:96]) == (1, addrs[i % 8]), i
    # the existing path on the decoded fields, FullHash as the claimed hash: the same decisions
    invs = [raw[g.span[0]:g.span[0] + g.span[1]] for g in got]
    acc, det = nat.receipts_verify_batch(b"".join(g.record for g in got), invs, b"".join(g.sig for g in got), L,
                                         b"".join(g.full32 for g in got), new, chain)
    assert acc == bytes(g.accept for g in got)
    raw32, full32 = nat.tx_hash_batch(b"".join(g.record for g in got), invs, b"".join(g.sig for g in got), L, new, chain)
    ok = [g.status == 0 for g in got]
    assert [raw32[32 * i:32 * i + 32] for i in range(64) if ok[i]] == [g.raw32 for g in got if g.status == 0]
    assert [full32[32 * i:32 * i + 32] for i in range(64) if ok[i]] == [g.full32 for g in got if g.status == 0]
    # the mirror: SendRawTransactionBatch with a pool that turns one sender's second transaction down
    seen = []

    def pool_add(t, sig):
        seen.append((t, sig))
        return "InvalidNonce" if (t.From == addrs[1] and t.Nonce == 2) else "Ok"

    res = tx.SendRawTransactionBatch(wires, new, pool_add)
    names = {3: "InvalidSignature", 7: "BadChainId", 11: "InvalidSignature", 15: "InvalidSignature",
             19: "Refused: ListLength", 23: "Refused: Width", 27: "Refused: ListLength", 31: "Refused: NotList"}
    for i in range(64):
        if i in names:
            assert res[i] == names[i], i
        elif i == 9:
            assert res[i] == "InvalidNonce"
        else:
            assert res[i] == "0x" + o.keccak256(wires[i]).hex(), i
    assert len(seen) == 64 - len(pinned)
    made = tx.MakeTransactions(wires, new)
    assert [m is None for m in made] == [want[i].status != 0 for i in range(64)]
    t0, s0 = made[0]
    assert (t0.From, s0, t0.Invocation) == (addrs[0], want[0].sig, invs[0])
    assert tx.TransactionUtils.RlpWithSignature(t0, s0, new) == wires[0]


def test_bad_arguments_fail_the_call(nat):
    wire = C.kats()[0][0]
    lib = nat.lib()
    (b_raw, p_raw), (b_st, p_st) = guarded(wire + wire), guarded(bytes(2))

    def call(off=(0, len(wire), 2 * len(wire)), new=0, chain=25, status=p_st, raw=p_raw, with_off=True):
        offs = (ctypes.c_uint64 * len(off))(*off)
        return lib.lcb_raw_txs_ingest_batch(None, status, None, None, None, None, None, None, raw, offs if with_off else None,
                                            2, new, chain)

    assert call() == 0 and inner(b_st) == bytes(2)
    assert call(status=None) == -1 and call(raw=None) == -1 and call(with_off=False) == -1
    assert call(chain=0) == -1 and call(chain=-1) == -1
    assert call(chain=109) == 0 and call(chain=110) == -1                # 2 chain + 36 must fit one byte
    assert call(new=1, chain=32749) == 0 and call(new=1, chain=32750) == -1
    assert call(off=(5, 4, 4)) == -1                                     # decreasing offsets
    assert call(off=(0, 2 ** 31, 2 ** 31)) == -1                         # an item of 2^31 bytes: refused before any read
    assert inner(b_raw) == wire + wire
