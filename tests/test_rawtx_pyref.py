"""CPU check of the raw-transaction restatement (tests/pyref/rawtx.py) against what the reference pins: the six signed
strings of its own tests (tests/golden/rawtx_kats.json) decode to nine elements, hash to Keccak-256 of their wire bytes
and recover to their senders; every item of the transaction sweep survives the trip through the wire; and wherever an
accepted item re-encodes to its own wire bytes, FullHash is the oracle's Keccak-256 of those bytes.  TEST
INFRASTRUCTURE for tests/test_rawtx_emul.py and tests/test_gpu_rawtx.py, which compare the lane with the restatement."""
import os
import sys

import pytest

import oracle as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rawtx_cases as C  # noqa: E402
import tx_cases as X  # noqa: E402
from pyref import rawtx as W  # noqa: E402
from pyref import txhash as T  # noqa: E402


def test_six_vectors():
    kats = C.kats()
    assert len(kats) == 6
    signer = bytes.fromhex(C.K["signer"]["address"])
    assert signer == bytes.fromhex("6bc32575acb8754886dc283c2c8ac54b1bd93195")
    assert T.address_of(o.ecdsa_pubkey(bytes.fromhex(C.K["signer"]["private_key"]))[0]) == signer
    assert [c for _, _, c, _, _ in kats] == [25, 225, 25, 225, 1, 41]
    for k, (wire, new, chain, frm, pinned) in enumerate(kats):
        got = W.ingest(wire, 0, new, chain)
        assert (got.accept, got.status, got.detail) == (1, 0, 7), k
        assert got.full32 == o.keccak256(wire), k
        if pinned is not None:
            assert got.full32 == pinned, k
        assert got.record[76:96] == frm, k
        assert frm == (signer if k < 5 else bytes.fromhex("2605c1ad496f428ab2b700edd257f0a378f83750")), k
        d = W.decode(wire, new, chain)
        assert T.rlp_with_signature(*d.tx, d.sig) == wire, k
        assert wire[got.span[0]:got.span[0] + got.span[1]] == d.tx[5], k
    # the two CryptographyTest strings are the ones tx_kats.json already holds, decoded back to its fields
    for k, new in ((2, False), (3, True)):
        (tx, sig, full, frm), = [c for c in X.kat_cases(new) if c[0][0] == 1]
        d = W.decode(kats[k][0], new, kats[k][2])
        assert (d.tx, d.sig) == (tx, sig) and kats[k][4] == full and kats[k][3] == frm


@pytest.mark.parametrize("new,chain", X.CALLS)
def test_round_trip(new, chain):
    L = 66 if new else 65
    seen = set()
    for it in X.sweep(new, chain):
        wire = T.rlp_with_signature(*it.tx, it.sig)
        d = W.decode(wire, new, chain)
        if len(T.signature_fields(it.sig)[0]) != L - 64:      # v stripped to another width: ToSignature throws
            assert d.status == W.WIDTH, it.note
            seen.add("width")
            continue
        assert d.status == W.OK and (d.tx, d.sig) == (it.tx, it.sig), it.note
        assert d.detail & W.SAME_ENCODING, it.note
        assert wire[d.span[0]:d.span[0] + d.span[1]] == it.tx[5]
        seen.add("ok")
    assert "ok" in seen and (not new or "width" in seen)


@pytest.mark.parametrize("new", [False, True])
def test_full_hash_is_keccak_of_canonical_wire(new):
    cases, chain = C.hostile(new)
    cases = cases + C.roundtrip(new, chain)
    same = other = refused = 0
    statuses = set()
    for c in cases:
        got = W.ingest(c.wire, 0, new, chain, recover=False)
        statuses.add(got.status)
        if got.status != W.OK:
            refused += 1
            assert got == W.Ingested(0, got.status, 0, bytes(104), (0, 0), bytes(66 if new else 65), bytes(32), bytes(32))
            continue
        d = W.decode(c.wire, new, chain)
        if T.rlp_with_signature(*d.tx, d.sig) == c.wire:
            assert got.full32 == o.keccak256(c.wire), c.note
            assert got.detail & W.SAME_ENCODING, c.note
            same += 1
        else:
            other += 1
    assert statuses == {0, 1, 2, 3, 4, 5}
    assert same > 100 and other > 10 and refused > 250
    base, _ = C.base_vector(new)
    for k in range(len(base)):
        assert W.decode(base[:k], new, chain).status != W.OK, k


def test_same_encoding_cases():
    cases, chain = C.hostile(False)
    by_note = {c.note: W.decode(c.wire, False, chain) for c in cases}
    for note in ("nonce = 00", "nonce = 00 05", "gasPrice empty", "gasLimit empty", "gasPrice = 00 05", "gasLimit = 00 05",
                 "value = 00 01", "value 32 bytes, leading zero"):
        assert (by_note[note].status, by_note[note].detail & 1) == (0, 0), note
    for note in ("nonce empty", "gasPrice = 00", "gasLimit = 00", "value empty", "base", "to empty", "r leading zero byte"):
        assert (by_note[note].status, by_note[note].detail & 1) == (0, 1), note
    for note, st in (("nonce 9 bytes", 5), ("value 33 bytes", 5), ("to 19 bytes", 5), ("to 21 bytes", 5), ("r 33 bytes", 5),
                     ("v two bytes", 5), ("v empty", 5), ("8 elements", 4), ("10 elements", 4), ("trailing byte", 2),
                     ("element: nested list", 3), ("element: 81 before a byte below 80", 3),
                     ("list length 2^32 - 1, nothing behind", 2), ("prefix 0", 1)):
        assert by_note[note].status == st, note
    assert by_note["v +1"].detail & 2 == 0 or by_note["v -1"].detail & 2 == 0
    assert by_note["v -2"].detail & 2 == 0 and by_note["v +2"].detail & 2 == 0 and by_note["v all zero"].detail & 2 == 0
