"""Shared inputs of the transaction-hash tests (tests/test_tx_emul.py on the CPU, tests/test_gpu_tx_hash.py on the
device): the reference's known answers and one sweep per (use_new_chain_id, chain_id) call.  Nothing is computed here
but inputs; expectations come from tests/pyref/txhash.py.  TEST INFRASTRUCTURE."""
import collections
import json
import os
import random
import struct

from pyref import txhash as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = json.load(open(os.path.join(ROOT, "tests", "golden", "tx_kats.json")))

# tx = (nonce, gas_price, gas_limit, to, value32, invocation); align: the invocation's offset mod 8 in the call's buffer
Item = collections.namedtuple("Item", "tx sig align note")
U64 = [0, 1, 0x7f, 0x80, 0xff, 0x100, 2 ** 63, 2 ** 64 - 1]
VALUES = [0, 1, 0x7f, 0x80, 2 ** 255, 2 ** 256 - 1]
INVOCATIONS = [b"", b"\x00", b"\x7f", b"\x80", 2, 55, 56, 255, 256, 65535, 65536,
               1023, 1024]                  # the library's threshold between its short-item and long-item kernels
EDGES = [135, 136, 137, 271, 272, 273]
# one call each: the signature width goes with use_new_chain_id, the chain id is free
CALLS = [(False, 1), (False, 25), (False, 127), (True, 128), (True, 225), (True, 2 ** 31 - 1)]


def kat_tx(name):
    t = K["transactions"][name]
    return (t["nonce"], t["gas_price"], t["gas_limit"], bytes.fromhex(t["to"]), bytes.fromhex(t["value"]),
            bytes.fromhex(t["invocation"]))


def kat_cases(new):
    """(tx, sig, full hash, from) of the reference's strings under one signature width"""
    return [(kat_tx(c["tx"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["full_hash"]),
             bytes.fromhex(K["transactions"][c["tx"]]["from"])) for c in K["signed"] if c["use_new_chain_id"] == new]


def sweep(new: bool, chain_id: int):
    """the items of one call, in buffer order.  Invocations lie back to back (the ABI's offsets leave no gaps), so an
    item reaches a wanted alignment through a short spacer item before it, itself hashed and checked like the rest."""
    rng = random.Random(1000003 * chain_id + new)
    L = 66 if new else 65
    to = bytes.fromhex("316fd97d8e47a2dec2c8783db740f08a10a13f4e")
    zero = bytes(L)

    def sig(r=None, s=None):
        r = rng.randbytes(32) if r is None else r
        s = rng.randbytes(32) if s is None else s
        v = (2 * chain_id + 35 + rng.randrange(2)) & (0xffff if new else 0xff)
        return r + s + v.to_bytes(L - 64, "big")

    def val(v):
        return v.to_bytes(32, "big")

    base = (5, 3, 21000, to, val(10 ** 19), b"")
    items, pos = [], 0

    def add(tx, sg, note, align=None):
        nonlocal pos
        if align is not None and pos % 8 != align:
            items.append(Item(base[:5] + (rng.randbytes((align - pos) % 8),), sig(), pos % 8, "spacer"))
            pos += (align - pos) % 8
        items.append(Item(tx, sg, pos % 8, note))
        pos += len(tx[5])

    def with_inv(tx, inv):
        return tx[:5] + (inv,)

    def solve(target, full, payload=False):
        """a transaction whose raw (or full) RLP, or its list payload, has the wanted length"""
        for nonce in (5, 0x100, 0x10000, 0):
            for t, sg in ((to, sig()), (b"", zero)):
                for n in range(0, 300):
                    tx = (nonce, 3, 21000, t, val(10 ** 19), bytes(n))
                    enc = T.rlp_with_signature(*tx, sg) if full else T.rlp(*tx, chain_id)
                    size = len(enc) - (1 if enc[0] < 0xf8 else 1 + enc[0] - 0xf7) if payload else len(enc)
                    if size == target:
                        return with_inv(tx, rng.randbytes(n)), sg
        raise AssertionError((target, full, payload))

    for kt, ks, _, _ in kat_cases(new):
        add(kt, ks, "kat")
    for t in (to, b""):                                                     # every field value, To present and empty
        for f in range(3):
            for v in U64:
                tx = list(base)
                tx[f], tx[3] = v, t
                add(tuple(tx), sig() if v & 1 else zero, "u64")
        for v in VALUES:
            add((5, 3, 21000, t, val(v), rng.randbytes(3)), sig(), "value")
    for inv in INVOCATIONS:                                                 # every length at every alignment
        for a in range(8):
            add(with_inv(base, inv if isinstance(inv, bytes) else rng.randbytes(inv)), sig(), "invocation", a)
    for full in (False, True):                                              # the Keccak block edges of each encoding
        for target in EDGES:
            tx, sg = solve(target, full)
            for a in range(8):
                add(with_inv(tx, rng.randbytes(len(tx[5]))), sg, "edge", a)
        for target in (55, 56):                                             # the short / long list header
            add(*solve(target, full, payload=True), "payload")
    for z in (1, 2, 31):                                                    # leading zero bytes in r and in s
        add(with_inv(base, rng.randbytes(36)), sig(r=bytes(z) + b"\x01" + rng.randbytes(31 - z)), "r zeros")
        add(with_inv(base, rng.randbytes(36)), sig(s=bytes(z) + b"\x80" + rng.randbytes(31 - z)), "s zeros")
    add(base, zero, "zero signature")
    add(base, sig(r=bytes(32)), "r = 0 alone (unpinned)")
    add(base, sig(s=bytes(32)), "s = 0 alone (unpinned)")
    tails = [b"\x00\x00", b"\x00\x55", b"\x01\xe5", b"\xff\xff"] if new else [b"\x00", b"\x55", b"\x7f", b"\x80"]
    for tail in tails:                                                      # v: whole when zero, else stripped
        add(base, rng.randbytes(64) + tail, "v")
    return items


def flatten(items):
    """(records, invocations, inv_off, sigs) as the ABI takes them; a record is lcb_tx_fields (104 B), From zero"""
    recs, off = bytearray(), [0]
    for it in items:
        nonce, gp, gl, to, value, inv = it.tx
        recs += struct.pack("<QQQ32s20s20sII", nonce, gp, gl, value, to.ljust(20, b"\0"), bytes(20), len(to), 0)
        off.append(off[-1] + len(inv))
    return bytes(recs), b"".join(it.tx[5] for it in items), off, b"".join(it.sig for it in items)


def expected(items, chain_id):
    """(raw hashes, full hashes) from the restatement"""
    return (b"".join(T.raw_hash(*it.tx, chain_id) for it in items),
            b"".join(T.full_hash(*it.tx, it.sig) for it in items))
