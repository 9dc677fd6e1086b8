"""Shared inputs of the raw-transaction ingress tests (tests/test_rawtx_emul.py on the CPU, tests/test_gpu_rawtx.py on
the device): the reference's six signed strings, the round trip of tests/tx_cases.py's sweep through the wire, and the
hostile items.  Nothing is computed here but inputs; expectations come from tests/pyref/rawtx.py.  TEST
INFRASTRUCTURE."""
import collections
import json
import os
import random

import tx_cases as X
from pyref import rawtx as W
from pyref import txhash as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = json.load(open(os.path.join(ROOT, "tests", "golden", "rawtx_kats.json")))

Case = collections.namedtuple("Case", "wire note")
# the calls of tx_cases.CALLS whose chain id the ingress takes (2 chain + 36 fits the signature's v)
CALLS = [(new, chain) for new, chain in X.CALLS if 2 * chain + 36 <= (0xffff if new else 0xff)]
MUTATIONS = [0x00, 0x7f, 0x80, 0x81, 0xb7, 0xb8, 0xbb, 0xbc, 0xbf, 0xc0, 0xf7, 0xf8, 0xfb, 0xfc, 0xff]


def kats():
    """[(wire, use_new_chain_id, chain_id, from20, pinned full hash or None)] in the fixture's order"""
    return [(bytes.fromhex(v["raw"]), v["use_new_chain_id"], v["chain_id"], bytes.fromhex(v["from"]),
             bytes.fromhex(v["full_hash"]) if "full_hash" in v else None) for v in K["vectors"]]


def base_vector(new: bool):
    """the TransactionsTest.cs vector of one signature width (113 bytes under the old chain id) and its chain id"""
    wire, _, chain, _, _ = kats()[1 if new else 0]
    return wire, chain


def elements(wire: bytes, new: bool, chain: int):
    """the nine element bodies of an accepted item"""
    d = W.decode(wire, new, chain)
    assert d.status == W.OK
    parts = []
    pos = 1 + (wire[0] - 0xf7 if wire[0] >= 0xf8 else 0)
    for _ in range(9):
        b = wire[pos]
        if b < 0x80:
            parts.append(wire[pos:pos + 1]); pos += 1
        elif b <= 0xb7:
            parts.append(wire[pos + 1:pos + 1 + b - 0x80]); pos += 1 + b - 0x80
        else:
            ll = b - 0xb7
            k = int.from_bytes(wire[pos + 1:pos + 1 + ll], "big")
            parts.append(wire[pos + 1 + ll:pos + 1 + ll + k]); pos += 1 + ll + k
    return parts


def build(parts) -> bytes:
    """a list of strings, canonically encoded"""
    return T.encode_list([T.encode_element(p) for p in parts])


def roundtrip(new: bool, chain: int):
    """every item of tx_cases.sweep on the wire, as the reference's encoder writes it"""
    return [Case(T.rlp_with_signature(*it.tx, it.sig), "roundtrip " + it.note) for it in X.sweep(new, chain)]


def hostile(new: bool):
    """the refusals, the non-canonical encodings and the size edges, built on the reference's vector of this width"""
    base, chain = base_vector(new)
    rng = random.Random(77 + new)
    e = elements(base, new, chain)
    out = []

    def add(wire, note):
        out.append(Case(bytes(wire), note))

    def sub(k, body, note):
        p = list(e)
        p[k] = body
        add(build(p), note)

    add(base, "base")
    for k in range(len(base)):                                             # every prefix: all refused
        add(base[:k], "prefix %d" % k)
    for k in range(len(base)):                                             # every byte set to every edge value
        for m in MUTATIONS:
            add(base[:k] + bytes([m]) + base[k + 1:], "byte %d = %02x" % (k, m))
    # length fields that claim 2^32 - 1, and more length bytes than four
    body = base[2:] if base[0] >= 0xf8 else base[1:]
    for ll in range(1, 9):
        add(bytes([0xf7 + ll]) + b"\xff" * ll + body, "list length ff x %d" % ll)
        p5 = T.encode_list([T.encode_element(x) for x in e[:5]])[1:]
        payload = p5 + bytes([0xb7 + ll]) + b"\xff" * ll + b"".join(T.encode_element(x) for x in e[6:])
        add(T._length(len(payload), 0xc0) + payload, "element length ff x %d" % ll)
    add(b"\xfb\xff\xff\xff\xff", "list length 2^32 - 1, nothing behind")
    add(b"\xc5\xbb\xff\xff\xff\xff", "element length 2^32 - 1, nothing behind")
    add(b"\xf8\x00" + body, "list: zero length byte")
    add(b"\xf8\x37" + bytes(55), "list: long form below 56")
    add(b"\xf9\x00\x70" + body, "list: leading zero length byte")
    for inv, note in ((b"\xb8\x24" + e[5], "long form below 56"), (b"\xb9\x00\x24" + e[5], "zero first length byte"),
                      (b"\x81\x05", "81 before a byte below 80"), (b"\xc0", "empty list"), (b"\xc1\x80", "nested list")):
        payload = b"".join(T.encode_element(x) for x in e[:5]) + inv + b"".join(T.encode_element(x) for x in e[6:])
        add(T._length(len(payload), 0xc0) + payload, "element: " + note)
    # SAME_ENCODING: each way elements 0-5 can differ from Lachain's own encoding, and the lone 00 that does not
    for k, name in ((0, "nonce"), (1, "gasPrice"), (2, "gasLimit")):
        sub(k, b"\x00", name + " = 00")
        sub(k, b"\x00\x05", name + " = 00 05")
        sub(k, b"", name + " empty")
        sub(k, b"\x7f", name + " = 7f")
        sub(k, b"\x80", name + " = 80")
        sub(k, b"\xff" * 8, name + " 8 bytes")
        sub(k, b"\x01" + bytes(8), name + " 9 bytes")
    sub(4, b"\x00\x01", "value = 00 01")
    sub(4, b"\x00" + rng.randbytes(31), "value 32 bytes, leading zero")
    sub(4, b"", "value empty")
    sub(4, b"\xff" * 32, "value 32 bytes")
    sub(4, b"\x01" + bytes(32), "value 33 bytes")
    sub(3, b"", "to empty")
    sub(3, rng.randbytes(19), "to 19 bytes")
    sub(3, rng.randbytes(21), "to 21 bytes")
    # v: off by one on either side, the other width, empty, all zero
    v = int.from_bytes(e[6], "big")
    w = len(e[6])
    for d in (-2, -1, 1, 2):
        sub(6, (v + d).to_bytes(w, "big"), "v %+d" % d)
    sub(6, b"", "v empty")
    sub(6, b"\x25", "v one byte")
    sub(6, b"\x01\xe5", "v two bytes")
    sub(6, b"\x00\x00\x25", "v three bytes")
    sub(6, bytes(w), "v all zero")
    for k, name in ((7, "r"), (8, "s")):
        sub(k, b"", name + " empty")
        sub(k, bytes(32), name + " 32 zero bytes")
        sub(k, b"\x00" + e[k][1:], name + " leading zero byte")
        sub(k, e[k][:31], name + " 31 bytes")
        sub(k, b"\x01" + e[k], name + " 33 bytes")
    add(build(e[:8]), "8 elements")
    add(build(e + [b""]), "10 elements")
    add(build(e + [b"\x01" * 60]), "10 elements, the tenth long")
    add(base + b"\x00", "trailing byte")
    add(base + base, "two lists")
    add(base[:-1], "truncated")
    # the size edges: list payloads and invocations
    for target in (55, 56, 255, 256, 65535, 65536):
        hit = 0
        for to, r, s in ((e[3], e[7], e[8]), (b"", b"\x01", b"\x02")):     # the short one reaches 55 and 56
            def wire_of(inv):
                return build(e[:3] + [to, e[4], inv, e[6], r, s])
            fixed = len(wire_of(b"")) - 1                                  # the payload with an empty invocation
            for k in range(max(0, target - fixed - 6), max(0, target - fixed + 2)):
                wire = wire_of(rng.randbytes(k))
                if len(wire) - (1 if wire[0] < 0xf8 else 1 + wire[0] - 0xf7) == target:
                    add(wire, "payload %d" % target)
                    hit += 1
        assert hit, target
    for inv in (b"", b"\x7f", b"\x80", 55, 56, 1023, 1024, 65536):
        sub(5, inv if isinstance(inv, bytes) else rng.randbytes(inv), "invocation")
    return out, chain


def pack(cases, aligned=()):
    """(raw, raw_off, cases in buffer order): the items back to back.  An item whose index is in `aligned` is put at
    each of the 8 start alignments in turn, through filler items of random bytes (decoded and checked like the rest)."""
    rng = random.Random(len(cases))
    items = []
    pos = 0
    for i, c in enumerate(cases):
        for a in (range(8) if i in aligned else (None,)):
            if a is not None and pos % 8 != a:
                fill = rng.randbytes((a - pos) % 8)
                items.append(Case(fill, "filler"))
                pos += len(fill)
            items.append(c)
            pos += len(c.wire)
    off = [0]
    for c in items:
        off.append(off[-1] + len(c.wire))
    return b"".join(c.wire for c in items), off, items


def expected(items, off, new: bool, chain: int, recover: bool):
    return [W.ingest(c.wire, off[i], new, chain, recover) for i, c in enumerate(items)]
