"""CPU checks of the ECIES kernels (lachain_amd/csrc/k_ecies.hip, ecies_lane.hpp) compiled for the host by
tools/emul/ecies_emul.cpp and run lane by lane, against the OpenSSL answers (tests/golden/ecies_kats.json) and the
pure-Python restatement (tests/pyref/ecies.py).  TEST INFRASTRUCTURE: catches logic errors in the device code without a
GPU; the GPU itself is covered by tests/test_gpu_ecies.py, which shares the mixed batches built here.

Reference: DefaultCrypto.Secp256K1Encrypt / Secp256K1Decrypt / AesGcmEncrypt / AesGcmDecrypt (DefaultCrypto.cs:264-336)."""
import ctypes
import functools
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pyref import ecies as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emul", "ecies_emul.cpp")
LIB = os.path.join(ROOT, "tools", "emul", "libecies_emul.so")
CSRC = os.path.join(ROOT, "lachain_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("k_ecies.hip", "ecies_lane.hpp", "k_secp.hip", "secp_comb.hpp", "secp.hpp")]
K = json.load(open(os.path.join(ROOT, "tests", "golden", "ecies_kats.json")))
P, N = E.P, E.N
GCM_LENGTHS = [g["len"] for g in K["gcm"]]
b32 = lambda v: v.to_bytes(32, "big")

# the restatement is slow (affine arithmetic, byte-wise AES): every distinct case is computed once
ref_ecdh = functools.lru_cache(maxsize=None)(E.ecdh)
ref_gcm_encrypt = functools.lru_cache(maxsize=None)(E.gcm_encrypt)
ref_gcm_decrypt = functools.lru_cache(maxsize=None)(E.gcm_decrypt)
ref_encrypt = functools.lru_cache(maxsize=None)(E.secp256k1_encrypt)
ref_decrypt = functools.lru_cache(maxsize=None)(E.secp256k1_decrypt)


# ---------------------------------------------------------------- the mixed batches (shared with the GPU test)
def _off_curve_x(rng):
    while True:
        x = rng.randrange(1, P)
        if pow((x ** 3 + 7) % P, (P - 1) // 2, P) != 1:
            return x


def _bad_keys(rng, good33: bytes):
    """a 33-byte slot of every rejected kind: prefixes 0, 4, 6; x = p, x = p + 1; an x off the curve"""
    return [bytes([pfx]) + good33[1:] for pfx in (0, 4, 6)] + \
           [b"\x02" + b32(P), b"\x03" + b32(P + 1), b"\x02" + b32(_off_curve_x(rng))]


BAD_SCALARS = [b32(0), b32(N), b32(2 ** 256 - 1)]


@functools.lru_cache(maxsize=None)
def pools():
    """every class of item once, with nothing computed but the inputs: ECDH pairs, GCM encryptions and decryptions,
    envelope encryptions and decryptions.  Expectations come from the restatement (expected_*), never from here."""
    rng = random.Random(424242)
    keys = [b32(rng.randrange(1, N)) for _ in range(4)]
    pubs = [E.pubkey(k) for k in keys]
    ecdh = [(bytes.fromhex(e["pub"]), bytes.fromhex(e["scalar"])) for e in K["ecdh"]]
    ecdh += [(bad, keys[0]) for bad in _bad_keys(rng, pubs[1])] + [(pubs[1], d) for d in BAD_SCALARS]
    ecdh += [(pubs[i % 4], b32(rng.randrange(1, N))) for i in range(8)]
    # recipient keys with the smallest x on the curve (1, 2, 3), both parities; a generator of their own, so that the
    # other pools keep their inputs
    erng = random.Random(0xEC1E5)
    ecdh += [(bytes([pfx]) + b32(x), d) for x in (1, 2, 3) for pfx, d in ((2, b32(erng.randrange(1, N))), (3, b32(N - 1)))]
    ecdh += [(b"\x02" + b32(1), b32(1)), (b"\x03" + b32(2), b32(2))]
    gcm_enc = [tuple(bytes.fromhex(g[k]) for k in ("key", "nonce", "pt")) for g in K["gcm"]]
    gcm_enc += [(rng.randbytes(32), rng.randbytes(16), rng.randbytes(ln)) for ln in GCM_LENGTHS[:9]]
    gcm_dec = [(bytes.fromhex(g["key"]), bytes.fromhex(g["out"])) for g in K["gcm"]]
    key, item = gcm_dec[4]
    gcm_dec += [(key, item[:ln]) for ln in (0, 1, 31)] + [(key, item[:32])]              # too short; 32 fails its tag
    gcm_dec += [(key, _flip(item, bit)) for bit in (0, 127, 128, 8 * len(item) - 129, 8 * len(item) - 1)]
    gcm_dec += [(rng.randbytes(32), item)]
    enc = [tuple(bytes.fromhex(e[k]) for k in ("recipient_pub", "eph_priv", "nonce", "pt")) for e in K["envelopes"]]
    enc += [(pubs[i % 4], b32(rng.randrange(1, N)), rng.randbytes(16), rng.randbytes(ln))
            for i, ln in enumerate(GCM_LENGTHS[:9])]
    enc += [(bad, keys[2], rng.randbytes(16), rng.randbytes(32)) for bad in _bad_keys(rng, pubs[0])]
    enc += [(pubs[0], d, rng.randbytes(16), rng.randbytes(32)) for d in BAD_SCALARS]
    dec = [(bytes.fromhex(e["recipient_priv"]), bytes.fromhex(e["envelope"])) for e in K["envelopes"]]
    for i, ln in enumerate(GCM_LENGTHS[:9]):
        dec.append((keys[i % 4], E.secp256k1_encrypt(pubs[i % 4], b32(rng.randrange(1, N)), rng.randbytes(16), rng.randbytes(ln))))
    priv, env = dec[0]
    assert len(env) == 97
    dec += [(priv, bad + env[33:]) for bad in _bad_keys(rng, env[:33])]
    dec += [(d, env) for d in BAD_SCALARS]
    empty = E.secp256k1_encrypt(pubs[0], keys[1], rng.randbytes(16), b"")
    dec += [(priv, env[:ln]) for ln in (0, 33, 64)] + [(keys[0], empty), (priv, env[:65])]   # 65: valid when empty
    dec += [(priv, _flip(env, bit)) for bit in (8 * 1 + 3, 8 * 32 + 7, 8 * 33, 8 * 48 + 5, 8 * 49, 8 * 80 + 7,
                                                 8 * 81, 8 * 96 + 7)]
    dec += [(priv, bytes([env[0] ^ 1]) + env[1:]), (keys[3], env)]                            # other parity; wrong key
    return {"ecdh": ecdh, "gcm_enc": gcm_enc, "gcm_dec": gcm_dec, "enc": enc, "dec": dec}


def _flip(data: bytes, bit: int) -> bytes:
    b = bytearray(data)
    b[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(b)


def mixed_batch(kind: str, n: int, seed: int = 0):
    """n items of one pool, every class present as soon as n allows, in a seeded order so that neighbouring lanes
    differ in kind and length"""
    pool = list(pools()[kind])
    random.Random(seed).shuffle(pool)
    return [pool[i % len(pool)] for i in range(n)]


def expected_ecdh(items):
    keys = [ref_ecdh(p, d) for p, d in items]
    return b"".join(k or bytes(32) for k in keys), bytes(int(k is not None) for k in keys)


def expected_gcm_encrypt(items):
    return [ref_gcm_encrypt(*it) for it in items]


def expected_gcm_decrypt(items):
    out = [ref_gcm_decrypt(*it) for it in items]
    return out, bytes(int(p is not None) for p in out)


def expected_encrypt(items):
    out = [ref_encrypt(*it) for it in items]
    return out, bytes(int(e is not None) for e in out)


def expected_decrypt(items):
    out = [ref_decrypt(*it) for it in items]
    return out, bytes(int(p is not None) for p in out)


def packed(plain, lens):
    """the library's packed plaintext layout: a rejected item of valid length keeps a zeroed slot"""
    return b"".join(p if p is not None else bytes(ln) for p, ln in zip(plain, lens))


def offsets(chunks):
    off = [0]
    for c in chunks:
        off.append(off[-1] + len(c))
    return off


# ---------------------------------------------------------------- the emulation
@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC], check=True)
    lib = ctypes.CDLL(LIB)
    lib.emu_ecdh.restype = ctypes.c_ulonglong
    return lib


def _u64(vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


def emu_ecdh(emu, items, indexed=False):
    n = len(items)
    key, ok = ctypes.create_string_buffer(32 * n + 1), ctypes.create_string_buffer(n + 1)
    pubs = b"".join(p for p, _ in items)
    if indexed:
        table = sorted({d for _, d in items})
        idx = (ctypes.c_uint32 * n)(*[table.index(d) for _, d in items])
        prod = emu.emu_ecdh(key, ok, pubs, b"".join(table), idx, len(table), n)
    else:
        prod = emu.emu_ecdh(key, ok, pubs, b"".join(d for _, d in items), None, n, n)
    return key.raw[:32 * n], ok.raw[:n], prod


def test_tables_and_sha256(emu):
    box = ctypes.create_string_buffer(256)
    emu.emu_aes_sbox(box)
    assert list(box.raw) == E.SBOX
    rng = random.Random(3)
    out = ctypes.create_string_buffer(32)
    for _ in range(4):
        msg = rng.randbytes(55)
        emu.emu_sha256_block(out, msg + b"\x80" + (8 * 55).to_bytes(8, "big"))
        assert out.raw == hashlib.sha256(msg).digest()


def test_kats(emu):
    for e in K["ecdh"]:
        key, ok, _ = emu_ecdh(emu, [(bytes.fromhex(e["pub"]), bytes.fromhex(e["scalar"]))])
        assert (key, ok) == (bytes.fromhex(e["key"]), b"\x01"), e["note"]
    for g in K["gcm"]:
        key, nonce, pt, want = (bytes.fromhex(g[k]) for k in ("key", "nonce", "pt", "out"))
        out = ctypes.create_string_buffer(len(want) + 1)
        emu.emu_gcm_encrypt(out, key, nonce, pt, _u64([0, len(pt)]), 1)
        assert out.raw[:-1] == want, g["len"]
    for e in K["envelopes"]:
        rpriv, rpub, eph, nonce, pt, want = (bytes.fromhex(e[k]) for k in ("recipient_priv", "recipient_pub", "eph_priv",
                                                                            "nonce", "pt", "envelope"))
        out, ok = ctypes.create_string_buffer(len(want) + 1), ctypes.create_string_buffer(2)
        emu.emu_secp256k1_encrypt(out, ok, rpub, eph, nonce, pt, _u64([0, len(pt)]), 1)
        assert (out.raw[:-1], ok.raw[:1]) == (want, b"\x01")
        back = ctypes.create_string_buffer(len(pt) + 1)
        emu.emu_secp256k1_decrypt(back, ok, rpriv, None, 1, want, _u64([0, len(want)]), 1)
        assert (back.raw[:-1], ok.raw[:1]) == (pt, b"\x01")


@pytest.mark.parametrize("indexed", [False, True])
def test_ecdh_mixed_batch(emu, indexed):
    items = mixed_batch("ecdh", len(pools()["ecdh"]) + 3, seed=1)
    want_key, want_ok = expected_ecdh(items)
    key, ok, _ = emu_ecdh(emu, items, indexed)
    assert ok == want_ok
    assert key == want_key
    assert ok.count(0) >= 9 and ok.count(1) >= 34


def test_gcm_mixed_batch(emu):
    items = mixed_batch("gcm_enc", len(pools()["gcm_enc"]), seed=2)
    want = expected_gcm_encrypt(items)
    pts = [it[2] for it in items]
    out = ctypes.create_string_buffer(sum(map(len, want)) + 1)
    emu.emu_gcm_encrypt(out, b"".join(it[0] for it in items), b"".join(it[1] for it in items), b"".join(pts),
                        _u64(offsets(pts)), len(items))
    assert out.raw[:-1] == b"".join(want)
    items = mixed_batch("gcm_dec", len(pools()["gcm_dec"]), seed=3)
    want, want_ok = expected_gcm_decrypt(items)
    cts = [it[1] for it in items]
    lens = [max(len(c) - 32, 0) for c in cts]
    back, ok = ctypes.create_string_buffer(sum(lens) + 1), ctypes.create_string_buffer(len(items) + 1)
    emu.emu_gcm_decrypt(back, ok, b"".join(it[0] for it in items), b"".join(cts), _u64(offsets(cts)), len(items))
    assert ok.raw[:-1] == want_ok
    assert back.raw[:-1] == packed(want, lens)
    assert want_ok.count(0) == 10 and want_ok.count(1) == len(K["gcm"])


def test_envelope_mixed_batch(emu):
    items = mixed_batch("enc", len(pools()["enc"]), seed=4)
    want, want_ok = expected_encrypt(items)
    pts = [it[3] for it in items]
    total = sum(len(p) + 65 for p in pts)
    out, ok = ctypes.create_string_buffer(total + 1), ctypes.create_string_buffer(len(items) + 1)
    emu.emu_secp256k1_encrypt(out, ok, b"".join(it[0] for it in items), b"".join(it[1] for it in items),
                              b"".join(it[2] for it in items), b"".join(pts), _u64(offsets(pts)), len(items))
    assert ok.raw[:-1] == want_ok
    assert out.raw[:-1] == b"".join(w if w is not None else bytes(len(p) + 65) for w, p in zip(want, pts))
    assert want_ok.count(0) == 9
    items = mixed_batch("dec", len(pools()["dec"]), seed=5)
    want, want_ok = expected_decrypt(items)
    cts = [it[1] for it in items]
    lens = [max(len(c) - 65, 0) for c in cts]
    back, ok = ctypes.create_string_buffer(sum(lens) + 1), ctypes.create_string_buffer(len(items) + 1)
    emu.emu_secp256k1_decrypt(back, ok, b"".join(it[0] for it in items), None, len(items), b"".join(cts),
                              _u64(offsets(cts)), len(items))
    assert ok.raw[:-1] == want_ok
    assert back.raw[:-1] == packed(want, lens)
    # valid: the KAT envelopes, the nine lengths, the two empty plaintexts; everything else is rejected
    assert want_ok.count(1) == len(K["envelopes"]) + 9 + 1


def test_field_products_per_ecdh_below_a_recovery(emu):
    """condition (a): the ladder is the recovery's minus the 33 comb additions"""
    import oracle as o
    import test_secp_recover_emul as R
    if not os.path.exists(R.LIB) or os.path.getmtime(R.LIB) < max(os.path.getmtime(d) for d in R.DEPS):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", R.LIB, R.SRC], check=True)
    rec = ctypes.CDLL(R.LIB)
    rec.emu_recover.restype = ctypes.c_ulonglong
    rng = random.Random(6)
    hs, sigs = [], []
    while len(hs) < 32:
        h = rng.randbytes(32)
        try:
            c, rid = o.ecdsa_sign_compact(h, b32(rng.randrange(1, N)), b32(rng.randrange(1, N)))
        except ValueError:
            continue
        hs.append(h)
        sigs.append(c + R.v_bytes(rid, 25, False))
    ok, _, _, _, products = R.emu_recover(rec, hs, sigs, 65, False, False, 25)
    assert ok == b"\x01" * 32
    per_recovery = products[1] / 32
    items = [(E.pubkey(b32(rng.randrange(1, N))), b32(rng.randrange(1, N))) for _ in range(32)]
    _, ok, prod = emu_ecdh(emu, items)
    assert ok == b"\x01" * 32
    per_ecdh = prod / 32
    print("field products per item: ECDH multiplication %.1f, recovery %.1f" % (per_ecdh, per_recovery))
    assert per_ecdh < per_recovery
