"""CPU checks of the pure-Python ECIES restatement (tests/pyref/ecies.py) against a third implementation's answers
(tests/golden/ecies_kats.json, OpenSSL through tests/golden/make_ecies_kats.py) and against itself.

Reference: DefaultCrypto.Secp256K1Encrypt / Secp256K1Decrypt / AesGcmEncrypt / AesGcmDecrypt (DefaultCrypto.cs:264-336).
Parity with the reference itself is unpinned (neither libsecp256k1 nor BouncyCastle runs here): it rests on the
published definitions and on three independent implementations agreeing."""
import json
import os
import random

from pyref import ecies as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = json.load(open(os.path.join(ROOT, "tests", "golden", "ecies_kats.json")))
GCM_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 64, 255, 256, 2752]


def test_kat_file_shape():
    assert [g["len"] for g in K["gcm"]] == GCM_LENGTHS
    assert len(K["ecdh"]) == 26 and {int(e["pub"][:2], 16) for e in K["ecdh"]} == {2, 3}
    assert sorted((e["len"], int(e["envelope"][:2], 16)) for e in K["envelopes"]) == [(32, 2), (32, 3), (2752, 2), (2752, 3)]


def test_sbox_known_entries():
    # FIPS 197 figure 7
    assert E.SBOX[0x00] == 0x63 and E.SBOX[0x01] == 0x7C and E.SBOX[0x53] == 0xED and E.SBOX[0xFF] == 0x16
    assert sorted(E.SBOX) == list(range(256))


def test_gcm_kats():
    for g in K["gcm"]:
        key, nonce, pt, out = (bytes.fromhex(g[k]) for k in ("key", "nonce", "pt", "out"))
        assert E.gcm_encrypt(key, nonce, pt) == out, g["len"]
        assert E.gcm_decrypt(key, out) == pt, g["len"]


def test_ecdh_kats():
    for e in K["ecdh"]:
        assert E.ecdh(bytes.fromhex(e["pub"]), bytes.fromhex(e["scalar"])) == bytes.fromhex(e["key"]), e["note"]


def test_envelope_kats():
    for e in K["envelopes"]:
        rpriv, rpub, eph, nonce, pt, env = (bytes.fromhex(e[k]) for k in ("recipient_priv", "recipient_pub", "eph_priv",
                                                                           "nonce", "pt", "envelope"))
        assert E.pubkey(rpriv) == rpub
        assert E.secp256k1_encrypt(rpub, eph, nonce, pt) == env
        assert E.secp256k1_decrypt(rpriv, env) == pt


def test_ecdh_symmetry():
    rng = random.Random(1)
    for _ in range(8):
        a, b = (rng.randrange(1, E.N).to_bytes(32, "big") for _ in range(2))
        assert E.ecdh(E.pubkey(b), a) == E.ecdh(E.pubkey(a), b)


def test_round_trip_and_every_single_bit_flip_is_rejected():
    rng = random.Random(2)
    priv = rng.randrange(1, E.N).to_bytes(32, "big")
    pt = rng.randbytes(5)
    env = E.secp256k1_encrypt(E.pubkey(priv), rng.randrange(1, E.N).to_bytes(32, "big"), rng.randbytes(16), pt)
    assert len(env) == len(pt) + 65 and E.secp256k1_decrypt(priv, env) == pt
    for bit in range(8, 8 * len(env)):                 # the ephemeral key's x, the nonce, C and the tag
        bad = bytearray(env)
        bad[bit // 8] ^= 0x80 >> (bit % 8)
        assert E.secp256k1_decrypt(priv, bytes(bad)) is None, bit
    assert E.secp256k1_decrypt(priv, env[:64]) is None and E.secp256k1_decrypt(priv, b"") is None
    assert E.secp256k1_decrypt(rng.randrange(1, E.N).to_bytes(32, "big"), env) is None
