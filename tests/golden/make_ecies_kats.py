"""Writes tests/golden/ecies_kats.json: a third implementation's answers for the ECIES envelope (OpenSSL's libcrypto
through ctypes), beside the kernels and tests/pyref/ecies.py.

  GCM        EVP_aes_256_gcm with EVP_CTRL_GCM_SET_IVLEN = 16 (the 16-byte nonce of DefaultCrypto.cs:267-299)
  ECDH       EC_POINT_mul on NID_secp256k1 (714), then SHA256 of the compressed point (libsecp256k1's default hash)
  envelope   eph_pub33 || nonce || C || tag (DefaultCrypto.cs:301-336)

Before anything is written the script checks that this libcrypto reproduces McGrew-Viega test case 14 (AES-256, 96-bit
zero IV, one zero block).  The file holds data only.  Run:  python3 tests/golden/make_ecies_kats.py
"""
import ctypes
import ctypes.util
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
P = 2 ** 256 - 2 ** 32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GCM_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 64, 255, 256, 2752]

vp, ci, cz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def load():
    lib = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
    sig = {
        "EVP_CIPHER_CTX_new": (vp, []), "EVP_CIPHER_CTX_free": (None, [vp]), "EVP_aes_256_gcm": (vp, []),
        "EVP_EncryptInit_ex": (ci, [vp, vp, vp, ctypes.c_char_p, ctypes.c_char_p]),
        "EVP_CIPHER_CTX_ctrl": (ci, [vp, ci, ci, vp]),
        "EVP_EncryptUpdate": (ci, [vp, vp, ctypes.POINTER(ci), ctypes.c_char_p, ci]),
        "EVP_EncryptFinal_ex": (ci, [vp, vp, ctypes.POINTER(ci)]),
        "EC_GROUP_new_by_curve_name": (vp, [ci]), "EC_POINT_new": (vp, [vp]), "EC_POINT_free": (None, [vp]),
        "EC_POINT_oct2point": (ci, [vp, vp, ctypes.c_char_p, cz, vp]),
        "EC_POINT_point2oct": (cz, [vp, vp, ci, vp, cz, vp]),
        "EC_POINT_mul": (ci, [vp, vp, vp, vp, vp, vp]),
        "BN_bin2bn": (vp, [ctypes.c_char_p, ci, vp]), "BN_free": (None, [vp]),
        "SHA256": (vp, [ctypes.c_char_p, cz, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


L = load()
GROUP = L.EC_GROUP_new_by_curve_name(714)
assert GROUP, "this libcrypto has no secp256k1"


def gcm(key: bytes, iv: bytes, pt: bytes):
    ctx = L.EVP_CIPHER_CTX_new()
    assert L.EVP_EncryptInit_ex(ctx, L.EVP_aes_256_gcm(), None, None, None) == 1
    assert L.EVP_CIPHER_CTX_ctrl(ctx, 0x9, len(iv), None) == 1            # EVP_CTRL_GCM_SET_IVLEN
    assert L.EVP_EncryptInit_ex(ctx, None, None, key, iv) == 1
    out = ctypes.create_string_buffer(len(pt) + 16)
    n = ci(0)
    assert L.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), pt, len(pt)) == 1
    got = n.value
    assert L.EVP_EncryptFinal_ex(ctx, ctypes.byref(out, got), ctypes.byref(n)) == 1
    got += n.value
    tag = ctypes.create_string_buffer(16)
    assert L.EVP_CIPHER_CTX_ctrl(ctx, 0x10, 16, tag) == 1                  # EVP_CTRL_GCM_GET_TAG
    L.EVP_CIPHER_CTX_free(ctx)
    assert got == len(pt)
    return out.raw[:got], tag.raw


def point_mul(pub33, scalar: bytes) -> bytes:
    """compressed scalar * P, or scalar * G when pub33 is None"""
    bn = L.BN_bin2bn(scalar, len(scalar), None)
    r = L.EC_POINT_new(GROUP)
    if pub33 is None:
        assert L.EC_POINT_mul(GROUP, r, bn, None, None, None) == 1
    else:
        p = L.EC_POINT_new(GROUP)
        assert L.EC_POINT_oct2point(GROUP, p, pub33, len(pub33), None) == 1
        assert L.EC_POINT_mul(GROUP, r, None, p, bn, None) == 1
        L.EC_POINT_free(p)
    out = ctypes.create_string_buffer(33)
    assert L.EC_POINT_point2oct(GROUP, r, 2, out, 33, None) == 33          # POINT_CONVERSION_COMPRESSED
    L.EC_POINT_free(r)
    L.BN_free(bn)
    return out.raw


def sha256(data: bytes) -> bytes:
    out = ctypes.create_string_buffer(32)
    L.SHA256(data, len(data), out)
    return out.raw


def ecdh(pub33: bytes, scalar: bytes) -> bytes:
    return sha256(point_mul(pub33, scalar))


def self_check():
    c, t = gcm(bytes(32), bytes(12), bytes(16))
    assert c.hex() == "cea7403d4d606b6e074ec5d3baf39d18" and t.hex() == "d0d1c8a799996bf0265b98b5d48ab919", \
        "libcrypto does not reproduce McGrew-Viega test case 14"
    g = point_mul(None, (1).to_bytes(32, "big"))
    assert g.hex() == "0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798"
    assert sha256(b"abc").hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"


def main():
    self_check()
    rng = random.Random(20260)
    b32 = lambda v: v.to_bytes(32, "big")
    lam = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
    assert (lam * lam + lam + 1) % N == 0
    kats = {"source": "OpenSSL libcrypto through ctypes (tests/golden/make_ecies_kats.py)", "gcm": [], "ecdh": [],
            "envelopes": []}
    for n in GCM_LENGTHS:
        key, nonce, pt = rng.randbytes(32), rng.randbytes(16), rng.randbytes(n)
        c, t = gcm(key, nonce, pt)
        kats["gcm"].append({"len": n, "key": key.hex(), "nonce": nonce.hex(), "pt": pt.hex(), "out": (nonce + c + t).hex()})
    # points of both parities
    pubs = {0: [], 1: []}
    while len(pubs[0]) < 14 or len(pubs[1]) < 14:
        pk = point_mul(None, b32(rng.randrange(1, N)))
        pubs[pk[0] & 1].append(pk)
    nib8 = int("8" * 32, 16)                       # all nibbles of the low half 8: every window carries
    nibf = int("f" * 63, 16)                       # all nibbles f (below n)
    assert nibf < N
    scalars = [("random", rng.randrange(1, N)) for _ in range(16)]
    scalars += [("1", 1), ("2", 2), ("8", 8), ("9", 9), ("2^128", 2 ** 128), ("lambda", lam), ("n-lambda", N - lam),
                ("n-1", N - 1), ("low nibbles 8", nib8), ("nibbles f", nibf)]
    for i, (note, d) in enumerate(scalars):
        pub = pubs[i & 1][i // 2]
        kats["ecdh"].append({"note": note, "pub": pub.hex(), "scalar": b32(d).hex(), "key": ecdh(pub, b32(d)).hex()})
    for n in (32, 2752):
        for parity in (0, 1):
            rpriv = b32(rng.randrange(1, N))
            rpub = point_mul(None, rpriv)
            while True:
                eph = b32(rng.randrange(1, N))
                epub = point_mul(None, eph)
                if epub[0] & 1 == parity:
                    break
            nonce, pt = rng.randbytes(16), rng.randbytes(n)
            key = ecdh(rpub, eph)
            assert key == ecdh(epub, rpriv)
            c, t = gcm(key, nonce, pt)
            kats["envelopes"].append({"len": n, "recipient_priv": rpriv.hex(), "recipient_pub": rpub.hex(),
                                      "eph_priv": eph.hex(), "nonce": nonce.hex(), "pt": pt.hex(),
                                      "envelope": (epub + nonce + c + t).hex()})
    with open(os.path.join(HERE, "ecies_kats.json"), "w") as f:
        json.dump(kats, f, indent=1)
        f.write("\n")
    print("wrote", len(kats["gcm"]), "gcm,", len(kats["ecdh"]), "ecdh,", len(kats["envelopes"]), "envelope cases")


if __name__ == "__main__":
    main()
