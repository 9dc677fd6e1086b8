"""Pure-Python restatement of the secp256k1 ECIES envelope of the trustless DKG (DefaultCrypto.Secp256K1Encrypt /
Secp256K1Decrypt, DefaultCrypto.cs:264-336): TEST INFRASTRUCTURE, written from the published definitions and on purpose
with other algorithms than the kernels (lachain_amd/csrc/ecies_lane.hpp):

  ECDH      textbook affine double-and-add with Python integers; key = SHA-256(compressed d P) through hashlib
            (libsecp256k1's default ECDH hash function)
  AES-256   byte-oriented FIPS 197 (SubBytes / ShiftRows / MixColumns on a 16-byte state); the S-box is generated from
            the GF(2^8) inverse and the affine map
  GCM       NIST SP 800-38D with a bitwise GHASH on Python integers; 16-byte nonce, so J0 = GHASH(nonce || 0^64 || [128])

Where the reference throws, the functions here return None.
"""
import hashlib

from .secp import G, N, P, compress, pt_add, pt_mul  # noqa: F401  (the affine group law lives in tests/pyref/secp.py)


# ---------------------------------------------------------------- secp256k1, affine
def parse33(pub: bytes):
    """secp256k1_ec_pubkey_parse on a 33-byte slot: the point, or None"""
    if len(pub) != 33 or pub[0] not in (2, 3):
        return None
    x = int.from_bytes(pub[1:], "big")
    if x >= P:
        return None
    y2 = (x * x * x + 7) % P
    y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2:
        return None
    return x, (y if (y & 1) == (pub[0] & 1) else P - y)


def pubkey(priv: bytes) -> bytes:
    return compress(pt_mul(int.from_bytes(priv, "big"), G))


def ecdh(pub33: bytes, scalar32: bytes):
    """Secp256K1.Ecdh: SHA-256 of the compressed d P, or None where libsecp256k1 returns 0"""
    pt = parse33(pub33)
    d = int.from_bytes(scalar32, "big")
    if pt is None or not 1 <= d < N:
        return None
    return hashlib.sha256(compress(pt_mul(d, pt))).digest()


# ---------------------------------------------------------------- AES-256, byte-oriented
def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11B
        b >>= 1
    return r


def _make_sbox():
    box = []
    for x in range(256):
        inv = next((y for y in range(1, 256) if _gmul(x, y) == 1), 0)
        s = 0
        for bit in range(8):
            v = (inv >> bit) ^ (inv >> ((bit + 4) % 8)) ^ (inv >> ((bit + 5) % 8)) ^ (inv >> ((bit + 6) % 8)) ^ \
                (inv >> ((bit + 7) % 8)) ^ (0x63 >> bit)
            s |= (v & 1) << bit
        box.append(s)
    return box


SBOX = _make_sbox()


def aes256_round_keys(key: bytes):
    assert len(key) == 32
    w = [list(key[4 * i:4 * i + 4]) for i in range(8)]
    rcon = 1
    for i in range(8, 60):
        t = list(w[i - 1])
        if i % 8 == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = _gmul(rcon, 2)
        elif i % 8 == 4:
            t = [SBOX[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - 8], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(15)]


def aes256_encrypt_block(rks, block: bytes) -> bytes:
    s = [a ^ b for a, b in zip(block, rks[0])]                  # column-major: s[4 c + r]
    for rnd in range(1, 15):
        s = [SBOX[b] for b in s]
        s = [s[4 * ((c + r) % 4) + r] for c in range(4) for r in range(4)]          # ShiftRows
        if rnd < 14:
            m = []
            for c in range(4):
                col = s[4 * c:4 * c + 4]
                m += [_gmul(col[r], 2) ^ _gmul(col[(r + 1) % 4], 3) ^ col[(r + 2) % 4] ^ col[(r + 3) % 4]
                      for r in range(4)]
            s = m
        s = [a ^ b for a, b in zip(s, rks[rnd])]
    return bytes(s)


# ---------------------------------------------------------------- GCM
def _ghash_mul(x: int, y: int) -> int:
    z, v = 0, y
    for i in range(128):
        if (x >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ (0xE1 << 120 if v & 1 else 0)
    return z


def _ghash(h: int, data: bytes) -> int:
    y = 0
    for o in range(0, len(data), 16):
        y = _ghash_mul(y ^ int.from_bytes(data[o:o + 16].ljust(16, b"\0"), "big"), h)
    return y


def _gcm(key: bytes, nonce: bytes, data: bytes, c_of):
    """(data xor key stream, tag); c_of picks the ciphertext (what the tag covers) from (input, output)"""
    assert len(key) == 32 and len(nonce) == 16
    rks = aes256_round_keys(key)
    h = int.from_bytes(aes256_encrypt_block(rks, bytes(16)), "big")
    j0 = _ghash(h, nonce + bytes(8) + (128).to_bytes(8, "big"))
    out = bytearray()
    ctr = j0
    for o in range(0, len(data), 16):
        ctr = (ctr & ~0xFFFFFFFF) | ((ctr + 1) & 0xFFFFFFFF)
        ks = aes256_encrypt_block(rks, ctr.to_bytes(16, "big"))
        out += bytes(a ^ b for a, b in zip(data[o:o + 16], ks))
    c = c_of(data, bytes(out))
    pad = (-len(c)) % 16
    s = _ghash(h, c + bytes(pad) + bytes(8) + (8 * len(c)).to_bytes(8, "big"))
    tag = int.from_bytes(aes256_encrypt_block(rks, j0.to_bytes(16, "big")), "big") ^ s
    return bytes(out), tag.to_bytes(16, "big")


def gcm_encrypt(key: bytes, nonce: bytes, pt: bytes) -> bytes:
    """AesGcmEncrypt: nonce || C || tag"""
    c, tag = _gcm(key, nonce, pt, lambda i, o: o)
    return nonce + c + tag


def gcm_decrypt(key: bytes, item: bytes):
    """AesGcmDecrypt of nonce || C || tag: the plaintext, or None (too short, tag mismatch)"""
    if len(item) < 32:
        return None
    pt, tag = _gcm(key, item[:16], item[16:-16], lambda i, o: i)
    return pt if tag == item[-16:] else None


# ---------------------------------------------------------------- the envelope
def secp256k1_encrypt(recipient_pub33: bytes, eph_priv32: bytes, nonce: bytes, pt: bytes):
    """Secp256K1Encrypt with the given ephemeral key and nonce: eph_pub33 || nonce || C || tag, or None"""
    key = ecdh(recipient_pub33, eph_priv32)
    if key is None:
        return None
    return pubkey(eph_priv32) + gcm_encrypt(key, nonce, pt)


def secp256k1_decrypt(priv32: bytes, env: bytes):
    """Secp256K1Decrypt: the plaintext, or None where the reference throws"""
    if len(env) < 65:
        return None
    key = ecdh(env[:33], priv32)
    if key is None:
        return None
    return gcm_decrypt(key, env[33:])
