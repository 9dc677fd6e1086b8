"""tests/pyref/rlc.py — TEST INFRASTRUCTURE: a plain-Python model of the random exponents of the randomized batch check
(lachain_amd/csrc/rlc_common.hpp, the header of k_batch.hip), restated from those comments and from RFC 8439, not
from the kernels' code.

A share's exponent is s = a + b lambda with (a, b) the first two words of one ChaCha20 block: the key is the call's 32
secret bytes, word 12 a counter (the share's index, or its bin), word 13 a domain (0: per share, 1: per group position),
words 14 and 15 the call's nonce.  lambda = z^2 - 1 is the eigenvalue of phi(x, y) = (beta x, y) on G1 and of
psi^4(x, y) = (beta' x, y) on G2, so the multiple is formed as a P + b phi(P) with 32-bit a and b.  The model forms
exactly that sum on affine big-integer points (pyref/bls12_381.py): for a point outside the r-torsion (the wire accepts
such points) it is NOT [(a + b lambda) mod r] P.  The cube roots beta and beta' are found here, as the ones for which
the endomorphism acts as lambda on the generators; nothing is taken from the library's constants.
"""
from pyref import bls12_381 as B

MASK = 0xFFFFFFFF
Z_ABS = 0xD201000000010000
LAMBDA = Z_ABS * Z_ABS - 1

DOM_SHARE = 0           # counter = the share's index
DOM_POS = 1             # counter = the share's bin, 32 set + pos
POS_CAP = 32            # positions per level-1 group
POS_SETS = 4            # a group of ciphertext c uses set c & 3

# the generators of G1 and G2 (draft-irtf-cfrg-pairing-friendly-curves, BLS12-381)
G1 = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
      0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
G2 = ((0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
       0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
      (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
       0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE))


# ------------------------------------------------------------------------------------------------ ChaCha20 (RFC 8439)
def _rotl(x, r):
    return ((x << r) & MASK) | (x >> (32 - r))


def _quarter(s, a, b, c, d):
    s[a] = (s[a] + s[b]) & MASK; s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & MASK; s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b]) & MASK; s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & MASK; s[b] = _rotl(s[b] ^ s[c], 7)


def chacha_block(key32, w12, w13, w14, w15):
    """the RFC 8439 §2.3 block function on constants || key (eight little-endian words) || w12..w15 -> 16 words"""
    assert len(key32) == 32
    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574]
    init += [int.from_bytes(key32[4 * j:4 * j + 4], "little") for j in range(8)]
    init += [w12 & MASK, w13 & MASK, w14 & MASK, w15 & MASK]
    s = list(init)
    for _ in range(10):
        _quarter(s, 0, 4, 8, 12)
        _quarter(s, 1, 5, 9, 13)
        _quarter(s, 2, 6, 10, 14)
        _quarter(s, 3, 7, 11, 15)
        _quarter(s, 0, 5, 10, 15)
        _quarter(s, 1, 6, 11, 12)
        _quarter(s, 2, 7, 8, 13)
        _quarter(s, 3, 4, 9, 14)
    return [(x + y) & MASK for x, y in zip(s, init)]


def rlc_scalar(key32, nonce, ctr, dom):
    """(a, b): words 0 and 1 of the block (ctr, dom, nonce low, nonce high); never (0, 0), which reads as (1, 0)"""
    blk = chacha_block(key32, ctr, dom, nonce & MASK, (nonce >> 32) & MASK)
    a, b = blk[0], blk[1]
    return (1, 0) if a == 0 and b == 0 else (a, b)


def exponent(a, b):
    return a + b * LAMBDA


# ------------------------------------------------------------------------------------------------ TPKE positions
def tpke_bins(ct_idx, n_cts, i0=0):
    """per share its bin 32 (c & 3) + (offset in its run of equal ciphertext index) mod 32; shares below i0 (the census
    prefix) have none, and runs start afresh at i0.  An out-of-range index reads as ciphertext 0."""
    cs = [c if c < n_cts else 0 for c in ct_idx]
    bins = [None] * len(cs)
    start = i0
    for i in range(i0, len(cs)):
        if i > i0 and cs[i] != cs[i - 1]:
            start = i
        bins[i] = POS_CAP * (cs[i] & (POS_SETS - 1)) + (i - start) % POS_CAP
    return bins


# ------------------------------------------------------------------------------------------------ the endomorphisms
def _cube_roots():
    """the two primitive cube roots of unity in Fp: (-1 +- sqrt(-3)) / 2"""
    s = B.sqrt_fp(-3 % B.P)
    assert s is not None
    half = B.inv(2)
    return [(-1 + s) * half % B.P, (-1 - s) * half % B.P]


def _pick(roots, apply, mul, gen):
    want = mul(gen, LAMBDA)
    hits = [w for w in roots if apply(gen, w) == want]
    assert len(hits) == 1, "exactly one cube root makes the endomorphism act as lambda"
    return hits[0]


def _phi_with(p, w):
    return None if p is None else (p[0] * w % B.P, p[1])


def _psi4_with(p, w):
    return None if p is None else ((p[0][0] * w % B.P, p[0][1] * w % B.P), p[1])


BETA = _pick(_cube_roots(), _phi_with, B.g1_mul, G1)          # phi(G1) = [lambda] G1
BETA2 = _pick(_cube_roots(), _psi4_with, B.g2_mul, G2)        # psi^4(G2) = [lambda] G2


def phi(p):
    """(x, y) -> (beta x, y) on E(Fp)"""
    return _phi_with(p, BETA)


def psi4(p):
    """(x, y) -> (beta' x, y) on E'(Fp2): the fourth power of psi"""
    return _psi4_with(p, BETA2)


def g1_ab(p, a, b):
    """a P + b phi(P) for an affine point of E(Fp) (None: infinity), as a sum of the two multiples"""
    return B.g1_add(B.g1_mul(p, a), B.g1_mul(phi(p), b))


def g2_ab(s, a, b):
    """a S + b psi^4(S) for an affine point of E'(Fp2)"""
    return B.g2_add(B.g2_mul(s, a), B.g2_mul(psi4(s), b))
