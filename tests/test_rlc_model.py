"""CPU tests of the model of the batch check's random exponents (tests/pyref/rlc.py): its ChaCha20 block against the
RFC 8439 vector, lambda and the exponents' range, the two endomorphisms against the oracle's scalar multiplications on
G1 and G2 (and their difference from them off the subgroups), and the position bins.  tests/test_gpu_rlc_exponents.py
holds the device to this model."""
import oracle as o
from helpers import Drbg, R
from pyref import bls12_381 as B
from pyref import rlc as M

# RFC 8439 §2.3.2: key 00 01 .. 1f, block counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00
RFC_KEY = bytes(range(32))
RFC_WORDS = (1, 0x09000000, 0x4A000000, 0)
RFC_BLOCK = [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3,
             0xC7F4D1C7, 0x0368C033, 0x9AAA2204, 0x4E6CD4C3,
             0x466482D2, 0x09AA9F07, 0x05D7C214, 0xA2028BD9,
             0xD19C12B5, 0xB94E16DE, 0xE883D0CB, 0x4E3C50A2]


def test_chacha_block_rfc8439_vector():
    assert M.chacha_block(RFC_KEY, *RFC_WORDS) == RFC_BLOCK


def test_rlc_scalar_is_words_0_and_1():
    # w12 = ctr, w13 = dom, w14 / w15 = the nonce's halves: the RFC block again
    nonce = RFC_WORDS[2] | (RFC_WORDS[3] << 32)
    assert M.rlc_scalar(RFC_KEY, nonce, RFC_WORDS[0], RFC_WORDS[1]) == (RFC_BLOCK[0], RFC_BLOCK[1])
    # every input word reaches the output
    base = M.rlc_scalar(RFC_KEY, 5, 7, 1)
    assert M.rlc_scalar(RFC_KEY, 5, 8, 1) != base and M.rlc_scalar(RFC_KEY, 5, 7, 0) != base
    assert M.rlc_scalar(RFC_KEY, 6, 7, 1) != base and M.rlc_scalar(RFC_KEY, 5 + (1 << 32), 7, 1) != base
    for j in range(8):
        k = bytearray(RFC_KEY)
        k[4 * j + 3] ^= 0x80
        assert M.rlc_scalar(bytes(k), 5, 7, 1) != base


def test_zero_pair_reads_as_one(monkeypatch):
    monkeypatch.setattr(M, "chacha_block", lambda *a: [0] * 16)
    assert M.rlc_scalar(bytes(32), 0, 0, 0) == (1, 0)
    monkeypatch.setattr(M, "chacha_block", lambda *a: [0, 3] + [0] * 14)
    assert M.rlc_scalar(bytes(32), 0, 0, 0) == (0, 3)


def test_lambda_is_a_cube_root_of_unity_mod_r():
    assert M.LAMBDA == 0xD201000000010000 ** 2 - 1
    assert (M.LAMBDA * M.LAMBDA + M.LAMBDA + 1) % R == 0
    assert B.R == R


def test_exponent_range():
    top = M.exponent(2 ** 32 - 1, 2 ** 32 - 1)
    assert top.bit_length() == 160 and top < R
    assert M.exponent(1, 0) == 1 and M.exponent(0, 1) == M.LAMBDA
    # distinct pairs give distinct exponents: b is the quotient by lambda, a the remainder (a < 2^32 < lambda)
    assert divmod(M.exponent(0xDEADBEEF, 0x12345678), M.LAMBDA) == (0x12345678, 0xDEADBEEF)


def test_generators_and_cube_roots():
    # the model's base points (the standard generators; the library's own are mcl's, other points of the same groups)
    assert o.g1_valid(B.g1_to_bytes(M.G1)) and o.g2_valid(B.g2_to_bytes(M.G2))
    assert (M.G1[1] ** 2 - M.G1[0] ** 3 - B.B1) % B.P == 0
    assert B.f2sub(B.f2mul(M.G2[1], M.G2[1]), B.f2add(B.f2mul(B.f2mul(M.G2[0], M.G2[0]), M.G2[0]), B.B2)) == (0, 0)
    assert B.g1_mul(M.G1, R) is None and B.g2_mul(M.G2, R) is None
    for w in (M.BETA, M.BETA2):
        assert w != 1 and pow(w, 3, B.P) == 1
    assert M.phi(M.G1) == B.g1_mul(M.G1, M.LAMBDA) and M.psi4(M.G2) == B.g2_mul(M.G2, M.LAMBDA)
    # psi^4 from psi's definition (pyref/bls12_381.py g2_psi), on a point that is not the generator
    s = B.g2_mul(M.G2, 0x1234567)
    t = s
    for _ in range(4):
        t = B.g2_psi(t)
    assert M.psi4(s) == t


PAIRS = [(1, 0), (0, 1), (1, 1), (2 ** 32 - 1, 2 ** 32 - 1), (0x80000000, 1), (0xE4E7F110, 0x15593BD1), (0, 0)]


def test_g1_ab_is_the_exponent_on_g1():
    d = Drbg(b"rlc-model-g1")
    for a, b in PAIRS:
        pb = o.g1_mul(o.g1_gen(), o.fr(d.fr_int()))
        want = o.g1_mul(pb, o.fr(M.exponent(a, b) % R))
        assert B.g1_to_bytes(M.g1_ab(B.g1_from_bytes(pb), a, b)) == want, (a, b)
    assert M.g1_ab(None, 5, 7) is None


def test_g2_ab_is_the_exponent_on_g2():
    d = Drbg(b"rlc-model-g2")
    for a, b in PAIRS:
        sb = o.g2_mul(o.g2_gen(), o.fr(d.fr_int()))
        want = o.g2_mul(sb, o.fr(M.exponent(a, b) % R))
        assert B.g2_to_bytes(M.g2_ab(B.g2_from_bytes(sb), a, b)) == want, (a, b)
    assert M.g2_ab(None, 5, 7) is None


def off_subgroup_g1():
    x = 1
    while True:
        y = B.sqrt_fp(x ** 3 + B.B1)
        if y is not None and B.g1_mul((x, y), R) is not None:
            return (x, y)
        x += 1


def off_subgroup_g2():
    k = 1
    while True:
        x = (k, 1)
        y = B.f2sqrt(B.f2add(B.f2mul(B.f2mul(x, x), x), B.B2))
        if y is not None and B.g2_mul((x, y), R) is not None:
            return (x, y)
        k += 1


def test_ab_off_the_subgroups_is_not_the_reduced_exponent():
    """phi and psi^4 act as lambda on the r-torsion only: elsewhere the sum of the two multiples differs from the
    multiple by (a + b lambda) mod r, and the sum is what the batch check forms (and what the pairing argument needs)"""
    a, b = 0xE4E7F110, 0x15593BD1
    e = M.exponent(a, b) % R
    p = off_subgroup_g1()
    assert M.g1_ab(p, a, b) == B.g1_add(B.g1_mul(p, a), B.g1_mul(M.phi(p), b))
    assert M.g1_ab(p, a, b) != B.g1_mul(p, e)
    s = off_subgroup_g2()
    assert M.g2_ab(s, a, b) != B.g2_mul(s, e)
    # the order-3 point (0, -2): phi fixes it, so the sum is (a + b) P
    k3 = (0, B.P - 2)
    assert B.g1_mul(k3, 3) is None and M.phi(k3) == k3
    assert M.g1_ab(k3, 1, 1) == B.g1_mul(k3, 2) and M.g1_ab(k3, 2, 1) is None
    # ... and the r-torsion component is still multiplied by the exponent: [h] (a P + b phi(P)) = [e] [h] P for the
    # cofactor part h killed (here: multiply by the order of the other component's group, #E / r)
    n1 = (B.P + 1 - (B.Z + 1))                       # #E(Fp) = p + 1 - t, t = z + 1
    assert n1 % R == 0 and B.g1_mul(p, n1) is None
    h = n1 // R
    assert B.g1_mul(M.g1_ab(p, a, b), h) == B.g1_mul(B.g1_mul(p, h), e)


def test_bins_runs_and_wrap():
    n_cts = 6
    for ln in (1, 32, 33, 40):
        assert M.tpke_bins([2] * ln, n_cts) == [64 + k % 32 for k in range(ln)]
    # positions wrap at 32 inside a run; the set is the ciphertext's low two bits
    bins = M.tpke_bins([5] * 40 + [4] * 2, n_cts)
    assert bins[31] == 32 + 31 and bins[32] == 32 and bins[39] == 32 + 7 and bins[40:] == [0, 1]


def test_bins_separate_runs_range_and_census_prefix():
    # ciphertext 1 in two separate runs: each run counts from 0
    assert M.tpke_bins([1, 1, 1, 0, 1, 1], 4) == [32, 33, 34, 0, 32, 33]
    # an out-of-range index reads as ciphertext 0, and joins a neighbouring run of ciphertext 0
    assert M.tpke_bins([0, 9, 0, 3, 7], 4) == [0, 1, 2, 96, 0]
    assert M.tpke_bins([4, 4], 4) == [0, 1]                   # 4 is out of range for n_cts = 4
    assert M.tpke_bins([4, 4], 5) == [0, 1]                   # and in range: set 4 & 3 = 0
    assert M.tpke_bins([5, 5], 6) == [32, 33]
    # i0 > 0: the census prefix has no bins, and a run that straddles i0 starts afresh there
    assert M.tpke_bins([2, 2, 2, 2, 3], 4, i0=2) == [None, None, 64, 65, 96]
    assert M.tpke_bins([2] * 70, 4, i0=3)[3:] == [64 + k % 32 for k in range(67)]
