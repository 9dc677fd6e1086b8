"""tests/pyref/tower.py — TEST INFRASTRUCTURE: a big-integer model of the Fp12 operations of the pairing tower
(field.hpp / pairing.hpp, coop.hpp, asm_tower.hpp), stated on the flat ring of tests/pyref/bls12_381.py,
Fp[w] / (w^12 - 2 w^6 + 2), whose product, power and conjugate share no algorithm with the kernels:

  * Frobenius, inverse, easy part, hard part and final exponentiation are plain powers (e_pow) by the exponent
    that defines them: no Frobenius constant, no norm descent, no cyclotomic squaring, no addition chain;
  * the sparse line of fp12_mul_line_n is expanded to a full element and multiplied by e_mul;
  * the Granger-Scott squaring, which is not a ring operation off the cyclotomic subgroup, is restated as the
    polynomial map it computes, over the Montgomery residues the kernels hold, with unreduced Python integers for the
    double-width sums and one reduction per coefficient at the end.

The kernels see an Fp12 as 144 u32 words: 12 Fp in struct order (c0.c0.a, c0.c0.b, c0.c1.a, ... c1.c2.b; Fp12 =
c0 + c1 w over Fp6 = Fp2[v], v = w^2), each the 12 little-endian limbs of the Montgomery residue m = x R mod p,
R = 2^384.  A "tower" value here is the list of the 12 canonical x in that order.
"""
from . import bls12_381 as B

P, R_ORDER, Z_ABS = B.P, B.R, -B.Z
RM = 1 << 384
RM_INV = pow(RM, -1, P)
HARD_EXP = 3 * (P ** 4 - P ** 2 + 1) // R_ORDER
EASY_EXP = (P ** 6 - 1) * (P ** 2 + 1)
FE_EXP3 = 3 * (P ** 12 - 1) // R_ORDER
assert (P ** 4 - P ** 2 + 1) % R_ORDER == 0 and EASY_EXP * HARD_EXP == FE_EXP3


# ------------------------------------------------------------------------------------------------ conversions
def tower_to_flat(t):
    """the Fp2 coefficient x + y i of v^c w^d stands at t[6 d + 2 c], t[6 d + 2 c + 1] and multiplies w^(2 c + d);
    i = w^6 - 1"""
    e = [0] * 12
    for d in range(2):
        for c in range(3):
            x, y = t[6 * d + 2 * c], t[6 * d + 2 * c + 1]
            e[2 * c + d] = (x - y) % P
            e[2 * c + d + 6] = y % P
    return e


def flat_to_tower(e):
    t = [0] * 12
    for d in range(2):
        for c in range(3):
            y = e[2 * c + d + 6]
            t[6 * d + 2 * c] = (e[2 * c + d] + y) % P
            t[6 * d + 2 * c + 1] = y % P
    return t


def residues_to_words(m):
    """12 Montgomery residues -> the 144 words the kernels read"""
    return [(v >> (32 * j)) & 0xFFFFFFFF for v in m for j in range(12)]


def words_to_residues(w):
    """144 words -> 12 integers as they stand (not reduced: a kernel that leaves a value >= p is seen)"""
    return [sum(w[12 * k + j] << (32 * j) for j in range(12)) for k in range(12)]


def residues_to_flat(m):
    return tower_to_flat([v * RM_INV % P for v in m])


def flat_to_residues(e):
    return [x * RM % P for x in flat_to_tower(e)]


def words_to_flat(w):
    return residues_to_flat(words_to_residues(w))


def flat_to_words(e):
    return residues_to_words(flat_to_residues(e))


def gt_from_bytes(b):
    """the inverse of bls12_381.gt_bytes (576 bytes: 12 canonical Fp, 48 B little-endian, in struct order)"""
    assert len(b) == 576
    t = [int.from_bytes(b[48 * k:48 * k + 48], "little") for k in range(12)]
    assert all(x < P for x in t)
    return tower_to_flat(t)


# ------------------------------------------------------------------------------------------------ the operations
def frob(a, k):
    return B.e_pow(a, P ** k)


def inv(a):
    """a^(p^12 - 2): the inverse, and 0 for 0 (what the kernels' fp_inv = a^(p - 2) gives at the bottom)"""
    return B.e_pow(a, P ** 12 - 2)


def easy(a):
    return B.e_pow(a, EASY_EXP)


def hard(x):
    """for x in the cyclotomic subgroup (mcl's expHardPartBLS12 exponent, three times the minimal one)"""
    return B.e_pow(x, HARD_EXP)


def final_exp(a):
    return B.e_pow(a, FE_EXP3)


def pow_z(x):
    """x^z for unitary x (z = -|z|)"""
    return B.e_conj(B.e_pow(x, Z_ABS))


def line(b, c):
    """1 + b v + c v w as a flat element (b, c canonical Fp2 pairs): v = w^2, v w = w^3"""
    return B.e_add(B.e_one(), B.e_add(B.e_from_f2(b, 2), B.e_from_f2(c, 3)))


def mul_line(a, b, c):
    return B.e_mul(a, line(b, c))


def is_unitary(a):
    return B.e_mul(a, B.e_conj(a)) == B.e_one()


# ------------------------------------------------------------------------------------------------ Granger-Scott
def _fp4_sqr(a, b):
    """(a + b s)^2 over Fp2 with s^2 = xi = 1 + i, unreduced: (a^2 + xi b^2, 2 a b)"""
    a2 = (a[0] * a[0] - a[1] * a[1], 2 * a[0] * a[1])
    b2 = (b[0] * b[0] - b[1] * b[1], 2 * b[0] * b[1])
    ab = (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])
    return (a2[0] + b2[0] - b2[1], a2[1] + b2[0] + b2[1]), (2 * ab[0], 2 * ab[1])


def gs_sqr_residues(m):
    """The map fp12_cyc_sqr (field.hpp) and lcb_r_cyc_sqr (asm_tower.hpp) compute on ANY twelve Fp, stated on the
    Montgomery residues the kernel holds (struct order): with z0, z4, z3 = c0's and z2, z1, z5 = c1's Fp2 coefficients
    and (A, B) = (a^2 + xi b^2, 2 a b) R^-1,
        (t0, t1) = (A, B)(z0, z1):  z0' = 3 t0 - 2 z0,  z1' = 3 t1 + 2 z1
        (t0, t1) = (A, B)(z2, z3),  (t2, t3) = (A, B)(z4, z5):
                                    z4' = 3 t0 - 2 z4,  z5' = 3 t1 + 2 z5,  z2' = 3 xi t3 + 2 z2,  z3' = 3 t2 - 2 z3.
    It equals the square exactly on the cyclotomic subgroup.  The double-width sums of _fp4_sqr are the integers the
    assembly's lazily reduced sums hold (up to an offset of a multiple of p^2): saturated residues give them their
    largest magnitudes.  They stay unreduced, signed, until the one `R^-1 mod p` per coefficient."""
    f2 = lambda k: (m[2 * k], m[2 * k + 1])             # noqa: E731
    z0, z4, z3, z2, z1, z5 = (f2(k) for k in range(6))
    redc = lambda x: tuple(c * RM_INV % P for c in x)    # noqa: E731
    xi = lambda x: (x[0] - x[1], x[0] + x[1])            # noqa: E731
    comb = lambda s, z, sign: tuple((3 * s[k] + sign * 2 * z[k]) % P for k in range(2))   # noqa: E731
    t0, t1 = (redc(x) for x in _fp4_sqr(z0, z1))
    n0, n1 = comb(t0, z0, -1), comb(t1, z1, +1)
    t0, t1 = (redc(x) for x in _fp4_sqr(z2, z3))
    t2, t3 = (redc(x) for x in _fp4_sqr(z4, z5))
    n4, n5 = comb(t0, z4, -1), comb(t1, z5, +1)
    n2, n3 = comb(xi(t3), z2, +1), comb(t2, z3, -1)
    return [c for x in (n0, n4, n3, n2, n1, n5) for c in x]


def gs_sqr(a):
    """gs_sqr_residues on a flat element"""
    return residues_to_flat(gs_sqr_residues(flat_to_residues(a)))
