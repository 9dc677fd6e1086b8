"""CPU test of the model side of the hash-to-G2 / point-decoder edge suite: the operands of tests/h2g2_cases.py populate
every branch the device tests are meant to reach (a condition of the suite: an empty class fails here, with the counts),
and the model (tests/pyref/bls12_381.py) is consistent with itself on them — roots square back, map outputs lie on the
twist, cleared points have order dividing r, and the cofactor constant of the build is #E'(Fp2) / r."""
import collections
import os
import re

import h2g2_cases as C
from pyref import bls12_381 as B

P = B.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _count(labels):
    return dict(collections.Counter(labels))


# ------------------------------------------------------------------------------------------------ coverage
def test_fp_operands_cover_roots_and_edges():
    vals = [v for _, v in C.fp_cases()]
    assert all(0 <= v < P for v in vals)
    for must in (0, 1, 2, 4, P - 1, P - 4, (P + 1) // 2, (P - 1) // 2):
        assert must in vals
    sym = _count(C.legendre(v) for v in vals)
    assert sym.get(1, 0) >= 40 and sym.get(-1, 0) >= 10 and sym.get(0, 0) == 1, sym
    # the word patterns are the Montgomery words the routine sees
    assert all(C.to_m(C.from_m(v)) == v for _, v in C.TC.S)


def test_fp2_operands_populate_every_root_branch():
    counts = _count(C.f2sqrt_branch(x) for _, x in C.fp2_cases())
    for branch in ("zero", "b0-residue", "b0-nonresidue", "try1", "try2", "norm-nonsquare"):
        assert counts.get(branch, 0) >= (1 if branch == "zero" else 5), counts


def test_map_operands_populate_every_branch():
    counts = _count(C.map_branch(t) for _, t in C.t_cases())
    assert counts.get(("norm-zero",), 0) == 1, counts
    # t^2 = -(5 + 4i) would make the map's denominator vanish, but N(5 + 4i) = 41 is a non-residue: no such t exists
    # in Fp2 (h2g2_cases.t_cases adds both roots whenever the model finds one), and the class is empty by arithmetic
    assert C.legendre(41) == -1 and B.f2sqrt(((-5) % P, (-4) % P)) is None
    assert counts.get(("denominator-zero",), 0) == 0, counts
    for sign in ("positive", "negative"):
        for cand in (1, 2, 3):
            assert sum(v for k, v in counts.items() if k[:2] == (sign, cand)) >= 1, counts
    for tr in ("try1", "try2"):
        assert sum(v for k, v in counts.items() if k[-1] == tr) >= 5, counts


def test_messages_populate_every_hash_class():
    msgs = C.messages()
    counts = _count(label for _, label in msgs)
    for cls in C.HASH_CLASSES:
        assert counts.get(cls, 0) >= C.PER_CLASS, (cls, counts)
    assert sorted(len(m) for m, _ in msgs[-7:]) == [0, 111, 112, 127, 128, 239, 240]
    assert len(msgs) <= 64                                 # one-lane hashes on the device: the list stays short


def test_encodings_populate_every_class():
    g1 = _count(C.model_g1(b)[:2] for _, b in C.g1_encodings())
    # accepted by construction: two residue x under both flags and the flag-only string (the order-3 point (0, -2))
    assert g1.get((True, True), 0) == 1 and g1.get((True, False), 0) >= 5 and g1.get((False, False), 0) >= 12, g1
    assert C.model_g1(bytes(47) + b"\x80") == (True, False, (0, P - 2))
    assert pow(P - 4, (P - 1) // 3, P) != 1                 # -4 is no cube: x^3 + 4 = 0 has no solution in Fp
    for sign_b in (False, True):
        g2 = _count(C.model_g2(b, sign_b)[:2] for _, b in C.g2_encodings())
        assert g2.get((True, True), 0) == 0 and g2.get((True, False), 0) >= 12 and g2.get((False, False), 0) >= 20, g2
    kinds = _count(k for _, _, _, k in C.y_zero_points())
    assert kinds.get("y.a=0", 0) >= 2 and kinds.get("y.b=0", 0) >= 2, kinds
    assert any(b == 2 for b, _, _, _ in C.y_zero_points())   # the a^2 = 2/3 construction


# ------------------------------------------------------------------------------------------------ model consistency
def test_model_roots_square_back():
    for name, v in C.fp_cases():
        r = B.sqrt_fp(v)
        assert (r is not None) == (C.legendre(v) >= 0), name
        assert r is None or r * r % P == v, name
    for name, x in C.fp2_cases():
        r = B.f2sqrt(x)
        assert (r is None) == (C.f2sqrt_branch(x) == "norm-nonsquare"), name
        assert r is None or B.f2mul(r, r) == x, name


def test_model_map_outputs_are_on_the_twist():
    for name, t in C.t_cases():
        q = B.map_to_g2_bn(t)
        assert (q is None) == (len(C.map_branch(t)) == 1), name
        assert C.on_twist(q), name


def test_cofactor_constant_is_the_twist_order_over_r():
    text = open(os.path.join(ROOT, "lachain_amd", "csrc", "bls_constants.hpp")).read()
    m = re.search(r"LCB_H2_COFACTOR\[16\] = \{([^}]*)\}", text)
    h2 = C.unwords([int(w.strip().rstrip("u"), 16) for w in m.group(1).split(",")])
    assert h2 == C.H2
    assert int(re.search(r"#define LCB_H2_BITS (\d+)", text).group(1)) == h2.bit_length()
    rest = h2
    for q, e in ((13, 2), (23, 2), (2713, 1), (11953, 1), (262069, 1)):
        assert rest % q ** e == 0 and rest // q ** e % q != 0, q
        rest //= q ** e
    assert len(str(rest)) == 135 and pow(2, rest - 1, rest) == 1      # the large factor (a Fermat test, base 2)
    q = B.map_to_g2_bn((B.fp_hash_of(b"order"), 0))
    assert B.g2_mul(q, h2 * B.R) is None and B.g2_mul(q, h2) is not None


def test_model_clearings():
    z = B.Z
    for name, p in C.clear_points():
        assert C.on_twist(p), name
        h = B.clear_cofactor_g2(p)
        assert C.on_twist(h) and B.g2_mul(h, B.R) is None, name
        # as written in the model: (z^2 - z - 1) P + psi((z - 1) P) + psi^2(2 P), the integers acting through psi
        want = B.g2_add(B.g2_add(B.g2_mul(p, z * z - z - 1), B.g2_psi(B.g2_mul(p, z - 1))),
                        B.g2_psi(B.g2_psi(B.g2_mul(p, 2))))
        assert h == want, name
    small = [(n, p) for n, p in C.clear_points() if n.startswith("order dividing")]
    assert len(small) == 4
    # on order 13 both 64-bit ladders of the clearing leave the generic formulas (the "add equal" case is not met at
    # these exponents for any order dividing 13 * 23)
    for k in (-z, -z + 1):
        assert C.ladder_events(k, 13) >= {"double infinity", "add to infinity", "add inverse"}
    for name, p in small:
        q = int(name.split()[2])
        assert p is not None and B.g2_mul(p, q) is None, name


def test_y_zero_encodings_decode_to_two_points():
    for sign_b, kind in ((False, "y.a=0"), (True, "y.b=0")):
        n = 0
        for b, a, _, k in C.y_zero_points():
            if k != kind:
                continue
            n += 1
            enc = a.to_bytes(48, "little") + b.to_bytes(48, "little")
            flagged = enc[:95] + bytes([enc[95] | 0x80])
            p0, p1 = B.g2_from_bytes(enc, sign_b), B.g2_from_bytes(flagged, sign_b)
            assert p0 != p1 and p0 == B.g2_neg(p1) and C.on_twist(p0)
            assert p0[1][1 if sign_b else 0] == 0
            if not sign_b:
                assert B.g2_to_bytes(p0) == enc and B.g2_to_bytes(p1) == enc      # both re-serialise to the flag-0 bytes
        assert n >= 2
