"""Pins the big-integer tower model (tests/pyref/tower.py) that the device edge tests compare the kernels with: against
the C oracle's Fp12 arithmetic on random values (a different implementation: the Fp2/Fp6/Fp12 tower in Montgomery
form), against the identities that tie its operations together, and against the catalogue's own construction of
unitary operands (tests/tower_cases.py).  No GPU needed."""
import random

import oracle as o
import tower_cases as C
from pyref import bls12_381 as B
from pyref import tower as T

P = B.P


def rand_flat(rng):
    return [rng.randrange(P) for _ in range(12)]


def test_conversions_round_trip():
    rng = random.Random(1)
    for _ in range(4):
        a = rand_flat(rng)
        assert T.tower_to_flat(T.flat_to_tower(a)) == a
        assert T.gt_from_bytes(B.gt_bytes(a)) == a
        w = T.flat_to_words(a)
        assert len(w) == 144 and all(0 <= x < 1 << 32 for x in w)
        assert T.words_to_flat(w) == a
    one = T.flat_to_words(B.e_one())
    assert T.words_to_residues(one) == [T.RM % P] + [0] * 11
    # struct order: the word block k = 6 d + 2 c + j holds coefficient j of v^c w^d = w^(2 c + d); i = w^6 - 1
    for d in range(2):
        for c in range(3):
            t = [0] * 12
            t[6 * d + 2 * c] = 1
            assert T.tower_to_flat(t) == [1 if k == 2 * c + d else 0 for k in range(12)]
            t = [0] * 12
            t[6 * d + 2 * c + 1] = 1
            want = [0] * 12
            want[2 * c + d], want[2 * c + d + 6] = P - 1, 1
            assert T.tower_to_flat(t) == want


def test_model_matches_oracle():
    """gt_mul, gt_pow and final_exp of the C oracle on random values"""
    rng = random.Random(2)
    for _ in range(3):
        a, b = rand_flat(rng), rand_flat(rng)
        assert B.gt_bytes(B.e_mul(a, b)) == o.gt_mul(B.gt_bytes(a), B.gt_bytes(b))
        k = rng.randrange(1 << 64)
        assert B.gt_bytes(B.e_pow(a, k)) == o.gt_pow(B.gt_bytes(a), o.fr(k))
    for _ in range(2):
        a = rand_flat(rng)
        assert B.gt_bytes(T.final_exp(a)) == o.final_exp(B.gt_bytes(a))


def test_model_identities():
    rng = random.Random(3)
    a = rand_flat(rng)
    f1, f2, f3 = T.frob(a, 1), T.frob(a, 2), T.frob(a, 3)
    assert T.frob(f1, 1) == f2 and T.frob(f2, 1) == f3 and T.frob(f1, 2) == f3
    assert T.frob(f3, 3) == B.e_conj(a)                                   # p^6: w -> -w
    assert T.frob(B.e_mul(a, f1), 1) == B.e_mul(f1, f2)
    ai = T.inv(a)
    assert B.e_mul(a, ai) == B.e_one()
    assert ai == C._inv_solve(a)
    assert T.inv(B.e_zero()) == B.e_zero()
    e = T.easy(a)
    assert T.is_unitary(e) and not T.is_unitary(a)
    assert T.hard(e) == T.final_exp(a)
    assert T.pow_z(e) == T.inv(B.e_pow(e, T.Z_ABS))
    assert T.easy(B.e_zero()) == B.e_zero() and T.final_exp(B.e_zero()) == B.e_zero()


def test_line_is_sparse_element():
    rng = random.Random(4)
    b, c = (rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P))
    t = [1, 0] + list(b) + [0] * 4 + list(c) + [0, 0]                   # c0 = (1, b, 0), c1 = (0, c, 0)
    assert T.line(b, c) == T.tower_to_flat(t)
    assert T.line((0, 0), (0, 0)) == B.e_one()


def test_granger_scott_is_the_square_on_unitary_values():
    for u in C.unit():
        a = T.residues_to_flat(u.m)
        assert T.is_unitary(a), u.name
        assert T.gs_sqr(a) == B.e_mul(a, a), u.name
    rng = random.Random(5)
    a = rand_flat(rng)
    assert T.gs_sqr(a) != B.e_mul(a, a)                                   # and not elsewhere
    assert T.gs_sqr(B.e_zero()) == B.e_zero()


def test_catalogue_unit_operands_are_the_models_easy_part():
    """the catalogue builds its unitary operands by a quick route (conjugate over inverse, one power by p^2); they
    must be the model's plain power, and the subfield operands must give 1"""
    src, units = C.unit_sources(), C.unit()
    assert len(units) == 1 + 2 * len(src)
    for k in (0, 3, 5, 6, 11):                                            # SAT and MIX operands: one plain power each
        assert T.residues_to_flat(units[1 + k].m) == T.easy(T.residues_to_flat(src[k].m)), src[k].name
    for k, s in enumerate(src):
        if s.name.startswith("sub"):
            assert T.residues_to_flat(units[1 + k].m) == B.e_one(), s.name
    w6 = T.residues_to_flat(C.sub()[3].m)
    assert B.e_pow(w6, P ** 6 - 1) == T.residues_to_flat(C.special()[2].m)  # w Fp6: -1 on the way


def test_crafted_g1_points():
    pts = C.g1_patterned()
    assert len(pts) == 6 and pts[0][1][0] == 0 and pts[0][1][1] in (2, P - 2)          # the order-3 point
    for (name, (x, y)), pat in zip(pts, C.G1_PATTERNS):
        assert (y * y - x ** 3 - 4) % P == 0
        assert abs(x * T.RM % P - C.SV[pat]) < 4, name                                  # the words are the pattern's
        for yy in (y, P - y):
            enc = B.g1_to_bytes((x, yy))
            assert B.g1_from_bytes(enc) == (None if enc == bytes(48) else (x, yy))
    assert B.g1_mul(pts[0][1], 3) is None


def test_catalogue_shape():
    names = [n for n, _ in C.S]
    for n in ["0", "1", "2", "p-1", "p-2", "(p+1)/2", "(p-1)/2", "R", "p-R", "2^380", "2^380-1", "alt", "~alt"]:
        assert n in names
    for k in range(1, 12):
        assert {f"2^{32 * k}", f"2^{32 * k}-1", f"p-2^{32 * k}"} <= set(names)
    used = {v for c in C.mix() for v in c.m}
    assert {v for _, v in C.S} <= used                                    # every member of S appears in MIX
    assert len(C.basis()) == 36 and len(C.sat()) == 6 and len(C.sub()) == 4
    lines = C.line_operands()
    assert ((0, 0), (0, 0)) in lines
    assert any(c == (0, 0) and b != (0, 0) for b, c in lines) and any(b == (0, 0) and c != (0, 0) for b, c in lines)
    assert {v for _, v in C.S} <= {v for b, c in lines for v in b + c}
    for items in (C.special(), C.sat(), C.sub(), C.basis(), list(range(14)), list(range(105))):
        idx = C.spread(items)
        assert len(idx) % 7 and len(idx) % 64 and set(idx) == set(range(len(items)))
        if len(items) < 28:
            assert all({p % 7 for p, i in enumerate(idx) if i == k} == set(range(7)) for k in range(len(items)))
    assert C.everything() == C.everything()                               # deterministic
