"""The pairing tower on the device at edge operands (tests/tower_cases.py) against the big-integer model
(tests/pyref/tower.py), through the hooks the library already has:

  lcb_debug_coop_op    ops 0..10: the nine-lane tower (coop.hpp) AND the compiled one-lane tower (field.hpp /
                       pairing.hpp), each compared with the model on its own (a bug the two share must fail), and with
                       each other word for word as before
  lcb_debug_fp12       routines 0..11 of the compiled one-lane tower, one value per launch
  lcb_debug_final_exp  the nine-lane final exponentiation and the assembly one (fe_asm.hpp over asm_tower.hpp)

Every comparison is exact: integers mod p, or words.  Inverses are checked by multiplication (the inverse is unique),
with inv(0) = 0."""
import ctypes
import functools

import pytest

import tower_cases as C
from helpers import gpu_native
from pyref import bls12_381 as B
from pyref import tower as T

pytestmark = pytest.mark.gpu
P = B.P
ONE, ZERO = B.e_one(), B.e_zero()


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


def words(case):
    return T.residues_to_words(case.m)


def flat(case):
    return T.residues_to_flat(case.m)


@functools.lru_cache(maxsize=None)
def _model(op, m):
    a = T.residues_to_flat(list(m))
    if op == "sqr":
        return tuple(B.e_mul(a, a))
    if op.startswith("frob"):
        return tuple(T.frob(a, int(op[4])))
    if op == "conj":
        return tuple(B.e_conj(a))
    if op == "easy":
        return tuple(T.easy(a))
    if op == "hard":
        return tuple(T.hard(a))
    if op == "pow_z":
        return tuple(T.pow_z(a))
    if op == "final_exp":
        return tuple(T.final_exp(a))
    raise AssertionError(op)


def model(op, case):
    return list(_model(op, tuple(case.m)))


def is_inverse(a, got):
    """got == a^-1 by multiplication; 0 for 0"""
    return got == ZERO if a == ZERO else B.e_mul(a, got) == ONE


def coop_run(nat, op, a_cases, b_cases=None):
    """one launch in the spread order -> [(index into a_cases, nine-lane words, one-lane words)]"""
    idx = C.spread(a_cases)
    b_cases = a_cases if b_cases is None else b_cases
    out, ref = nat.debug_coop_op(op, [words(a_cases[i]) for i in idx], [words(b_cases[i]) for i in idx])
    assert len(out) == len(idx) and len(idx) % 7 != 0
    return [(i, out[p], ref[p]) for p, i in enumerate(idx)]


def compare(rows, names, want_of):
    """every launched item: nine-lane == model, one-lane == model (both mod p), nine-lane == one-lane (words)"""
    bad = []
    for p, (i, out, ref) in enumerate(rows):
        want = want_of(i)
        for tower, got in (("nine-lane", out), ("one-lane", ref)):
            ok = want(T.words_to_flat(got)) if callable(want) else T.words_to_flat(got) == want
            if not ok:
                bad.append((tower, names[i], p % 7))
        if out != ref:
            bad.append(("words differ", names[i], p % 7))
    assert not bad, bad[:12]


CLASS_NAMES = list(C.CLASSES)
UNARY = {0: "sqr", 4: "frob1", 5: "frob2", 6: "frob3", 8: "conj"}


@pytest.mark.parametrize("cls", CLASS_NAMES)
@pytest.mark.parametrize("op", sorted(UNARY))
def test_coop_unary_ops(nat, op, cls):
    """sqr12, frob1..3 and conj on every class; BASIS meets every Frobenius constant"""
    cases = C.CLASSES[cls]()
    rows = coop_run(nat, op, cases)
    compare(rows, [c.name for c in cases], lambda i: model(UNARY[op], cases[i]))


@pytest.mark.parametrize("cls", CLASS_NAMES)
def test_coop_inverse(nat, cls):
    cases = C.CLASSES[cls]()
    rows = coop_run(nat, 7, cases)
    compare(rows, [c.name for c in cases], lambda i: functools.partial(is_inverse, flat(cases[i])))


def test_coop_cyclotomic_square(nat):
    """op 1 is defined on the cyclotomic subgroup only: UNIT"""
    cases = C.unit()
    rows = coop_run(nat, 1, cases)
    compare(rows, [c.name for c in cases], lambda i: model("sqr", cases[i]))


PAIRS = None


def pairs(kind):
    global PAIRS
    if PAIRS is None:
        PAIRS = C.pair_classes()
    return PAIRS[kind]


@pytest.mark.parametrize("kind", ["self", "conj", "inverse", "zero", "one", "sat x sat", "basis table"])
@pytest.mark.parametrize("op", [2, 3])
def test_coop_products(nat, op, kind):
    """mul12 and mul12 with conj(a); the SAT x SAT pairs are the worst case of every lazily reduced sum, the BASIS
    table meets every structure constant"""
    ps = pairs(kind)
    a, b = [x for x, _ in ps], [y for _, y in ps]
    rows = coop_run(nat, op, a, b)

    def want(i):
        fa = flat(a[i])
        return B.e_mul(B.e_conj(fa) if op == 3 else fa, flat(b[i]))
    compare(rows, [f"{x.name} * {y.name}" for x, y in ps], want)
    if kind == "inverse" and op == 2:
        assert all(T.words_to_flat(o_) == (ZERO if flat(a[i]) == ZERO else ONE) for i, o_, _ in rows)


def test_coop_line(nat):
    """f (1 + b v + c v w): every catalogue value with a line built on S, every line with saturated values"""
    lines = C.line_operands()
    every = C.everything()
    ps = [(f, lines[k % len(lines)]) for k, f in enumerate(every)]
    ps += [(f, ln) for f in (C.sat()[0], C.sat()[2], C.unit()[3]) for ln in lines]
    a, b = [f for f, _ in ps], [C.line_as_case(ln) for _, ln in ps]
    rows = coop_run(nat, 9, a, b)
    compare(rows, [f"{f.name} line {k}" for k, (f, _) in enumerate(ps)],
            lambda i: T.mul_line(flat(a[i]), *C.line_canonical(ps[i][1])))


FE_SUBSETS = {"special": C.special, "basis": lambda: C.basis()[::4], "sat": C.sat, "sub": C.sub,
              "mix": lambda: C.mix()[:10], "unit": lambda: C.unit()[:10]}


@pytest.mark.parametrize("cls", list(FE_SUBSETS))
def test_coop_final_exp(nat, cls):
    """op 10: at most ten values per class (a model exponentiation is a third of a second)"""
    cases = FE_SUBSETS[cls]()
    assert len(cases) <= 10
    rows = coop_run(nat, 10, cases)
    compare(rows, [c.name for c in cases], lambda i: model("final_exp", cases[i]))


# ------------------------------------------------------------------------------------------------ lcb_debug_fp12
# the reduced catalogue of the one-value-per-launch hook: 0, 1, SAT, BASIS at R mod p, six MIX, and UNIT in three parts
REDUCED ={"special": C.special()[:2], "sat": C.sat(), "basis": C.basis(("R",)), "mix": C.mix()[:6]}
N_UNIT = 1 + 2 * len(C.unit_sources())
UNIT_CHUNKS = [(k, min(k + 11, N_UNIT)) for k in range(0, N_UNIT, 11)]
REDUCED_IDS = list(REDUCED) + [f"unit[{lo}:{hi}]" for lo, hi in UNIT_CHUNKS]


def reduced_group(gid):
    if gid in REDUCED:
        return REDUCED[gid]
    lo, hi = UNIT_CHUNKS[REDUCED_IDS.index(gid) - len(REDUCED)]
    return C.unit()[lo:hi]


def fp12_routine(nat, which, case):
    buf = (ctypes.c_uint32 * 144)(*words(case))
    out = (ctypes.c_uint32 * 144)()
    assert nat.lib().lcb_debug_fp12(which, buf, out) == 0, (which, case.name)
    return list(out)


def fp6_of(t6):
    """six canonical Fp (an Fp6 in struct order) as the flat element with c1 = 0"""
    return T.tower_to_flat(list(t6) + [0] * 6)


ROUTINES_ALL = {0: "inv", 2: "frob1", 3: "frob2", 4: "frob3", 5: "easy", 7: "sqr", 8: "fp6_inv", 9: "fp2_inv",
                10: "conj"}
ROUTINES_UNIT = {1: "sqr", 6: "pow_z", 11: "hard"}


@pytest.mark.parametrize("gid", REDUCED_IDS)
@pytest.mark.parametrize("which", sorted(ROUTINES_ALL))
def test_fp12_routines(nat, which, gid):
    """fp12_inv_n, frob1..3, fe_easy, fp12_sqr_n, fp6_inv (on c0), fp2_inv_n (on c0.c0) and conj of the compiled
    one-lane tower on the reduced catalogue"""
    bad = []
    for c in reduced_group(gid):
        got = fp12_routine(nat, which, c)
        res = [v * T.RM_INV % P for v in T.words_to_residues(got)]            # canonical, struct order
        a = flat(c)
        at = T.flat_to_tower(a)
        if which == 0:
            ok = is_inverse(a, T.tower_to_flat(res))
        elif which in (8, 9):
            k = 6 if which == 8 else 2                                        # the part inverted; the rest is a's
            ok = is_inverse(fp6_of(at[:k] + [0] * (6 - k)), fp6_of(res[:k] + [0] * (6 - k))) and res[k:] == at[k:]
        else:
            ok = T.tower_to_flat(res) == model(ROUTINES_ALL[which], c)
        if not ok:
            bad.append(c.name)
    assert not bad, bad


@pytest.mark.parametrize("chunk", range(len(UNIT_CHUNKS)))
@pytest.mark.parametrize("which", sorted(ROUTINES_UNIT))
def test_fp12_routines_unitary(nat, which, chunk):
    """fp12_cyc_sqr_n, cyc_pow_z and fe_hard are defined on the cyclotomic subgroup: UNIT"""
    lo, hi = UNIT_CHUNKS[chunk]
    bad = [c.name for c in C.unit()[lo:hi]
           if T.words_to_flat(fp12_routine(nat, which, c)) != model(ROUTINES_UNIT[which], c)]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ lcb_debug_final_exp
FE_GROUPS = {"special": C.special, "sub": C.sub, "sat": C.sat, "basis": lambda: C.basis(("R",))}
FE_GROUPS.update({f"mix[{k}:{k + 8}]": (lambda k=k: C.mix()[k:k + 8]) for k in range(0, len(C.mix()), 8)})


@pytest.mark.parametrize("gid", list(FE_GROUPS))
def test_final_exp_three_towers(nat, gid):
    """nine-lane == assembly == model, words between the two device forms"""
    cases = FE_GROUPS[gid]()
    idx = C.spread(cases)
    vals = [words(cases[i]) for i in idx]
    coop = nat.debug_final_exp(vals, coop=True)
    lane = nat.debug_final_exp(vals, coop=False)
    bad = []
    for p, i in enumerate(idx):
        want = model("final_exp", cases[i])
        if T.words_to_flat(coop[p]) != want:
            bad.append(("nine-lane", cases[i].name, p))
        if T.words_to_flat(lane[p]) != want:
            bad.append(("assembly", cases[i].name, p))
        if coop[p] != lane[p]:
            bad.append(("words differ", cases[i].name, p))
    assert not bad, bad[:12]
