"""The comparisons of the secp256k1 edge tests, shared by tests/test_secp_edges_emul.py (the C++ path compiled for the
CPU) and tests/test_gpu_secp_edges.py (the device, where the field operations are the generated assembly): the
operands of tests/secp_cases.py through the routine switch of lachain_amd/csrc/secp_debug.hpp, against the model
tests/pyref/secp.py.  Every comparison is exact: integers mod p or n, or words.  TEST INFRASTRUCTURE.

A runner is run(op name, a items, b items or None) -> 44-word results (include/lachain_bls.h, lcb_debug_secp_op).
Every check returns the list of failures, launch position included; the tests assert it empty."""
import secp_cases as C
from pyref import secp as S

P, N, W = S.P, S.N, C.W
OPS = {"mul": 0, "sqr": 1, "add": 2, "sub": 3, "neg": 4, "dbl": 5, "canon": 6, "inv": 7, "sqrt": 8, "pred": 9,
       "sc_mont_mul": 10, "sc_mont_inv": 11, "glv_split": 12, "comb_recode": 13, "jac_dbl": 14, "jac_add_aff": 15,
       "jac_add": 16}
IN_WORDS, OUT_WORDS = 25, 44


def item(x=0, y=0, z=0, inf=False):
    return C.words(x) + C.words(y) + C.words(z) + [1 if inf else 0]


def jac_item(j):
    return item(j.x, j.y, j.z, j.inf)


def val(out, k=0):
    return C.from_words(out[8 * k:8 * k + 8])


def digits(out, first, count):
    """`count` signed bytes of the digit area from byte `first`"""
    raw = b"".join(int(w).to_bytes(4, "little") for w in out[26:44])[first:first + count]
    return [b - 256 if b >= 128 else b for b in raw]


def launch(run, op, a_items, b_items=None):
    """one launch in the spread order (every case on more than one lane, never whole waves) -> [(case, position,
    result)]"""
    idx = C.spread(a_items)
    outs = run(op, [a_items[i] for i in idx], None if b_items is None else [b_items[i] for i in idx])
    assert len(outs) == len(idx) and len(idx) % 64 != 0 and all(len(o_) == OUT_WORDS for o_ in outs)
    return [(i, pos, outs[pos]) for pos, i in enumerate(idx)]


# ------------------------------------------------------------------------------------------------ field
FIELD_ITEMS = [item(v) for _, v in C.FIELD]
BINARY = {"mul": lambda a, b: a * b, "add": lambda a, b: a + b, "sub": lambda a, b: a - b}


def check_field_pairs(run, op, sim=None):
    """mul / add / sub on every ordered pair: congruent to the integer result, and (sim: {(i, j): value}) the very
    words the simulated assembly gives"""
    a = [FIELD_ITEMS[i] for i, _ in C.FIELD_PAIRS]
    b = [FIELD_ITEMS[j] for _, j in C.FIELD_PAIRS]
    bad = []
    for k, pos, out in launch(run, op, a, b):
        i, j = C.FIELD_PAIRS[k]
        got, want = val(out), BINARY[op](C.FIELD[i][1], C.FIELD[j][1])
        if got % P != want % P:
            bad.append((op, "value", C.FIELD[i][0], C.FIELD[j][0], pos, hex(got)))
        elif sim is not None and got != sim[i, j]:
            bad.append((op, "words differ from the simulation", C.FIELD[i][0], C.FIELD[j][0], pos, hex(got)))
    return bad


def _unary_ok(op, a, got):
    if op == "sqr":
        return got % P == a * a % P
    if op == "neg":
        return got % P == -a % P
    if op == "dbl":
        return got % P == 2 * a % P
    if op == "canon":
        return got == a % P
    if op == "inv":
        return got % P == 0 if a % P == 0 else a * got % P == 1
    if op == "sqrt":
        return got % P == S.fe_sqrt_candidate(a % P)
    raise AssertionError(op)


def check_field_unary(run, op, sim=None):
    """sqr / neg / dbl / canon / inv / sqrt on every operand (sim: {i: value} for sqr)"""
    bad = []
    for i, pos, out in launch(run, op, FIELD_ITEMS):
        got = val(out)
        if not _unary_ok(op, C.FIELD[i][1], got):
            bad.append((op, "value", C.FIELD[i][0], pos, hex(got)))
        elif sim is not None and got != sim[i]:
            bad.append((op, "words differ from the simulation", C.FIELD[i][0], pos, hex(got)))
    return bad


def check_predicates(run):
    """fe_is_zero(a), fe_is_odd(a), fe_eq(a, b) on every ordered pair: 0 and p, x and x + p are among them"""
    a = [FIELD_ITEMS[i] for i, _ in C.FIELD_PAIRS]
    b = [FIELD_ITEMS[j] for _, j in C.FIELD_PAIRS]
    bad = []
    for k, pos, out in launch(run, "pred", a, b):
        i, j = C.FIELD_PAIRS[k]
        x, y = C.FIELD[i][1] % P, C.FIELD[j][1] % P
        want = (1 if x == 0 else 0) | (2 if x & 1 else 0) | (4 if x == y else 0)
        if out[25] != want:
            bad.append(("pred", C.FIELD[i][0], C.FIELD[j][0], pos, out[25], want))
    return bad


# ------------------------------------------------------------------------------------------------ scalars
def check_sc_mont_mul(run):
    pairs = C.scalar_pairs()
    bad = []
    for k, pos, out in launch(run, "sc_mont_mul", [item(a) for (_, a), _ in pairs], [item(b) for _, (_, b) in pairs]):
        (na, a), (nb, b) = pairs[k]
        if val(out) != S.sc_mont_mul(a, b):
            bad.append(("sc_mont_mul", na, nb, pos, hex(val(out))))
    return bad


def check_sc_mont_inv(run):
    sc = C.scalars()
    return [("sc_mont_inv", sc[k][0], pos, hex(val(out)))
            for k, pos, out in launch(run, "sc_mont_inv", [item(v) for _, v in sc]) if val(out) != S.sc_mont_inv(sc[k][1])]


def check_split(run):
    """k = k1 + k2 lambda (mod n) with both halves below 2^129, and the 33 signed 4-bit digits of each half: within
    [-8, 8], reconstructing the half, nothing above position 32 (the conditions of the CPU test_scalar_split)"""
    lam, _ = C.glv()
    sc = C.raw_scalars()
    bad = []
    for i, pos, out in launch(run, "glv_split", [item(v) for _, v in sc]):
        name, k = sc[i]
        k1 = -val(out, 0) if out[25] & 1 else val(out, 0)
        k2 = -val(out, 1) if out[25] & 2 else val(out, 1)
        if (k1 + k2 * lam - k) % N != 0 or abs(k1) >= 1 << 129 or abs(k2) >= 1 << 129 or out[25] > 3:
            bad.append(("split", name, pos, hex(k1), hex(k2)))
        for half, h in ((0, k1), (1, k2)):
            e = digits(out, 36 * half, 36)
            if not (all(abs(d) <= 8 for d in e) and all(d == 0 for d in e[33:])
                    and sum(d * 16 ** w for w, d in enumerate(e)) == h):
                bad.append(("digits", name, half, pos, e))
    return bad


def check_comb_recode(run):
    """the comb's 33 signed 8-bit digits: int8 range, reconstructing the scalar, nothing above position 32"""
    sc = C.raw_scalars()
    bad = []
    for i, pos, out in launch(run, "comb_recode", [item(v) for _, v in sc]):
        d = digits(out, 0, 36)
        if not (all(x == 0 for x in d[33:]) and d[32] in (0, 1) and sum(x * 256 ** w for w, x in enumerate(d)) == sc[i][1]):
            bad.append(("comb digits", sc[i][0], pos, d))
        if digits(out, 36, 36) != [0] * 36 or any(out[:26]):
            bad.append(("comb digits: stray output", sc[i][0], pos))
    return bad


# ------------------------------------------------------------------------------------------------ points
def _point_bad(out, want):
    """None when the Jacobian result is the model's point: infinity exactly when the model says so, Z != 0 otherwise"""
    if out[24] not in (0, 1):
        return "flag"
    if out[24]:
        return None if want is None and not any(out[:24]) else "flagged infinite"
    if want is None:
        return "not flagged infinite"
    if val(out, 2) % P == 0:
        return "Z = 0 without the flag"
    return None if S.from_jacobian(val(out, 0), val(out, 1), val(out, 2)) == want else "another point"


def check_jac_dbl(run):
    ops = C.jac_operands()
    bad = []
    for i, pos, out in launch(run, "jac_dbl", [jac_item(j) for j in ops]):
        why = _point_bad(out, S.pt_add(ops[i].aff, ops[i].aff))
        if why:
            bad.append(("jac_dbl", ops[i].name, pos, why))
    return bad


def check_jac_add(run, affine):
    pairs = C.aff_pairs() if affine else C.jac_pairs()
    op = "jac_add_aff" if affine else "jac_add"
    bad = []
    for k, pos, out in launch(run, op, [jac_item(a) for _, a, _ in pairs], [jac_item(b) for _, _, b in pairs]):
        cls, a, b = pairs[k]
        why = _point_bad(out, S.pt_add(a.aff, b.aff))
        if why:
            bad.append((op, cls, a.name, b.name, pos, why))
    return bad
