"""Shared operands of the pairing-tower edge tests (tests/test_tower_ref.py and the simulator tests on the CPU,
tests/test_gpu_tower_edges.py, tests/test_gpu_asm_tower.py and tests/test_gpu_miller_edges.py on the device).
Deterministic; nothing is computed here but inputs, and no operand is ever filtered out of a comparison:
expectations come from tests/pyref/tower.py.  TEST INFRASTRUCTURE.

An Fp12 operand is the list of the 12 Montgomery residues the kernel sees (struct order c0.c0.a .. c1.c2.b; the
canonical value of a residue m is m R^-1 mod p, R = 2^384): the patterns below are patterns of the WORDS the
carry chains and lazily reduced sums work on."""
import collections
import functools
import random

from pyref import bls12_381 as B
from pyref import tower as T

P = B.P
RP = T.RM % P
W32 = 0xFFFFFFFF
ALT = sum(W32 << (64 * k) for k in range(6))              # words F, 0, F, 0, ...: top word 0, so below p
Case = collections.namedtuple("Case", "name m")            # m: 12 Montgomery residues


# ------------------------------------------------------------------------------------------------ residue patterns S
def _residues():
    s = [("0", 0), ("1", 1), ("2", 2), ("p-1", P - 1), ("p-2", P - 2), ("(p+1)/2", (P + 1) // 2),
         ("(p-1)/2", (P - 1) // 2), ("R", RP), ("p-R", P - RP), ("2^380", 1 << 380), ("2^380-1", (1 << 380) - 1)]
    for k in range(1, 12):
        s += [(f"2^{32 * k}", 1 << (32 * k)), (f"2^{32 * k}-1", (1 << (32 * k)) - 1), (f"p-2^{32 * k}", P - (1 << (32 * k)))]
    s += [("alt", ALT), ("~alt", ((1 << 380) - 1) ^ ALT)]
    assert all(0 <= v < P for _, v in s) and len({v for _, v in s}) == len(s)
    return s


S = _residues()
SV = dict(S)


def _rand12(rng):
    return [rng.randrange(P) for _ in range(12)]


# ------------------------------------------------------------------------------------------------ Fp12 classes
def special():
    return [Case("0", [0] * 12), Case("1", [RP] + [0] * 11), Case("-1", [P - RP] + [0] * 11)]


def basis(residues=("R", "p-1", "2^380-1")):
    """one non-zero coefficient at each of the 12 positions: every Frobenius constant and structure constant"""
    return [Case(f"basis[{k}]={r}", [SV[r] if j == k else 0 for j in range(12)]) for r in residues for k in range(12)]


def sat():
    hi = P - 1
    return [Case("sat p-1", [hi] * 12), Case("sat p-2", [P - 2] * 12), Case("sat 2^380-1", [(1 << 380) - 1] * 12),
            Case("sat c0", [hi] * 6 + [0] * 6), Case("sat c1", [0] * 6 + [hi] * 6),
            Case("sat alternating", [hi if k % 2 == 0 else 0 for k in range(12)])]


def sub():
    """elements of the proper subfields Fp, Fp2, Fp6 (c1 = 0) and of w Fp6 (c0 = 0): the easy part sends the first
    three to 1, the last to 1 by way of -1"""
    rng = random.Random(0x5B)
    r = _rand12(rng)
    return [Case("sub Fp", r[:1] + [0] * 11), Case("sub Fp2", r[1:3] + [0] * 10), Case("sub Fp6", r[3:9] + [0] * 6),
            Case("sub wFp6", [0] * 6 + _rand12(rng)[:6])]


def mix():
    """random elements with one to three coefficients replaced, cycling through S (every member appears) and
    through the 12 positions"""
    rng = random.Random(0x31C5)
    out, k, pos = [], 0, 0
    while k < len(S):
        m, names = _rand12(rng), []
        for _ in range(len(out) % 3 + 1):
            name, v = S[k % len(S)]
            m[pos % 12] = v
            names.append(f"{pos % 12}:{name}")
            k += 1
            pos += 5                                         # 5 is coprime to 12
        out.append(Case("mix " + " ".join(names), m))
    return out


def s_dense():
    """every member of S in four elements, twelve patterned coefficients each (the simulator tests, where one routine
    call costs what hundreds cost on the device)"""
    v = [x for _, x in S]
    return [Case(f"S[{k}:{k + 12}]", [v[(k + j) % len(v)] for j in range(12)]) for k in range(0, len(v), 12)]


def _inv_solve(a):
    """a^-1 by elimination on the 12 x 12 matrix of x -> a x (an operand generator, not an expectation: callers
    assert a * result == 1)"""
    cols = []
    for j in range(12):
        wj = [0] * 12
        wj[j] = 1
        cols.append(B.e_mul(a, wj))
    m = [[cols[j][i] for j in range(12)] + [1 if i == 0 else 0] for i in range(12)]
    for c in range(12):
        piv = next(r for r in range(c, 12) if m[r][c])
        m[c], m[piv] = m[piv], m[c]
        iv = pow(m[c][c], -1, P)
        m[c] = [x * iv % P for x in m[c]]
        for r in range(12):
            if r != c and m[r][c]:
                f = m[r][c]
                m[r] = [(x - f * y) % P for x, y in zip(m[r], m[c])]
    x = [m[i][12] for i in range(12)]
    assert B.e_mul(a, x) == B.e_one()
    return x


def inverse_of(case):
    """the operand a^-1 of the pair (a, a^-1); 0 for 0"""
    a = T.residues_to_flat(case.m)
    if not any(a):
        return Case("inv " + case.name, [0] * 12)
    return Case("inv " + case.name, T.flat_to_residues(_inv_solve(a)))


def conj_of(case):
    return Case("conj " + case.name, case.m[:6] + [(P - v) % P for v in case.m[6:]])


def _easy_operand(case):
    """the easy-part image as an operand: (conj a / a)^(p^2 + 1), asserted unitary here and pinned against the
    model's plain power in tests/test_tower_ref.py"""
    a = T.residues_to_flat(case.m)
    t = B.e_mul(B.e_conj(a), _inv_solve(a))
    u = B.e_mul(B.e_pow(t, P * P), t)
    assert T.is_unitary(u)
    return Case("easy " + case.name, T.flat_to_residues(u))


N_UNIT_MIX = 6


@functools.lru_cache(maxsize=None)
def _unit():
    src = sat() + mix()[:N_UNIT_MIX] + sub()
    img = [_easy_operand(c) for c in src]
    return tuple([special()[1]] + img + [conj_of(c) for c in img])


def unit():
    """1, the easy-part images of the SAT, MIX (the first six) and SUB operands, and their conjugates: all of the
    cyclotomic subgroup"""
    return list(_unit())


def unit_sources():
    return sat() + mix()[:N_UNIT_MIX] + sub()


CLASSES = {"special": special, "basis": basis, "sat": sat, "sub": sub, "mix": mix, "dense": s_dense, "unit": unit}


def everything():
    return [c for f in CLASSES.values() for c in f()]


# ------------------------------------------------------------------------------------------------ pairs
ZERO, ONE = special()[0], special()[1]


def pair_classes(cases=None):
    """{name: [(a, b)]} for the binary operations"""
    cases = everything() if cases is None else cases
    s, b = sat(), basis(("R",))
    return {
        "self": [(a, a) for a in cases],
        "conj": [(a, conj_of(a)) for a in cases],
        "inverse": [(a, inverse_of(a)) for a in cases],
        "zero": [(a, ZERO) for a in cases] + [(ZERO, a) for a in s],
        "one": [(a, ONE) for a in cases] + [(ONE, a) for a in s],
        "sat x sat": [(x, y) for x in s for y in s],
        "basis table": [(x, y) for x in b for y in b],
    }


# ------------------------------------------------------------------------------------------------ line operands
def line_operands():
    """(b, c): Fp2 pairs of Montgomery residues built on S, with (0, 0), (b, 0) and (0, c)"""
    f2 = [(S[k][1], S[(7 * k + 3) % len(S)][1]) for k in range(len(S))]         # every member as a and as b
    hi = (P - 1, P - 1)
    out = [((0, 0), (0, 0)), (hi, (0, 0)), ((0, 0), hi), (hi, hi), ((RP, 0), (0, 0)), ((0, 0), (RP, 0)),
           ((0, RP), (0, RP)), (((1 << 380) - 1,) * 2, ((1 << 380) - 1,) * 2)]
    out += [(f2[k], f2[(k + 11) % len(f2)]) for k in range(len(f2))]
    out += [(f2[k], (0, 0)) for k in range(0, len(f2), 5)] + [((0, 0), f2[k]) for k in range(2, len(f2), 5)]
    return out


def line_as_case(bc):
    """the line's coefficients as an Fp12 operand: b at Fp2 coefficient 0, c at coefficient 1 (the hooks read them
    there)"""
    b, c = bc
    return Case("line", [b[0], b[1], c[0], c[1]] + [0] * 8)


def line_canonical(bc):
    return tuple(tuple(v * T.RM_INV % P for v in x) for x in bc)


# ------------------------------------------------------------------------------------------------ crafted G1 points
G1_PATTERNS = ["0", "p-1", "2^380-1", "alt", "2^352-1", "p-2^32"]


def g1_patterned():
    """[(name, (x, y))]: on-curve points of y^2 = x^3 + 4 whose x has the Montgomery words of a member of S (a share
    U_i is any on-curve point, so its words are the adversary's choice).  The pattern is stepped (+1) until x^3 + 4
    is a square (-1 next to p); x = 0 gives the point of order 3.  y is the root sqrt_fp returns; callers use both
    signs."""
    out = []
    for name in G1_PATTERNS:
        m, step = SV[name], (-1 if SV[name] > P - 64 else 1)
        while True:
            x = m * T.RM_INV % P
            y = B.sqrt_fp(x ** 3 + 4)
            if y is not None:
                break
            m += step
        out.append((name if m == SV[name] else f"{name}{m - SV[name]:+d}", (x, y)))
    return out


# ------------------------------------------------------------------------------------------------ launches
def spread(items, group=7):
    """a launch order in which every item of a short list, and every run of `group` neighbours of a long one, lands
    on each of `group` positions (the nine-lane kernels hold seven values per wave), with a part-filled last
    block: -> indices into items"""
    n = len(items)
    if n >= 4 * group:
        idx = list(range(n))
    else:
        idx = []
        for _ in range(group):
            idx += list(range(n))
            if n % group == 0:
                idx.append(0)
    while len(idx) % group == 0 or len(idx) % 64 == 0:
        idx.append(idx[0])
    return idx
