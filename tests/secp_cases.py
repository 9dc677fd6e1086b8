"""Shared operands of the secp256k1 edge tests: tests/test_secp_asm_sim.py (the committed assembly, simulated),
tests/test_secp_edges_emul.py (the C++ path on the CPU) and tests/test_gpu_secp_edges.py (the device).  Deterministic;
nothing is computed here but inputs and, for the coverage assertions of tests/test_secp_asm_sim.py, the class of each
pair from the written definition of the reduction (Python integers only, never the code under test).  Expectations
come from tests/pyref/secp.py.  TEST INFRASTRUCTURE.

A field operand is any value in [0, 2^256): secp.hpp's elements are "weakly reduced", so values >= p are legal inputs.
"""
import collections
import functools
import random

from pyref import secp as S

P, N, C = S.P, S.N, S.C
W = 1 << 256


# ------------------------------------------------------------------------------------------------ field operands
def _limb_mask(m):
    return sum(0xFFFFFFFF << (32 * i) for i in range(8) if (m >> i) & 1)


def _field_values():
    v = [("0", 0), ("1", 1), ("2", 2), ("976", 976), ("977", 977), ("978", 978), ("2^32", 1 << 32), ("C-1", C - 1),
         ("C", C), ("C+1", C + 1), ("p-2", P - 2), ("p-1", P - 1), ("p", P), ("p+1", P + 1), ("p+2", P + 2),
         ("2^256-1", W - 1), ("2^256-2", W - 2), ("2^256-977", W - 977), ("2^256-978", W - 978), ("2^255", 1 << 255),
         ("2^255-1", (1 << 255) - 1), ("2^128", 1 << 128), ("2^128-1", (1 << 128) - 1), ("2^224", 1 << 224),
         ("2^224-1", (1 << 224) - 1)]
    v += [(f"2^256-2^{k}", W - (1 << k)) for k in (1, 31, 32, 33, 64, 96, 128, 224, 255)]
    v += [(f"2^{k}-1", (1 << k) - 1) for k in (32, 33, 64, 65, 96, 160, 192, 223)]
    v += [(f"limbs {m:08b}", _limb_mask(m)) for m in range(0, 256, 5)]
    out, seen = [], set()
    for name, x in v:                                       # the first name of a value stays
        if x not in seen:
            seen.add(x)
            out.append((name, x))
    assert all(0 <= x < W for _, x in out)
    return out


FIELD = _field_values()                                     # [(name, value)]: 88 distinct values
FIELD_PAIRS = [(a, b) for a in range(len(FIELD)) for b in range(len(FIELD))]     # all ordered pairs, as indices


# the written definition of the reduction (the issue's notation): t = a b, lo = t mod 2^256, hi = t div 2^256,
# s = lo + hi C, R = s mod 2^256, k8 = s div 2^256, w = (R + k8 C) div 2^256, result = (R + k8 C) mod 2^256 + w C
Product = collections.namedtuple("Product", "k8 w result")


def product_class(a, b):
    t = a * b
    s = t % W + (t // W) * C
    r, k8 = s % W, s // W
    w = (r + k8 * C) // W
    res = (r + k8 * C) % W + w * C
    assert w <= 1 and res < W and res % P == t % P
    return Product(k8, w, res)


def add_class(a, b):
    """(corrections, weakly reduced result): + C per carry out, twice at most (a + b >= 2^257 - C wraps twice)"""
    s, n = a + b, 0
    while s >= W:
        s, n = s - W + C, n + 1
    assert n <= 2 and s % P == (a + b) % P
    return n, s


def sub_class(a, b):
    """(corrections, result): - C per borrow, twice at most (a - b + 2^256 < C borrows twice)"""
    s, n = a - b, 0
    while s < 0:
        s, n = s + W - C, n + 1
    assert n <= 2 and s % P == (a - b) % P
    return n, s


@functools.lru_cache(maxsize=None)
def coverage():
    """{class name: [pair or operand names]} over FIELD_PAIRS (products, sums, differences) and FIELD (squares)"""
    cov = collections.defaultdict(list)
    for i, j in FIELD_PAIRS:
        (na, a), (nb, b) = FIELD[i], FIELD[j]
        name = f"{na} , {nb}"
        pc = product_class(a, b)
        if pc.w == 1:
            cov["product w=1"].append(name)
            if a < P and b < P:
                cov["product w=1 canonical"].append(name)
        if pc.k8 >= 1 << 32:
            cov["product k8>=2^32"].append(name)
        if pc.k8 == 0:
            cov["product k8=0"].append(name)
        if pc.result >= P:
            cov["product result>=p"].append(name)
        if pc.result == P:
            cov["product result=p"].append(name)
        n, s = add_class(a, b)
        if n >= 1:
            cov["add >=1 correction"].append(name)
        if n == 1:
            cov["add one correction"].append(name)
        if n == 2:
            cov["add two corrections"].append(name)
        if n == 0 and s >= P:
            cov["add no carry, sum>=p"].append(name)
        n, s = sub_class(a, b)
        if n >= 1:
            cov["sub >=1 correction"].append(name)
        if n == 1:
            cov["sub one correction"].append(name)
        if n == 2:
            cov["sub two corrections"].append(name)
    for na, a in FIELD:
        pc = product_class(a, a)
        if pc.w == 1:
            cov["square w=1"].append(na)
        if pc.k8 >= 1 << 32:
            cov["square k8>=2^32"].append(na)
    return dict(cov)


# the counts measured over the 88 values when the catalogue was written: the floor a later edit must keep
COVERAGE_FLOOR = {"product w=1": 64, "product w=1 canonical": 5, "product k8>=2^32": 1600, "product k8=0": 3926,
                  "product result>=p": 252, "product result=p": 173, "square w=1": 6, "square k8>=2^32": 40,
                  "add >=1 correction": 3595, "add one correction": 3558, "add two corrections": 37,
                  "add no carry, sum>=p": 207, "sub >=1 correction": 3828, "sub one correction": 3786,
                  "sub two corrections": 42}


# ------------------------------------------------------------------------------------------------ scalars
def glv():
    """(lambda, (a1, -b1, a2)) from the derivation the recovery tests repeat with Python integers"""
    from test_secp_recover_emul import BASIS, LAMBDA
    a1, b1, a2, _ = BASIS
    return LAMBDA, (a1, -b1, a2)


def _nibbles(pattern, count):
    return sum(d << (4 * k) for k, d in enumerate((pattern * count)[:count]))


@functools.lru_cache(maxsize=None)
def scalars():
    """[(name, value)] below n: the edges of the Montgomery routines, of the split and of both recodings"""
    lam, (a1, mb1, a2) = glv()
    s = [("0", 0), ("1", 1), ("2", 2), ("n-1", N - 1), ("n-2", N - 2), ("(n-1)/2", (N - 1) // 2),
         ("(n+1)/2", (N + 1) // 2), ("lambda", lam), ("lambda-1", lam - 1), ("lambda+1", lam + 1), ("n-lambda", N - lam),
         ("2^128-1", (1 << 128) - 1), ("2^128", 1 << 128), ("2^129-1", (1 << 129) - 1)]
    for name, v in (("a1", a1), ("-b1", mb1), ("a2", a2)):
        s += [(f"{name}{d:+d}" if d else name, v + d) for d in (-1, 0, 1)]
    # halves with zero nibbles, nibbles of 8 (the signed digit's boundary: 8 stays, 9 carries) and runs of 7 / 8 / f
    # that carry through every window: k = k1 + k2 lambda for patterned k1, k2 below 2^124 (well inside the lattice's
    # cell, so the split returns these halves), and with either sign
    halves = [("8..8", _nibbles([8], 31)), ("08..", _nibbles([0, 8], 31)), ("80..", _nibbles([8, 0], 31)),
              ("7f..", _nibbles([15, 7], 31)), ("f..f", _nibbles([15], 31)), ("9..9", _nibbles([9], 31)),
              ("87..", _nibbles([7, 8], 31)), ("0..08", 8), ("10..0", 1 << 120), ("70..08", (7 << 120) + 8)]
    for k, (n1, h1) in enumerate(halves):
        n2, h2 = halves[(k + 3) % len(halves)]
        s.append((f"{n1} + {n2} lambda", (h1 + h2 * lam) % N))
        s.append((f"-{n1} + {n2} lambda", (-h1 + h2 * lam) % N))
        s.append((f"{n1} - {n2} lambda", (h1 - h2 * lam) % N))
    rng = random.Random(0x5EC9)
    s += [(f"random {k}", rng.randrange(N)) for k in range(4)]
    assert all(0 <= v < N for _, v in s) and len({v for _, v in s}) == len(s)
    return s


def raw_scalars():
    """256-bit inputs of the routines specified for any word pattern (the split, the comb's recoding): the scalars
    and the values from n upward"""
    return scalars() + [("n", N), ("n+1", N + 1), ("2^256-1", W - 1), ("2^255", 1 << 255), ("ff00..", _limb_mask(0xAA))]


def scalar_pairs():
    """Montgomery products: every ordered pair of the first fourteen, and each scalar with itself"""
    s = scalars()
    return [(a, b) for a in s[:14] for b in s[:14]] + [(a, a) for a in s[14:]]


# ------------------------------------------------------------------------------------------------ points
Jac = collections.namedtuple("Jac", "name x y z inf aff")     # words of (X, Y, Z), the flag, and the affine point meant
INF = Jac("inf", 0, 0, 0, True, None)
N_EDGE_X = 6


@functools.lru_cache(maxsize=None)
def edge_xs():
    """the six smallest and the six largest x with a point on the curve, found by search"""
    lo, hi, x = [], [], 1
    while len(lo) < N_EDGE_X:
        if S.lift_x(x):
            lo.append(x)
        x += 1
    x = P - 1
    while len(hi) < N_EDGE_X:
        if S.lift_x(x):
            hi.append(x)
        x -= 1
    return lo, hi


MULTIPLES = ["1", "2", "3", "n-1", "n-2", "(n-1)/2", "(n+1)/2", "lambda", "lambda^2"]


@functools.lru_cache(maxsize=None)
def points():
    """[(name, affine point)]: k G for the named k, and both points of every edge x"""
    lam, _ = glv()
    ks = {"1": 1, "2": 2, "3": 3, "n-1": N - 1, "n-2": N - 2, "(n-1)/2": (N - 1) // 2, "(n+1)/2": (N + 1) // 2,
          "lambda": lam, "lambda^2": lam * lam % N}
    out = [(f"{k} G", S.pt_mul(ks[k], S.G)) for k in MULTIPLES]
    lo, hi = edge_xs()
    for x in lo + hi:
        name = f"x={x}" if x < C else f"x=p-{P - x}"
        even, odd = S.lift_x(x)
        out += [(name + " even", even), (name + " odd", odd)]
    assert all(S.on_curve(pt) for _, pt in out)
    return out


_RNG_LAMBDA = random.Random(0x1ACB).randrange(2, P)
FORMS = [("Z=1", 1), ("Z=2", 2), ("Z=p-1", P - 1), ("Z=2^255", 1 << 255), ("Z=p+1", P + 1), ("Z=random", _RNG_LAMBDA)]


def form(name, pt, which):
    """the Jacobian form (x l^2, y l^3, l) of an affine point; l = p + 1 is the weak form of 1 (the words of Z are
    p + 1, X and Y stay)"""
    fname, l = FORMS[which]
    x, y, _ = S.to_jacobian(pt, l)
    return Jac(f"{name} {fname}", x, y, l, False, pt)


def weak_x(name, pt):
    """x + p for x < C (still below 2^256): the affine operand, and X with Z = 1"""
    assert pt[0] < C
    return Jac(f"{name} x+p", pt[0] + P, pt[1], 1, False, pt)


@functools.lru_cache(maxsize=None)
def jac_operands():
    """every point in every form, the weak forms of the small x, and infinity"""
    out = [form(n, pt, k) for n, pt in points() for k in range(len(FORMS))]
    out += [weak_x(n, pt) for n, pt in points() if pt[0] < C]
    return out + [INF]


def _neg(j):
    return Jac("-" + j.name, j.x, (P - j.y) % P, j.z, j.inf, S.pt_neg(j.aff))


@functools.lru_cache(maxsize=None)
def jac_pairs():
    """[(class, P, Q)] for jac_add: Jacobian operands on both sides"""
    pts = points()
    nf = len(FORMS)
    out = []
    for i, (n, pt) in enumerate(pts):
        f0, f1 = i % nf, (i + 1 + i // nf) % nf
        if f1 == f0:
            f1 = (f0 + 1) % nf
        a, b = form(n, pt, f0), form(n, pt, f1)
        out.append(("P+P same form", a, a))
        out.append(("P+P different Z", a, b))
        out.append(("P-P same Z", a, _neg(a)))
        out.append(("P-P different Z", a, _neg(b)))
        out.append(("inf+Q", INF, b))
        out.append(("P+inf", a, INF))
        m, qt = pts[(i + 5) % len(pts)]
        out.append(("generic", a, form(m, qt, f1)))
        out.append(("generic", form(m, qt, f0), b))
        two = S.pt_add(pt, pt)
        out.append(("2P+P", form("2(" + n + ")", two, f1), a))
        out.append(("2P+P", b, form("2(" + n + ")", two, f0)))
        if pt[0] < C:
            wk = weak_x(n, pt)
            out.append(("x equal mod p only: P+P", wk, form(n, pt, 0)))
            out.append(("x equal mod p only: P+P", form(n, pt, f1), wk))
            out.append(("x equal mod p only: P-P", wk, _neg(form(n, pt, 0))))
            out.append(("x equal mod p only: P-P", _neg(form(n, pt, f1)), wk))
            # Z = 1 on the left: u2 = x + p keeps its words, so h = u2 - x is the WORDS of p, zero only mod p
            out.append(("x equal mod p only: P+P", form(n, pt, 0), wk))
            out.append(("x equal mod p only: P-P", _neg(form(n, pt, 0)), wk))
    out.append(("inf+inf", INF, INF))
    lam, _ = glv()
    for k in (1, 2, 3, N - 2, (N - 1) // 2, lam, lam * lam % N - 1, N - 1):       # k G + (k + 1) G; the last is -G + inf
        a, b = S.pt_mul(k, S.G), S.pt_mul((k + 1) % N, S.G)
        fa = form(f"{k:#x} G", a, k % nf)
        fb = INF if b is None else form(f"{k + 1:#x} G", b, (k + 2) % nf)
        out.append(("kG+(k+1)G", fa, fb))
        out.append(("kG+(k+1)G", fb, fa))
    return out


@functools.lru_cache(maxsize=None)
def aff_pairs():
    """[(class, P, Q)] for jac_add_aff: Q is an affine operand (Z = 1; its x may be the weak form)"""
    out = []
    for cls, a, b in jac_pairs():
        if b.inf:
            continue
        if b.z != 1:
            b = Jac(b.name + " as affine", b.aff[0], b.aff[1], 1, False, b.aff)
        out.append((cls, a, b))
    return out


# ------------------------------------------------------------------------------------------------ launches
def spread(items, group=7):
    """after tests/tower_cases.spread, for one lane per item: a short list goes `group` times so that every item
    lands on each of `group` lane positions; a long list goes twice, the second copy shifted off the first one's
    lanes; no launch is a multiple of a wave (a part-filled last wave and block): -> indices into items"""
    n = len(items)
    idx, short = [], n < 4 * group
    for _ in range(group if short else 2):
        idx += list(range(n))
        if len(idx) % 64 == 0 or (short and n % group == 0):
            idx.append(0)
    while len(idx) % 64 == 0:
        idx.append(idx[0])
    return idx


def words(v):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]


def from_words(w):
    return sum(int(x) << (32 * k) for k, x in enumerate(w))
