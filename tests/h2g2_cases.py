"""Shared operands of the hash-to-G2 and point-decoder edge tests (tests/test_h2g2_ref.py on the CPU,
tests/test_gpu_h2g2_edges.py and tests/test_gpu_parity.py on the device).  Deterministic; nothing is computed here but
inputs, the branch each input takes (so that the CPU test can assert every branch is populated) and conversions between
Python integers and the words of lcb_debug_h2g2_op.  No operand is ever filtered out of a comparison: expectations come
from tests/pyref/bls12_381.py (sqrt_fp, f2sqrt, fp_hash_of, map_to_g2_bn, clear_cofactor_g2, g1_from_bytes,
g2_from_bytes).  TEST INFRASTRUCTURE.

A field operand of the hook is the 12 Montgomery words the routine sees: m = a R mod p, R = 2^384."""
import functools
import hashlib
import random

import tower_cases as TC
from pyref import bls12_381 as B

P = B.P
RM = 1 << 384
RINV = pow(RM, -1, P)
Z = B.Z
# #E'(Fp2) = h2 r with h2 = (z^8 - 4 z^7 + 5 z^6 - 4 z^4 + 6 z^3 - 4 z^2 - 4 z + 13) / 9 (the BLS12 twist-order polynomial)
_H2_NUM = Z ** 8 - 4 * Z ** 7 + 5 * Z ** 6 - 4 * Z ** 4 + 6 * Z ** 3 - 4 * Z ** 2 - 4 * Z + 13
assert _H2_NUM % 9 == 0
H2 = _H2_NUM // 9
# h2 = 13^2 23^2 2713 11953 262069 (a 135-digit cofactor that passes a Fermat test): tests/test_h2g2_ref.py


# ------------------------------------------------------------------------------------------------ words
def to_m(a): return a * RM % P
def from_m(m): return m * RINV % P
def words(v, n=12): return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(n)]
def unwords(w): return sum(int(x) << (32 * k) for k, x in enumerate(w))
def fp_item(a): return words(to_m(a))
def fp2_item(x): return words(to_m(x[0])) + words(to_m(x[1]))
def fp_of(w): return from_m(unwords(w[:12]))
def fp2_of(w): return (from_m(unwords(w[:12])), from_m(unwords(w[12:24])))
def raw_words(w): return unwords(w)                        # the words as they are: for the canonical (< p) checks
def point_item(p): return fp2_item(p[0]) + fp2_item(p[1])


def bytes_item(b):
    b = bytes(b) + bytes(-len(b) % 4)
    return [int.from_bytes(b[4 * k:4 * k + 4], "little") for k in range(len(b) // 4)]


def jac_to_affine(w):
    """72 words (X, Y, Z) -> affine point, None for Z = 0"""
    x, y, z = fp2_of(w[0:24]), fp2_of(w[24:48]), fp2_of(w[48:72])
    if z == (0, 0):
        return None
    zi = B.f2inv(z)
    zi2 = B.f2mul(zi, zi)
    return (B.f2mul(x, zi2), B.f2mul(y, B.f2mul(zi2, zi)))


def g1_jac_to_affine(w):
    """36 words (X, Y, Z) -> affine G1 point, None for Z = 0"""
    x, y, z = fp_of(w[0:12]), fp_of(w[12:24]), fp_of(w[24:36])
    if z == 0:
        return None
    zi = B.inv(z)
    return (x * zi * zi % P, y * zi * zi * zi % P)


def legendre(a):
    a %= P
    return 0 if a == 0 else (1 if pow(a, (P - 1) // 2, P) == 1 else -1)


def g_twist(x): return B.f2add(B.f2mul(B.f2mul(x, x), x), B.B2)
def on_twist(p): return p is None or B.f2mul(p[1], p[1]) == g_twist(p[0])


# ------------------------------------------------------------------------------------------------ Fp operands
def _dedup(cases):
    seen, out = set(), []
    for name, v in cases:
        if v not in seen:
            seen.add(v)
            out.append((name, v))
    return out


@functools.lru_cache(None)
def fp_cases():
    """(name, canonical value): edge values, the word patterns of tower_cases.S taken as Montgomery residues, and the
    square of every one of them (an operand with a known root)"""
    base = [("0", 0), ("1", 1), ("2", 2), ("4", 4), ("p-1", P - 1), ("p-4", P - 4), ("(p+1)/2", (P + 1) // 2),
            ("(p-1)/2", (P - 1) // 2), ("9", 9), ("16", 16), ("25", 25), ("8", 8), ("18", 18), ("50", 50)]
    base += [("m:" + name, from_m(v)) for name, v in TC.S]
    return _dedup(base + [(f"({name})^2", v * v % P) for name, v in base])


# ------------------------------------------------------------------------------------------------ Fp2 operands
def _fp2_edge_set():
    e = [0, 1, 2, P - 1, (P + 1) // 2, from_m((1 << 380) - 1), from_m(TC.ALT)]
    return [(a, b) for a in e for b in e]


def f2sqrt_branch(x):
    """the branch of the model's f2sqrt (mcl's Fp2::squareRoot) that x takes — a label for the coverage assertions of
    tests/test_h2g2_ref.py, never an expectation"""
    a, b = x
    if b == 0:
        if a == 0:
            return "zero"
        return "b0-residue" if legendre(a) == 1 else "b0-nonresidue"
    c = B.sqrt_fp(a * a + b * b)
    if c is None:
        return "norm-nonsquare"
    return "try1" if legendre((a + c) * B.inv(2)) == 1 else "try2"


@functools.lru_cache(None)
def fp2_cases():
    """(name, (a, b)) for the three Fp2 roots"""
    rng = random.Random(0x2F5C)
    res = [a for a in range(2, 40) if legendre(a) == 1][:4]
    non = [a for a in range(2, 40) if legendre(a) == -1][:4]
    out = [("0", (0, 0)), ("1", (1, 0)), ("-1", (P - 1, 0)), ("i", (0, 1)), ("-i", (0, P - 1))]
    out += [(f"({a},0) residue", (a, 0)) for a in res + [from_m((1 << 380) - 1) ** 2 % P]]
    out += [(f"({a},0) non-residue", (a, 0)) for a in non + [P - 4, P - 9]]
    out += [(f"(0,{b})", (0, b)) for b in (2, 3, P - 2, (P + 1) // 2, from_m(TC.ALT))]
    out += [(f"y^2 y=({y[0] % 1000},{y[1] % 1000})#{k}", B.f2mul(y, y)) for k, y in enumerate(_fp2_edge_set())]
    rnd = [(rng.randrange(P), rng.randrange(P)) for _ in range(24)]
    out += [(f"random square {k}", B.f2mul(y, y)) for k, y in enumerate(rnd)]
    out += [(f"random non-square {k}", B.f2mul(B.f2mul(y, y), B.XI)) for k, y in enumerate(rnd[:12])]   # N(xi) = 2
    out += [(f"random {k}", (rng.randrange(P), rng.randrange(P))) for k in range(12)]
    pat = [from_m(TC.SV[n]) for n in ("p-1", "2^380-1", "alt", "~alt", "p-2^352", "2^32-1")]
    out += [(f"patterns {i},{j}", (pat[i], pat[j])) for i in range(len(pat)) for j in range(len(pat))]
    return _dedup(out)


# ------------------------------------------------------------------------------------------------ t for the map
def map_candidates(t):
    """the three SvdW candidates of the model's map_to_g2_bn, restated for the coverage labels only"""
    den = B.f2add(B.f2add(B.f2mul(t, t), B.B2), (1, 0))
    w = B.f2mul(B.f2mul(B.f2inv(den), (B._SQRT_M3, 0)), t)
    x1 = B.f2add(B.f2neg(B.f2mul(t, w)), (B._HALF_M1_SQRT_M3, 0))
    x2 = B.f2sub(B.f2neg(x1), (1, 0))
    x3 = B.f2add(B.f2inv(B.f2mul(w, w)), (1, 0))
    return x1, x2, x3


def map_branch(t):
    """(failure reason) or (sign of N(t), chosen candidate 1..3, f2sqrt branch of its g(x)) — a label, as above"""
    leg = legendre(t[0] * t[0] + t[1] * t[1])
    if leg == 0:
        return ("norm-zero",)
    if B.f2add(B.f2add(B.f2mul(t, t), B.B2), (1, 0)) == (0, 0):
        return ("denominator-zero",)
    for k, x in enumerate(map_candidates(t)):
        br = f2sqrt_branch(g_twist(x))
        if br != "norm-nonsquare" and B.f2sqrt(g_twist(x)) is not None:
            return ("negative" if leg < 0 else "positive", k + 1, br)
    return ("no-candidate",)


@functools.lru_cache(None)
def t_cases():
    rng = random.Random(0x7A11)
    out = [("0", (0, 0)), ("1", (1, 0)), ("-1", (P - 1, 0)), ("i", (0, 1)), ("-i", (0, P - 1))]
    r = B.f2sqrt(((-5) % P, (-4) % P))                     # t^2 + 4(1 + i) + 1 = 0: the map's denominator vanishes
    if r is not None:
        out += [("sqrt(-(5+4i))", r), ("-sqrt(-(5+4i))", B.f2neg(r))]
    out += [(f"hash form {k}", (B.fp_hash_of(b"t-case-%d" % k), 0)) for k in range(12)]
    out += [(f"({a},0)", (a, 0)) for a in (2, 3, P - 2, (P - 1) // 2, from_m((1 << 380) - 1))]
    out += [(f"general {k}", (rng.randrange(P), rng.randrange(P))) for k in range(40)]
    pat = [from_m(TC.SV[n]) for n in ("p-1", "2^380-1", "alt", "~alt")]
    out += [(f"patterns {i},{j}", (pat[i], pat[j])) for i in range(4) for j in range(4)]
    return _dedup(out)


# ------------------------------------------------------------------------------------------------ points for the clearings
@functools.lru_cache(None)
def clear_points():
    """(name, affine point on the twist): map outputs of both signs, points already in G2, and points of small order
    [#E' / q] Q, q | h2 (a short ladder over one meets the doubling, inverse and infinity cases of the additions)"""
    n_twist = H2 * B.R
    mapped = []
    for name, t in t_cases():
        q = B.map_to_g2_bn(t)
        if q is not None:
            mapped.append((name, q))
    out = [("map " + name, q) for name, q in mapped[:6]]
    neg = [(name, q) for name, q in mapped if map_branch(dict(t_cases())[name])[0] == "negative"]
    out += [("map " + name, q) for name, q in neg[:2]]
    in_g2 = B.clear_cofactor_g2(mapped[0][1])
    out += [("in G2", in_g2), ("in G2, doubled", B.g2_add(in_g2, in_g2))]
    # 13^2 and 23^2 divide #E', and [#E' / 13] Q is infinity for every Q tried: the 13-part is not cyclic, so the whole
    # power is taken out and the multiple has order q or 1 (tests/test_h2g2_ref.py asserts it is q)
    for q, part in ((13, 13 * 13), (23, 23 * 23), (13 * 23, 13 * 13 * 23 * 23), (2713, 2713)):
        name, pt = mapped[len(out) % len(mapped)]
        out.append((f"order dividing {q} from map {name}", B.g2_mul(pt, n_twist // part)))
    return out


def ladder_events(k, q):
    """the special cases a left-to-right double-and-add ladder [k] P from acc = P (g2_mul_u64_z1_inl, jac_mul_u64_inl,
    pt_mul_u64) meets on a point of order q — a label for tests/test_h2g2_ref.py, from the multiples of P mod q"""
    acc, ev = 1 % q, set()
    for i in range(k.bit_length() - 2, -1, -1):
        if acc == 0:
            ev.add("double infinity")
        acc = acc * 2 % q
        if (k >> i) & 1:
            if acc == 0:
                ev.add("add to infinity")
            elif acc == 1 % q:
                ev.add("add equal")
            elif acc == (q - 1) % q:
                ev.add("add inverse")
            acc = (acc + 1) % q
    return ev


# ------------------------------------------------------------------------------------------------ messages
def hash_branch(msg):
    """(second mask taken, chosen candidate, f2sqrt branch) of G2.SetHashOf(msg) — a label, as above"""
    d = hashlib.sha512(msg).digest()
    masked = (int.from_bytes(d[:48], "little") & ((1 << 381) - 1)) >= P
    br = map_branch((B.fp_hash_of(msg), 0))
    return (masked,) + tuple(br[1:])


HASH_CLASSES = [(m, c, t) for m in (False, True) for c in (1, 2, 3) for t in ("try1", "try2")]
PER_CLASS = 2
SCAN_LIMIT = 4000


@functools.lru_cache(None)
def messages():
    """short messages b"h2g2-<i>", the first PER_CLASS of every class of HASH_CLASSES in order of i (the scan stops when
    every class is full, or at SCAN_LIMIT), then the SHA-512 padding lengths; [(message, label)]"""
    count = {c: 0 for c in HASH_CLASSES}
    out = []
    for i in range(SCAN_LIMIT):
        m = b"h2g2-%d" % i
        br = hash_branch(m)
        if br in count and count[br] < PER_CLASS:
            count[br] += 1
            out.append((m, br))
            if all(v >= PER_CLASS for v in count.values()):
                break
    for n in (0, 111, 112, 127, 128, 239, 240):
        m = bytes((7 * k + n) & 0xFF for k in range(n))
        out.append((m, hash_branch(m)))
    return out


@functools.lru_cache(None)
def digests():
    """(name, 64 bytes) for fp_set_hash_digest: the digests of the messages, and first-48-byte values around the two
    masks and p (bits 381..383 set and clear; the last 16 bytes are never read)"""
    out = [(repr(m[:12]), hashlib.sha512(m).digest()) for m, _ in messages()]
    top = 7 << 381
    for name, v in (("0", 0), ("p-1", P - 1), ("p", P), ("p+1", P + 1), ("2^380-1", (1 << 380) - 1), ("2^380", 1 << 380),
                    ("2^381-1", (1 << 381) - 1), ("2^384-1", (1 << 384) - 1)):
        for hi in (0, top):
            out.append((f"{name} | {hi >> 381} << 381", ((v | hi) & ((1 << 384) - 1)).to_bytes(48, "little") + bytes(range(16))))
    return out


TPKE_V_LENGTHS =(62, 63, 64, 78, 79, 80, 190, 191, 192)   # 48 + |V| around the SHA-512 block boundaries 112, 128, 240


# ------------------------------------------------------------------------------------------------ encodings
def _enc48(x, flag):
    b = bytearray((x & ((1 << 384) - 1)).to_bytes(48, "little"))
    b[47] |= flag
    return bytes(b)


def _x_with(sym, start):
    """the first x >= start whose x^3 + 4 has Legendre symbol sym"""
    x = start
    while legendre(x ** 3 + B.B1) != sym:
        x += 1
    return x


@functools.lru_cache(None)
def g1_encodings():
    """(name, 48 bytes).  x^3 + 4 = 0 has no solution in Fp (-4 is not a cube: asserted in tests/test_h2g2_ref.py), so
    that class is empty by arithmetic, not by omission"""
    xs = [("0", 0), ("1", 1), ("p-1", P - 1), ("p", P), ("p+1", P + 1), ("2^381-1", (1 << 381) - 1),
          ("2^381+1", (1 << 381) + 1), ("2^382", 1 << 382), ("all ones", (1 << 383) - 1),
          ("residue", _x_with(1, 2)), ("residue'", _x_with(1, P - 40)), ("non-residue", _x_with(-1, 2)),
          ("non-residue'", _x_with(-1, P - 40))]
    return [(f"x={name} flag={flag:#x}", _enc48(x, flag)) for name, x in xs for flag in (0, 0x80)]


def y_zero_points(limit=20):
    """x = (a, b) with Im(x^3 + 4(1 + i)) = 0, i.e. a^2 = (b^3 - 4) / (3 b): g(x) = v lies in Fp, so y = (sqrt v, 0)
    when v is a residue (y.b = 0) and y = (0, sqrt -v) when it is not (y.a = 0).  [(b, a, v, "y.a=0" | "y.b=0")]"""
    out = []
    for b in range(1, limit + 1):
        a = B.sqrt_fp((b ** 3 - 4) * B.inv(3 * b))
        if a is None:
            continue
        for sa in (a, P - a):
            g = g_twist((sa, b))
            assert g[1] == 0
            out.append((b, sa, g[0], "y.b=0" if legendre(g[0]) == 1 else "y.a=0"))
    return out


@functools.lru_cache(None)
def g2_encodings():
    """(name, 96 bytes)"""
    edge = [("0", 0), ("1", 1), ("p-1", P - 1), ("p", P), ("p+1", P + 1), ("2^381-1", (1 << 381) - 1),
            ("2^381+1", (1 << 381) + 1), ("all ones", (1 << 383) - 1)]
    out = []
    for name, v in edge:
        for flag in (0, 0x80):
            out.append((f"x.a={name} x.b=2 flag={flag:#x}", _enc48(v, 0) + _enc48(2, flag)))
            out.append((f"x.a=2 x.b={name} flag={flag:#x}", _enc48(2, 0) + _enc48(v, flag)))
    out.append(("x.a all ones with bit 383", _enc48((1 << 384) - 1, 0) + _enc48(2, 0)))
    out.append(("flag bit in byte 47", _enc48(2, 0x80) + _enc48(2, 0)))
    out.append(("flag bit in byte 47 only", _enc48(0, 0x80) + _enc48(0, 0)))
    out.append(("flag only", _enc48(0, 0) + _enc48(0, 0x80)))
    # x.a, x.b small with g(x) a square / a non-square in Fp2
    sq = [(a, b) for a in range(1, 12) for b in range(1, 4) if B.f2sqrt(g_twist((a, b))) is not None][:3]
    ns = [(a, b) for a in range(1, 12) for b in range(1, 4) if B.f2sqrt(g_twist((a, b))) is None][:3]
    for a, b in sq + ns:
        for flag in (0, 0x80):
            out.append((f"x=({a},{b}) flag={flag:#x}", _enc48(a, 0) + _enc48(b, flag)))
    for b, a, _, kind in y_zero_points():
        for flag in (0, 0x80):
            out.append((f"{kind} x=(+-sqrt,{b}) a%1000={a % 1000} flag={flag:#x}", _enc48(a, 0) + _enc48(b, flag)))
    return out


def parity_encodings(o):
    """the encodings of tests/test_gpu_parity.py::test_decompression_validity_matches_oracle, drawn as that test draws
    them (o: the oracle module): {48: [G1 encodings], 96: [G2 encodings]}"""
    from helpers import Drbg
    d = Drbg(b"gpu-decompress")
    out = {}
    for size, gen, mul in ((48, o.g1_gen(), o.g1_mul), (96, o.g2_gen(), o.g2_mul)):
        encs = [gen, mul(gen, d.fr())]
        for i in range(24):
            b = bytearray(d.bytes(size))
            b[47] = (b[47] & 0x1f) | (gen[47] & 0xe0)
            if size == 96:
                b[95] = (b[95] & 0x1f) | (gen[95] & 0xe0)
            if i == 0:
                b[47] |= 0x1f
            encs.append(bytes(b))
        out[size] = encs
    return out


def model_g1(b):
    """(ok, inf, point) of the model's decoder"""
    try:
        p = B.g1_from_bytes(b)
    except ValueError:
        return (False, False, None)
    return (True, p is None, p)


def model_g2(b, sign_b=False):
    try:
        p = B.g2_from_bytes(b, sign_b)
    except ValueError:
        return (False, False, None)
    return (True, p is None, p)
