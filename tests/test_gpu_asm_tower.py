"""The hand-written assembly tower (asm_tower.hpp: lcb_r_fp12_mul_n, lcb_r_cyc_sqr_n, lcb_r_pow_z, through fe_asm.hpp's
fx_mul / fx_pow_z wrappers) on arbitrary operands on the device, through lcb_debug_asm_tower, against the big-integer
model (tests/pyref/tower.py).  In the library these routines only ever see the unitary, random-looking values of the
final exponentiation and the batch levels; their lazily reduced double-width sums rest on magnitude bounds that only
saturated operands reach (tests/tower_cases.py).

The Granger-Scott squaring is the square on the cyclotomic subgroup only; elsewhere the reference is the restatement of
the polynomial map it computes (tower.gs_sqr).  Every comparison is exact, mod p."""
import ctypes
import functools

import pytest

import tower_cases as C
from helpers import gpu_native
from pyref import bls12_381 as B
from pyref import tower as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


def words(case):
    return T.residues_to_words(case.m)


def flat(case):
    return T.residues_to_flat(case.m)


def launch_order(n):
    """indices of one launch: as tower_cases.spread, so n is no multiple of 64 (a part-filled last wave)"""
    return C.spread(list(range(n)))


def run(nat, op, a, b=None, k=1):
    idx = launch_order(len(a))
    assert len(idx) % 64 != 0
    got = nat.debug_asm_tower(op, [words(a[i]) for i in idx], None if b is None else [words(b[i]) for i in idx], run=k)
    assert len(got) == len(idx)
    return idx, got


def mismatches(idx, got, names, want_of):
    return [(names[i], p) for p, i in enumerate(idx) if T.words_to_flat(got[p]) != want_of(i)]


@functools.lru_cache(maxsize=None)
def all_pairs():
    return C.pair_classes()


PAIR_KINDS = ["self", "conj", "inverse", "zero", "one", "sat x sat", "basis table"]


@pytest.mark.parametrize("kind", PAIR_KINDS)
@pytest.mark.parametrize("op", ["mul", "mul_conj"])
def test_products(nat, op, kind):
    """fx_mul and fx_mul with conj(a): SAT x SAT is the worst case of the lazily reduced Fp6 products"""
    ps = all_pairs()[kind]
    a, b = [x for x, _ in ps], [y for _, y in ps]
    idx, got = run(nat, op, a, b)

    def want(i):
        fa = flat(a[i])
        return B.e_mul(B.e_conj(fa) if op == "mul_conj" else fa, flat(b[i]))
    bad = mismatches(idx, got, [f"{x.name} * {y.name}" for x, y in ps], want)
    assert not bad, bad[:12]


def test_products_many_items(nat):
    """every pair of the catalogue in ONE launch: more items than a 256-lane block holds, a part-filled last wave, and
    every item its own result"""
    ps = [p for kind in PAIR_KINDS for p in all_pairs()[kind]]
    assert len(ps) > 256
    a, b = [x for x, _ in ps], [y for _, y in ps]
    idx, got = run(nat, "mul", a, b)
    assert len(idx) > 256 and len(idx) % 64
    bad = mismatches(idx, got, [f"{x.name} * {y.name}" for x, y in ps], lambda i: B.e_mul(flat(a[i]), flat(b[i])))
    assert not bad, bad[:12]


def gs_chain(a, k):
    for _ in range(k):
        a = T.gs_sqr(a)
    return a


CHAINS = [2, 3, 63]


@pytest.mark.parametrize("k", [0] + CHAINS)
def test_squarings_unitary(nat, k):
    """one squaring (op 2; k = 0 here) and runs of 2, 3 and 63 (op 3) on UNIT against the ring's own power"""
    cases = C.unit()
    idx, got = run(nat, "cyc_sqr" if k == 0 else "cyc_sqr_run", cases, k=max(k, 1))
    bad = mismatches(idx, got, [c.name for c in cases], lambda i: B.e_pow(flat(cases[i]), 1 << max(k, 1)))
    assert not bad, bad[:12]


@pytest.mark.parametrize("cls", ["sat", "mix", "dense", "special", "basis"])
@pytest.mark.parametrize("k", [0] + CHAINS)
def test_squarings_off_the_subgroup(nat, k, cls):
    """the same on SAT and MIX (and the dense patterns, 0, 1, -1 and BASIS) against the Granger-Scott restatement:
    3 t -+ 2 z reaches its 8p range, and the fp4 sums their 9.5 p^2 range, only with saturated coefficients"""
    cases = C.CLASSES[cls]()
    idx, got = run(nat, "cyc_sqr" if k == 0 else "cyc_sqr_run", cases, k=max(k, 1))
    bad = mismatches(idx, got, [c.name for c in cases], lambda i: gs_chain(flat(cases[i]), max(k, 1)))
    assert not bad, bad[:12]


def test_squarings_many_items(nat):
    """the whole catalogue three times over in one launch of more than one block"""
    every = C.everything()
    cases = every + every[1:] + every[2:]
    assert len(cases) > 256
    idx, got = run(nat, "cyc_sqr", cases)
    assert len(idx) % 64
    bad = mismatches(idx, got, [c.name for c in cases], lambda i: T.gs_sqr(flat(cases[i])))
    assert not bad, bad[:12]


def test_pow_z_unitary(nat):
    """fx_pow_z: conj(x^|z|), the accumulator in AGPRs through 63 squarings and five products"""
    cases = C.unit()
    idx, got = run(nat, "pow_z", cases)
    bad = mismatches(idx, got, [c.name for c in cases], lambda i: T.pow_z(flat(cases[i])))
    assert not bad, bad[:12]


def test_pow_z_many_items(nat):
    cases = [C.unit()[k % len(C.unit())] for k in range(300)]
    idx, got = run(nat, "pow_z", cases)
    assert len(idx) > 256 and len(idx) % 64
    want = {tuple(c.m): T.pow_z(flat(c)) for c in C.unit()}
    bad = mismatches(idx, got, [c.name for c in cases], lambda i: want[tuple(cases[i].m)])
    assert not bad, bad[:12]


def test_rejects_bad_arguments(nat):
    one = [words(C.ONE)]
    lib = nat.lib()
    buf = (ctypes.c_uint32 * 144)(*one[0])
    out = (ctypes.c_uint32 * 144)()
    for op, b in ((5, buf), (3, buf), (2 | (4 << 8), buf), (0, None), (3 | (256 << 8), buf)):
        assert lib.lcb_debug_asm_tower(op, buf, b, 1, out) == -1, op
    assert lib.lcb_debug_asm_tower(2, buf, None, 0, out) == -1
