"""The exact per-share check's Miller kernel (k_tpke_miller: lcb_r_miller2 in assembly over normalised line sets, the
compiled fallback otherwise) at crafted shares.  A decryption share U_i is any on-curve G1 point, so the Montgomery
words of its x are the adversary's choice, and they go straight into the assembly loop's line evaluations; a wrong
Miller value there would let validators disagree on a share.  lcb_debug_tpke_miller runs the library's own prepare and
the kernel unchanged and returns each share's parked value, before any final exponentiation.

The device's value differs from a textbook Miller value by factors in proper subfields (normalised lines), which the
final exponentiation removes, so the comparison is
    fe(f_device) == fe(miller(U_i, H) miller(-Y_i, W))
with the big-integer model's plain power for fe and tests/pyref/bls12_381.py's affine Miller loop.  The cooperative
Miller kernel stays covered by decisions only (tests/test_gpu_coop.py)."""
import functools

import pytest

import oracle as o
import tower_cases as C
from helpers import Drbg, gpu_native
from pyref import bls12_381 as B
from pyref import tower as T

pytestmark = pytest.mark.gpu
P = B.P
ONE = B.e_one()


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


@functools.lru_cache(maxsize=None)
def _fe(a):
    return tuple(T.final_exp(list(a)))


def fe(a):
    return list(_fe(tuple(a)))


class Setup:
    """one decryptor key, one honest ciphertext, and the same ciphertext with W replaced by a twist point outside G2"""

    def __init__(self):
        d = Drbg(b"gpu-miller-edges")
        self.x = d.fr_int()
        self.yi = o.g1_mul(o.g1_gen(), o.fr(self.x))
        y = o.g1_mul(o.g1_gen(), o.fr(d.fr_int()))
        self.ct = o.tpke_encrypt(y, b"crafted shares", o.fr(d.fr_int()))
        u, v, w = self.ct
        self.honest = o.tpke_decrypt(u, v, w, o.fr(self.x))
        while True:                                   # a random point of the twist: on the curve, not in G2
            xq = (int.from_bytes(d.bytes(48), "little") % P, int.from_bytes(d.bytes(48), "little") % P)
            yq = B.f2sqrt(B.f2add(B.f2mul(B.f2mul(xq, xq), xq), B.B2))
            if yq is not None:
                break
        self.w_out = B.g2_to_bytes((xq, yq))
        assert o.g2_valid(self.w_out) and not o.g2_in_subgroup(self.w_out)
        self.h = o.g2_hash(u + v)


@pytest.fixture(scope="module")
def setup():
    return Setup()


def crafted(group):
    """two patterns of tower_cases.G1_PATTERNS, both signs of y: [(name, 48 bytes)]"""
    out = []
    for name, (x, y) in C.g1_patterned()[2 * group:2 * group + 2]:
        for sign, yy in (("+", y), ("-", (P - y) % P)):
            assert (yy * yy - x ** 3 - 4) % P == 0, name
            out.append((f"x~{name} y{sign}", B.g1_to_bytes((x, yy))))
    return out


def check(nat, s, w, group):
    shares = crafted(group) + [("honest", s.honest), ("infinity", bytes(48))]
    assert len(shares) <= 10
    u, v, _ = s.ct
    got = nat.debug_tpke_miller([s.yi], [(u, v, w)], [(0, 0, ui) for _, ui in shares])
    hq, wq = B.g2_from_bytes(s.h), B.g2_from_bytes(w)
    right = B.miller(B.g1_neg(B.g1_from_bytes(s.yi)), wq)
    bad = []
    for (name, ui), (f, ok) in zip(shares, got):
        # the share as the wire format gives it: x = 0 with an even y IS the encoding of the point at infinity
        want = fe(B.e_mul(B.miller(B.g1_from_bytes(ui), hq), right))
        have = fe(T.words_to_flat(f))
        if have != want:
            bad.append((name, "value"))
        if not ok or not o.g1_valid(ui):
            bad.append((name, "flag"))
        if (have == ONE) != (o.tpke_verify_share(s.yi, u, v, w, ui) == 1):
            bad.append((name, "decision"))
    assert not bad, bad
    return dict(zip([n for n, _ in shares], got))


GROUPS = range(len(C.G1_PATTERNS) // 2)


@pytest.mark.parametrize("group", GROUPS)
def test_honest_w_assembly_loop(nat, setup, group):
    """normalised line sets: miller2_asm"""
    got = check(nat, setup, setup.ct[2], group)
    assert fe(T.words_to_flat(got["honest"][0])) == ONE


@pytest.mark.parametrize("group", GROUPS)
def test_w_outside_g2(nat, setup, group):
    """W on the twist but outside G2 (a point of generic order: the loop meets no exceptional step, which is the only
    case with a value to compare — its line set normalises like any other, and the forced fallback below computes the
    lines on the fly): the same function of (U_i, H, Y_i, W), and the honest share no longer verifies.  A W of small
    order, whose set stays un-normalised, has no model value; tests/test_gpu_batched.py covers it by decisions."""
    check(nat, setup, setup.w_out, group)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("w", ["honest", "outside"])
def test_general_lines_fallback(nat, setup, w, group):
    """every line set marked un-normalised: miller2_sets_fallback, lines computed on the fly, for the honest W and for
    the W outside G2"""
    nat.set_line_mode(True)
    try:
        got = check(nat, setup, setup.ct[2] if w == "honest" else setup.w_out, group)
    finally:
        nat.set_line_mode(False)
    assert (fe(T.words_to_flat(got["honest"][0])) == ONE) == (w == "honest")
