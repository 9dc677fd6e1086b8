"""The routines under G2.SetHashOf and the device point decoders at the edge operands of tests/h2g2_cases.py, through
lcb_debug_h2g2_op (k_h2g2_debug in k_ptmul.hip, one routine of h2g2_debug.hpp per lane; op 12 runs k_mcl_g2_clear
alone), against the big-integer model tests/pyref/bls12_381.py.  Every comparison is exact and no case is left out;
tests/test_h2g2_ref.py (CPU) asserts that the cases reach every branch."""
import functools

import pytest

import h2g2_cases as C
import oracle as o
from helpers import gpu_native
from pyref import bls12_381 as B

pytestmark = pytest.mark.gpu
P = B.P


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


@pytest.fixture(scope="module")
def mcl(nat):
    from lachain_amd import mcl as m
    return m


def _canonical(words):
    return all(C.raw_words(words[k:k + 12]) < P for k in range(0, len(words), 12))


# ------------------------------------------------------------------------------------------------ hook arguments
def test_hook_rejects_bad_arguments(nat):
    import ctypes
    lib = nat.lib()
    a = (ctypes.c_uint32 * nat.H2G2_DEBUG_IN)()
    out = (ctypes.c_uint32 * nat.H2G2_DEBUG_OUT)()
    assert lib.lcb_debug_h2g2_op(-1, a, 1, out) == -1
    assert lib.lcb_debug_h2g2_op(len(nat.H2G2_DEBUG_OPS), a, 1, out) == -1
    assert lib.lcb_debug_h2g2_op(0, a, 0, out) == -1
    assert lib.lcb_debug_h2g2_op(0, a, 65537, out) == -1
    assert lib.lcb_debug_h2g2_op(0, None, 1, out) == -1
    assert lib.lcb_debug_h2g2_op(0, a, 1, out) == 0 and list(out[:12]) == [0] * 12 and out[72] == 1   # sqrt(0) = 0


# ------------------------------------------------------------------------------------------------ roots
def test_fp_sqrt(nat):
    cases = C.fp_cases()
    got = nat.debug_h2g2_op("fp_sqrt", [C.fp_item(v) for _, v in cases])
    for (name, v), g in zip(cases, got):
        want = B.sqrt_fp(v)
        assert g[72] == (want is not None), name
        assert _canonical(g[:12]), name
        assert C.fp_of(g) == pow(v, (P + 1) // 4, P), name     # the value the routine leaves, a root or not
        if want is not None:
            assert C.fp_of(g) == want, name


def test_fp2_sqrt_and_normed(nat):
    cases = C.fp2_cases()
    items = [C.fp2_item(x) for _, x in cases]
    full = nat.debug_h2g2_op("fp2_sqrt", items)
    normed = nat.debug_h2g2_op("fp2_sqrt_normed", items)
    for (name, x), g, h in zip(cases, full, normed):
        want = B.f2sqrt(x)
        assert g[72] == (want is not None), name
        assert h[72] == (B.sqrt_fp(x[0] * x[0] + x[1] * x[1]) is not None) == (want is not None), name
        for r in (g, h):
            assert _canonical(r[:24]), name
            assert C.fp2_of(r) == (want if want is not None else (0, 0)), name


def test_fp2_sqrt_any(nat):
    cases = C.fp2_cases()
    got = nat.debug_h2g2_op("fp2_sqrt_any", [C.fp2_item(x) for _, x in cases])
    for (name, x), g in zip(cases, got):
        want = B.f2sqrt(x)
        assert g[72] == (want is not None), name
        if want is not None:
            assert _canonical(g[:24]), name
            assert C.fp2_of(g) in (want, B.f2neg(want)), name
            if x[1] == 0:
                assert C.fp2_of(g) == want, name            # g(x) in Fp: the decoders need the model's root there


# ------------------------------------------------------------------------------------------------ inverses
def test_fp_inv_gcd(nat):
    cases = C.fp_cases()
    got = nat.debug_h2g2_op("fp_inv_gcd", [C.fp_item(v) for _, v in cases])
    for (name, v), g in zip(cases, got):
        assert _canonical(g[:12]), name
        assert C.fp_of(g) * v % P == (1 if v else 0), name
        assert v or C.fp_of(g) == 0, name


def test_fp2_inv_g(nat):
    cases = C.fp2_cases()
    got = nat.debug_h2g2_op("fp2_inv_g", [C.fp2_item(x) for _, x in cases])
    for (name, x), g in zip(cases, got):
        assert _canonical(g[:24]), name
        assert B.f2mul(C.fp2_of(g), x) == ((1, 0) if x != (0, 0) else (0, 0)), name
        assert x != (0, 0) or C.fp2_of(g) == (0, 0), name


# ------------------------------------------------------------------------------------------------ the hash's Fp element and the map
def test_fp_set_hash_digest(nat):
    cases = C.digests()
    got = nat.debug_h2g2_op("fp_set_hash_digest", [C.bytes_item(d) for _, d in cases])
    for (name, d), g in zip(cases, got):
        assert _canonical(g[:12]) and C.fp_of(g) == B.fp_from_digest(d), name


def test_g2_calc_bn(nat):
    cases = C.t_cases()
    got = nat.debug_h2g2_op("g2_calc_bn", [C.fp2_item(t) for _, t in cases])
    for (name, t), g in zip(cases, got):
        want = B.map_to_g2_bn(t)
        assert g[72] == (want is not None), (name, C.map_branch(t))
        assert _canonical(g[:48]), name
        assert (C.fp2_of(g[0:24]), C.fp2_of(g[24:48])) == (want if want is not None else ((0, 0), (0, 0))), \
            (name, C.map_branch(t))


# ------------------------------------------------------------------------------------------------ cofactor clearings
@functools.lru_cache(None)
def _cleared():
    return [(name, p, B.clear_cofactor_g2(p), B.g2_mul(p, C.H2)) for name, p in C.clear_points()]


def test_cofactor_clearing_one_lane_and_cooperative(nat):
    """g2_clear_cofactor_bp (one lane, mixed additions) and k_mcl_g2_clear (pt_clear_cofactor_bp on four-lane groups,
    general additions) on the same points, the small-order ones included: on order 13 both ladders double infinity,
    add to infinity and add a point to its inverse (tests/test_h2g2_ref.py; coop_pt.hpp's pt_add is complete, as
    jac_add and jac_add_aff are)"""
    ref = _cleared()
    items = [C.point_item(p) for _, p, _, _ in ref]
    lane = nat.debug_h2g2_op("g2_clear_cofactor_bp", items)
    coop = nat.debug_h2g2_op("k_mcl_g2_clear", items)
    for (name, _, want, _), g, h in zip(ref, lane, coop):
        assert _canonical(g[:72]) and _canonical(h[:72]), name
        assert C.jac_to_affine(g) == want, name
        assert C.jac_to_affine(h) == want, name
    assert any(want is None for _, _, want, _ in ref)       # a point of order 13 clears to infinity


def test_original_cofactor_ladder(nat):
    ref = _cleared()
    got = nat.debug_h2g2_op("g2_clear_cofactor_h2", [C.point_item(p) for _, p, _, _ in ref])
    for (name, _, _, want), g in zip(ref, got):
        assert _canonical(g[:72]), name
        assert C.jac_to_affine(g) == want, name


# ------------------------------------------------------------------------------------------------ decoders
def _g1_device(nat, encs):
    got = nat.debug_h2g2_op("g1_decompress", [C.bytes_item(b) for b in encs])
    out = []
    for g in got:
        assert _canonical(g[:24])
        ok, inf = bool(g[72]), bool(g[73])
        out.append((ok, inf, (C.fp_of(g[0:12]), C.fp_of(g[12:24])) if ok and not inf else None))
    return out


def _g2_device(nat, encs):
    got = nat.debug_h2g2_op("g2_decompress", [C.bytes_item(b) for b in encs])
    out = []
    for g in got:
        assert _canonical(g[:48])
        ok, inf = bool(g[72]), bool(g[73])
        out.append((ok, inf, (C.fp2_of(g[0:24]), C.fp2_of(g[24:48])) if ok and not inf else None))
    return out


def _host(mcl, cls, b):
    """the host decoder (mclBn*_deserialize): (ok, inf, affine point) from the record's Jacobian words"""
    try:
        pt = cls.FromBytes(b)
    except ValueError:
        return (False, False, None)
    w = C.bytes_item(bytes(pt.v))
    p = C.g1_jac_to_affine(w) if cls is mcl.G1 else C.jac_to_affine(w)
    return (True, p is None, p)


def _g1_to_affine_dev(nat, encs):
    """lcb_g1_to_affine_dev (k_g1_to_affine): the decoder as the MSM path runs it, with its per-item ok array"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(encs)
    s = torch.cuda.current_stream(dev).cuda_stream
    d_in = torch.frombuffer(bytearray(b"".join(encs)), dtype=torch.uint8).to(dev)
    d_aff = torch.zeros(96 * n, dtype=torch.uint8, device=dev)
    d_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    assert nat.lib().lcb_g1_to_affine_dev(d_aff.data_ptr(), d_ok.data_ptr(), d_in.data_ptr(), n, s) == 0
    torch.cuda.synchronize(dev)
    aff, ok = d_aff.cpu().numpy().tobytes(), d_ok.cpu().tolist()
    out = []
    for i in range(n):
        w = C.bytes_item(aff[96 * i:96 * i + 96])
        out.append((bool(ok[i]), (C.fp_of(w[0:12]), C.fp_of(w[12:24]))))
    return out


def test_g1_decoders_match_model_host_and_oracle(nat, mcl):
    encs = [b for _, b in C.g1_encodings()] + C.parity_encodings(o)[48] + [bytes(48)]
    device = _g1_device(nat, encs)
    msm = _g1_to_affine_dev(nat, encs)
    for b, dv, (mok, mpt) in zip(encs, device, msm):
        want = C.model_g1(b)
        assert dv == want, b.hex()
        assert _host(mcl, mcl.G1, b) == want, b.hex()
        assert o.g1_valid(b) == want[0], b.hex()
        assert mok == want[0] and mpt == (want[2] if want[2] is not None else (0, 0)), b.hex()
        assert want[1] == (b == bytes(48)), b.hex()          # infinity is only the all-zero string
    assert sum(dv[0] for dv in device) >= 8 and sum(not dv[0] for dv in device) >= 20


@pytest.mark.parametrize("sign_b", [False, True])
def test_g2_decoders_match_model_host_and_oracle(nat, mcl, sign_b):
    encs = [b for _, b in C.g2_encodings()] + C.parity_encodings(o)[96] + [bytes(96)]
    nat.set_g2_sign_from_b(sign_b)
    o.set_g2_sign_from_b(1 if sign_b else 0)
    try:
        device = _g2_device(nat, encs)
        host = [_host(mcl, mcl.G2, b) for b in encs]
        orc = [o.g2_valid(b) for b in encs]
        # the oracle's decoded point, seen through a doubling: [2] Q and [2] (-Q) differ in their flag even where Q and
        # -Q serialise alike (y.a = 0 or y.b = 0)
        two = o.fr(2)
        orc2 = [o.g2_mul(b, two) if v else None for b, v in zip(encs, orc)]
        dev2 = [(mcl.G2.FromBytes(b) * mcl.Fr.FromInt(2)).ToBytes() if v else None for b, v in zip(encs, orc)]
    finally:
        nat.set_g2_sign_from_b(False)
        o.set_g2_sign_from_b(0)
    for k, b in enumerate(encs):
        want = C.model_g2(b, sign_b)
        assert device[k] == want, b.hex()
        assert host[k] == want, b.hex()
        assert orc[k] == want[0], b.hex()
        assert orc2[k] == dev2[k], b.hex()
        assert want[1] == (b == bytes(96)), b.hex()
    assert sum(dv[0] for dv in device) >= 20 and sum(not dv[0] for dv in device) >= 20


@pytest.mark.parametrize("sign_b", [False, True])
def test_y_coordinate_zero_encodings_decode_to_the_models_two_points(nat, sign_b):
    """x = (a, b) with g(x) in Fp: y = (0, s) or (s, 0), the flagged coordinate is zero and the flag cannot be honoured;
    flag 0 and flag 1 decode to f2sqrt's root and its negative (curve.hpp g2_decompress)"""
    kind = "y.b=0" if sign_b else "y.a=0"
    pts = [(a, b) for b, a, _, k in C.y_zero_points() if k == kind]
    assert len(pts) >= 2
    encs = []
    for a, b in pts:
        e = a.to_bytes(48, "little") + b.to_bytes(48, "little")
        encs += [e, e[:95] + bytes([e[95] | 0x80])]
    nat.set_g2_sign_from_b(sign_b)
    try:
        device = _g2_device(nat, encs)
    finally:
        nat.set_g2_sign_from_b(False)
    for k in range(0, len(encs), 2):
        p0, p1 = device[k][2], device[k + 1][2]
        assert device[k] == C.model_g2(encs[k], sign_b) and device[k + 1] == C.model_g2(encs[k + 1], sign_b)
        assert p0[1][1 if sign_b else 0] == 0 and p1 == B.g2_neg(p0) and p0 != p1
