"""CPU checks of the public-key recovery kernels (lachain_amd/csrc/k_secp_recover.hip) compiled for the host by
tools/emul/secp_recover_emul.cpp and run lane by lane (no LDS, no barriers, so that is exact), against the oracle
(o.ecdsa_recover, o.keccak256, o.ecdsa_pubkey) and Python integers.  TEST INFRASTRUCTURE: catches logic errors in the
device code without a GPU; the GPU itself is covered by tests/test_gpu_ecdsa_recover.py, which shares the mixed batch
built here.

Reference: DefaultCrypto.RecoverSignatureHashed / ComputeAddress (DefaultCrypto.cs:146-168,197-200)."""
import ctypes
import json
import math
import os
import random
import subprocess

import pytest

import oracle as o
import secp_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emul", "secp_recover_emul.cpp")
LIB = os.path.join(ROOT, "tools", "emul", "libsecp_recover_emul.so")
CSRC = os.path.join(ROOT, "lachain_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("k_secp_recover.hip", "k_secp.hip", "secp_comb.hpp", "secp.hpp",
                                                 "secp_debug.hpp")]
K = json.load(open(os.path.join(ROOT, "tests", "golden", "secp256k1_kats.json")))
P, N = o.SECP_P, o.SECP_N
KECCAK_LENGTHS = [0, 1, 55, 135, 136, 137, 271, 272, 273, 1000]


# ---------------------------------------------------------------- the endomorphism's constants, from first principles
def glv_constants():
    """lambda, beta (the pair with phi(G) = lambda G) and the lattice basis, derived with Python integers"""
    gx = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
    lam = next(l for l in (pow(g, (N - 1) // 3, N) for g in range(2, 50)) if l != 1)
    lam = min(lam, lam * lam % N)         # the two roots of x^2 + x + 1; the kernels use the smaller one
    beta = next(b for b in (pow(g, (P - 1) // 3, P) for g in range(2, 50)) if b != 1)
    lg = o.ecdsa_pubkey(lam.to_bytes(32, "big"))[0]
    if int.from_bytes(lg[1:], "big") != beta * gx % P:
        beta = beta * beta % P
    assert int.from_bytes(lg[1:], "big") == beta * gx % P
    r0, r1, t0, t1, rows = N, lam, 0, 1, []
    while r1:
        q = r0 // r1
        r0, r1, t0, t1 = r1, r0 - q * r1, t1, t0 - q * t1
        rows.append((r0, t0))
    sq = math.isqrt(N)
    l = max(i for i, (r, _) in enumerate(rows) if r >= sq)
    a1, b1 = rows[l + 1][0], -rows[l + 1][1]
    a2, b2 = min(((r, -t) for r, t in (rows[l], rows[l + 2])), key=lambda v: v[0] ** 2 + v[1] ** 2)
    return lam, beta, (a1, b1, a2, b2)


LAMBDA, BETA, BASIS = glv_constants()


# ---------------------------------------------------------------- expected results (the oracle)
def _tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def rec_id(sig: bytes, chain: int, new: bool):
    """recId = (enc - 36) / 2 / chainId (DefaultCrypto.cs:155-158; C# truncates), or None"""
    if len(sig) != (66 if new else 65) or chain == 0:
        return None
    rec = _tdiv(_tdiv(int.from_bytes(sig[64:], "big") - 36, 2), chain)
    return rec if 0 <= rec <= 3 else None


def address_of(pub33: bytes) -> bytes:
    """ComputeAddress: keccak256(uncompressed[1:])[12:]"""
    x = int.from_bytes(pub33[1:], "big")
    y = pow((x ** 3 + 7) % P, (P + 1) // 4, P)
    if (y & 1) != (pub33[0] & 1):
        y = P - y
    assert y * y % P == (x ** 3 + 7) % P
    return o.keccak256(x.to_bytes(32, "big") + y.to_bytes(32, "big"))[12:]


def expected(hs, sigs, rec_of):
    """(ok, keys, addresses) of a batch; rec_of(sig) gives the recovery id or None"""
    ok, pub, addr = bytearray(), bytearray(), bytearray()
    for h, s in zip(hs, sigs):
        rec = rec_of(s)
        pk = o.ecdsa_recover(h, s[:64], rec) if rec is not None else None
        ok.append(1 if pk else 0)
        pub += pk if pk else bytes(33)
        addr += address_of(pk) if pk else bytes(20)
    return bytes(ok), bytes(pub), bytes(addr)


# ---------------------------------------------------------------- the mixed batch (shared with the GPU test)
def v_bytes(rec: int, chain: int, new: bool, rng=None) -> bytes:
    """a trailer that DECODES to rec (the reference's own encoding, o.ecdsa_encode, decodes 2 and 3 to 1)"""
    width = 2 if new else 1
    if rng is None and (rec, chain, new) in _V_CACHE:
        return _V_CACHE[rec, chain, new]
    vs = [v for v in range(256 ** width) if rec_id(bytes(64) + v.to_bytes(width, "big"), chain, new) == rec]
    assert vs, (rec, chain, new)
    _V_CACHE[rec, chain, new] = vs[0].to_bytes(width, "big")
    return (rng.choice(vs) if rng else vs[0]).to_bytes(width, "big")


_V_CACHE = {}
SPLIT_T = [1, 2, N - 1, LAMBDA, N - LAMBDA, LAMBDA + 1, 2 ** 128 - 1, 2 ** 128]
N_KINDS = 16
EDGE_X = [x for xs in secp_cases.edge_xs() for x in xs]       # 1, 2, 3, 4, 6, 8, p - 3, p - 4, p - 10, ...


def mixed_batch(rng, chain, new, n=1500):
    """hashes, signatures and per-item notes: (kind, detail).  Every class of the recovery's decision tree; the
    expectations come from the oracle (expected), never from this builder."""
    vb = {rec: v_bytes(rec, chain, new) for rec in range(4)}
    gx = int.from_bytes(o.ecdsa_pubkey((1).to_bytes(32, "big"))[0][1:], "big")
    hs, sigs, notes = [], [], []

    def signed(h, priv):
        while True:
            try:
                c, rid = o.ecdsa_sign_compact(h, priv.to_bytes(32, "big"), rng.randrange(1, N).to_bytes(32, "big"))
                return c, rid
            except ValueError:
                continue

    def point(k):
        pk = o.ecdsa_pubkey(k.to_bytes(32, "big"))[0]
        return int.from_bytes(pk[1:], "big"), pk[0] & 1

    for i in range(n):
        kind, sub = i % N_KINDS, i // N_KINDS
        priv = rng.randrange(1, N)
        h = rng.randbytes(32)
        note = None
        if kind == 2:
            h = [bytes(32), N.to_bytes(32, "big"), b"\xff" * 32][sub % 3]
        c, rid = signed(h, priv)
        r, s = int.from_bytes(c[:32], "big"), int.from_bytes(c[32:], "big")
        sig = c + vb[rid]
        if kind == 1:
            sig = o.ecdsa_encode(c, rid, chain, new)            # the reference's own (lossy) trailer
        elif kind == 3:
            flip = sub % 2 == 0                                 # high-s twin, parity flipped or not
            sig = c[:32] + (N - s).to_bytes(32, "big") + vb[rid ^ 1 if flip else rid]
            note = ("flipped" if flip else "unflipped", o.ecdsa_pubkey(priv.to_bytes(32, "big"))[0])
        elif kind == 4:
            rr, ss = [(0, s), (r, 0), (N + rng.randrange(2 ** 100), s), (r, N + rng.randrange(2 ** 100)), (N, s),
                      (r, N)][sub % 6]
            sig = rr.to_bytes(32, "big") + ss.to_bytes(32, "big") + vb[rid]
        elif kind == 5:
            sig = c + rng.randbytes(2 if new else 1)
        elif kind == 6:                                         # recId >= 2 with r < p - n
            rr = rng.randrange(1, P - N)
            sig = rr.to_bytes(32, "big") + c[32:] + vb[2 + sub % 2]
            note = ("high-x",)
        elif kind == 7:                                         # recId >= 2 with r >= p - n
            assert r >= P - N
            sig = c + vb[2 + (rid & 1)]
        elif kind == 8:                                         # x not on the curve
            while True:
                rr = rng.randrange(1, N)
                if pow((rr ** 3 + 7) % P, (P - 1) // 2, P) != 1:
                    break
            sig = rr.to_bytes(32, "big") + c[32:] + vb[sub % 2]
        elif kind in (9, 10):
            # R = k G.  kind 9: hash = s k, so s R - z G is infinity (the other parity recovers); kind 10:
            # hash = -s k, so u1 G == u2 R and the last step doubles
            while True:
                k = rng.randrange(1, N)
                x, par = point(k)
                if x < N:
                    break
            z = s * k % N if kind == 9 else -s * k % N
            h = z.to_bytes(32, "big")
            other = kind == 9 and sub % 2 == 1
            sig = x.to_bytes(32, "big") + c[32:] + vb[par ^ 1 if other else par]
            note = ("infinity",) if kind == 9 and not other else ("recovers",)
        elif kind == 11:                                        # u2 = t: halves 0, +-1 or at the width boundary
            t = SPLIT_T[sub % len(SPLIT_T)]
            sig = c[:32] + (r * t % N).to_bytes(32, "big") + vb[rid]
        elif kind == 12:                                        # r = x(G)
            sig = gx.to_bytes(32, "big") + c[32:] + vb[sub % 2]
        elif kind == 13:
            # R = G (even y), u2 = d < 128 and u1 = +-d: the comb sum meets d G again (doubling) or -d G (infinity)
            d = 1 + sub % 127
            z = (-d * gx if sub % 2 == 0 else d * gx) % N
            h = z.to_bytes(32, "big")
            sig = gx.to_bytes(32, "big") + (d * gx % N).to_bytes(32, "big") + vb[0]
            note = ("recovers",) if sub % 2 == 0 else ("infinity",)
        elif kind == 14:
            c, rid = signed(h, 1 if sub % 2 else N - 1)         # the keys G and -G
            sig = c + vb[rid]
        elif kind == 15:
            # x(R) is one of the smallest (1, 2, 3, ...) or largest (p - 3, ...) x on the curve, with either parity:
            # as r itself, or as r + n through recovery ids 2 and 3 (every large one is above n)
            x = EDGE_X[sub % len(EDGE_X)]
            par = (sub // len(EDGE_X)) % 2
            rr, rec = (x, par) if x < N else (x - N, 2 + par)
            sig = rr.to_bytes(32, "big") + c[32:] + vb[rec]
        hs.append(h)
        sigs.append(sig)
        notes.append((kind, note))
    return hs, sigs, notes


# ---------------------------------------------------------------- the emulation
@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC], check=True)
    lib = ctypes.CDLL(LIB)
    lib.emu_recover.restype = ctypes.c_ulonglong
    return lib


def emu_recover(emu, hs, sigs, L, special, new, chain, from20=None):
    n = len(hs)
    pub, addr = ctypes.create_string_buffer(33 * n + 1), ctypes.create_string_buffer(20 * n + 1)
    ok, acc = ctypes.create_string_buffer(n + 1), ctypes.create_string_buffer(n + 1)
    p3 = (ctypes.c_ulonglong * 3)()
    emu.emu_recover(pub, addr, ok, acc if from20 is not None else None, b"".join(hs), b"".join(sigs), L, from20, n,
                    int(special), int(new), chain, p3)
    return ok.raw[:n], pub.raw[:33 * n], addr.raw[:20 * n], acc.raw[:n], list(p3)


def test_scalar_split(emu):
    lam, beta, (a1, b1, a2, b2) = LAMBDA, BETA, BASIS
    assert (lam * lam + lam + 1) % N == 0 and pow(beta, 3, P) == 1 and beta != 1
    assert (a1 + b1 * lam) % N == 0 and (a2 + b2 * lam) % N == 0
    rng = random.Random(7)
    vals = [0, 1, N - 1, lam, N - lam, 2 ** 128 - 1, 2 ** 128] + [rng.randrange(N) for _ in range(2000)]
    m1, m2 = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    e1, e2 = (ctypes.c_int8 * 36)(), (ctypes.c_int8 * 36)()
    n1, n2 = ctypes.c_int(0), ctypes.c_int(0)
    for u2 in vals:
        emu.emu_glv_split(m1, ctypes.byref(n1), m2, ctypes.byref(n2), e1, e2, u2.to_bytes(32, "little"))
        k1 = int.from_bytes(m1.raw, "little") * (-1 if n1.value else 1)
        k2 = int.from_bytes(m2.raw, "little") * (-1 if n2.value else 1)
        assert (k1 + k2 * lam - u2) % N == 0, hex(u2)
        # the ladder's width: 33 signed 4-bit digits in [-8, 8] hold any magnitude below 2^129
        assert abs(k1) < 2 ** 129 and abs(k2) < 2 ** 129, hex(u2)
        for k, e in ((k1, e1), (k2, e2)):
            assert all(abs(d) <= 8 for d in e) and all(d == 0 for d in e[33:])
            assert sum(d * 16 ** w for w, d in enumerate(e)) == k, hex(u2)


def test_endomorphism(emu):
    rng = random.Random(11)
    out = ctypes.create_string_buffer(32)
    for k in [1] + [rng.randrange(1, N) for _ in range(50)]:
        pk = o.ecdsa_pubkey(k.to_bytes(32, "big"))[1]
        lp = o.ecdsa_pubkey((k * LAMBDA % N).to_bytes(32, "big"))[1]
        emu.emu_phi(out, pk[1:33][::-1])
        assert out.raw[::-1] == lp[1:33] and pk[33:] == lp[33:]
        assert int.from_bytes(lp[1:33], "big") == BETA * int.from_bytes(pk[1:33], "big") % P


@pytest.mark.parametrize("chain,new", [(25, False), (225, True)])
def test_pipeline_vs_oracle(emu, chain, new):
    hs, sigs, notes = mixed_batch(random.Random(2000 + chain), chain, new, n=400)
    L = 66 if new else 65
    want_ok, want_pub, want_addr = expected(hs, sigs, lambda s: rec_id(s, chain, new))
    from20 = bytearray(want_addr)
    for i in range(0, len(hs), 3):
        from20[20 * i + 7] ^= 0x10
    ok, pub, addr, acc, products = emu_recover(emu, hs, sigs, L, False, new, chain, bytes(from20))
    assert ok == want_ok
    assert pub == want_pub
    assert addr == want_addr
    assert acc == bytes(int(want_ok[i] and i % 3 != 0) for i in range(len(hs)))
    assert 0 < sum(want_ok) < len(hs)
    print("field products per item (scalars, recovery, finish):", [p / len(hs) for p in products])


def test_golden_signatures_and_special_form(emu):
    priv = bytes.fromhex(K["priv_address"]["priv"])
    key = o.ecdsa_pubkey(priv)[0]
    want_addr = bytes.fromhex(K["priv_address"]["address"])
    assert address_of(key) == want_addr
    for s in K["signatures"]:
        h, sig = o.keccak256(bytes.fromhex(s["msg_rlp"])), bytes.fromhex(s["sig"])
        ok, pub, addr, _, _ = emu_recover(emu, [h], [sig], len(sig), False, s["use_new_chain_id"], s["chain_id"])
        assert (ok, pub, addr) == (b"\x01", key, want_addr)
    rng = random.Random(5)
    hs, sigs = [], []
    for v in (27, 28, 26, 29):
        h = rng.randbytes(32)
        c, rid = o.ecdsa_sign_compact(h, priv, rng.randrange(1, N).to_bytes(32, "big"))
        hs.append(h)
        sigs.append(c + bytes([v]))
    want = expected(hs, sigs, lambda s: {27: 0, 28: 1}.get(s[64]))
    assert want[0] == b"\x01\x01\x00\x00"
    assert emu_recover(emu, hs, sigs, 65, True, False, 0)[:3] == want


def test_keccak(emu):
    rng = random.Random(13)
    msgs = [rng.randbytes(l) for l in KECCAK_LENGTHS] + [K["keccak256"]["msg_ascii"].encode()]
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    out = ctypes.create_string_buffer(32 * len(msgs))
    emu.emu_keccak256(out, b"".join(msgs), (ctypes.c_uint64 * len(off))(*off), len(msgs))
    assert out.raw == b"".join(o.keccak256(m) for m in msgs)
    assert out.raw[-32:] == bytes.fromhex(K["keccak256"]["hex"])
