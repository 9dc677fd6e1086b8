"""GPU parity of the batched secp256k1 ECIES envelope (k_ecies.hip through the C ABI): ECDH, AES-256-GCM with 16-byte
nonces and the fused Secp256K1Encrypt / Secp256K1Decrypt, against the pure-Python restatement (tests/pyref/ecies.py)
and the OpenSSL answers (tests/golden/ecies_kats.json).

Reference: DefaultCrypto.cs:264-336; TrustlessKeygen.cs:63-76,90-135.  ok, keys, plaintexts and envelopes must be
byte-identical on every class of tests/test_ecies_emul.pools, with zero bytes where ok = 0; no item is filtered out of
a comparison.  Parity with libsecp256k1 / BouncyCastle themselves is unpinned."""
import ctypes
import math
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ecies_emul import (K, N, b32, expected_decrypt, expected_ecdh, expected_encrypt, expected_gcm_decrypt,  # noqa: E402
                             expected_gcm_encrypt, mixed_batch, offsets, packed)
from pyref import ecies as E  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 130, 16 * 256 + 1]
MODES = ["host", "dev", "ctx"]


@pytest.fixture(scope="module")
def nat():
    from lachain_amd import native
    native.load()
    return native


# ---------------------------------------------------------------- one call of an entry point in one of its three forms
def _call(nat, mode, name, outs, ins, tail):
    """outs: byte counts of the output arrays; ins: bytes / (ctype, values) / None; tail: the trailing integers.
    host: lcb_<name>_batch; dev: lcb_<name>_dev on the current stream; ctx: lcb_ctx_<name>_dev on a stream of its own"""
    lib = nat.lib()
    if mode == "host":
        bufs = [(ctypes.c_uint8 * max(1, b))() for b in outs]
        args = []
        for v in ins:
            if v is None:
                args.append(None)
            elif isinstance(v, bytes):
                args.append((ctypes.c_uint8 * max(1, len(v))).from_buffer_copy(v or b"\0"))
            else:
                args.append((v[0] * max(1, len(v[1])))(*v[1]))
        cast = [ctypes.cast(a, f) if a is not None else None
                for a, f in zip(bufs + args, getattr(lib, "lcb_%s_batch" % name).argtypes)]
        rc = getattr(lib, "lcb_%s_batch" % name)(*cast, *tail)
        assert rc == 0, nat.last_error()
        return [bytes(b)[:k] for b, k in zip(bufs, outs)]
    import torch
    dev = torch.device("cuda:0")
    np_of = {ctypes.c_uint32: "int32", ctypes.c_uint64: "int64"}
    with nat.Context() as ctx:
        st = torch.cuda.Stream(dev) if mode == "ctx" else torch.cuda.current_stream()
        with torch.cuda.stream(st):
            bufs = [torch.full((max(1, b),), 0xAA, dtype=torch.uint8, device=dev) for b in outs]
            args = []
            for v in ins:
                if v is None:
                    args.append(None)
                elif isinstance(v, bytes):
                    args.append(torch.frombuffer(bytearray(v or b"\0"), dtype=torch.uint8).to(dev))
                else:
                    args.append(torch.tensor(list(v[1]) or [0], dtype=getattr(torch, np_of[v[0]]), device=dev))
        ptrs = [a.data_ptr() if a is not None else None for a in bufs + args]
        if mode == "ctx":
            rc = getattr(lib, "lcb_ctx_%s_dev" % name)(ctx.ptr, *ptrs, *tail, st.cuda_stream)
        else:
            rc = getattr(lib, "lcb_%s_dev" % name)(*ptrs, *tail, st.cuda_stream)
        assert rc == 0, nat.last_error()
        st.synchronize()
        return [bytes(b.cpu().numpy())[:k] for b, k in zip(bufs, outs)]


def run_ecdh(nat, mode, items, indexed):
    n = len(items)
    pubs = b"".join(p for p, _ in items)
    if indexed:
        table = sorted({d for _, d in items})
        pos = {d: i for i, d in enumerate(table)}
        ins = [pubs, b"".join(table), (ctypes.c_uint32, [pos[d] for _, d in items])]
        tail = [len(table), n]
    else:
        ins, tail = [pubs, b"".join(d for _, d in items), None], [n, n]
    # the ABI's order is (key32_out, ok, pub33, scalars32, scalar_idx, n_scalars, n)
    return _call(nat, mode, "secp_ecdh", [32 * n, n], ins, tail)


def run_gcm_encrypt(nat, mode, items):
    pts = [it[2] for it in items]
    total = sum(len(p) + 32 for p in pts)
    return _call(nat, mode, "aes256_gcm_encrypt", [total],
                 [b"".join(it[0] for it in items), b"".join(it[1] for it in items), b"".join(pts),
                  (ctypes.c_uint64, offsets(pts))], [len(items)])[0]


def run_gcm_decrypt(nat, mode, items):
    cts = [it[1] for it in items]
    total = sum(max(len(c) - 32, 0) for c in cts)
    return _call(nat, mode, "aes256_gcm_decrypt", [total, len(items)],
                 [b"".join(it[0] for it in items), b"".join(cts), (ctypes.c_uint64, offsets(cts))], [len(items)])


def run_encrypt(nat, mode, items):
    pts = [it[3] for it in items]
    total = sum(len(p) + 65 for p in pts)
    return _call(nat, mode, "secp256k1_encrypt", [total, len(items)],
                 [b"".join(it[0] for it in items), b"".join(it[1] for it in items), b"".join(it[2] for it in items),
                  b"".join(pts), (ctypes.c_uint64, offsets(pts))], [len(items)])


def run_decrypt(nat, mode, items, indexed=False):
    cts = [it[1] for it in items]
    total = sum(max(len(c) - 65, 0) for c in cts)
    n = len(items)
    if indexed:
        table = sorted({d for d, _ in items})
        pos = {d: i for i, d in enumerate(table)}
        head, mid = [b"".join(table), (ctypes.c_uint32, [pos[d] for d, _ in items])], [len(table)]
    else:
        head, mid = [b"".join(d for d, _ in items), None], [n]
    lib = nat.lib()
    # the ABI's order is (pt_out, ok, privs32, priv_idx, n_privs, ct, ct_off, n): n_privs sits between the pointers
    if mode == "host":
        out, ok = (ctypes.c_uint8 * max(1, total))(), (ctypes.c_uint8 * n)()
        keep = [(ctypes.c_uint8 * len(head[0])).from_buffer_copy(head[0]),
                (ctypes.c_uint32 * n)(*head[1][1]) if indexed else None,
                (ctypes.c_uint8 * max(1, sum(map(len, cts)))).from_buffer_copy(b"".join(cts) or b"\0"),
                (ctypes.c_uint64 * (n + 1))(*offsets(cts))]
        f = lib.lcb_secp256k1_decrypt_batch
        u8p, u32p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
        rc = f(ctypes.cast(out, u8p), ctypes.cast(ok, u8p), ctypes.cast(keep[0], u8p),
               ctypes.cast(keep[1], u32p) if indexed else None, mid[0], ctypes.cast(keep[2], u8p),
               ctypes.cast(keep[3], u64p), n)
        assert rc == 0, nat.last_error()
        return [bytes(out)[:total], bytes(ok)]
    import torch
    dev = torch.device("cuda:0")
    with nat.Context() as ctx:
        st = torch.cuda.Stream(dev) if mode == "ctx" else torch.cuda.current_stream()
        with torch.cuda.stream(st):
            out = torch.full((max(1, total),), 0xAA, dtype=torch.uint8, device=dev)
            ok = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
            dp = torch.frombuffer(bytearray(head[0]), dtype=torch.uint8).to(dev)
            di = torch.tensor(head[1][1], dtype=torch.int32, device=dev) if indexed else None
            dc = torch.frombuffer(bytearray(b"".join(cts) or b"\0"), dtype=torch.uint8).to(dev)
            do = torch.tensor(offsets(cts), dtype=torch.int64, device=dev)
        a = (out.data_ptr(), ok.data_ptr(), dp.data_ptr(), di.data_ptr() if indexed else None, mid[0], dc.data_ptr(),
             do.data_ptr(), n, st.cuda_stream)
        rc = lib.lcb_ctx_secp256k1_decrypt_dev(ctx.ptr, *a) if mode == "ctx" else lib.lcb_secp256k1_decrypt_dev(*a)
        assert rc == 0, nat.last_error()
        st.synchronize()
        return [bytes(out.cpu().numpy())[:total], bytes(ok.cpu().numpy())]


# ---------------------------------------------------------------- tests
def test_kats_every_entry_point(nat):
    for mode in MODES:
        items = [(bytes.fromhex(e["pub"]), bytes.fromhex(e["scalar"])) for e in K["ecdh"]]
        key, ok = run_ecdh(nat, mode, items, False)
        assert (key, ok) == (b"".join(bytes.fromhex(e["key"]) for e in K["ecdh"]), b"\x01" * len(items))
        items = [tuple(bytes.fromhex(g[k]) for k in ("key", "nonce", "pt")) for g in K["gcm"]]
        assert run_gcm_encrypt(nat, mode, items) == b"".join(bytes.fromhex(g["out"]) for g in K["gcm"])
        items = [tuple(bytes.fromhex(e[k]) for k in ("recipient_pub", "eph_priv", "nonce", "pt")) for e in K["envelopes"]]
        out, ok = run_encrypt(nat, mode, items)
        assert (out, ok) == (b"".join(bytes.fromhex(e["envelope"]) for e in K["envelopes"]), b"\x01" * 4)
        items = [(bytes.fromhex(e["recipient_priv"]), bytes.fromhex(e["envelope"])) for e in K["envelopes"]]
        out, ok = run_decrypt(nat, mode, items)
        assert (out, ok) == (b"".join(bytes.fromhex(e["pt"]) for e in K["envelopes"]), b"\x01" * 4)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("indexed", [False, True])
def test_ecdh_sizes(nat, n, indexed):
    items = mixed_batch("ecdh", n, seed=n)
    want = expected_ecdh(items)
    for mode in MODES if n <= 130 else ["host", "ctx"]:
        key, ok = run_ecdh(nat, mode, items, indexed)
        assert ok == want[1], mode
        assert key == want[0], mode


@pytest.mark.parametrize("n", SIZES)
def test_gcm_sizes(nat, n):
    enc = mixed_batch("gcm_enc", n, seed=n)
    dec = mixed_batch("gcm_dec", n, seed=n + 1)
    want_enc = b"".join(expected_gcm_encrypt(enc))
    plain, want_ok = expected_gcm_decrypt(dec)
    want_dec = packed(plain, [max(len(c) - 32, 0) for _, c in dec])
    for mode in MODES if n <= 130 else ["host", "ctx"]:
        assert run_gcm_encrypt(nat, mode, enc) == want_enc, mode
        out, ok = run_gcm_decrypt(nat, mode, dec)
        assert ok == want_ok, mode
        assert out == want_dec, mode


@pytest.mark.parametrize("n", SIZES)
def test_envelope_sizes(nat, n):
    enc = mixed_batch("enc", n, seed=n)
    dec = mixed_batch("dec", n, seed=n + 1)
    envs, want_eok = expected_encrypt(enc)
    want_enc = b"".join(e if e is not None else bytes(len(it[3]) + 65) for e, it in zip(envs, enc))
    plain, want_dok = expected_decrypt(dec)
    want_dec = packed(plain, [max(len(c) - 65, 0) for _, c in dec])
    for mode in MODES if n <= 130 else ["host", "ctx"]:
        out, ok = run_encrypt(nat, mode, enc)
        assert ok == want_eok, mode
        assert out == want_enc, mode
        for indexed in (False, True):
            out, ok = run_decrypt(nat, mode, dec, indexed)
            assert ok == want_dok, (mode, indexed)
            assert out == want_dec, (mode, indexed)


def test_round_trip_and_python_binding(nat):
    rng = random.Random(9)
    lens = [g["len"] for g in K["gcm"]]
    n = 300
    privs = [b32(rng.randrange(1, N)) for _ in range(5)]
    pubs, pok = nat.ecdsa_pubkey_batch(b"".join(privs))
    assert pok == b"\x01" * 5
    who = [rng.randrange(5) for _ in range(n)]
    pts = [rng.randbytes(lens[i % len(lens)]) for i in range(n)]
    eph = b"".join(b32(rng.randrange(1, N)) for _ in range(n))
    envs, ok = nat.secp256k1_encrypt_batch(b"".join(pubs[33 * w:33 * w + 33] for w in who), eph, rng.randbytes(16 * n), pts)
    assert ok == b"\x01" * n and [len(e) for e in envs] == [len(p) + 65 for p in pts]
    back, ok = nat.secp256k1_decrypt_batch(b"".join(privs), envs, who)
    assert ok == b"\x01" * n and back == pts
    # a spoiled item is rejected and its neighbours keep their plaintexts
    bad = list(envs)
    bad[7] = bad[7][:-1] + bytes([bad[7][-1] ^ 1])
    bad[8] = bad[8][:40]
    back, ok = nat.secp256k1_decrypt_batch(b"".join(privs), bad, who)
    assert ok == bytes(int(i not in (7, 8)) for i in range(n))
    assert back == [None if i in (7, 8) else p for i, p in enumerate(pts)]
    # the halves on their own: the envelope is eph_pub || AesGcmEncrypt(Ecdh(recipient, eph))
    keys, ok = nat.secp_ecdh_batch(b"".join(e[:33] for e in envs), b"".join(privs), who)
    assert ok == b"\x01" * n
    assert nat.aes256_gcm_decrypt_batch(keys, [e[33:] for e in envs]) == (pts, b"\x01" * n)
    assert nat.aes256_gcm_encrypt_batch(keys, b"".join(e[33:49] for e in envs), pts) == [e[33:] for e in envs]
    for i in (0, 150, 299):
        assert E.secp256k1_decrypt(privs[who[i]], envs[i]) == pts[i]
    ms = nat.ecies_phase_ms()
    assert len(ms) == 4 and all(math.isfinite(m) and m >= 0 for m in ms), ms


def test_phase_ms_of_an_explicit_context(nat):
    import torch
    lib = nat.lib()
    dev = torch.device("cuda:0")
    e = K["ecdh"][0]
    pub = torch.frombuffer(bytearray.fromhex(e["pub"]), dtype=torch.uint8).to(dev)
    d = torch.frombuffer(bytearray.fromhex(e["scalar"]), dtype=torch.uint8).to(dev)
    key = torch.zeros(32, dtype=torch.uint8, device=dev)
    ok = torch.zeros(1, dtype=torch.uint8, device=dev)
    ms = (ctypes.c_float * 4)()
    with nat.Context() as ctx:
        assert lib.lcb_ctx_ecies_phase_ms(ctx.ptr, ms) == -1 and b"no ECIES call" in lib.lcb_last_error()
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream())
        assert lib.lcb_ctx_secp_ecdh_dev(ctx.ptr, key.data_ptr(), ok.data_ptr(), pub.data_ptr(), d.data_ptr(), None, 1, 1,
                                         st.cuda_stream) == 0, nat.last_error()
        assert lib.lcb_ctx_ecies_phase_ms(ctx.ptr, ms) == 0, nat.last_error()
        st.synchronize()
    assert all(math.isfinite(m) and m >= 0 for m in ms), list(ms)
    assert bytes(key.cpu().numpy()) == bytes.fromhex(e["key"]) and ok.cpu().tolist() == [1]


def test_empty_batches_and_bad_arguments(nat):
    lib = nat.lib()
    assert nat.secp_ecdh_batch(b"", b"") == (b"", b"")
    assert nat.aes256_gcm_encrypt_batch(b"", b"", []) == []
    assert nat.aes256_gcm_decrypt_batch(b"", []) == ([], b"")
    assert nat.secp256k1_encrypt_batch(b"", b"", b"", []) == ([], b"")
    assert nat.secp256k1_decrypt_batch(b"", []) == ([], b"")
    for f in (lib.lcb_secp_ecdh_batch, lib.lcb_aes256_gcm_encrypt_batch, lib.lcb_aes256_gcm_decrypt_batch,
              lib.lcb_secp256k1_encrypt_batch, lib.lcb_secp256k1_decrypt_batch):
        args = [None if issubclass(a, ctypes._Pointer) else 0 for a in f.argtypes]
        assert f(*args) == 0                                         # n = 0: nothing is read
        args = [None if issubclass(a, ctypes._Pointer) else 1 for a in f.argtypes]
        assert f(*args) == -1 and b"null pointer" in lib.lcb_last_error(), f.__name__
    e = K["envelopes"][0]
    pt, env = bytes.fromhex(e["pt"]), bytes.fromhex(e["envelope"])
    u8 = lambda b: ctypes.cast((ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b or b"\0"), ctypes.POINTER(ctypes.c_uint8))
    out, ok = u8(bytes(400)), u8(bytes(2))
    down = (ctypes.c_uint64 * 3)(0, 97, 32)
    assert lib.lcb_secp256k1_decrypt_batch(out, ok, u8(bytes.fromhex(e["recipient_priv"]) * 2), None, 2, u8(env * 2),
                                           down, 2) == -1
    assert b"offsets must not decrease" in lib.lcb_last_error()
    assert lib.lcb_secp256k1_encrypt_batch(out, ok, u8(env[:33] * 2), u8(bytes([1]) * 64), u8(bytes(32)), u8(pt * 2),
                                           (ctypes.c_uint64 * 3)(0, 32, 31), 2) == -1
    assert b"offsets must not decrease" in lib.lcb_last_error()
    assert lib.lcb_aes256_gcm_encrypt_batch(out, u8(bytes(64)), u8(bytes(32)), u8(pt * 2),
                                            (ctypes.c_uint64 * 3)(5, 4, 4), 2) == -1
    assert lib.lcb_aes256_gcm_decrypt_batch(out, ok, u8(bytes(64)), u8(env * 2), down, 2) == -1
    assert b"offsets must not decrease" in lib.lcb_last_error()
    # a scalar index past the table fails its item, not the call
    c = K["ecdh"][0]
    keys, ok = nat.secp_ecdh_batch(bytes.fromhex(c["pub"]) * 3, bytes.fromhex(c["scalar"]), [0, 1, 0])
    assert ok == b"\x01\x00\x01" and keys == bytes.fromhex(c["key"]) + bytes(32) + bytes.fromhex(c["key"])
    # the library still works after the refused calls
    assert nat.secp256k1_decrypt_batch(bytes.fromhex(e["recipient_priv"]), [env]) == ([pt], b"\x01")
