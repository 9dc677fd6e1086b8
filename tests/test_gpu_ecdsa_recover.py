"""GPU parity of batched secp256k1 public-key recovery (k_secp_recover.hip through the C ABI) and the device Keccak-256
against the oracle (o.ecdsa_recover, o.keccak256, o.ecdsa_pubkey; pinned by tests/golden/secp256k1_kats.json).

Reference: TransactionVerifier.cs:72-91,124-130 -> DefaultCrypto.RecoverSignatureHashed / SpecialRecoverSignatureHashed /
ComputeAddress (DefaultCrypto.cs:146-200).  ok, key and address must be byte-identical to the oracle's on every class of
tests/test_secp_recover_emul.mixed_batch; no item is filtered out of a comparison."""
import ctypes
import os
import random
import sys

import pytest

import oracle as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_secp_recover_emul import K, KECCAK_LENGTHS, N, address_of, expected, mixed_batch, rec_id  # noqa: E402

pytestmark = pytest.mark.gpu

PRIV = bytes.fromhex(K["priv_address"]["priv"])
ADDR = bytes.fromhex(K["priv_address"]["address"])


@pytest.fixture(scope="module")
def nat():
    from lachain_amd import native
    native.load()
    return native


@pytest.fixture(scope="module")
def big():
    """one batch of 16 * 256 + 1 items with the oracle's results, shared by the size and device-form tests"""
    hs, sigs, _ = mixed_batch(random.Random(77), 25, False, n=16 * 256 + 1)
    return hs, sigs, expected(hs, sigs, lambda s: rec_id(s, 25, False))


def _flip(addr: bytes, i: int, bit: int) -> bytes:
    b = bytearray(addr)
    b[20 * i + bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def test_golden_signatures_every_entry_point(nat):
    import torch
    key = o.ecdsa_pubkey(PRIV)[0]
    assert address_of(key) == ADDR
    dev = torch.device("cuda:0")
    lib = nat.lib()
    for s in K["signatures"]:
        h, sig = o.keccak256(bytes.fromhex(s["msg_rlp"])), bytes.fromhex(s["sig"])
        new, chain, L = s["use_new_chain_id"], s["chain_id"], len(sig)
        assert nat.ecdsa_recover_hashed_batch(h * 3, sig * 3, L, new, chain) == (key * 3, ADDR * 3, b"\x01" * 3)
        rec = rec_id(sig, chain, new)
        assert rec in (0, 1)
        assert nat.ecdsa_special_recover_hashed_batch(h, sig[:64] + bytes([27 + rec])) == (key, ADDR, b"\x01")
        # transaction check: the right From, one flipped bit, chain id 0, the other chain-id form, a wrong length
        assert nat.tx_verify_batch(h * 2, sig * 2, L, ADDR * 2, new, chain) == b"\x01\x01"
        for bit in (0, 77, 159):
            assert nat.tx_verify_batch(h * 2, sig * 2, L, _flip(ADDR * 2, 1, bit), new, chain) == b"\x01\x00"
        assert nat.tx_verify_batch(h * 2, sig * 2, L, ADDR * 2, new, 0) == b"\x00\x00"
        assert nat.tx_verify_batch(h * 2, sig * 2, L, ADDR * 2, not new, chain) == b"\x00\x00"
        assert nat.tx_verify_batch(h * 2, (sig + b"\0") * 2, L + 1, ADDR * 2, new, chain) == b"\x00\x00"
        assert nat.ecdsa_recover_hashed_batch(h, sig, L, new, 0) == (bytes(33), bytes(20), b"\x00")
        assert nat.ecdsa_recover_hashed_batch(h, sig, L, not new, chain) == (bytes(33), bytes(20), b"\x00")
        assert nat.ecdsa_recover_hashed_batch(h, sig[:64], 64, new, chain) == (bytes(33), bytes(20), b"\x00")
        # device-pointer forms, without and with an explicit context; null outputs are allowed
        dh = torch.tensor(list(h), dtype=torch.uint8, device=dev)
        ds = torch.tensor(list(sig), dtype=torch.uint8, device=dev)
        dsp = torch.tensor(list(sig[:64] + bytes([27 + rec])), dtype=torch.uint8, device=dev)
        dfrom = torch.tensor(list(ADDR), dtype=torch.uint8, device=dev)
        with nat.Context() as ctx:
            for c in (None, ctx.ptr):
                pub = torch.zeros(33, dtype=torch.uint8, device=dev)
                addr = torch.zeros(20, dtype=torch.uint8, device=dev)
                ok = torch.zeros(3, dtype=torch.uint8, device=dev)
                st = torch.cuda.current_stream().cuda_stream
                pre = (c,) if c else ()
                f = lib.lcb_ctx_ecdsa_recover_hashed_dev if c else lib.lcb_ecdsa_recover_hashed_dev
                assert f(*pre, pub.data_ptr(), None, ok.data_ptr(), dh.data_ptr(), ds.data_ptr(), L, 1, int(new), chain,
                         st) == 0, lib.lcb_last_error()
                f = lib.lcb_ctx_ecdsa_special_recover_hashed_dev if c else lib.lcb_ecdsa_special_recover_hashed_dev
                assert f(*pre, None, addr.data_ptr(), ok[1:].data_ptr(), dh.data_ptr(), dsp.data_ptr(), 65, 1,
                         st) == 0, lib.lcb_last_error()
                f = lib.lcb_ctx_tx_verify_dev if c else lib.lcb_tx_verify_dev
                assert f(*pre, ok[2:].data_ptr(), dh.data_ptr(), ds.data_ptr(), L, dfrom.data_ptr(), 1, int(new), chain,
                         st) == 0, lib.lcb_last_error()
                torch.cuda.synchronize()
                assert bytes(pub.cpu().tolist()) == key and bytes(addr.cpu().tolist()) == ADDR
                assert ok.cpu().tolist() == [1, 1, 1]


def test_special_form(nat):
    rng = random.Random(5)
    hs, sigs = [], []
    for i in range(64):
        h = rng.randbytes(32)
        c, rid = o.ecdsa_sign_compact(h, PRIV, rng.randrange(1, N).to_bytes(32, "big"))
        hs.append(h)
        sigs.append(c + bytes([(27 + rid, 27 + (rid ^ 1), 26, 29)[i % 4]]))    # the signer's id, the other id, bad v
    want = expected(hs, sigs, lambda s: {27: 0, 28: 1}.get(s[64]))
    assert want[0] == b"\x01\x01\x00\x00" * 16
    pub, addr, ok = nat.ecdsa_special_recover_hashed_batch(b"".join(hs), b"".join(sigs))
    assert (ok, pub, addr) == want
    key = o.ecdsa_pubkey(PRIV)[0]
    assert [i for i in range(64) if pub[33 * i:33 * i + 33] == key] == list(range(0, 64, 4))
    # a 66-byte stride is not the special form
    assert nat.ecdsa_special_recover_hashed_batch(hs[0], sigs[0] + b"\0", 66) == (bytes(33), bytes(20), b"\x00")


@pytest.mark.parametrize("chain,new", [(25, False), (225, True), (1, False), (-3, True)])
def test_mixed_batch_vs_oracle(nat, chain, new):
    hs, sigs, notes = mixed_batch(random.Random(3000 + chain), chain, new, n=1500)
    L = 66 if new else 65
    want_ok, want_pub, want_addr = expected(hs, sigs, lambda s: rec_id(s, chain, new))
    H, S = b"".join(hs), b"".join(sigs)
    pub, addr, ok = nat.ecdsa_recover_hashed_batch(H, S, L, new, chain)
    assert ok == want_ok
    assert pub == want_pub
    assert addr == want_addr
    from20 = want_addr
    for i in range(0, len(hs), 3):
        from20 = _flip(from20, i, (7 * i) % 160)
    assert nat.tx_verify_batch(H, S, L, from20, new, chain) == bytes(int(want_ok[i] and i % 3 != 0) for i in range(len(hs)))
    # what the oracle says about the classes (the inputs are what the batch builder claims)
    high = [want_ok[i] for i, (_, nt) in enumerate(notes) if nt and nt[0] == "high-x"]
    assert sum(high) >= 20 and len(high) - sum(high) >= 20, (sum(high), len(high))
    for i, (kind, nt) in enumerate(notes):
        key = want_pub[33 * i:33 * i + 33]
        if nt and nt[0] == "infinity":
            assert want_ok[i] == 0, i
        elif nt and nt[0] == "recovers":
            assert want_ok[i] == 1, i
        elif nt and nt[0] == "flipped":
            assert want_ok[i] == 1 and key == nt[1], i
        elif nt and nt[0] == "unflipped":
            assert want_ok[i] == 1 and key != nt[1], i
        elif kind in (4, 7, 8):
            assert want_ok[i] == 0, i
        elif kind in (0, 2, 11, 14, 15):
            assert want_ok[i] == 1, i


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 16 * 256 + 1])
def test_sizes(nat, big, n):
    hs, sigs, (want_ok, want_pub, want_addr) = big
    pub, addr, ok = nat.ecdsa_recover_hashed_batch(b"".join(hs[:n]), b"".join(sigs[:n]), 65, False, 25)
    assert (ok, pub, addr) == (want_ok[:n], want_pub[:33 * n], want_addr[:20 * n])


def test_round_trip(nat):
    rng = random.Random(41)
    n = 4097
    privs = b"".join(rng.randrange(1, N).to_bytes(32, "big") for _ in range(n))
    hashes, nonces = rng.randbytes(32 * n), b"".join(rng.randrange(1, N).to_bytes(32, "big") for _ in range(n))
    keys, kok = nat.ecdsa_pubkey_batch(privs)
    assert kok == b"\x01" * n
    for chain, new in ((25, False), (225, True)):
        sigs, sok = nat.ecdsa_sign_hashed_batch(hashes, privs, nonces, new, chain)
        assert sok == b"\x01" * n
        pub, addr, ok = nat.ecdsa_recover_hashed_batch(hashes, sigs, 66 if new else 65, new, chain)
        assert ok == b"\x01" * n
        assert pub == keys
    for i in (0, n // 2, n - 1):
        assert addr[20 * i:20 * i + 20] == address_of(keys[33 * i:33 * i + 33])


def test_device_forms_on_a_stream(nat, big):
    import torch
    hs, sigs, (want_ok, want_pub, want_addr) = big
    n = 1500
    H, S = b"".join(hs[:n]), b"".join(sigs[:n])
    host = nat.ecdsa_recover_hashed_batch(H, S, 65, False, 25)
    assert host == (want_pub[:33 * n], want_addr[:20 * n], want_ok[:n])
    acc_host = nat.tx_verify_batch(H, S, 65, want_addr[:20 * n], False, 25)
    assert acc_host == want_ok[:n]
    dev = torch.device("cuda:0")
    lib = nat.lib()
    st = torch.cuda.Stream(dev)
    with nat.Context() as ctx:
        for c in (None, ctx.ptr):
            with torch.cuda.stream(st):
                dh = torch.frombuffer(bytearray(H), dtype=torch.uint8).to(dev)
                ds = torch.frombuffer(bytearray(S), dtype=torch.uint8).to(dev)
                dfrom = torch.frombuffer(bytearray(want_addr[:20 * n]), dtype=torch.uint8).to(dev)
                pub = torch.zeros(33 * n, dtype=torch.uint8, device=dev)
                addr = torch.zeros(20 * n, dtype=torch.uint8, device=dev)
                ok = torch.zeros(n, dtype=torch.uint8, device=dev)
                acc = torch.zeros(n, dtype=torch.uint8, device=dev)
            pre = (c,) if c else ()
            f = lib.lcb_ctx_ecdsa_recover_hashed_dev if c else lib.lcb_ecdsa_recover_hashed_dev
            assert f(*pre, pub.data_ptr(), addr.data_ptr(), ok.data_ptr(), dh.data_ptr(), ds.data_ptr(), 65, n, 0, 25,
                     st.cuda_stream) == 0, lib.lcb_last_error()
            ms = (ctypes.c_float * 3)()
            f = lib.lcb_ctx_ecdsa_recover_phase_ms if c else lib.lcb_ecdsa_recover_phase_ms
            assert f(*pre, ms) == 0, lib.lcb_last_error()
            assert all(m > 0 for m in ms), list(ms)
            f = lib.lcb_ctx_tx_verify_dev if c else lib.lcb_tx_verify_dev
            assert f(*pre, acc.data_ptr(), dh.data_ptr(), ds.data_ptr(), 65, dfrom.data_ptr(), n, 0, 25,
                     st.cuda_stream) == 0, lib.lcb_last_error()
            st.synchronize()
            got = (bytes(pub.cpu().numpy()), bytes(addr.cpu().numpy()), bytes(ok.cpu().numpy()))
            assert got == host
            assert bytes(acc.cpu().numpy()) == acc_host
    assert all(m > 0 for m in nat.ecdsa_recover_phase_ms())


def test_device_keccak(nat):
    import torch
    rng = random.Random(13)
    msgs = [rng.randbytes(l) for l in KECCAK_LENGTHS] + [K["keccak256"]["msg_ascii"].encode()]
    msgs += [rng.randbytes(rng.randrange(601)) for _ in range(300)]
    want = b"".join(o.keccak256(m) for m in msgs)
    assert want[32 * len(KECCAK_LENGTHS):][:32] == bytes.fromhex(K["keccak256"]["hex"])
    assert nat.keccak256_batch(msgs) == want
    assert nat.keccak256_batch([]) == b""
    # device form: raw transaction RLPs hashed on the device feed the recovery (RecoverSignature = Keccak + recover)
    dev = torch.device("cuda:0")
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    dd = torch.frombuffer(bytearray(b"".join(msgs)), dtype=torch.uint8).to(dev)
    doff = torch.tensor(off, dtype=torch.int64, device=dev)
    out = torch.zeros(32 * len(msgs), dtype=torch.uint8, device=dev)
    lib = nat.lib()
    with nat.Context() as ctx:
        for c in (None, ctx.ptr):
            out.zero_()
            pre = (c,) if c else ()
            f = lib.lcb_ctx_keccak256_dev if c else lib.lcb_keccak256_dev
            assert f(*pre, out.data_ptr(), dd.data_ptr(), doff.data_ptr(), len(msgs),
                     torch.cuda.current_stream().cuda_stream) == 0, lib.lcb_last_error()
            torch.cuda.synchronize()
            assert bytes(out.cpu().numpy()) == want
