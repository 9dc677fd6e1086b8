"""GPU parity of the secp256k1 ECDSA header-signature checks (k_secp.hip through the C ABI)
against the oracle (oracle/secp.c, pinned by tests/golden/secp256k1_kats.json).

Reference: RootProtocol.cs:91-105 -> DefaultCrypto.VerifySignatureHashed (DefaultCrypto.cs:79-101).  Decisions must be
bit-identical to the oracle's on: the reference's own signatures, valid signatures of random keys, high-s twins,
r / s = 0, r >= n, wrong keys / hashes, recovery-id encodings outside [0, 3], chain id 0, wrong signature length, key
indices out of range, unparsable / hybrid / uncompressed keys, x(R) in [n, p) (the r + n branch), R = infinity and
u1 G == u2 Q (the doubling inside the comb sum)."""
import json
import os
import random

import pytest

import oracle as o
import secp_cases
from pyref import secp as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
K = json.load(open(os.path.join(HERE, "golden", "secp256k1_kats.json")))
N, P = o.SECP_N, o.SECP_P
EDGE_X = [x for xs in secp_cases.edge_xs() for x in xs]       # 1, 2, 3, 4, 6, 8, p - 3, p - 4, p - 10, ...


@pytest.fixture(scope="module")
def nat():
    from lachain_amd import native
    native.load()
    return native


def _sign(rng, h, priv, chain, new):
    while True:
        k = rng.randrange(1, N).to_bytes(32, "big")
        try:
            c, rid = o.ecdsa_sign_compact(h, priv, k)
            return o.ecdsa_encode(c, rid, chain, new)
        except ValueError:
            continue


def test_reference_signatures(nat):
    priv = bytes.fromhex(K["priv_address"]["priv"])
    c33, c65 = o.ecdsa_pubkey(priv)
    for s in K["signatures"]:
        h = o.keccak256(bytes.fromhex(s["msg_rlp"]))
        sig = bytes.fromhex(s["sig"])
        new, chain = s["use_new_chain_id"], s["chain_id"]
        L = len(sig)
        for pk, pl in ((c33, 33), (c65, 65)):
            got = nat.ecdsa_verify_hashed_batch(h * 4, sig * 4, L, pk, pl, [0, 0, 0, 1], new, chain)
            assert got == b"\x01\x01\x01\x00"
        assert nat.ecdsa_verify_hashed_batch(h, sig, L, c33, 33, [0], new, 0) == b"\x00"
        assert nat.ecdsa_verify_hashed_batch(h, sig, L, c33, 33, [0], not new, chain) == b"\x00"


def test_header_keccak(nat):
    kh = K["header_keccak"]
    rec = nat.header_bytes(kh["index"], bytes.fromhex(kh["prev"]), bytes.fromhex(kh["merkle"]), bytes.fromhex(kh["state"]),
                           kh["nonce"])
    rng = random.Random(5)
    recs, want = [rec], [bytes.fromhex(kh["hex"])]
    for _ in range(300):
        f = [rng.randbytes(32) for _ in range(3)]
        idx, nonce = rng.getrandbits(64), rng.getrandbits(64)
        recs.append(nat.header_bytes(idx, f[0], f[1], f[2], nonce))
        want.append(o.header_keccak(f[0], f[2], f[1], idx, nonce))   # RLP order: prev, state, merkle
    assert nat.header_keccak_batch(b"".join(recs)) == b"".join(want)


def _mixed_batch(rng, chain, new, n_keys=6, n=1500):
    privs = [rng.randrange(1, N) for _ in range(n_keys)]
    privs[0] = 1                                      # the generator itself as a key
    keys = [o.ecdsa_pubkey(p.to_bytes(32, "big"))[0] for p in privs]
    bad_x = 5
    while o.ecdsa_recover(b"\x01" * 32, bad_x.to_bytes(32, "big") + (1).to_bytes(32, "big"), 0) is not None:
        bad_x += 1
    keys.append(b"\x02" + bad_x.to_bytes(32, "big"))  # x not on the curve
    keys.append(b"\x03" + P.to_bytes(32, "big"))      # x = p
    # the points with the smallest and largest x on the curve (1, 2, 3, ..., p - 3, ...) as keys, both y each
    n_plain = len(keys)
    edge_pts = [pt for x in EDGE_X for pt in S.lift_x(x)]
    keys += [S.compress(pt) for pt in edge_pts]
    hs, sigs, idx = [], [], []
    L = 66 if new else 65
    for i in range(n):
        j = rng.randrange(n_keys)
        priv = privs[j].to_bytes(32, "big")
        kind = i % 16
        h = rng.randbytes(32)
        if kind == 1:
            h = bytes(32)                             # u1 = 0
        elif kind == 2:
            h = N.to_bytes(32, "big")                 # hash >= n reduces to 0
        elif kind == 3:
            h = b"\xff" * 32
        sig = _sign(rng, h, priv, chain, new)
        r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:64], "big")
        tail = sig[64:]
        if kind == 4:
            sig = sig[:32] + (N - s).to_bytes(32, "big") + tail
        elif kind == 5:
            sig = bytes(32) + sig[32:]
        elif kind == 6:
            sig = sig[:32] + bytes(32) + tail
        elif kind == 7 and r + N < 2 ** 256:
            sig = (r + N).to_bytes(32, "big") + sig[32:]
        elif kind == 8:
            j = (j + 1) % n_keys
        elif kind == 9:
            h = bytes([h[0] ^ 0x80]) + h[1:]
        elif kind == 10:
            v = rng.randrange(0, 65536 if new else 256)
            sig = sig[:64] + (v.to_bytes(2, "big") if new else bytes([v]))
        elif kind == 11:
            j = rng.choice([n_keys, n_keys + 1, -1, len(keys) + 3])   # bad keys / out of range
        elif kind == 12 and privs[j] == 1:
            # u1 == u2 with Q == G: the comb sum adds equal points (doubling branch)
            while True:
                k = rng.randrange(1, N).to_bytes(32, "big")
                c, rid = o.ecdsa_sign_compact(b"\0" * 32, priv, k)
                h = c[:32]
                try:
                    c, rid = o.ecdsa_sign_compact(h, priv, k)
                except ValueError:
                    continue
                if c[:32] == h:
                    sig = o.ecdsa_encode(c, rid, chain, new)
                    break
        elif kind == 13:
            # R = infinity: z = -r d (mod n)  =>  u1 + u2 d = 0
            rr = rng.randrange(1, N)
            ss = rng.randrange(1, N // 2)
            h = ((-rr * privs[j]) % N).to_bytes(32, "big")
            sig = rr.to_bytes(32, "big") + ss.to_bytes(32, "big") + tail
        elif kind == 14:
            # x(R) in [n, p): a key recovered for recovery id 2 (appended to the key list)
            while True:
                rr = rng.randrange(1, P - N)
                sig64 = rr.to_bytes(32, "big") + rng.randrange(1, N // 2).to_bytes(32, "big")
                pk = o.ecdsa_recover(h, sig64, 2)
                if pk is not None:
                    break
            keys.append(pk)
            j = len(keys) - 1
            sig = sig64 + tail
        elif kind == 15:
            # an edge-x key Q, whose private key nobody knows: R = a G + b Q, r = x(R), s = r / b, hash = a s verifies
            # under Q by construction (the oracle decides).  Every third one carries an edge x as r instead.
            e = (i // 16) % len(edge_pts)
            j = n_plain + e
            a, b = rng.randrange(1, N), rng.randrange(1, N)
            rr = S.pt_add(S.pt_mul(a, S.G), S.pt_mul(b, edge_pts[e]))[0] % N
            ss = rr * pow(b, -1, N) % N
            if ss > N // 2:
                ss, a = N - ss, N - a
            h = (a * ss % N).to_bytes(32, "big")
            if (i // 16) % 3 == 2:
                rr = EDGE_X[(i // 48) % (len(EDGE_X) // 2)]
            sig = rr.to_bytes(32, "big") + ss.to_bytes(32, "big") + tail
        hs.append(h)
        sigs.append(sig)
        idx.append(j)
    return keys, hs, sigs, idx


@pytest.mark.parametrize("chain,new", [(25, False), (225, True), (1, False), (-3, True)])
def test_mixed_batch_vs_oracle(nat, chain, new):
    rng = random.Random(1000 + chain)
    keys, hs, sigs, idx = _mixed_batch(rng, chain, new)
    L = 66 if new else 65
    H, S, PK = b"".join(hs), b"".join(sigs), b"".join(keys)
    want = o.ecdsa_verify_batch(H, S, L, PK, 33, idx, len(hs), new, chain)
    got = nat.ecdsa_verify_hashed_batch(H, S, L, PK, 33, idx, new, chain)
    assert got == want
    n_acc = sum(want)
    assert 0 < n_acc < len(hs)
    # the 65-byte uncompressed and hybrid encodings of the same keys decide identically
    unc = []
    for k in keys:
        x = int.from_bytes(k[1:], "big")
        y2 = (x ** 3 + 7) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P != y2 or x >= P:
            unc.append(b"\x04" + bytes(64))
            continue
        if (y & 1) != (k[0] & 1):
            y = P - y
        unc.append(bytes([6 + (y & 1)]) + x.to_bytes(32, "big") + y.to_bytes(32, "big"))
    got65 = nat.ecdsa_verify_hashed_batch(H, S, L, b"".join(unc), 65, idx, new, chain)
    assert got65 == o.ecdsa_verify_batch(H, S, L, b"".join(unc), 65, idx, len(hs), new, chain)
    assert got65 == want


def test_wrong_signature_length_rejects_all(nat):
    rng = random.Random(3)
    keys, hs, sigs, idx = _mixed_batch(rng, 25, False, n=64)
    got = nat.ecdsa_verify_hashed_batch(b"".join(hs), b"".join(sigs), 65, b"".join(keys), 33, idx, True, 25)
    assert got == bytes(64)


def test_root_header_batch(nat):
    rng = random.Random(8)
    privs = [rng.randrange(1, N) for _ in range(7)]
    keys = [o.ecdsa_pubkey(p.to_bytes(32, "big"))[0] for p in privs]
    era = 1234
    recs, sigs, idx, want = [], [], [], []
    for i in range(500):
        j = i % 7
        index = era if i % 9 else era + 1
        f = [rng.randbytes(32) for _ in range(3)]
        nonce = rng.getrandbits(64)
        rec = nat.header_bytes(index, f[0], f[1], f[2], nonce)
        h = o.header_keccak(f[0], f[2], f[1], index, nonce)
        sig = _sign(rng, h, privs[j].to_bytes(32, "big"), 225, True)
        if i % 11 == 5:
            j = (j + 3) % 7
        recs.append(rec); sigs.append(sig); idx.append(j)
        want.append(int(index == era and o.ecdsa_verify_hashed(h, sig, keys[j], True, 225)))
    got = nat.root_header_verify_batch(b"".join(recs), era, b"".join(sigs), 66, b"".join(keys), 33, idx, True, 225)
    assert list(got) == want
    assert 0 < sum(want) < len(want)


def test_keyset_device_api_and_cache(nat):
    import torch
    rng = random.Random(21)
    keys, hs, sigs, idx = _mixed_batch(rng, 25, False, n=700)
    H, S, PK = b"".join(hs), b"".join(sigs), b"".join(keys)
    want = o.ecdsa_verify_batch(H, S, 65, PK, 33, idx, len(hs), False, 25)
    ks = nat.EcdsaKeySet(PK, 33)
    try:
        valid = ks.valid()
        assert valid[:6] == b"\x01" * 6 and valid[6:8] == b"\x00\x00"
        dev = torch.device("cuda:0")
        st = torch.cuda.Stream(dev)
        with torch.cuda.stream(st):
            dh = torch.tensor(list(H), dtype=torch.uint8, device=dev)
            ds = torch.tensor(list(S), dtype=torch.uint8, device=dev)
            di = torch.tensor(idx, dtype=torch.int32, device=dev)
            out = torch.zeros(len(hs), dtype=torch.uint8, device=dev)
        rc = nat.lib().lcb_ecdsa_verify_hashed_dev(out.data_ptr(), dh.data_ptr(), ds.data_ptr(), 65, di.data_ptr(),
                                                   len(hs), ks.h, 0, 25, ctypes_stream(st))
        assert rc == 0, nat.lib().lcb_last_error()
        st.synchronize()
        assert bytes(out.cpu().tolist()) == want
    finally:
        ks.close()
    # host API: the same key list twice (cache hit), then a different list
    assert nat.ecdsa_verify_hashed_batch(H, S, 65, PK, 33, idx, False, 25) == want
    assert nat.ecdsa_verify_hashed_batch(H, S, 65, PK, 33, idx, False, 25) == want
    keys2 = keys[1:] + keys[:1]
    idx2 = [(j - 1) % len(keys) if 0 <= j < len(keys) else j for j in idx]
    PK2 = b"".join(keys2)
    assert nat.ecdsa_verify_hashed_batch(H, S, 65, PK2, 33, idx2, False, 25) == \
        o.ecdsa_verify_batch(H, S, 65, PK2, 33, idx2, len(hs), False, 25)


def ctypes_stream(st):
    return st.cuda_stream


def test_empty_batch(nat):
    k = o.ecdsa_pubkey((7).to_bytes(32, "big"))[0]
    assert nat.ecdsa_verify_hashed_batch(b"", b"", 65, k, 33, [], False, 25) == b""


def test_pubkey_and_sign_vs_oracle(nat):
    rng = random.Random(31)
    n = 300
    privs = [rng.randrange(1, N) for _ in range(n)]
    privs[0], privs[1], privs[2] = 0, N, N - 1                 # invalid, invalid, valid edge
    # the smallest and largest keys, the endomorphism's eigenvalue, the halves' width, and every boundary of the comb's
    # signed 8-bit windows: a digit of -128 with its carry, a run of 0xff digits that carries into the window above
    lam, _ = secp_cases.glv()
    edge = [1, 2, 3, N - 2, lam, 2 ** 128, 2 ** 128 - 1] + [0x80 << (8 * w) for w in range(32)] + \
        [(1 << (8 * w)) - 1 for w in range(1, 32)] + [(0x7F << (8 * w)) | ((1 << (8 * w)) - 1) for w in range(1, 32)]
    assert all(0 < e < N for e in edge) and 5 + len(edge) < n
    privs[5:5 + len(edge)] = edge
    pb = b"".join(p.to_bytes(32, "big") for p in privs)
    keys, ok = nat.ecdsa_pubkey_batch(pb)
    for i, p in enumerate(privs):
        if 0 < p < N:
            assert ok[i] == 1 and keys[33 * i:33 * i + 33] == o.ecdsa_pubkey(p.to_bytes(32, "big"))[0]
        else:
            assert ok[i] == 0
    hs = [rng.randbytes(32) for _ in range(n)]
    hs[3] = b"\xff" * 32
    nonces = [rng.randrange(1, N).to_bytes(32, "big") for _ in range(n)]
    nonces[4] = bytes(32)                                     # invalid nonce
    for chain, new in ((25, False), (225, True)):
        sigs, sok = nat.ecdsa_sign_hashed_batch(b"".join(hs), pb, b"".join(nonces), new, chain)
        L = 66 if new else 65
        for i in range(n):
            if not (0 < privs[i] < N) or i == 4:
                assert sok[i] == 0
                continue
            assert sok[i] == 1
            c, rid = o.ecdsa_sign_compact(hs[i], privs[i].to_bytes(32, "big"), nonces[i])
            assert sigs[L * i:L * i + L] == o.ecdsa_encode(c, rid, chain, new)
