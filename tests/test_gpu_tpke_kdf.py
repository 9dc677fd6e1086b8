"""GPU tests of the device keystream (k_kdf_xor, lachain_amd/csrc/kdf_lane.hpp) and the two TPKE operations it completes:
Utils.XorWithHash for a batch, PublicKey.Encrypt in one call and PublicKey.FullDecrypt in one call (grouped behind the
share selection, and literally), against the oracle.  The keystream's cases are those of the CPU emulation
(tests/kdf_cases.py): one batch of more than one wave and fewer than two, run from every base alignment.  Keys are
N = 4, F = 1 throughout.  Bit-exact: ciphertexts, plaintexts, status bytes, and every byte around an output range."""
import json
import os
import sys
import threading

import numpy as np
import pytest

import oracle as o
from helpers import Drbg, R, gpu_native

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kdf_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
H = bytes.fromhex
N, F = 4, 1
K = F + 1
ABSENT = 0xFFFFFFFF
INF = bytes(48)
LENS = [0, 1, 33, 289, 1000]


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


@pytest.fixture(scope="module")
def tdev():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def batch():
    items = C.items()
    return items, C.expected(o, items)


@pytest.fixture(scope="module")
def keys():
    """(x_i, y, Y_i) of a degree-F polynomial"""
    d = Drbg(b"gpu-tpke-kdf keys")
    coeffs = [d.fr_int() for _ in range(F + 1)]
    poly = lambda x: sum(c * pow(x, i, R) for i, c in enumerate(coeffs)) % R
    xs = [poly(i + 1) for i in range(N)]
    return xs, o.g1_mul(o.g1_gen(), o.fr(poly(0))), [o.g1_mul(o.g1_gen(), o.fr(x)) for x in xs]


@pytest.fixture(scope="module")
def cts(keys):
    """ciphertexts of the payload lengths LENS with every decryptor's share: [(plain, (U, V, W), [U_i])]"""
    xs, y, _ = keys
    d = Drbg(b"gpu-tpke-kdf cts")
    out = []
    for n in LENS:
        plain = d.bytes(n)
        ct = o.tpke_encrypt(y, plain, o.fr(d.fr_int()))
        out.append((plain, ct, [o.g1_mul(ct[0], o.fr(x)) for x in xs]))
    return out


def up(torch, dev, b):
    if isinstance(b, np.ndarray):
        b = b.tobytes()
    return torch.frombuffer(bytearray(b if len(b) else b"\0"), dtype=torch.uint8).to(dev)


def placed(torch, dev, b, align, fill=0xC3, tail=24):
    """a device buffer with b at byte `align` of an 8-byte aligned base, sentinel bytes around it"""
    t = up(torch, dev, bytes([fill]) * align + b + bytes([fill]) * tail)
    assert t.data_ptr() % 8 == 0
    return t


def u32s(vals):
    return np.array(vals, dtype=np.uint32)


def mismatches(items, got, want):
    return [(i, len(items[i][0]), len(items[i][1])) for i in range(len(items)) if got[i] != want[i]]


# ---------------------------------------------------------------- 1. the primitive against the oracle
@pytest.mark.parametrize("align", C.ALIGNMENTS)
def test_host_form_matches_oracle(nat, batch, align):
    """a leading item of `align` bytes moves every item of the batch to the next start alignment"""
    items, want = batch
    lead = (b"", bytes([0x5A]) * align)
    got = nat.xor_with_hash_batch([lead[0]] + [s for s, _ in items], [lead[1]] + [d for _, d in items])
    assert got[0] == C.expected(o, [lead])[0]
    assert not mismatches(items, got[1:], want)
    assert got[1 + C.reference_index()] == C.reference_vector()[2]


@pytest.mark.parametrize("align", C.ALIGNMENTS)
def test_dev_form_matches_oracle(nat, tdev, batch, align):
    """device pointers at every base alignment; the seeds and the output at other phases than the data"""
    torch, dev = tdev
    items, want = batch
    lib = nat.lib()
    seeds, data = b"".join(s for s, _ in items), b"".join(d for _, d in items)
    sa, oa = (3 * align + 1) % 8, (5 * align + 3) % 8
    d_seed, d_data = placed(torch, dev, seeds, sa), placed(torch, dev, data, align)
    d_out = placed(torch, dev, bytes(len(data)), oa)
    doff = C.offsets([d for _, d in items])
    d_soff, d_doff = up(torch, dev, u32s(C.offsets([s for s, _ in items]))), up(torch, dev, u32s(doff))
    sh = torch.cuda.current_stream(dev).cuda_stream
    assert lib.lcb_xor_with_hash_dev(d_out.data_ptr() + oa, d_seed.data_ptr() + sa, d_soff.data_ptr(),
                                     d_data.data_ptr() + align, d_doff.data_ptr(), len(items), sh) == 0, nat.last_error()
    torch.cuda.synchronize(dev)
    raw = d_out.cpu().numpy().tobytes()
    got = [raw[oa + doff[i]:oa + doff[i + 1]] for i in range(len(items))]
    assert not mismatches(items, got, want)
    assert got[C.reference_index()] == C.reference_vector()[2]
    assert raw[:oa] == b"\xC3" * oa and raw[oa + len(data):] == b"\xC3" * 24


def test_empty_batch_is_a_no_op(nat):
    assert nat.xor_with_hash_batch([], []) == []
    assert nat.tpke_encrypt_batch(bytes(48), [], []) == []
    assert nat.tpke_full_decrypt_batch([]) == []


def test_kernel_time_is_reported(nat):
    assert nat.xor_with_hash_batch([bytes(48)], [bytes(100)]) == [o.xor_with_hash(bytes(48), bytes(100))]
    assert 0 < nat.kdf_phase_ms() < 1000


def test_decreasing_offsets_fail_the_host_call(nat):
    import ctypes
    lib = nat.lib()
    out = (ctypes.c_uint8 * 64)()
    buf = (ctypes.c_uint8 * 64)()
    good, bad = (ctypes.c_uint32 * 3)(0, 8, 16), (ctypes.c_uint32 * 3)(0, 16, 8)
    p8, p32 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    c8 = lambda a: ctypes.cast(a, p8)
    c32 = lambda a: ctypes.cast(a, p32)
    assert lib.lcb_xor_with_hash_batch(c8(out), c8(buf), c32(good), c8(buf), c32(bad), 2) == -1
    assert "must not decrease" in nat.last_error()
    assert lib.lcb_xor_with_hash_batch(c8(out), c8(buf), c32(bad), c8(buf), c32(good), 2) == -1
    assert lib.lcb_xor_with_hash_batch(c8(out), c8(buf), c32(good), c8(buf), c32(good), 2) == 0


# ---------------------------------------------------------------- 2. guard bytes and in place
@pytest.mark.parametrize("in_place", [False, True])
def test_guard_bytes_and_in_place(nat, tdev, batch, in_place):
    """a sub-range of a sentinel-filled buffer (data_off[0] > 0, the buffer longer than data_off[n]): every byte outside
    the range stays; once with out == data"""
    torch, dev = tdev
    items, want = batch
    lib = nat.lib()
    pre, post = 13, 29
    data = b"".join(d for _, d in items)
    doff = C.offsets([d for _, d in items], start=pre)
    whole = b"\xC3" * pre + data + b"\xC3" * post
    d_data = up(torch, dev, whole)
    d_out = d_data if in_place else up(torch, dev, b"\xC3" * len(whole))
    d_seed = up(torch, dev, b"".join(s for s, _ in items))
    d_soff, d_doff = up(torch, dev, u32s(C.offsets([s for s, _ in items]))), up(torch, dev, u32s(doff))
    sh = torch.cuda.current_stream(dev).cuda_stream
    assert lib.lcb_xor_with_hash_dev(d_out.data_ptr(), d_seed.data_ptr(), d_soff.data_ptr(), d_data.data_ptr(),
                                     d_doff.data_ptr(), len(items), sh) == 0, nat.last_error()
    torch.cuda.synchronize(dev)
    raw = d_out.cpu().numpy().tobytes()
    assert raw[:pre] == b"\xC3" * pre and raw[doff[-1]:] == b"\xC3" * post
    got = [raw[doff[i]:doff[i + 1]] for i in range(len(items))]
    assert not mismatches(items, got, want)
    if not in_place:
        assert d_data.cpu().numpy().tobytes() == whole


# ---------------------------------------------------------------- 3. Encrypt
def test_encrypt_batch(nat, tdev, keys):
    torch, dev = tdev
    _, y, _ = keys
    d = Drbg(b"gpu-tpke-kdf encrypt")
    rs = [o.fr(d.fr_int()) for _ in LENS]
    datas = [d.bytes(n) for n in LENS]
    want = [o.tpke_encrypt(y, data, r) for data, r in zip(datas, rs)]
    got = nat.tpke_encrypt_batch(y, rs, datas)
    assert got == want
    # the sequence the one call replaces: phase 1, the host keystream per item, phase 2
    us, ts = nat.tpke_encrypt_phase1(y, rs)
    vs = [nat.xor_with_hash(t, data) for t, data in zip(ts, datas)]
    ws = nat.tpke_encrypt_phase2(us, rs, vs)
    assert got == list(zip(us, vs, ws))
    # r >= the group order fails as phase 1 does
    big = [rs[0], R.to_bytes(32, "little"), rs[2]]
    with pytest.raises(RuntimeError, match="invalid public key or scalar"):
        nat.tpke_encrypt_phase1(y, big)
    with pytest.raises(RuntimeError, match="invalid public key or scalar"):
        nat.tpke_encrypt_batch(y, big, datas[1:4])
    # the device form reports it per item: ok = 0 and a zero V, the neighbours as the oracle
    lib = nat.lib()
    part = datas[1:4]
    off = C.offsets(part)
    d_u, d_w = torch.zeros(48 * 3, dtype=torch.uint8, device=dev), torch.zeros(96 * 3, dtype=torch.uint8, device=dev)
    d_v = up(torch, dev, b"\x77" * off[-1])
    d_ok = torch.zeros(3, dtype=torch.uint8, device=dev)
    d_y, d_r, d_data, d_off = up(torch, dev, y), up(torch, dev, b"".join(big)), up(torch, dev, b"".join(part)), \
        up(torch, dev, u32s(off))
    sh = torch.cuda.current_stream(dev).cuda_stream
    assert lib.lcb_tpke_encrypt_dev(d_u.data_ptr(), d_v.data_ptr(), d_w.data_ptr(), d_ok.data_ptr(), d_y.data_ptr(),
                                    d_r.data_ptr(), d_data.data_ptr(), d_off.data_ptr(), 3, sh) == 0, nat.last_error()
    torch.cuda.synchronize(dev)
    assert d_ok.cpu().numpy().tolist() == [1, 0, 1]
    u, v, w = (t.cpu().numpy().tobytes() for t in (d_u, d_v, d_w))
    assert v[off[1]:off[2]] == bytes(off[2] - off[1])
    for i in (0, 2):
        assert (u[48 * i:48 * i + 48], v[off[i]:off[i + 1]], w[96 * i:96 * i + 96]) == o.tpke_encrypt(y, part[i], big[i])


# ---------------------------------------------------------------- 4. FullDecrypt, grouped form
def full_decrypt_dev(nat, tdev, accept, shares, order, per_ct, k, vs):
    """lcb_tpke_full_decrypt_dev over sentinel-filled outputs -> (status list, plaintext slots)"""
    torch, dev = tdev
    lib = nat.lib()
    n = len(vs)
    voff = C.offsets(vs)
    d_acc, d_sh = up(torch, dev, bytes(accept)), up(torch, dev, b"".join(shares))
    d_ord = up(torch, dev, u32s(order)) if order is not None else None
    d_v, d_voff = up(torch, dev, b"".join(vs)), up(torch, dev, u32s(voff))
    d_pt, d_st = up(torch, dev, b"\x77" * voff[-1]), up(torch, dev, b"\x77" * n)
    sh = torch.cuda.current_stream(dev).cuda_stream
    assert lib.lcb_tpke_full_decrypt_dev(d_pt.data_ptr(), d_st.data_ptr(), d_acc.data_ptr(), d_sh.data_ptr(),
                                         d_ord.data_ptr() if d_ord is not None else None, per_ct, k, d_v.data_ptr(),
                                         d_voff.data_ptr(), n, sh) == 0, nat.last_error()
    torch.cuda.synchronize(dev)
    pt = d_pt.cpu().numpy().tobytes()
    return d_st.cpu().numpy().tolist()[:n], [pt[voff[i]:voff[i + 1]] for i in range(n)]


def test_full_decrypt_grouped(nat, tdev, cts):
    plains = [p for p, _, _ in cts]
    vs = [ct[1] for _, ct, _ in cts]
    flat = [s for _, _, sh in cts for s in sh]
    # valid shares everywhere: the oracle's plaintexts (which are the payloads)
    st, pt = full_decrypt_dev(nat, tdev, [1] * (N * len(cts)), flat, None, N, K, vs)
    assert st == [1] * len(cts) and pt == plains
    for (_, ct, sh), p in zip(cts, pt):
        assert p == o.tpke_full_decrypt(ct[1], [0, 1], sh[:2])
    # group 2 has one accepted share (< k): status 0 and an all-zero slot, the neighbours intact; group 3's accepted
    # shares are 1 and 3
    accept = [1] * (N * len(cts))
    accept[2 * N:3 * N] = [0, 0, 1, 0]
    accept[3 * N:4 * N] = [0, 1, 0, 1]
    st, pt = full_decrypt_dev(nat, tdev, accept, flat, None, N, K, vs)
    assert st == [1, 1, 0, 1, 1]
    assert pt[2] == bytes(len(vs[2])) and len(vs[2]) == 33
    assert [pt[i] for i in (0, 1, 3, 4)] == [plains[i] for i in (0, 1, 3, 4)]
    # every share the point at infinity: u is the point at infinity
    st, pt = full_decrypt_dev(nat, tdev, [1] * (N * len(cts)), [INF] * len(flat), None, N, K, vs)
    assert st == [1] * len(cts)
    assert pt == [o.xor_with_hash(INF, v) for v in vs]
    assert pt[3] == o.tpke_full_decrypt(vs[3], [0, 1], [INF, INF])


def test_full_decrypt_ordered_picks_by_arrival(nat, tdev, cts, keys):
    """decryptor 0's share is another valid point with its accept bit set, so a combination that takes it gives another
    plaintext: index order takes it, the arrival orders below do or do not"""
    vs = [ct[1] for _, ct, _ in cts]
    shares = [list(sh) for _, _, sh in cts]
    for sh in shares:
        sh[0] = o.g1_add(sh[0], o.g1_gen())
    flat = [s for sh in shares for s in sh]
    orders = [[3, 1, 0, 2], [0, 3, 1, 2], [2, ABSENT, 0, ABSENT], [ABSENT, 1, 2, 3], [1, 1, 2, 3]]
    st, pt = full_decrypt_dev(nat, tdev, [1] * len(flat), flat, [x for r in orders for x in r], N, K, vs)
    assert st == [1, 1, 1, 1, 0]                             # a position listed twice: repeated abscissa
    for c, ids in enumerate([[3, 1], [0, 3], [2, 0], [1, 2]]):
        assert pt[c] == o.tpke_full_decrypt(vs[c], ids, [shares[c][i] for i in ids]), c
    assert pt[0] == cts[0][0] and pt[3] == cts[3][0] and pt[1] != cts[1][0] and pt[2] != cts[2][0]
    assert pt[4] == bytes(len(vs[4]))
    st, pt = full_decrypt_dev(nat, tdev, [1] * len(flat), flat, None, N, K, vs)
    assert st == [1] * 5
    assert pt == [o.tpke_full_decrypt(vs[c], [0, 1], shares[c][:2]) for c in range(5)]


@pytest.mark.parametrize("key", ["tpke_n4", "tpke_n22"])
def test_full_decrypt_replays_transcripts(nat, tdev, key):
    """tests/golden/transcripts.json: the fixture's accept bits, its combine_ids as the arrival order"""
    with open(os.path.join(HERE, "golden", "transcripts.json")) as f:
        t = json.load(f)[key]
    n, k = t["n"], t["f"] + 1
    accept, flat, order, vs = [], [], [], []
    for c in t["ciphertexts"]:
        accept += [int(a) for a in c["accept"]]
        flat += [H(s) for s in c["shares"]]
        order += list(c["combine_ids"]) + [ABSENT] * (n - len(c["combine_ids"]))
        vs.append(H(c["v"]))
    st, pt = full_decrypt_dev(nat, tdev, accept, flat, order, n, k, vs)
    assert st == [1] * len(vs)
    assert [p.hex() for p in pt] == [c["plaintext"] for c in t["ciphertexts"]]


# ---------------------------------------------------------------- 5. FullDecrypt, literal form, and the mirror
def test_full_decrypt_literal(nat, cts):
    picks = [[0, 1], [1, 2, 3], [3, 0, 2, 1], [2, 0], [1, 3, 0]]
    problems = [(ids, [cts[c][2][i] for i in ids], cts[c][1][1]) for c, ids in enumerate(picks)]
    got = nat.tpke_full_decrypt_batch(problems)
    assert got == [o.tpke_full_decrypt(v, ids, uis) for ids, uis, v in problems]
    assert got == [p for p, _, _ in cts]
    # a repeated id: status 0, the neighbours unaffected
    problems[2] = ([3, 0, 3], [cts[2][2][i] for i in (3, 0, 3)], cts[2][1][1])
    got = nat.tpke_full_decrypt_batch(problems)
    assert got[2] is None and [got[i] for i in (0, 1, 3, 4)] == [cts[i][0] for i in (0, 1, 3, 4)]


def test_mirror_batches_round_trip(nat):
    from lachain_amd import tpke
    from lachain_amd.mcl import Fr
    d = Drbg(b"gpu-tpke-kdf mirror")
    gen = tpke.TrustedKeyGen(N, F, [Fr.FromBytes(d.fr()) for _ in range(F)])
    pub = gen.GetPubKey()
    privs = [gen.GetPrivKey(i) for i in range(N)]
    vks = [gen.GetVerificationPubKey(i) for i in range(N)]
    raws = [tpke.RawShare(d.bytes(n), 10 + j) for j, n in enumerate(LENS)]
    rs = [Fr.FromBytes(d.fr()) for _ in raws]
    enc = pub.EncryptBatch(raws, rs)
    assert enc == [pub.Encrypt(raw, r) for raw, r in zip(raws, rs)]
    assert len(pub.EncryptBatch(raws)) == len(raws)                       # its own randomness
    parts = [priv.DecryptBatch(enc) for priv in privs]                     # parts[i][c]
    assert all(p is not None for row in parts for p in row)
    flat = [(c, parts[i][c]) for c in range(len(enc)) for i in range(N)]
    assert tpke.PublicKey.VerifyShares(vks, enc, flat) == [True] * len(flat)
    lists = [[parts[i][c] for i in ids] for c, ids in enumerate([[0], [1, 2], [3, 2, 1, 0], [2], [0, 3]])]
    got = pub.FullDecryptBatch(enc, lists)
    assert got == raws
    assert got == [pub.FullDecrypt(e, us) for e, us in zip(enc, lists)]
    assert tpke.Utils.XorWithHashBatch([e.U for e in enc], [e.V for e in enc]) == \
        [tpke.Utils.XorWithHash(e.U, e.V) for e in enc]
    # the reference's three checks: too few shares, a repeated DecryptorId, a ShareId of another ciphertext
    bad = list(lists)
    bad[0] = []
    bad[2] = [parts[1][2], parts[3][2], parts[1][2]]
    bad[4] = [parts[0][4], parts[3][3]]
    got = pub.FullDecryptBatch(enc, bad)
    assert [g is None for g in got] == [True, False, True, False, True]
    assert got[1] == raws[1] and got[3] == raws[3]
    for c in (0, 2, 4):
        with pytest.raises(ValueError):
            pub.FullDecrypt(enc[c], bad[c])


# ---------------------------------------------------------------- 6. two threads, each in its own context
def test_two_threads_host_forms(nat, keys, cts):
    """the host forms run in the calling thread's own context: named buffers and HostCall scopes must not mix"""
    _, y, _ = keys
    jobs = []
    for t in range(2):
        d = Drbg(b"gpu-tpke-kdf thread %d" % t)
        lens = LENS if t == 0 else LENS[::-1] + [64]
        rs = [o.fr(d.fr_int()) for _ in lens]
        datas = [d.bytes(n) for n in lens]
        picks = [[(c + t) % N, (c + t + 1 + (c % 2)) % N] for c in range(len(cts))]
        problems = [(ids, [cts[c][2][i] for i in ids], cts[c][1][1]) for c, ids in enumerate(picks)]
        jobs.append((rs, datas, [o.tpke_encrypt(y, data, r) for data, r in zip(datas, rs)], problems))
    plains = [p for p, _, _ in cts]
    errors = []
    start = threading.Barrier(2)

    def work(t):
        rs, datas, want, problems = jobs[t]
        try:
            start.wait(timeout=30)
            for _ in range(4):
                assert nat.tpke_encrypt_batch(y, rs, datas) == want
                assert nat.tpke_full_decrypt_batch(problems) == plains
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
