"""GPU reliable-broadcast Merkle layer (k_rbc.hip, batched k_rs.hip) against the plain-Python
restatement of the reference (tests/pyref/rbc_merkle.py over o.keccak256) and the oracle's Reed-Solomon codec
(o.rs_encode_shards / o.rs_decode_shards): ConstructValMessages, ConstructMerkleTree, CheckEchoMessage,
TrySendReadyMessageFromEchos and MerkleTree.ComputeRoot, bit for bit.  The cases are built in tests/test_rbc_cpu.py,
where the per-lane device functions run on the host against the same expectations.

CheckEchoMessage's n = 1 items run in a call of their own: the entry point takes one n_shards per call, and an empty
proof can only be accepted under T = 1 (at n = 7 the same empty proof is in the 257-item call, rejected)."""
import random

import pytest

import oracle as o
from helpers import gpu_native
from pyref import rbc_merkle as R
from test_rbc_cpu import (ECHO_ITEMS, VAL_CASES, echo_batch, echo_batch_single, flatten_echo, payloads_of, root_trees)

pytestmark = pytest.mark.gpu

UNSOLVABLE_256 = {0, 255} | set(range(1, 169))       # erased shards 0 and 255 share an evaluation point


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


@pytest.fixture(scope="module")
def rbc(nat):
    from lachain_amd import rbc as m
    return m


@pytest.mark.parametrize("n,f,lens", VAL_CASES, ids=[f"n{c[0]}" for c in VAL_CASES])
def test_val_batch_vs_pyref(nat, rbc, n, f, lens):
    payloads = payloads_of(n, lens)
    want = [R.val_messages(p, n, f) for p in payloads]
    shards, roots, proofs = nat.rbc_val_batch(payloads, n, f)
    assert shards == b"".join(b"".join(w[0]) for w in want)
    assert roots == b"".join(w[1] for w in want)
    assert proofs == b"".join(b"".join(b"".join(pr) for pr in w[2]) for w in want)
    assert len(proofs) == 32 * len(payloads) * n * R.depth(n)
    msgs = rbc.construct_val_messages(payloads, n, f)
    for w, inst in zip(want, msgs):
        assert [(m.root, m.proof, m.shard) for m in inst] == [(w[1], w[2][i], w[0][i]) for i in range(n)]


@pytest.mark.parametrize("n", [5, 256])
def test_merkle_tree_batch(nat, n):
    import torch
    rng = random.Random(n)
    insts = [[rng.randbytes(s) for _ in range(n)] for s in (33, 137, 1)]
    want = b"".join(b"".join(R.tree(sh)) for sh in insts)
    flat = b"".join(b"".join(sh) for sh in insts)
    off = [0]
    for sh in insts:
        off.append(off[-1] + sum(len(s) for s in sh))
    assert nat.rbc_merkle_tree_batch(flat, off, n) == want
    assert len(want) == 3 * 2 * R.tree_size(n) * 32
    dev = torch.device("cuda:0")
    dsh = torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(dev)
    doff = torch.tensor(off, dtype=torch.int64, device=dev)
    lib = nat.lib()
    with nat.Context() as ctx:
        for c in (None, ctx.ptr):
            out = torch.zeros(len(want), dtype=torch.uint8, device=dev)
            pre = (c,) if c else ()
            fn = lib.lcb_ctx_rbc_merkle_tree_dev if c else lib.lcb_rbc_merkle_tree_dev
            assert fn(*pre, out.data_ptr(), dsh.data_ptr(), doff.data_ptr(), 3, n,
                      torch.cuda.current_stream().cuda_stream) == 0, lib.lcb_last_error()
            torch.cuda.synchronize()
            assert bytes(out.cpu().numpy()) == want


def test_check_echo_batch(nat, rbc):
    import torch
    n, items = echo_batch()
    assert len(items) == ECHO_ITEMS
    want = bytes(R.check_echo(d, frm, root, pr, n) for d, frm, root, pr in items)
    assert want[:21] == b"\x01" * 21 and want[21:31] == bytes([0, 0, 0, 0, 0, 0, 1, 0, 0, 0])
    data, doff, frm, roots, proofs, poff = flatten_echo(items)
    assert nat.rbc_check_echo_batch(data, doff, frm, roots, proofs, poff, n) == want
    assert rbc.check_echo_messages(items, n) == [bool(w) for w in want]
    # the device form on a stream of the caller's
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    lib = nat.lib()
    with nat.Context() as ctx:
        for c in (None, ctx.ptr):
            with torch.cuda.stream(st):
                dd = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
                dr = torch.frombuffer(bytearray(roots), dtype=torch.uint8).to(dev)
                dp = torch.frombuffer(bytearray(proofs), dtype=torch.uint8).to(dev)
                ddo = torch.tensor(doff, dtype=torch.int64, device=dev)
                dpo = torch.tensor(poff, dtype=torch.int64, device=dev)
                dfr = torch.tensor(frm, dtype=torch.int32, device=dev)
                acc = torch.full((len(items),), 7, dtype=torch.uint8, device=dev)
            pre = (c,) if c else ()
            fn = lib.lcb_ctx_rbc_check_echo_dev if c else lib.lcb_rbc_check_echo_dev
            assert fn(*pre, acc.data_ptr(), dd.data_ptr(), ddo.data_ptr(), dfr.data_ptr(), dr.data_ptr(), dp.data_ptr(),
                      dpo.data_ptr(), len(items), n, st.cuda_stream) == 0, lib.lcb_last_error()
            st.synchronize()
            assert bytes(acc.cpu().numpy()) == want
    # n = 1: the empty proof accepted and rejected
    n1, items1 = echo_batch_single()
    want1 = bytes(R.check_echo(d, frm, root, pr, n1) for d, frm, root, pr in items1)
    assert want1 == bytes([1, 0, 0, 1, 0])
    assert nat.rbc_check_echo_batch(*flatten_echo(items1), n1) == want1


def echoes_of(shards, keep, rng):
    echos = [(j, shards[j]) for j in keep]
    rng.shuffle(echos)                                   # echoes arrive in any order
    return echos


@pytest.mark.parametrize("n,f", [(7, 2), (22, 7)])
def test_decode_batch(nat, rbc, n, f):
    rng = random.Random(n)
    k = n - 2 * f
    payloads = [rng.randbytes(l) for l in (1, 180, 1000, 77)]
    vals = rbc.construct_val_messages(payloads, n, f)
    insts, want_shards = [], []
    for b, msgs in enumerate(vals):
        shards = [m.shard for m in msgs]
        assert (shards, msgs[0].root) == R.val_messages(payloads[b], n, f)[:2]
        echos = echoes_of(shards, rng.sample(range(n), k), rng)
        assert o.rs_decode_shards(echos, len(shards[0]), n, 2 * f) == b"".join(shards)
        insts.append((msgs[0].root, echos))
        want_shards.append(shards)
    # instance 2: one corrupted echo byte decodes to another codeword, whose tree has another root
    frm, d = insts[2][1][1]
    insts[2] = (insts[2][0], [insts[2][1][0], (frm, d[:3] + bytes([d[3] ^ 1]) + d[4:])] + insts[2][1][2:])
    want_shards[2] = R.split(o.rs_decode_shards(insts[2][1], len(d), n, 2 * f), n)
    # instance 3: a duplicate from
    insts[3] = (insts[3][0], [insts[3][1][0]] * 2 + insts[3][1][2:])
    got = rbc.restore_from_echos(insts, n, f)
    for b in (0, 1):
        assert got[b] == (want_shards[b], vals[b][0].root, True)
        assert rbc.payload_from_restored(got[b].shards) == payloads[b]
    assert got[2].shards == want_shards[2] and got[2].root == R.tree(want_shards[2])[1]
    assert got[2].ok is False and got[2].root != vals[2][0].root
    assert got[3] == (None, None, False)
    # the flat form: status, zero output for the failed instance, and no expected roots
    off = [0]
    for _, echos in insts:
        off.append(off[-1] + sum(len(d) for _, d in echos))
    flat = b"".join(d for _, echos in insts for _, d in echos)
    frm = [i for _, echos in insts for i, _ in echos]
    shards, status, root_ok, roots = nat.rbc_decode_batch(flat, off, frm, b"".join(r for r, _ in insts), n, f)
    assert status == bytes([1, 1, 1, 0]) and root_ok == bytes([1, 1, 0, 0])
    s3 = (off[4] - off[3]) // k
    assert shards == b"".join(b"".join(w) for w in want_shards[:3]) + bytes(n * s3)
    assert roots == b"".join(R.tree(w)[1] for w in want_shards[:3]) + bytes(32)
    assert nat.rbc_decode_batch(flat, off, frm, None, n, f) == (shards, status, bytes(4), roots)


def test_decode_batch_256_unsolvable_instance(nat, rbc):
    n, f = 256, 85
    k = n - 2 * f
    rng = random.Random(256)
    payloads = [rng.randbytes(180), bytes(range(200))]
    vals = rbc.construct_val_messages(payloads, n, f)
    shards = [[m.shard for m in msgs] for msgs in vals]
    keep0 = sorted(set(rng.sample(range(1, n), k - 1)) | {0})            # shard 0 kept: solvable
    keep1 = [j for j in range(n) if j not in UNSOLVABLE_256]
    assert len(keep0) == len(keep1) == k
    insts = [(vals[0][0].root, echoes_of(shards[0], keep0, rng)), (vals[1][0].root, echoes_of(shards[1], keep1, rng))]
    assert o.rs_decode_shards(insts[0][1], len(shards[0][0]), n, 2 * f) == b"".join(shards[0])
    assert o.rs_decode_shards(insts[1][1], len(shards[1][0]), n, 2 * f) is None
    got = rbc.restore_from_echos(insts, n, f)
    assert got[0] == (shards[0], vals[0][0].root, True)
    assert rbc.payload_from_restored(got[0].shards) == payloads[0]
    assert got[1] == (None, None, False)


def test_merkle_root_batch(nat, rbc):
    import torch
    trees = root_trees()
    want = [R.compute_root(t) for t in trees]
    assert [w is None for w in want] == [len(t) == 0 for t in trees]
    assert nat.merkle_root_batch(trees) == want
    assert rbc.compute_root(trees[4]) == want[4] and rbc.compute_root([]) is None
    dev = torch.device("cuda:0")
    off = [0]
    for t in trees:
        off.append(off[-1] + len(t))
    dh = torch.frombuffer(bytearray(b"".join(b"".join(t) for t in trees)), dtype=torch.uint8).to(dev)
    doff = torch.tensor(off, dtype=torch.int64, device=dev)
    lib = nat.lib()
    with nat.Context() as ctx:
        for c in (None, ctx.ptr):
            roots = torch.full((32 * len(trees),), 9, dtype=torch.uint8, device=dev)
            status = torch.full((len(trees),), 9, dtype=torch.uint8, device=dev)
            pre = (c,) if c else ()
            fn = lib.lcb_ctx_merkle_root_dev if c else lib.lcb_merkle_root_dev
            assert fn(*pre, roots.data_ptr(), status.data_ptr(), dh.data_ptr(), doff.data_ptr(), len(trees), off[-1],
                      torch.cuda.current_stream().cuda_stream) == 0, lib.lcb_last_error()
            torch.cuda.synchronize()
            assert bytes(status.cpu().numpy()) == bytes(w is not None for w in want)
            assert bytes(roots.cpu().numpy()) == b"".join(w or bytes(32) for w in want)


def test_bad_arguments(nat):
    p = [b"abc"]
    for n, f in [(0, 0), (257, 0), (4, 2), (5, 3), (4, -1)]:
        with pytest.raises(RuntimeError):
            nat.rbc_val_batch(p, n, f)
        with pytest.raises(RuntimeError):
            nat.rbc_decode_batch(bytes(8), [0, 8], [0], None, n, f)
    for n in (0, 257):
        with pytest.raises(RuntimeError):
            nat.rbc_check_echo_batch(b"ab", [0, 2], [0], bytes(32), b"", [0, 0], n)
        with pytest.raises(RuntimeError):
            nat.rbc_merkle_tree_batch(b"ab", [0, 2], n)
    lib = nat.lib()
    keep = []
    down = nat._u64_keep(keep, [0, 8, 4])
    flat = nat._u64_keep(keep, [0, 0, 0])
    _, buf = nat._bytes_ptr_keep(keep, bytes(64))
    _, out = nat._bytes_ptr_keep(keep, bytes(4096))
    frm = nat._i32_keep(keep, [0, 0])
    assert lib.lcb_rbc_val_batch(out, out, out, buf, down, 2, 4, 1) == -1
    assert "offsets" in nat.last_error()
    assert lib.lcb_rbc_check_echo_batch(out, buf, down, frm, buf, buf, flat, 2, 4) == -1
    assert lib.lcb_rbc_check_echo_batch(out, buf, flat, frm, buf, buf, down, 2, 4) == -1
    assert lib.lcb_rbc_merkle_tree_batch(out, buf, down, 2, 4) == -1
    assert lib.lcb_rbc_decode_batch(out, out, out, out, buf, down, frm, None, 2, 4, 1) == -1
    assert lib.lcb_merkle_root_batch(out, out, buf, down, 2) == -1
    with pytest.raises(RuntimeError):
        nat.rbc_merkle_tree_batch(bytes(10), [0, 10], 4)        # 10 bytes are not four equal shards
    with pytest.raises(RuntimeError):
        nat.rbc_decode_batch(bytes(7), [0, 7], [0, 1], None, 4, 1)   # 7 bytes are not two equal echoes
