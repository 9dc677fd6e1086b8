"""CPU checks of the reliable-broadcast Merkle layer (lachain_amd/csrc/k_rbc.hip, rbc_lane.hpp):
the plain-Python restatement (tests/pyref/rbc_merkle.py) against itself and hand-written trees, the per-lane device
functions compiled for the host by tools/emul/rbc_emul.cpp and run lane by lane against the restatement, and the two
size functions of the built library.  TEST INFRASTRUCTURE: catches logic errors in the device code without a GPU; the
kernels themselves (the tree kernel's barriers included) are covered by tests/test_gpu_rbc.py, which shares the cases
built here.

Reference: ReliableBroadcast.cs:296-338,366-386 and MerkleTree.cs:139-191."""
import ctypes
import os
import random
import subprocess

import pytest

import oracle as o
from pyref import rbc_merkle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emul", "rbc_emul.cpp")
LIB = os.path.join(ROOT, "tools", "emul", "librbc_emul.so")
CSRC = os.path.join(ROOT, "lachain_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("rbc_lane.hpp", "keccak.hpp")]
SO = os.path.join(ROOT, "lachain_amd", "liblachain_bls.so")

# (n, f, payload lengths): one val_batch call each.  T = 1 (empty proofs), padding leaves (n = 3, 5, 7, 22), the
# Keccak rate boundaries at n = 4, f = 1 (266, 268, 270 -> S = 135, 136, 137: pad bytes merged into 0x81, a pad block of
# its own, one byte into the second block), a multi-block shard (1200 -> S = 602) and five instances of different
# lengths in one call at n = 7
VAL_CASES = [
    (1, 0, [1, 180]), (2, 0, [1, 180]), (3, 0, [1, 180]), (4, 1, [1, 180, 266, 268, 270, 1200]), (5, 1, [1, 180]),
    (7, 2, [1, 180, 0, 1000, 77]), (22, 7, [1, 180]), (256, 85, [1, 180]),
]
ROOT_TREE_SIZES = [0, 1, 2, 3, 5, 8, 257]
ECHO_ITEMS = 257


def payloads_of(n, lens):
    rng = random.Random(1000 * n + len(lens))
    return [rng.randbytes(l) for l in lens]


def echo_batch():
    """One check_echo call at n = 7: (n, items), item = (data, from, root, proof list).  Every valid (instance, i) of a
    three-instance batch with different shard lengths, then one of each way to be wrong, an over-long proof (accepted:
    the reference ignores the tail), and seeded random mutations up to 257 items (a second block partly filled)."""
    n, f = 7, 2
    rng = random.Random(77)
    inst = [R.val_messages(p, n, f) for p in payloads_of(n, [1, 180, 1000])]
    items = [(sh[i], i, root, pr[i]) for sh, root, pr in inst for i in range(n)]
    sh, root, pr = inst[1]

    def flip(b, at):
        return b[:at] + bytes([b[at] ^ 0x20]) + b[at + 1:]

    items += [
        (flip(sh[2], 5), 2, root, pr[2]),                                   # a flipped data byte
        (sh[2], 2, root, [flip(pr[2][0], 31)] + pr[2][1:]),                 # a flipped proof byte at the leaf level
        (sh[2], 2, root, pr[2][:-1] + [flip(pr[2][-1], 0)]),                # ... at the top level
        (sh[2], 2, inst[0][1], pr[2]),                                      # a wrong root
        (sh[2], 4, root, pr[2]),                                            # shard 2's proof presented with from = 4
        (sh[3], 3, root, pr[3][:-1]),                                       # one entry short
        (sh[3], 3, root, pr[3] + [rng.randbytes(32)]),                      # one extra entry: ignored
        (sh[0], -1, root, pr[0]), (sh[0], n, root, pr[0]),                  # from outside [0, n)
        (sh[0], 0, root, []),                                               # an empty proof under T = 8
    ]
    while len(items) < ECHO_ITEMS:
        b, i = rng.randrange(3), rng.randrange(n)
        sh, root, pr = inst[b]
        kind = rng.randrange(5)
        if kind == 0:
            items.append((sh[i], i, root, pr[i]))
        elif kind == 1:
            items.append((flip(sh[i], rng.randrange(len(sh[i]))), i, root, pr[i]))
        elif kind == 2:
            j = rng.randrange(3)
            items.append((sh[i], i, root, pr[i][:j] + [flip(pr[i][j], rng.randrange(32))] + pr[i][j + 1:]))
        elif kind == 3:
            items.append((sh[i], rng.randrange(-2, n + 2), root, pr[i]))
        else:
            items.append((sh[i], i, root, pr[i][:rng.randrange(5)] + [rng.randbytes(32)] * rng.randrange(2)))
    return n, items


def echo_batch_single():
    """n = 1 (T = 1): the root is the leaf hash and the proof is empty; extra entries are ignored"""
    sh, root, pr = R.val_messages(b"one validator", 1, 0)
    assert pr == [[]] and root == o.keccak256(sh[0])
    return 1, [(sh[0], 0, root, []), (sh[0], 0, bytes(32), []), (sh[0] + b"x", 0, root, []), (sh[0], 0, root, [root]),
               (sh[0], 1, root, [])]


def flatten_echo(items):
    """(data, data_off, from, roots, proofs, proof_off) as the ABI takes them; proof offsets in hashes"""
    doff, poff = [0], [0]
    for d, _, _, p in items:
        doff.append(doff[-1] + len(d))
        poff.append(poff[-1] + len(p))
    return (b"".join(it[0] for it in items), doff, [it[1] for it in items], b"".join(it[2] for it in items),
            b"".join(b"".join(it[3]) for it in items), poff)


def root_trees():
    rng = random.Random(99)
    return [[rng.randbytes(32) for _ in range(c)] for c in ROOT_TREE_SIZES]


# ---------------------------------------------------------------- the restatement against itself and by hand
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 22, 256])
def test_pyref_branches_pass_their_own_echo_check(n):
    rng = random.Random(n)
    shards = [rng.randbytes(33) for _ in range(n)]
    nodes = R.tree(shards)
    t = R.tree_size(n)
    assert len(nodes) == 2 * t and t >= n and (t == 1 or t // 2 < n)
    assert all(nodes[t + i] == bytes(32) for i in range(n, t))
    for i in range(n):
        br = R.branch(nodes, i)
        assert len(br) == R.depth(n)
        assert R.check_echo(shards[i], i, nodes[1], br, n)
        assert not R.check_echo(shards[i] + b"\0", i, nodes[1], br, n)
        if n > 1:
            assert not R.check_echo(shards[i], (i + 1) % n, nodes[1], br, n)
            assert not R.check_echo(shards[i], i, nodes[1], br[:-1], n)
            assert R.check_echo(shards[i], i, nodes[1], br + [bytes(32)], n)


def test_pyref_compute_root_by_hand():
    k = o.keccak256
    a, b, c, d, e = (bytes([i]) * 32 for i in range(1, 6))
    assert R.compute_root([]) is None
    assert R.compute_root([a]) == a
    assert R.compute_root([a, b, c]) == k(k(a + b) + k(c + c))
    assert R.compute_root([a, b, c, d, e]) == k(k(k(a + b) + k(c + d)) + k(k(e + e) + k(e + e)))


def test_pyref_augment():
    for n, f, plen in [(4, 1, 0), (4, 1, 1), (7, 2, 180), (256, 85, 65536)]:
        aug = R.augment(bytes(plen), n, f)
        assert len(aug) == (n - 2 * f) * R.shard_size(plen, n, f) and int.from_bytes(aug[:4], "little") == plen
        assert len(aug) - (plen + 4) < n - 2 * f


# ---------------------------------------------------------------- the per-lane device functions on the host
@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC], check=True)
    return ctypes.CDLL(LIB)


def u64s(vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


def test_emul_absorb(emu):
    """every shard of the GPU val cases (all lengths and, inside one buffer, all alignments) and the rate boundaries"""
    msgs = [s for n, f, lens in VAL_CASES if n <= 22 for p in payloads_of(n, lens) for s in R.val_messages(p, n, f)[0]]
    rng = random.Random(3)
    msgs += [rng.randbytes(l) for l in (0, 1, 7, 8, 9, 135, 136, 137, 271, 272, 273, 602, 1000)]
    assert {len(m) for m in msgs} >= {135, 136, 137, 602}
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    assert {a % 8 for a in off} == set(range(8))
    out = ctypes.create_string_buffer(32 * len(msgs))
    emu.emu_rbc_absorb(out, b"".join(msgs), u64s(off), len(msgs))
    assert out.raw == b"".join(o.keccak256(m) for m in msgs)


def test_emul_node_hash_and_depth(emu):
    rng = random.Random(4)
    out = ctypes.create_string_buffer(32)
    for _ in range(20):
        l, r = rng.randbytes(32), rng.randbytes(32)
        emu.emu_rbc_node(out, l, r)
        assert out.raw == o.keccak256(l + r)
    for n in range(1, 257):
        assert emu.emu_rbc_depth(n) == R.depth(n)


@pytest.mark.parametrize("batch", [echo_batch, echo_batch_single])
def test_emul_echo_walk(emu, batch):
    n, items = batch()
    want = bytes(R.check_echo(d, frm, root, pr, n) for d, frm, root, pr in items)
    assert 0 < sum(want) < len(items)
    data, doff, frm, roots, proofs, poff = flatten_echo(items)
    acc = ctypes.create_string_buffer(len(items))
    emu.emu_rbc_echo(acc, data, u64s(doff), (ctypes.c_int32 * len(frm))(*frm), roots, proofs, u64s(poff), len(items), n)
    assert acc.raw == want
    if n == 7:
        assert len(items) == ECHO_ITEMS and want[:21] == b"\x01" * 21
        assert want[21:31] == bytes([0, 0, 0, 0, 0, 0, 1, 0, 0, 0])
    else:
        assert want == bytes([1, 0, 0, 1, 0])


def test_emul_root_pairing(emu):
    out = ctypes.create_string_buffer(32)
    for hashes in root_trees():
        st = emu.emu_merkle_root(out, b"".join(hashes), ctypes.c_uint64(len(hashes)))
        want = R.compute_root(hashes)
        assert st == (want is not None) and out.raw == (want or bytes(32))


# ---------------------------------------------------------------- the library's size functions (no device needed)
@pytest.mark.skipif(not os.path.exists(SO), reason="library not built")
def test_library_shard_size_and_tree_depth():
    lib = ctypes.CDLL(SO)
    lib.lcb_rbc_shard_size.restype = ctypes.c_size_t
    lib.lcb_rbc_shard_size.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    for n, f in [(1, 0), (2, 0), (4, 1), (7, 2), (22, 7), (256, 85)]:
        k = n - 2 * f
        for s in (1, 2, 135, 763):
            lens = {0, 1, max(0, k * s - 4), max(0, k * s - 3), max(0, k * s - 5)}     # around a shard-size boundary
            for plen in lens:
                got = lib.lcb_rbc_shard_size(plen, n, f)
                assert got == len(R.augment(bytes(plen), n, f)) // k == R.shard_size(plen, n, f), (n, f, plen)
        assert lib.lcb_rbc_shard_size(k * 10 - 4, n, f) == 10 and lib.lcb_rbc_shard_size(k * 10 - 3, n, f) == 11
    for n in range(1, 257):
        assert lib.lcb_rbc_tree_depth(n) == R.depth(n)
    assert lib.lcb_rbc_tree_depth(0) == -1 and lib.lcb_rbc_tree_depth(257) == -1
    assert lib.lcb_rbc_shard_size(10, 4, 2) == 0 and lib.lcb_rbc_shard_size(10, 0, 0) == 0
    assert lib.lcb_rbc_shard_size(10, 257, 0) == 0
