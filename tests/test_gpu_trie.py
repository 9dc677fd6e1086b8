"""GPU state-trie layer (k_trie.hip through lcb_trie_node_hash_*, lcb_trie_rehash_*, lcb_trie_root_* and the mirror
lachain_amd/trie.py) against the plain-Python restatement (tests/pyref/trie.py over o.keccak256), bit for bit, in the
host-pointer and both device-pointer forms.  No reference vector pins a trie hash: the restatement is the pin.  The
node shapes (tests/trie_cases.py) are shared with the host emulation in tests/test_trie_emul.py.  Device buffers carry
a guard pattern on both sides that must be intact afterwards."""
import ctypes
import random
import struct

import pytest

import trie_cases as C
from helpers import Drbg, gpu_native
from pyref import trie as R

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xA5
PAD = bytes([PATTERN]) * GUARD
_cache = {}


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


@pytest.fixture(scope="module")
def T(nat):
    from lachain_amd import trie
    return trie


def flat_expected():
    """the restatement's hashes of the flat cases: computed once, shared by the host and device forms"""
    if "flat" not in _cache:
        nodes = C.flat_cases()
        _cache["flat"] = (nodes, b"".join(C.expected_hash(n) for n in nodes))
    return _cache["flat"]


def host_flat(nat, nodes, expected=None):
    recs, _, _ = C.flatten(nodes)
    return nat.trie_node_hash_batch(recs, [n.data for n in nodes], expected)


def dbuf(data):
    import torch
    return torch.frombuffer(bytearray(PAD + data + PAD), dtype=torch.uint8).to("cuda:0")


def inner(t, length):
    raw = bytes(t.cpu().numpy())
    assert raw[:GUARD] == PAD and raw[GUARD + length:] == PAD, "guard overwritten"
    return raw[GUARD:GUARD + length]


def both_forms(nat, name):
    """(function, leading arguments) of the implicit-context and the explicit-context device form"""
    lib = nat.lib()
    ctx = nat.Context()
    return ctx, [(getattr(lib, "lcb_" + name), ()), (getattr(lib, "lcb_ctx_" + name), (ctx.ptr,))]


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ (a) flat hashing and consistency
def test_flat_cases_host_form(nat):
    nodes, want = flat_expected()
    got, accept = host_flat(nat, nodes, want)
    bad = [(i, n.note, len(n.data)) for i, n in enumerate(nodes) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
    assert not bad, bad[:10]
    assert accept == b"\x01" * len(nodes)


def test_flat_cases_device_forms(nat):
    import torch
    nodes, want = flat_expected()
    recs, data, off = C.flatten(nodes)
    n = len(nodes)
    d_rec, d_data, d_exp = dbuf(recs), dbuf(data), dbuf(want)
    d_off = torch.tensor(off, dtype=torch.int64, device="cuda:0")
    ctx, forms = both_forms(nat, "trie_node_hash_dev")
    with ctx:
        for fn, pre in forms:
            d_out, d_acc = dbuf(bytes(32 * n)), dbuf(bytes(n))
            assert fn(*pre, d_out.data_ptr() + GUARD, d_acc.data_ptr() + GUARD, d_rec.data_ptr() + GUARD,
                      d_data.data_ptr() + GUARD, d_off.data_ptr(), d_exp.data_ptr() + GUARD, n, stream()) == 0, nat.last_error()
            torch.cuda.synchronize()
            assert inner(d_out, 32 * n) == want and inner(d_acc, n) == b"\x01" * n
            assert (inner(d_rec, len(recs)), inner(d_data, len(data)), inner(d_exp, len(want))) == (recs, data, want)
            # hashes alone, then the decision alone
            d_out2, d_acc2 = dbuf(bytes(32 * n)), dbuf(bytes(n))
            assert fn(*pre, d_out2.data_ptr() + GUARD, None, d_rec.data_ptr() + GUARD, d_data.data_ptr() + GUARD,
                      d_off.data_ptr(), None, n, stream()) == 0
            assert fn(*pre, None, d_acc2.data_ptr() + GUARD, d_rec.data_ptr() + GUARD, d_data.data_ptr() + GUARD,
                      d_off.data_ptr(), d_exp.data_ptr() + GUARD, n, stream()) == 0
            torch.cuda.synchronize()
            assert inner(d_out2, 32 * n) == want and inner(d_acc2, n) == b"\x01" * n


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_flat_batch_sizes(nat, n):
    nodes = C.batch_of(n)
    got, _ = host_flat(nat, nodes)
    assert got == b"".join(C.expected_hash(x) for x in nodes)


def test_flat_mixed_launch_agrees(nat, monkeypatch):
    """the measurement switch of DESIGN.md §21 (one launch, leaves and internal nodes in the same waves)"""
    nodes, want = flat_expected()
    monkeypatch.setenv("LCB_TRIE_MIXED", "1")
    assert host_flat(nat, nodes)[0] == want


def test_accept_flags(nat):
    d = Drbg(b"trie accept")
    nodes = [C.leaf(d, 50), C.internal(d, 0x80000013), C.leaf(d, 200), C.internal(d, 0x0000ff00), C.leaf(d, 7),
             C.internal(d, 0x00000006), C.leaf(d, 33)]
    want = bytearray(b"".join(C.expected_hash(x) for x in nodes))
    flip = lambda b, k: b[:k] + bytes([b[k] ^ 0x10]) + b[k + 1:]
    nodes[0] = nodes[0]._replace(data=flip(nodes[0].data, 60))              # a byte of a leaf's value
    nodes[1] = nodes[1]._replace(data=flip(nodes[1].data, 32 * 2 + 31))     # a byte of a child hash
    want[32 * 4 + 9] ^= 1                                                   # a byte of the expected hash
    nodes[5] = nodes[5]._replace(mask=0x0000000a)                           # a wrong mask, same child count
    _, accept = host_flat(nat, nodes, bytes(want))
    assert accept == bytes([0, 0, 1, 1, 0, 0, 1])


def test_flat_bad_arguments_fail_the_call(nat):
    d = Drbg(b"trie bad")
    good = [C.leaf(d, 10), C.internal(d, 5)]

    def rc(nodes, recs=None):
        r, data, off = C.flatten(nodes)
        keep = (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
        rb = (ctypes.c_uint8 * len(r)).from_buffer_copy(recs or r)
        out = (ctypes.c_uint8 * (32 * len(nodes)))()
        u8 = ctypes.POINTER(ctypes.c_uint8)
        return nat.lib().lcb_trie_node_hash_batch(ctypes.cast(out, u8), None, ctypes.cast(rb, u8), ctypes.cast(keep, u8),
                                                  (ctypes.c_uint64 * len(off))(*off), None, len(nodes))

    assert rc(good) == 0
    assert rc([good[0], good[1]._replace(kind=2)]) == -1 and "kind" in nat.last_error()
    recs = bytearray(C.flatten(good)[0])
    recs[12] = 1
    assert rc(good, bytes(recs)) == -1 and "reserved" in nat.last_error()
    assert rc([good[0], good[1]._replace(data=good[1].data + b"\0")]) == -1 and "32" in nat.last_error()
    assert rc([good[0]._replace(key_len=43), good[1]]) == -1 and "key_len" in nat.last_error()
    assert rc([good[0]._replace(key_len=42), good[1]]) == 0


# ------------------------------------------------------------------ (b) rehash by reference
def heights(children):
    h = [None] * len(children)

    def height(i):
        if h[i] is None:
            h[i] = max([height(r) + 1 for r in children[i] if r >= 0], default=0)
        return h[i]
    return [height(i) for i in range(len(children))]


def test_rehash_single_leaf_and_pair(nat):
    t = R.TrieHashMap()
    one = t.add_by_hash(0, C.craft([4]), b"only")
    two = t.add_by_hash(one, C.craft([5]), b"other")
    for root, count in ((one, 1), (two, 3)):
        records, items, children, literals, want = C.export(t, root)
        assert len(items) == count
        assert nat.trie_rehash_batch(records, items, children, literals) == want


def test_rehash_chain_of_51(nat):
    """two leaves that share 50 fragments: 51 internal nodes, heights 0 .. 51, parents before children in the array"""
    t, root = C.chain_trie(50)
    records, items, children, literals, want = C.export(t, root)
    order = sorted(range(len(items)), key=lambda i: -heights(children)[i])          # the root first
    remap = {old: new for new, old in enumerate(order)}
    recs = b"".join(records[16 * i:16 * i + 16] for i in order)
    kids = [[remap[r] for r in children[i]] for i in order]
    assert sorted(heights(kids)) == [0] + list(range(52)) and heights(kids)[0] == 51
    got = nat.trie_rehash_batch(recs, [items[i] for i in order], kids, [])
    assert got == b"".join(want[32 * i:32 * i + 32] for i in order)
    assert got[:32] == t.GetHash(root)


def test_rehash_literals_shuffled(nat):
    rng = random.Random(21)
    t, root = R.TrieHashMap(), 0
    for h in C.crafted_pool(rng, 40, 6):
        root = t.add_by_hash(root, h, bytes(rng.randrange(256) for _ in range(rng.randrange(120))))
    records, items, children, literals, want = C.export(t, root, rng, lambda i, n: i % 3 == 0 and i != root)
    assert literals and any(r >= 0 for c in children for r in c) and any(r < 0 for c in children for r in c)
    assert nat.trie_rehash_batch(records, items, children, literals) == want


def test_rehash_shared_child(nat):
    d = Drbg(b"shared child")
    leaf = C.leaf(d, 20)
    lh = C.expected_hash(leaf)
    lit = d.bytes(32)
    a = R.internal_hash(0x5, [lh, lit])
    b = R.internal_hash(0x80000001, [lit, lh])
    top = R.internal_hash(0x3, [a, b])
    rec = lambda kind, mask, kl=0: struct.pack("<IIII", kind, mask, kl, 0)
    records = rec(1, 0x3) + rec(1, 0x5) + rec(0, 0, 32) + rec(1, 0x80000001)
    got = nat.trie_rehash_batch(records, [b"", b"", leaf.data, b""], [[1, 3], [2, -1], [], [-1, 2]], [lit])
    assert got == top + a + lh + b


def test_rehash_errors(nat):
    rec = lambda kind, mask, kl=0: struct.pack("<IIII", kind, mask, kl, 0)
    leaf = bytes(40)
    with pytest.raises(RuntimeError, match="cycle"):
        nat.trie_rehash_batch(rec(1, 1) + rec(1, 2) + rec(0, 0, 32), [b"", b"", leaf], [[1], [0], []])
    with pytest.raises(RuntimeError, match="cycle"):
        nat.trie_rehash_batch(rec(1, 1), [b""], [[0]])
    with pytest.raises(RuntimeError, match="out of range"):
        nat.trie_rehash_batch(rec(1, 1) + rec(0, 0, 32), [b"", leaf], [[2], []])
    with pytest.raises(RuntimeError, match="out of range"):
        nat.trie_rehash_batch(rec(1, 1) + rec(0, 0, 32), [b"", leaf], [[-2], []], [bytes(32)])
    with pytest.raises(RuntimeError, match="popcount"):
        nat.trie_rehash_batch(rec(1, 3) + rec(0, 0, 32), [b"", leaf], [[1], []])
    with pytest.raises(RuntimeError, match="popcount"):
        nat.trie_rehash_batch(rec(1, 1) + rec(0, 0, 32), [b"", leaf], [[1, 1], []])


def test_rehash_device_forms(nat):
    import torch
    rng = random.Random(33)
    t, root = C.chain_trie(9, [(h, bytes(rng.randrange(256) for _ in range(rng.randrange(300))))
                               for h in C.crafted_pool(rng, 60, 5)])
    records, items, children, literals, want = C.export(t, root, rng, lambda i, n: i % 5 == 0 and i != root)
    n = len(items)
    hs = heights(children)
    order = sorted(range(n), key=lambda i: hs[i])
    level_off = [0] + [sum(1 for x in hs if x <= l) for l in range(max(hs) + 1)]
    off, coff = [0], [0]
    for it, c in zip(items, children):
        off.append(off[-1] + len(it))
        coff.append(coff[-1] + len(c))
    refs = [r for c in children for r in c]
    dev = "cuda:0"
    d_rec, d_data, d_lit = dbuf(records), dbuf(b"".join(items)), dbuf(b"".join(literals))
    d_off, d_coff = torch.tensor(off, dtype=torch.int64, device=dev), torch.tensor(coff, dtype=torch.int64, device=dev)
    d_ref, d_order = torch.tensor(refs, dtype=torch.int64, device=dev), torch.tensor(order, dtype=torch.int64, device=dev)
    h_level = (ctypes.c_uint64 * len(level_off))(*level_off)
    ctx, forms = both_forms(nat, "trie_rehash_dev")
    with ctx:
        for fn, pre in forms:
            d_out = dbuf(bytes(32 * n))
            assert fn(*pre, d_out.data_ptr() + GUARD, d_rec.data_ptr() + GUARD, d_data.data_ptr() + GUARD, d_off.data_ptr(),
                      d_coff.data_ptr(), d_ref.data_ptr(), d_lit.data_ptr() + GUARD, d_order.data_ptr(), h_level,
                      len(level_off) - 1, n, stream()) == 0, nat.last_error()
            torch.cuda.synchronize()
            assert inner(d_out, 32 * n) == want


def test_mirror_deferred_against_eager(nat, T):
    """about 300 random operations, deletes that fold among them: the mirror hashes once per GetHash, the restatement
    on every step; the roots agree wherever they are compared, and so do structure and exceptions"""
    rng = random.Random(77)
    pool = C.crafted_pool(rng, 40, 8)
    eager, mirror = R.TrieHashMap(), T.TrieHashMap()
    re_, rm = 0, 0
    for step, (op, h, v) in enumerate(C.random_ops(rng, pool, 300)):
        re_ = C.apply_op(eager, re_, op, h, v)
        rm = C.apply_op(mirror, rm, op, h, v)
        if step % 25 == 24 or step == 299:
            assert mirror.GetHash(rm) == eager.GetHash(re_), step
            assert mirror.find_by_hash(rm, h) == eager.find_by_hash(re_, h)
    assert len(mirror.GetAllNodes(rm)) == len(eager.GetAllNodes(re_))
    assert mirror.CheckAllNodeHashes(rm)
    victim = sorted(mirror.GetAllNodes(rm))[2]
    good = mirror.nodes[victim].Hash
    mirror.nodes[victim].Hash = good[:7] + bytes([good[7] ^ 4]) + good[8:]
    assert not mirror.CheckAllNodeHashes(rm)
    mirror.nodes[victim].Hash = good
    assert mirror.RecalculateHash(rm) == eager.RecalculateHash(re_)
    fresh = T.TrieHashMap()
    copy = fresh.InsertAllNodes(re_, eager.GetAllNodes(re_))
    assert fresh.GetHash(copy) == eager.GetHash(re_) and fresh.CheckAllNodeHashes(copy)
    live = pool[0]
    with pytest.raises(KeyError):
        mirror.delete_by_hash(0, live)
    with pytest.raises(KeyError):
        mirror.update_by_hash(0, live, b"")
    one = mirror.add_by_hash(0, live, b"v")
    with pytest.raises(ValueError):
        mirror.add_by_hash(one, live, b"w")


def test_mirror_hashed_keys_and_node_storage(nat, T):
    eager, mirror = R.TrieHashMap(), T.TrieHashMap()
    re_, rm = 0, 0
    for k in range(40):
        key, val = b"key %d" % k, bytes([k]) * k
        re_, rm = eager.Add(re_, key, val), mirror.Add(rm, key, val)
    re_, rm = eager.Delete(re_, b"key 3"), mirror.Delete(rm, b"key 3")
    re_, rm = eager.AddOrUpdate(re_, b"key 4", b"new"), mirror.AddOrUpdate(rm, b"key 4", b"new")
    re_, rm = eager.Update(re_, b"key 5", b"five"), mirror.Update(rm, b"key 5", b"five")
    re_, rm = eager.TryDelete(re_, b"absent"), mirror.TryDelete(rm, b"absent")      # a new id for the same node, as in
    assert mirror.GetHash(rm) == eager.GetHash(re_) and mirror.Find(rm, b"key 5") == b"five"     # the reference
    assert mirror.GetHash(0) == bytes(32)
    hx = lambda b: "0x" + b.hex()
    js = []
    for node in eager.GetAllNodes(re_).values():
        if node.Type == R.INTERNAL:
            js.append({"NodeType": "0x1", "ChildrenMask": hex(node.ChildrenMask), "Hash": hx(node.Hash),
                       "ChildrenHash": [hx(eager.nodes[c].Hash) for c in node.Children]})
        else:
            js.append({"NodeType": "0x0", "KeyHash": hx(node.KeyHash), "Value": hx(node.Value), "Hash": hx(node.Hash)})
    internal = next(k for k, j in enumerate(js) if j["NodeType"] == "0x1" and len(j["ChildrenHash"]) > 2)
    js.append(dict(js[internal], ChildrenHash=js[internal]["ChildrenHash"][:-1]))       # one child hash missing
    js.append(dict(js[0], Hash=js[0]["Hash"].upper().replace("0X", "0x")))             # the reference compares strings
    js.append({})
    want = [R.is_consistent(j) for j in js]
    assert want[:-3] == [True] * (len(js) - 3) and want[-3:] == [False, False, False]
    assert T.NodeStorage.IsConsistentBatch(js) == want


# ------------------------------------------------------------------ (c) roots from key/value sets
def test_root_sets_in_one_call(nat, T):
    sets = C.root_sets()
    names = list(sets)
    x = C.craft([1] * 51)
    extra = [[(x, b"a"), (C.craft([1] * 51, 1), b"b")],                      # differ in bit 255 only
             sets["two"] + [sets["two"][0]],                                 # a duplicate key hash
             [(x, b"a"), (C.craft([1] * 51, 1), b"b")] + sets["share 7"]]
    roots, status = T.state_root_from_items([sets[k] for k in names] + extra, keys_hashed=True)
    for k, name in enumerate(names):
        assert roots[k] == R.canonical_root(sets[name]), name
    assert status == b"\x01" * len(names) + b"\0\0\0" and roots[len(names):] == [bytes(32)] * 3
    assert roots[names.index("empty")] == bytes(32)
    one = sets["one"][0]
    assert roots[names.index("one")] == R.leaf_hash(*one)
    t, root = R.TrieHashMap(), 0                            # and against the eager trie itself, not only the builder
    for h, v in sets["share 50"]:
        root = t.add_by_hash(root, h, v)
    assert roots[names.index("share 50")] == t.GetHash(root)


def test_state_hash_over_six_sets(nat, T):
    sets = C.state_sets()
    assert [len(s) for s in sets] == [0, 1, 2, 33, 100, 1000]
    roots, status = T.state_root_from_items(sets, keys_hashed=True)
    want = [R.canonical_root(s) for s in sets]
    assert roots == want and status == b"\x01" * 6
    assert T.StateHash(roots) == R.state_hash(want)


def test_roots_from_unhashed_keys(nat, T):
    d = Drbg(b"trie raw keys")
    items = [(d.bytes(k), d.bytes(k % 50)) for k in (0, 1, 20, 32, 52, 136, 137)]
    items += [(b"balance:%d" % k, d.bytes(32)) for k in range(60)]
    roots, status = T.state_root_from_items([items, items[:1], []], keys_hashed=False)
    hashed = {R.TrieHashMap.Hash(k): v for k, v in items}
    assert roots == [R.canonical_root(hashed), R.leaf_hash(R.TrieHashMap.Hash(b""), b""), bytes(32)]
    assert status == b"\x01\x01\x01"
    with pytest.raises(RuntimeError, match="32 bytes"):
        T.state_root_from_items([items], keys_hashed=True)


def big_set():
    if "big" not in _cache:
        items = C.random_set(Drbg(b"trie 4096"), 4096, lambda i: 32 + i % 5)
        _cache["big"] = (items, R.canonical_root(items))
    return _cache["big"]


def test_root_of_4096_keys_any_order(nat, T):
    items, want = big_set()
    shuffled = list(items)
    random.Random(9).shuffle(shuffled)
    roots, status = T.state_root_from_items([items, shuffled], keys_hashed=True)
    assert roots == [want, want] and status == b"\x01\x01"


def test_root_device_forms(nat):
    import torch
    items, want = big_set()
    small = C.root_sets()["share 7"]
    tries = [small, [], items]
    flat = [kv for t in tries for kv in t]
    keys, vals = b"".join(k for k, _ in flat), b"".join(v for _, v in flat)
    koff, voff, toff = [0], [0], [0]
    for k, v in flat:
        koff.append(koff[-1] + len(k))
        voff.append(voff[-1] + len(v))
    for t in tries:
        toff.append(toff[-1] + len(t))
    dev = "cuda:0"
    d_keys, d_vals = dbuf(keys), dbuf(vals)
    d_koff, d_voff, d_toff = (torch.tensor(x, dtype=torch.int64, device=dev) for x in (koff, voff, toff))
    ctx, forms = both_forms(nat, "trie_root_dev")
    with ctx:
        for fn, pre in forms:
            d_roots, d_status = dbuf(bytes(96)), dbuf(bytes(3))
            assert fn(*pre, d_roots.data_ptr() + GUARD, d_status.data_ptr() + GUARD, d_keys.data_ptr() + GUARD,
                      d_koff.data_ptr(), d_vals.data_ptr() + GUARD, d_voff.data_ptr(), d_toff.data_ptr(), 3, len(flat), 1,
                      stream()) == 0, nat.last_error()
            torch.cuda.synchronize()
            assert inner(d_roots, 96) == R.canonical_root(small) + bytes(32) + want
            assert inner(d_status, 3) == b"\x01\x01\x01"
            assert inner(d_keys, len(keys)) == keys and inner(d_vals, len(vals)) == vals
