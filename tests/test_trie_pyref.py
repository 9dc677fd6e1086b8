"""CPU tests of the state-trie restatement (tests/pyref/trie.py), the yardstick of the emulation and GPU trie tests:
hand-built tries, HashFragment against a bit-string formula, the canonical-form property the device root builder rests
on (the root depends on the key/value set alone), folding on delete, and CheckAllNodeHashes.  No reference vector pins
a trie hash; the restatement is literal and its Keccak is pinned by the reference's vector (tests/test_oracle.py)."""
import random

import pytest

import oracle as o
import trie_cases as C
from pyref import trie as R


def K(data):
    return o.keccak256(data)


def test_one_leaf():
    t = R.TrieHashMap()
    root = t.Add(0, b"key", b"value")
    kh = K(b"key")
    assert t.GetHash(root) == K((32).to_bytes(4, "little") + kh + b"value")
    assert t.Find(root, b"key") == b"value" and t.Find(root, b"other") is None
    assert t.GetHash(0) == bytes(32)


def test_two_leaves_that_differ_at_fragment_0():
    a, b = C.craft([3], fill=1), C.craft([17], fill=2)
    t = R.TrieHashMap()
    root = t.add_by_hash(t.add_by_hash(0, b, b"vb"), a, b"va")
    la, lb = K(b"\x20\0\0\0" + a + b"va"), K(b"\x20\0\0\0" + b + b"vb")
    assert t.GetHash(root) == K(bytes([3]) + la + bytes([17]) + lb)
    assert t.nodes[root].ChildrenMask == (1 << 3) | (1 << 17)


@pytest.mark.parametrize("k", [1, 7, 50])
def test_shared_fragments_give_chain_nodes(k):
    a, b = C.craft([7] * k + [1], fill=3), C.craft([7] * k + [2], fill=5)
    t, root = C.chain_trie(k)
    h = K(bytes([1]) + R.leaf_hash(a, b"value a") + bytes([2]) + R.leaf_hash(b, b"value b"))
    for _ in range(k):                                      # k single-child chain nodes, label 7
        h = K(bytes([7]) + h)
    assert t.GetHash(root) == h
    nodes = t.GetAllNodes(root)
    assert sum(n.Type == R.INTERNAL for n in nodes.values()) == k + 1
    assert t.GetHash(root) == R.canonical_root({a: b"value a", b: b"value b"})


def test_fragment_formula_all_indices():
    rng = random.Random(1)
    for _ in range(20):
        h = bytes(rng.randrange(256) for _ in range(32))
        for n in range(51):
            assert R.hash_fragment(h, n) == C.fragment_formula(h, n) == (int.from_bytes(h, "little") >> (5 * n)) & 31
        with pytest.raises(IndexError):
            R.hash_fragment(h, 51)
    assert [R.hash_fragment(C.craft(range(51)), n) for n in range(51)] == [n % 32 for n in range(51)]


def test_root_depends_only_on_the_set():
    """300 random add / update / delete sequences over up to 40 crafted key hashes sharing up to 8 leading fragments:
    after every step the eager trie's root equals the recursive canonical build of the live set"""
    mismatches = steps = 0
    for seq in range(300):
        rng = random.Random(seq)
        pool = C.crafted_pool(rng)
        t, root, live = R.TrieHashMap(), 0, {}
        for op, h, v in C.random_ops(rng, pool, 30):
            root = C.apply_op(t, root, op, h, v)
            if op == "delete":
                del live[h]
            else:
                live[h] = v
            steps += 1
            mismatches += t.GetHash(root) != R.canonical_root(live)
    assert steps == 9000 and mismatches == 0


def test_same_set_any_order_same_root():
    rng = random.Random(5)
    pool = C.crafted_pool(rng, 30, 6)
    items = [(h, bytes([i])) for i, h in enumerate(pool)]
    roots = set()
    for _ in range(5):
        rng.shuffle(items)
        t, root = R.TrieHashMap(), 0
        for h, v in items:
            root = t.add_by_hash(root, h, v)
        roots.add(t.GetHash(root))
    assert roots == {R.canonical_root(dict(items))}


def test_delete_folds_back_up_a_chain():
    t, root = C.chain_trie(7)
    a, b = C.craft([7] * 7 + [1], fill=3), C.craft([7] * 7 + [2], fill=5)
    root = t.delete_by_hash(root, b)
    assert t.nodes[root].Type == R.LEAF and t.GetHash(root) == R.leaf_hash(a, b"value a")
    # with a third key at the top the chain folds up to that node only
    c = C.craft([9], fill=1)
    t, root = C.chain_trie(7, [(c, b"value c")])
    root = t.delete_by_hash(root, b)
    assert len(t.GetAllNodes(root)) == 3
    assert t.GetHash(root) == R.canonical_root({a: b"value a", c: b"value c"})
    assert t.delete_by_hash(t.delete_by_hash(root, a), c) == 0


def test_exceptions():
    t = R.TrieHashMap()
    root = t.Add(0, b"k", b"v")
    with pytest.raises(ValueError):
        t.Add(root, b"k", b"w")
    assert t.GetHash(t.AddOrUpdate(root, b"k", b"w")) == R.leaf_hash(K(b"k"), b"w")
    with pytest.raises(KeyError):
        t.Delete(root, b"missing")
    with pytest.raises(KeyError):
        t.Update(root, b"missing", b"v")
    assert t.TryDelete(root, b"missing") == root
    x = C.craft([1] * 51)
    with pytest.raises(IndexError):                         # differ in bit 255 only: HashFragment runs past the hash
        t.add_by_hash(t.add_by_hash(0, x, b""), C.craft([1] * 51, 1), b"")


def test_check_all_node_hashes_and_insert_all_nodes():
    t, root = C.chain_trie(3, [(C.craft([k], fill=k), bytes(k)) for k in range(8, 20)])
    assert t.CheckAllNodeHashes(root)
    fresh = R.TrieHashMap()
    copy = fresh.InsertAllNodes(root, t.GetAllNodes(root))
    assert fresh.GetHash(copy) == t.GetHash(root) and fresh.CheckAllNodeHashes(copy)
    victim = sorted(t.GetAllNodes(root))[3]
    h = bytearray(t.nodes[victim].Hash)
    h[5] ^= 1
    t.nodes[victim].Hash = bytes(h)
    assert not t.CheckAllNodeHashes(root)


def test_is_consistent_and_state_hash():
    leaf = {"NodeType": "0x0", "KeyHash": "0x" + bytes(range(32)).hex(), "Value": "0x0102",
            "Hash": "0x" + R.leaf_hash(bytes(range(32)), b"\x01\x02").hex()}
    kids = [K(b"a"), K(b"b"), K(b"c")]
    node = {"NodeType": "0x1", "ChildrenMask": "0x80000005", "ChildrenHash": ["0x" + k.hex() for k in kids],
            "Hash": "0x" + R.internal_hash(0x80000005, kids).hex()}
    assert R.is_consistent(leaf) and R.is_consistent(node) and not R.is_consistent({})
    short = dict(node, ChildrenHash=node["ChildrenHash"][:2])
    assert not R.is_consistent(short)
    assert R.is_consistent(dict(short, Hash="0x" + K(bytes([0]) + kids[0] + bytes([2]) + kids[1]).hex()))    # Zip
    roots = [K(bytes([i])) for i in range(6)]
    assert R.state_hash(roots) == K(b"".join(roots))
