"""The state-trie cases shared by the host emulation (tests/test_trie_emul.py) and the GPU tests
(tests/test_gpu_trie.py); expected values come from the restatement tests/pyref/trie.py.  TEST INFRASTRUCTURE."""
import random
import struct
from collections import namedtuple

from helpers import Drbg
from pyref import trie as R

Node = namedtuple("Node", "kind mask key_len data note")
LEAF, INTERNAL = 0, 1


def craft(frags, bit255=0, fill=0) -> bytes:
    """a key hash with the given leading fragments (HashFragment n = frags[n]); the remaining fragments are `fill`"""
    frags = list(frags) + [fill] * (51 - len(frags))
    v = sum((f & 31) << (5 * n) for n, f in enumerate(frags)) | (bit255 << 255)
    return v.to_bytes(32, "little")


def fragment_formula(h: bytes, n: int) -> int:
    """bits [5n, 5n + 5) of the hash as a bit string, least significant bit of byte 0 first"""
    bits = "".join(format(b, "08b")[::-1] for b in h)
    return int(bits[5 * n:5 * n + 5][::-1], 2)


# ------------------------------------------------------------------ flat nodes
def record(n: Node) -> bytes:
    return struct.pack("<IIII", n.kind, n.mask, n.key_len, 0)


def expected_hash(n: Node) -> bytes:
    if n.kind == LEAF:
        return R.leaf_hash(n.data[:n.key_len], n.data[n.key_len:])
    return R.internal_hash(n.mask, [n.data[32 * j:32 * j + 32] for j in range(len(n.data) // 32)])


def leaf(d: Drbg, value_len, key_len=32, note=""):
    return Node(LEAF, 0, key_len, d.bytes(key_len + value_len), note or "leaf v%d k%d" % (value_len, key_len))


def internal(d: Drbg, mask, c=None, note=""):
    c = bin(mask).count("1") if c is None else c
    return Node(INTERNAL, mask, 0, d.bytes(32 * c), note or "internal %08x c%d" % (mask, c))


def mask_of(d: Drbg, c, top=False):
    """a mask with c set bits; top: bit 31 among them"""
    labels = list(range(32))
    random.Random(d.bytes(8)).shuffle(labels)
    labels = labels[:c]
    if top and c and 31 not in labels:
        labels[0] = 31
    return sum(1 << x for x in labels)


VALUE_LENS = (0, 1, 99, 100, 101, 235, 236, 237, 1000)     # messages of 135 / 136 / 137, 271 / 272 / 273 around the rate
KEY_LENS = (0, 1, 31, 33)
CHILD_COUNTS = (0, 1, 2, 4, 5, 8, 9, 31, 32)


def flat_cases():
    """every leaf and internal shape of the issue, leaves and internal nodes interleaved; with the fillers of align()
    every shape starts at each of the 8 byte alignments"""
    d = Drbg(b"trie flat cases")
    base = []
    for v in VALUE_LENS:
        base.append(leaf(d, v))
    for k in KEY_LENS:
        base.append(leaf(d, 40, k))
        base.append(leaf(d, 0, k))
    for c in CHILD_COUNTS:
        base.append(internal(d, mask_of(d, c)))
        if c:
            base.append(internal(d, mask_of(d, c, top=True), note="internal c%d bit 31" % c))
    for c in (1, 2, 5, 9, 31):                              # Zip: one hash too few, one too many
        m = mask_of(d, c, top=True)
        base.append(internal(d, m, c - 1, "zip short %d" % c))
        base.append(internal(d, m, c + 1, "zip long %d" % c))
    base.append(internal(d, 0xffffffff, 33, "zip long 32"))
    base.append(internal(d, 0, 3, "empty mask with hashes"))
    out = []
    for a in range(8):
        for k, n in enumerate(base):
            out.append((n, (a + k) % 8))
    return align(out)


def align(wanted):
    """[(node, alignment)] -> nodes, with a filler leaf in front of a node whose start would not have its alignment"""
    out, pos = [], 0
    for n, a in wanted:
        gap = (a - pos) % 8
        if gap:
            out.append(Node(LEAF, 0, 0, bytes([0xf0 + gap]) * gap, "filler"))
            pos += gap
        out.append(n)
        pos += len(n.data)
    return out


def flatten(nodes):
    """(records, data, offsets)"""
    off = [0]
    for n in nodes:
        off.append(off[-1] + len(n.data))
    return b"".join(record(n) for n in nodes), b"".join(n.data for n in nodes), off


def batch_of(count, seed=b"trie batch"):
    """`count` nodes, leaves and internal nodes interleaved, of mixed sizes"""
    d = Drbg(seed + bytes([count & 255]))
    out = []
    for i in range(count):
        if i % 3 == 1:
            out.append(internal(d, mask_of(d, 1 + d.bytes(1)[0] % 32)))
        else:
            out.append(leaf(d, d.bytes(1)[0] % 150))
    return out


# ------------------------------------------------------------------ rehash batches from a restatement trie
def export(trie, root, rng=None, literal=lambda node_id, node: False):
    """the nodes below root as a rehash batch: (records, items, children, literals, expected hashes).  rng shuffles the
    array order; nodes for which literal(id, node) holds stay outside the batch and enter as literal hashes."""
    ids = [i for i, n in trie.GetAllNodes(root).items() if not literal(i, n)]
    # a literal's subtree is clean: drop nodes only reachable through literals
    keep, stack = set(), [root] if root and root in set(ids) else []
    while stack:
        r = stack.pop()
        if r in keep:
            continue
        keep.add(r)
        stack.extend(c for c in trie.nodes[r].Children if not literal(c, trie.nodes[c]))
    ids = [i for i in ids if i in keep]
    if rng:
        rng.shuffle(ids)
    index = {r: k for k, r in enumerate(ids)}
    records, items, children, literals, lit = [], [], [], [], {}
    for r in ids:
        n = trie.nodes[r]
        if n.Type == LEAF:
            records.append(struct.pack("<IIII", LEAF, 0, len(n.KeyHash), 0))
            items.append(n.KeyHash + n.Value)
            children.append([])
            continue
        refs = []
        for c in n.Children:
            if c in index:
                refs.append(index[c])
            else:
                if c not in lit:
                    lit[c] = len(literals)
                    literals.append(trie.nodes[c].Hash)
                refs.append(~lit[c])
        records.append(struct.pack("<IIII", INTERNAL, n.ChildrenMask, 0, 0))
        items.append(b"")
        children.append(refs)
    return b"".join(records), items, children, literals, b"".join(trie.nodes[r].Hash for r in ids)


def chain_trie(k, extra=()):
    """two leaves that share k fragments (k single-child chain nodes above the node that splits them), plus extras"""
    t = R.TrieHashMap()
    root = 0
    a, b = craft([7] * k + [1], fill=3), craft([7] * k + [2], fill=5)
    for h, v in [(a, b"value a"), (b, b"value b")] + list(extra):
        root = t.add_by_hash(root, h, v)
    return t, root


# ------------------------------------------------------------------ random operation sequences on crafted hashes
def crafted_pool(rng, count=40, depth=8):
    """key hashes that share up to `depth` leading fragments with one another"""
    pool = []
    stem = [rng.randrange(32) for _ in range(depth)]
    for _ in range(count):
        k = rng.randrange(depth + 1)
        pool.append(craft(stem[:k] + [rng.randrange(32) for _ in range(51 - k)], rng.randrange(2)))
    return list(dict.fromkeys(pool))


def random_ops(rng, pool, steps):
    """(op, key hash, value) with op in add / update / delete, always legal for the set so far"""
    live, ops = {}, []
    for _ in range(steps):
        h = rng.choice(pool)
        if h not in live:
            op = "add"
        else:
            op = rng.choice(("update", "delete", "delete"))
        v = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 70)))
        if op == "delete":
            del live[h]
        else:
            live[h] = v
        ops.append((op, h, v))
    return ops


def apply_op(trie, root, op, h, v):
    if op == "add":
        return trie.add_by_hash(root, h, v)
    if op == "update":
        return trie.update_by_hash(root, h, v)
    return trie.delete_by_hash(root, h)


# ------------------------------------------------------------------ key/value sets for the root builder
def random_set(d: Drbg, count, value_len=lambda i: 32):
    return [(d.bytes(32), d.bytes(value_len(i))) for i in range(count)]


def root_sets():
    """name -> list of (key hash, value); expected by R.canonical_root"""
    d = Drbg(b"trie root sets")
    sets = {"empty": [], "one": random_set(d, 1), "two": random_set(d, 2)}
    sets["all labels"] = [(craft([f], fill=f % 7), d.bytes(20)) for f in range(32)] + [(craft([5, 9], fill=1), b"x")]
    for k in (1, 7, 50):
        sets["share %d" % k] = [(craft([9] * k + [1], fill=2), b"a" * 33), (craft([9] * k + [30], fill=4), b"")]
    # byte order and fragment order disagree: fragments 1, 3, 4 and 6 straddle bytes
    for f in (1, 3, 4, 6):
        sets["straddle %d" % f] = [(craft([2] * f + [x], fill=x), bytes([x]) * x) for x in (1, 2, 4, 8, 16, 31, 17, 3)]
    sets["deep mix"] = ([(craft([4] * k + [k % 32 + 1 if k % 32 + 1 != 4 else 6], fill=11), d.bytes(k)) for k in range(0, 50, 3)]
                        + random_set(d, 20))
    return sets


def state_sets():
    """six sets of sizes {0, 1, 2, 33, 100, 1000}"""
    d = Drbg(b"trie state")
    return [random_set(d, c, lambda i: i % 90) for c in (0, 1, 2, 33, 100, 1000)]
