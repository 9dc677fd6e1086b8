"""Plain Python restatement of the reference's state trie, hashing eagerly and node by node as the reference does, over
the oracle's Keccak-256 (o.keccak256).  TEST INFRASTRUCTURE: the yardstick of tests/test_trie_pyref.py,
tests/test_trie_emul.py and tests/test_gpu_trie.py; the library is never compared with itself.  No reference vector
pins a trie hash (the only pinned value, the genesis StateHash of BlocksTest.cs:144, needs the whole genesis state), so
this literal restatement over a Keccak that the reference's vector pins is the pin of the trie layer.

Reference: src/Lachain.Storage/Trie/TrieHashMap.cs, InternalNode.cs, LeafNode.cs, src/Lachain.Core/Network/
FastSynchronizerBatch.cs/NodeStorage.cs:85-110 (IsConsistent), src/Lachain.Storage/State/BlockchainSnapshot.cs:71-80
(StateHash)."""
import oracle as o

LEAF, INTERNAL = 0, 1                                   # NodeType.cs


def children_labels(mask: int):
    """InternalNode.GetChildrenLabels (InternalNode.cs:48-51)"""
    return [i for i in range(32) if (mask >> i) & 1]


def leaf_hash(key_hash: bytes, value: bytes) -> bytes:
    """LeafNode.cs:17: KeyHash.Length.ToBytes() (int32, little-endian) || KeyHash || Value"""
    return o.keccak256(len(key_hash).to_bytes(4, "little") + bytes(key_hash) + bytes(value))


def internal_hash(mask: int, children_hashes) -> bytes:
    """InternalNode.UpdateHash (InternalNode.cs:53-59): Zip stops with the shorter of hashes and labels"""
    return o.keccak256(b"".join(bytes([i]) + bytes(h) for h, i in zip(children_hashes, children_labels(mask))))


def hash_fragment(h: bytes, n: int) -> int:
    """TrieHashMap.HashFragment (TrieHashMap.cs:307-316), branch for branch; raises IndexError where the reference's
    indexer throws (n = 51 reads hash[32])"""
    bit_offset = 5 * n
    if bit_offset % 8 <= 3:
        return (h[bit_offset // 8] >> (bit_offset % 8)) & 0x1F
    from_first = 8 - bit_offset % 8
    first = h[bit_offset // 8] >> (bit_offset % 8)
    second = h[bit_offset // 8 + 1] & ((1 << (5 - from_first)) - 1)
    return ((second << from_first) | first) & 0xFF


class LeafNode:
    Type = LEAF

    def __init__(self, key_hash, value):
        self.KeyHash, self.Value = bytes(key_hash), bytes(value)
        self.Hash = leaf_hash(self.KeyHash, self.Value)
        self.Children = []

    def GetChildByHash(self, h):
        return 0


class InternalNode:
    Type = INTERNAL

    def __init__(self, mask=0, children=(), children_hashes=()):
        self.ChildrenMask = mask
        self.Children = list(children)
        self.Hash = internal_hash(mask, list(children_hashes))

    def GetChildByHash(self, h):
        """InternalNode.cs:18-21; BitsUtils.PositionOf = set bits of the mask below h"""
        if not (self.ChildrenMask >> h) & 1:
            return 0
        return self.Children[bin(self.ChildrenMask & ((1 << h) - 1)).count("1")]

    @staticmethod
    def WithChildren(ids, labels, hashes):
        """InternalNode.cs:61-81"""
        labels = list(labels)
        if len(set(labels)) != len(labels):
            raise ValueError("Trying to create internal trie node with equal children labels")
        order = sorted(range(len(labels)), key=lambda k: labels[k])
        return InternalNode(sum(1 << x for x in labels), [list(ids)[k] for k in order], [list(hashes)[k] for k in order])

    @staticmethod
    def ModifyChildren(node, h, value, children_hashes, value_hash):
        """InternalNode.cs:83-134"""
        was = node.GetChildByHash(h)
        if was == value:
            return node
        pos = bin(node.ChildrenMask & ((1 << h) - 1)).count("1")
        hashes = list(children_hashes)
        if was == 0:
            assert value_hash is not None
            return InternalNode(node.ChildrenMask | (1 << h), node.Children[:pos] + [value] + node.Children[pos:],
                                hashes[:pos] + [value_hash] + hashes[pos:])
        if value == 0:
            if len(node.Children) == 1:
                return None
            return InternalNode(node.ChildrenMask ^ (1 << h), node.Children[:pos] + node.Children[pos + 1:],
                                hashes[:pos] + hashes[pos + 1:])
        assert value_hash is not None
        return InternalNode(node.ChildrenMask, node.Children[:pos] + [value] + node.Children[pos + 1:],
                            hashes[:pos] + [value_hash] + hashes[pos + 1:])


class TrieHashMap:
    """TrieHashMap.cs with the repository and caches reduced to one dictionary id -> node; ids are VersionFactory's
    counter.  Every method takes the root id and returns the new one, as the reference's do."""

    def __init__(self):
        self.nodes = {}
        self.version = 0

    def _new(self, node):
        self.version += 1
        self.nodes[self.version] = node
        return self.version

    def _get(self, node_id):
        return self.nodes.get(node_id) if node_id else None

    @staticmethod
    def Hash(key: bytes) -> bytes:
        return o.keccak256(bytes(key))                  # TrieHashMap.cs:90-93

    # ---- TrieHashMap.cs:95-129
    def Add(self, root, key, value):
        return self._add(root, 0, self.Hash(key), bytes(value), True)

    def AddOrUpdate(self, root, key, value):
        return self._add(root, 0, self.Hash(key), bytes(value), False)

    def Update(self, root, key, value):
        return self._update(root, 0, self.Hash(key), bytes(value))

    def Delete(self, root, key):
        return self._delete(root, 0, self.Hash(key), True)

    def TryDelete(self, root, key):
        return self._delete(root, 0, self.Hash(key), False)

    def Find(self, root, key):
        return self.find_by_hash(root, self.Hash(key))

    # ---- the same by key hash, for crafted hashes
    def add_by_hash(self, root, key_hash, value, check=True):
        return self._add(root, 0, bytes(key_hash), bytes(value), check)

    def update_by_hash(self, root, key_hash, value):
        return self._update(root, 0, bytes(key_hash), bytes(value))

    def delete_by_hash(self, root, key_hash, check=True):
        return self._delete(root, 0, bytes(key_hash), check)

    def find_by_hash(self, root, key_hash):
        """FindInternal (TrieHashMap.cs:428-447)"""
        height = 0
        while True:
            if root == 0:
                return None
            node = self._get(root)
            if node.Type == INTERNAL:
                root = node.GetChildByHash(hash_fragment(key_hash, height))
            else:
                return node.Value if node.KeyHash == bytes(key_hash) else None
            height += 1

    def GetHash(self, root) -> bytes:
        """TrieHashMap.cs:188-191: the zero hash for no node"""
        node = self._get(root)
        return node.Hash if node is not None else bytes(32)

    def RecalculateHash(self, root) -> bytes:
        """TrieHashMap.cs:213-233"""
        node = self._get(root)
        if node is None:
            return b""
        if node.Type == INTERNAL:
            return internal_hash(node.ChildrenMask, [self._get(c).Hash for c in node.Children])
        return leaf_hash(node.KeyHash, node.Value)

    def CheckAllNodeHashes(self, root) -> bool:
        """TrieHashMap.cs:170-179"""
        if root == 0:
            return True
        node = self._get(root)
        if node is None:
            raise RuntimeError("corrupted trie")
        if node.Hash != self.RecalculateHash(root):
            return False
        return all(self.CheckAllNodeHashes(c) for c in node.Children)

    def GetAllNodes(self, root) -> dict:
        """TrieHashMap.cs:181-186, :235-252"""
        out = {}

        def walk(r):
            if r == 0:
                return
            node = self._get(r)
            if node is None:
                raise RuntimeError("corrupted trie")
            out[r] = node
            for c in node.Children:
                walk(c)
        walk(root)
        return out

    def InsertAllNodes(self, root, all_nodes: dict):
        """TrieHashMap.cs:136-168: every internal node is rebuilt, and so rehashed, from its inserted children"""
        if root == 0:
            return 0
        node = all_nodes[root]
        if node.Type == INTERNAL:
            children = [self.InsertAllNodes(c, all_nodes) for c in node.Children]
            return self._new(InternalNode(node.ChildrenMask, children, [self._get(c).Hash for c in children]))
        return self._new(node)

    # ---- TrieHashMap.cs:268-289
    def _modify_internal(self, node, h, value, value_hash):
        if value == 0 and node.GetChildByHash(h) != 0 and len(node.Children) == 2:
            second = next(c for c in node.Children if c != node.GetChildByHash(h))
            if self._get(second).Type == LEAF:
                return second
        if value != 0 and node.GetChildByHash(h) != 0 and len(node.Children) == 1 and self._get(value).Type == LEAF:
            return value
        modified = InternalNode.ModifyChildren(node, h, value, [self._get(c).Hash for c in node.Children], value_hash)
        if modified is None:
            return 0
        return self._new(modified)

    # ---- TrieHashMap.cs:318-346
    def _split_leaf(self, node_id, leaf, height, key_hash, value):
        first, second = hash_fragment(leaf.KeyHash, height), hash_fragment(key_hash, height)
        if first != second:
            son = self._new(LeafNode(key_hash, value))
            return self._new(InternalNode.WithChildren([node_id, son], [first, second], [leaf.Hash, self._get(son).Hash]))
        son = self._split_leaf(node_id, leaf, height + 1, key_hash, value)
        return self._new(InternalNode.WithChildren([son], [first], [self._get(son).Hash]))

    # ---- TrieHashMap.cs:348-373
    def _add(self, root, height, key_hash, value, check):
        if root == 0:
            return self._new(LeafNode(key_hash, value))
        node = self._get(root)
        if node.Type == INTERNAL:
            h = hash_fragment(key_hash, height)
            updated = self._add(node.GetChildByHash(h), height + 1, key_hash, value, check)
            return self._modify_internal(node, h, updated, self._get(updated).Hash)
        if node.KeyHash != key_hash:
            return self._split_leaf(root, node, height, key_hash, value)
        if check:
            raise ValueError("Specified keyHash is already present or hash collision occured")
        return root if node.Value == value else self._new(LeafNode(node.KeyHash, value))      # UpdateLeafNode :298-305

    # ---- TrieHashMap.cs:375-405
    def _delete(self, root, height, key_hash, check):
        if root == 0:
            if check:
                raise KeyError("keyHash")
            return root
        node = self._get(root)
        if node.Type == INTERNAL:
            h = hash_fragment(key_hash, height)
            updated = self._delete(node.GetChildByHash(h), height + 1, key_hash, check)
            upd = self._get(updated)
            return self._modify_internal(node, h, updated, upd.Hash if upd is not None else None)
        if node.KeyHash != key_hash:
            if check:
                raise KeyError("keyHash")
            return root
        return 0

    # ---- TrieHashMap.cs:407-426
    def _update(self, root, height, key_hash, value):
        if root == 0:
            raise KeyError("keyHash")
        node = self._get(root)
        if node.Type == INTERNAL:
            h = hash_fragment(key_hash, height)
            updated = self._update(node.GetChildByHash(h), height + 1, key_hash, value)
            return self._modify_internal(node, h, updated, self._get(updated).Hash)
        if node.KeyHash != key_hash:
            raise KeyError("keyHash")
        return root if node.Value == value else self._new(LeafNode(node.KeyHash, value))


def canonical_root(items, depth=0):
    """The root hash of the canonical trie over {key hash: value}: a subtree holding one key is that leaf; a prefix
    shared by two or more key hashes is an internal node (single-child chain nodes included).  An empty set gives the
    zero hash.  Raises where the reference throws: equal key hashes are impossible in a dict, and two hashes that
    differ in bit 255 only run hash_fragment past the hash (IndexError)."""
    items = dict(items)
    if not items:
        return bytes(32)
    if len(items) == 1:
        (k, v), = items.items()
        return leaf_hash(k, v)
    groups = {}
    for k, v in items.items():
        groups.setdefault(hash_fragment(k, depth), {})[k] = v
    labels = sorted(groups)
    kids = []
    for f in labels:
        g = groups[f]
        kids.append(canonical_root(g, depth + 1) if len(g) > 1 else leaf_hash(*next(iter(g.items()))))
    return internal_hash(sum(1 << f for f in labels), kids)


def is_consistent(node: dict) -> bool:
    """NodeStorage.IsConsistent (NodeStorage.cs:85-110) over the parsed JSON object: hex strings as HexUtils reads and
    writes them (0x prefix, lower case)"""
    if not node:
        return False
    unhex = lambda s: bytes.fromhex(s[2:] if s.startswith("0x") else s)
    if node["NodeType"] == "0x1":
        h = internal_hash(int(node["ChildrenMask"], 16), [unhex(c) for c in node["ChildrenHash"]])
    else:
        h = leaf_hash(unhex(node["KeyHash"]), unhex(node["Value"]))
    return node["Hash"] == "0x" + h.hex()


STATE_TRIES = ("Balances", "Contracts", "Storage", "Transactions", "Events", "Validators")


def state_hash(roots) -> bytes:
    """BlockchainSnapshot.StateHash (BlockchainSnapshot.cs:71-80): the six roots in STATE_TRIES order, no Blocks"""
    roots = list(roots)
    assert len(roots) == 6 and all(len(r) == 32 for r in roots)
    return o.keccak256(b"".join(roots))
