"""Python mirror of the reference's state trie (Lachain.Storage/Trie: TrieHashMap, LeafNode, InternalNode) on the
device's node hashing, with the reference's method names.

Hashing is deferred: a structural edit (Add, Update, Delete ...) creates nodes without a hash, and GetHash /
CheckAllNodeHashes hash every such node once, in one lcb_trie_rehash_batch call, instead of rehashing the root path
for every key as the reference does.  The reference's folding rules (ModifyInternalNode, SplitLeafNode) look at node
types and child counts only, never at hashes, so deferral changes no structure and no hash.  CheckAllNodeHashes and
NodeStorage.IsConsistentBatch go through one flat lcb_trie_node_hash_batch call.  Storage proper (RocksDB, persisted
node ids, caches) is not mirrored: nodes live in a dictionary."""
from . import native

LEAF, INTERNAL = native.TRIE_LEAF, native.TRIE_INTERNAL
STATE_TRIES = ("Balances", "Contracts", "Storage", "Transactions", "Events", "Validators")


def _popcount_below(mask: int, h: int) -> int:
    return bin(mask & ((1 << h) - 1)).count("1")


def HashFragment(h: bytes, n: int) -> int:
    """TrieHashMap.HashFragment: bits [5n, 5n + 5) of the hash as a little-endian bit string, n = 0 .. 50"""
    if not 0 <= n <= 50:
        raise IndexError("a key hash has 51 whole fragments")
    return (int.from_bytes(h, "little") >> (5 * n)) & 31


class LeafNode:
    Type = LEAF
    Children = ()

    def __init__(self, key_hash, value, hash_=None):
        self.KeyHash, self.Value, self.Hash = bytes(key_hash), bytes(value), hash_

    def GetChildByHash(self, h):
        return 0


class InternalNode:
    Type = INTERNAL

    def __init__(self, mask, children, hash_=None):
        self.ChildrenMask, self.Children, self.Hash = mask, list(children), hash_

    def GetChildByHash(self, h):
        if not (self.ChildrenMask >> h) & 1:
            return 0
        return self.Children[_popcount_below(self.ChildrenMask, h)]


class TrieHashMap:
    """Every method takes the root id and returns the new root id, as the reference's do; old roots stay valid."""

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
        return native.keccak256_batch([bytes(key)])

    @staticmethod
    def HashBatch(keys):
        h = native.keccak256_batch([bytes(k) for k in keys])
        return [h[32 * i:32 * i + 32] for i in range(len(keys))]

    # ---- the reference's surface (keys are hashed on the device; *_by_hash take the key hash)
    def Add(self, root, key, value):
        return self.add_by_hash(root, self.Hash(key), value, True)

    def AddOrUpdate(self, root, key, value):
        return self.add_by_hash(root, self.Hash(key), value, False)

    def Update(self, root, key, value):
        return self.update_by_hash(root, self.Hash(key), value)

    def Delete(self, root, key):
        return self.delete_by_hash(root, self.Hash(key), True)

    def TryDelete(self, root, key):
        return self.delete_by_hash(root, self.Hash(key), False)

    def Find(self, root, key):
        return self.find_by_hash(root, self.Hash(key))

    def add_by_hash(self, root, key_hash, value, check=True):
        return self._add(root, 0, bytes(key_hash), bytes(value), check)

    def update_by_hash(self, root, key_hash, value):
        return self._update(root, 0, bytes(key_hash), bytes(value))

    def delete_by_hash(self, root, key_hash, check=True):
        return self._delete(root, 0, bytes(key_hash), check)

    def find_by_hash(self, root, key_hash):
        key_hash = bytes(key_hash)
        height = 0
        while root:
            node = self._get(root)
            if node.Type == LEAF:
                return node.Value if node.KeyHash == key_hash else None
            root = node.GetChildByHash(HashFragment(key_hash, height))
            height += 1
        return None

    # ---- hashing
    def _flush(self, root):
        """hash every node below root that has no hash yet: one rehash call, clean children as literals"""
        order, index, stack = [], {}, [root] if root else []
        while stack:
            r = stack.pop()
            node = self._get(r)
            if node is None:
                raise RuntimeError("corrupted trie")
            if node.Hash is not None or r in index:
                continue
            index[r] = len(order)
            order.append(r)
            stack.extend(node.Children)
        if not order:
            return
        records, items, children, literals, lit_index = [], [], [], [], {}
        for r in order:
            node = self.nodes[r]
            if node.Type == LEAF:
                records.append(native.trie_node(LEAF, 0, len(node.KeyHash)))
                items.append(node.KeyHash + node.Value)
                children.append([])
                continue
            refs = []
            for c in node.Children:
                if c in index:
                    refs.append(index[c])
                else:
                    if c not in lit_index:
                        lit_index[c] = len(literals)
                        literals.append(self.nodes[c].Hash)
                    refs.append(~lit_index[c])
            records.append(native.trie_node(INTERNAL, node.ChildrenMask, 0))
            items.append(b"")
            children.append(refs)
        hashes = native.trie_rehash_batch(b"".join(records), items, children, literals)
        for k, r in enumerate(order):
            self.nodes[r].Hash = hashes[32 * k:32 * k + 32]

    def GetHash(self, root) -> bytes:
        """the root's hash, the zero hash for no node; hashes what is pending first"""
        if self._get(root) is None:
            return bytes(32)
        self._flush(root)
        return self.nodes[root].Hash

    def _flat(self, ids):
        records, items = [], []
        for r in ids:
            node = self.nodes[r]
            if node.Type == LEAF:
                records.append(native.trie_node(LEAF, 0, len(node.KeyHash)))
                items.append(node.KeyHash + node.Value)
            else:
                records.append(native.trie_node(INTERNAL, node.ChildrenMask, 0))
                items.append(b"".join(self.nodes[c].Hash for c in node.Children))
        return b"".join(records), items

    def RecalculateHash(self, root) -> bytes:
        node = self._get(root)
        if node is None:
            return b""
        for c in node.Children:
            self._flush(c)
        return native.trie_node_hash_batch(*self._flat([root]))[0]

    def CheckAllNodeHashes(self, root) -> bool:
        """every node's stored hash against its recomputed one, in one flat call"""
        if root == 0:
            return True
        self._flush(root)
        ids = list(self.GetAllNodes(root))
        records, items = self._flat(ids)
        _, accept = native.trie_node_hash_batch(records, items, b"".join(self.nodes[r].Hash for r in ids))
        return all(accept)

    def GetAllNodes(self, root) -> dict:
        out, stack = {}, [root] if root else []
        while stack:
            r = stack.pop()
            node = self._get(r)
            if node is None:
                raise RuntimeError("corrupted trie")
            out[r] = node
            stack.extend(node.Children)
        return out

    def InsertAllNodes(self, root, all_nodes: dict):
        """copies a downloaded trie in; every internal node is rebuilt without a hash and the leaves keep theirs, as in
        the reference; the hashes come from one rehash call at the end"""
        def insert(r):
            if r == 0:
                return 0
            node = all_nodes[r]
            if node.Type == INTERNAL:
                return self._new(InternalNode(node.ChildrenMask, [insert(c) for c in node.Children]))
            return self._new(LeafNode(node.KeyHash, node.Value, node.Hash))
        new_root = insert(root)
        self._flush(new_root)
        return new_root

    # ---- structure: TrieHashMap.cs:268-426 without the hashes
    def _modify_internal(self, node, h, value):
        was = node.GetChildByHash(h)
        if value == 0 and was != 0 and len(node.Children) == 2:
            second = next(c for c in node.Children if c != was)
            if self._get(second).Type == LEAF:
                return second
        if value != 0 and was != 0 and len(node.Children) == 1 and self._get(value).Type == LEAF:
            return value
        pos = _popcount_below(node.ChildrenMask, h)
        if was == value:
            return self._new(node)
        if was == 0:
            return self._new(InternalNode(node.ChildrenMask | (1 << h), node.Children[:pos] + [value] + node.Children[pos:]))
        if value == 0:
            if len(node.Children) == 1:
                return 0
            return self._new(InternalNode(node.ChildrenMask ^ (1 << h), node.Children[:pos] + node.Children[pos + 1:]))
        return self._new(InternalNode(node.ChildrenMask, node.Children[:pos] + [value] + node.Children[pos + 1:]))

    def _split_leaf(self, node_id, leaf, height, key_hash, value):
        first, second = HashFragment(leaf.KeyHash, height), HashFragment(key_hash, height)
        if first != second:
            son = self._new(LeafNode(key_hash, value))
            kids = [node_id, son] if first < second else [son, node_id]
            return self._new(InternalNode((1 << first) | (1 << second), kids))
        return self._new(InternalNode(1 << first, [self._split_leaf(node_id, leaf, height + 1, key_hash, value)]))

    def _add(self, root, height, key_hash, value, check):
        if root == 0:
            return self._new(LeafNode(key_hash, value))
        node = self._get(root)
        if node.Type == INTERNAL:
            h = HashFragment(key_hash, height)
            return self._modify_internal(node, h, self._add(node.GetChildByHash(h), height + 1, key_hash, value, check))
        if node.KeyHash != key_hash:
            return self._split_leaf(root, node, height, key_hash, value)
        if check:
            raise ValueError("Specified keyHash is already present or hash collision occured")
        return root if node.Value == value else self._new(LeafNode(node.KeyHash, value))

    def _delete(self, root, height, key_hash, check):
        if root == 0:
            if check:
                raise KeyError("keyHash")
            return root
        node = self._get(root)
        if node.Type == INTERNAL:
            h = HashFragment(key_hash, height)
            return self._modify_internal(node, h, self._delete(node.GetChildByHash(h), height + 1, key_hash, check))
        if node.KeyHash != key_hash:
            if check:
                raise KeyError("keyHash")
            return root
        return 0

    def _update(self, root, height, key_hash, value):
        if root == 0:
            raise KeyError("keyHash")
        node = self._get(root)
        if node.Type == INTERNAL:
            h = HashFragment(key_hash, height)
            return self._modify_internal(node, h, self._update(node.GetChildByHash(h), height + 1, key_hash, value))
        if node.KeyHash != key_hash:
            raise KeyError("keyHash")
        return root if node.Value == value else self._new(LeafNode(node.KeyHash, value))


class NodeStorage:
    @staticmethod
    def IsConsistentBatch(json_nodes):
        """NodeStorage.IsConsistent for a list of parsed JSON nodes (fields NodeType, ChildrenMask, ChildrenHash,
        KeyHash, Value, Hash; hex strings as HexUtils reads them): a list of bools from one flat call.  A null or empty
        node is inconsistent, and so is a Hash string that is not HexUtils.ToHex's spelling (0x, lower case), since the
        reference compares strings."""
        def unhex(s):
            s = s or ""
            return bytes.fromhex(s[2:] if s[:2].lower() == "0x" else s)
        records, items, expected, where = [], [], [], []
        for k, node in enumerate(json_nodes):
            if not node:
                continue
            claimed = unhex(node["Hash"])
            if len(claimed) != 32 or node["Hash"] != "0x" + claimed.hex():
                continue
            if node["NodeType"] == "0x1":
                hashes = [unhex(c) for c in node["ChildrenHash"]]
                if any(len(c) != 32 for c in hashes):
                    raise ValueError("a child hash is 32 bytes")
                records.append(native.trie_node(INTERNAL, int(node["ChildrenMask"], 16), 0))
                items.append(b"".join(hashes))
            else:
                key_hash = unhex(node["KeyHash"])
                records.append(native.trie_node(LEAF, 0, len(key_hash)))
                items.append(key_hash + unhex(node["Value"]))
            expected.append(claimed)
            where.append(k)
        out = [False] * len(json_nodes)
        if where:
            _, accept = native.trie_node_hash_batch(b"".join(records), items, b"".join(expected))
            for k, a in zip(where, accept):
                out[k] = bool(a)
        return out


def StateHash(roots) -> bytes:
    """BlockchainSnapshot.StateHash: Keccak-256 of the six roots in STATE_TRIES order (Blocks is not part of it)"""
    roots = [bytes(r) for r in roots]
    if len(roots) != 6 or any(len(r) != 32 for r in roots):
        raise ValueError("six 32-byte roots: " + ", ".join(STATE_TRIES))
    return native.keccak256_batch([b"".join(roots)])


def state_root_from_items(tries, keys_hashed=False):
    """roots of key/value sets built on the device (lcb_trie_root_batch): tries is a list of lists of (key, value).
    Returns (roots, status); status 0 marks a set on which the reference throws."""
    return native.trie_root_batch([list(t) for t in tries], keys_hashed)
