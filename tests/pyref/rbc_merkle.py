"""Plain Python restatement of the reference's reliable-broadcast Merkle routines and the block root, over the oracle's
Keccak-256 (o.keccak256, pinned by the reference's KAT in tests/golden/secp256k1_kats.json).  TEST INFRASTRUCTURE: the
yardstick of tests/test_rbc_cpu.py and tests/test_gpu_rbc.py; the library is never compared with itself.

Reference: src/Lachain.Consensus/ReliableBroadcast/ReliableBroadcast.cs (tree size :41-43, CheckEchoMessage :296-309,
AugmentInput :311-319, MerkleTreeBranch :366-373, ConstructMerkleTree :375-386) and
src/Lachain.Crypto/Misc/MerkleTree.cs:139-191 (Build / ComputeRoot)."""
import struct

import oracle as o

ZERO = bytes(32)


def tree_size(n: int) -> int:
    """_merkleTreeSize: the smallest power of two >= n"""
    t = 1
    while t < n:
        t *= 2
    return t


def depth(n: int) -> int:
    return tree_size(n).bit_length() - 1


def augment(payload: bytes, n: int, f: int) -> bytes:
    """AugmentInput: int32 LE length prefix, zero padding up to shard size x data shards"""
    data = struct.pack("<i", len(payload)) + payload
    k = n - 2 * f
    size = (len(data) + k - 1) // k
    return data + bytes(k * size - len(data))


def shard_size(payload_len: int, n: int, f: int) -> int:
    k = n - 2 * f
    return (payload_len + 4 + k - 1) // k


def tree(shards):
    """ConstructMerkleTree: 2T nodes, node 0 zero (the reference leaves it null), leaves n..T-1 zero"""
    n, t = len(shards), tree_size(len(shards))
    nodes = [ZERO] * (2 * t)
    for i, s in enumerate(shards):
        nodes[t + i] = o.keccak256(bytes(s))
    for i in range(t - 1, 0, -1):
        nodes[i] = o.keccak256(nodes[2 * i] + nodes[2 * i + 1])
    return nodes


def branch(nodes, i: int):
    """MerkleTreeBranch: siblings from the leaf level up"""
    out = []
    i += len(nodes) // 2
    while i > 1:
        out.append(nodes[i ^ 1])
        i //= 2
    return out


def check_echo(data: bytes, frm: int, root: bytes, proof, n: int) -> bool:
    """CheckEchoMessage; from outside [0, n) never reaches it in the reference and is rejected"""
    if not 0 <= frm < n:
        return False
    value = o.keccak256(bytes(data))
    i, j = frm + tree_size(n), 0
    while i > 1 and j < len(proof):
        value = o.keccak256(value + proof[j]) if i % 2 == 0 else o.keccak256(proof[j] + value)
        i //= 2
        j += 1
    return value == root and i == 1


def compute_root(hashes):
    """MerkleTree.ComputeRoot: None for no hashes, the hash itself for one, else pair up with the odd last node doubled"""
    level = list(hashes)
    if not level:
        return None
    while len(level) > 1:
        level = [o.keccak256(level[2 * i] + (level[2 * i + 1] if 2 * i + 1 < len(level) else level[2 * i]))
                 for i in range((len(level) + 1) // 2)]
    return level[0]


def split(data: bytes, n: int):
    s = len(data) // n
    return [data[i * s:(i + 1) * s] for i in range(n)]


def val_messages(payload: bytes, n: int, f: int):
    """ConstructValMessages over the oracle's encoder: (shards, root, [proof of shard i])"""
    aug = augment(payload, n, f)
    shards = split(o.rs_encode_shards(aug, n, 2 * f) if f else aug, n)
    nodes = tree(shards)
    return shards, nodes[1], [branch(nodes, i) for i in range(n)]
