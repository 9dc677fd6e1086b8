"""lachain_amd/rbc.py — the reliable broadcast's byte work under the reference's names, over the batched entry points
of liblachain_bls.so (lachain_amd/native.py): erasure coding, Keccak-256 Merkle trees and proofs, echo checks and the
decode-and-recheck step, many RBC instances per call.  Also MerkleTree.ComputeRoot for block transaction roots.

Reference: src/Lachain.Consensus/ReliableBroadcast/ReliableBroadcast.cs and src/Lachain.Crypto/Misc/MerkleTree.cs.
"""
import struct
from typing import List, NamedTuple, Optional, Sequence, Tuple

from . import native


class ValMessage(NamedTuple):
    """one validator's VAL / ECHO content (ReliableBroadcast.cs:326-334)"""
    root: bytes
    proof: List[bytes]
    shard: bytes


class Restored(NamedTuple):
    """TrySendReadyMessageFromEchos' outcome for one instance"""
    shards: Optional[List[bytes]]     # all N restored shards, None when the echoes cannot be decoded
    root: Optional[bytes]             # the rebuilt tree's root
    ok: bool                          # decoded, and the rebuilt root equals the echoes' root


def construct_val_messages(payloads: Sequence[bytes], n: int, f: int) -> List[List[ValMessage]]:
    """HandleInputMessage's AugmentInput + ConstructValMessages (:116, :311-338) for each payload: N records each"""
    shards, roots, proofs = native.rbc_val_batch(payloads, n, f)
    depth = native.rbc_tree_depth(n)
    out, at = [], 0
    for b, p in enumerate(payloads):
        s = native.rbc_shard_size(len(p), n, f)
        root = roots[32 * b:32 * b + 32]
        msgs = []
        for i in range(n):
            base = 32 * depth * (b * n + i)
            msgs.append(ValMessage(root, [proofs[base + 32 * j:base + 32 * j + 32] for j in range(depth)],
                                   shards[at + i * s:at + (i + 1) * s]))
        out.append(msgs)
        at += n * s
    return out


def check_echo_messages(echos: Sequence[Tuple[bytes, int, bytes, Sequence[bytes]]], n: int) -> List[bool]:
    """CheckEchoMessage (:296-309) for each (data, from, root, proof) of RBC instances with n validators"""
    doff, poff = [0], [0]
    for data, _, _, proof in echos:
        doff.append(doff[-1] + len(data))
        poff.append(poff[-1] + len(proof))
    acc = native.rbc_check_echo_batch(b"".join(e[0] for e in echos), doff, [e[1] for e in echos],
                                      b"".join(e[2] for e in echos), b"".join(b"".join(e[3]) for e in echos), poff, n)
    return [bool(a) for a in acc]


def restore_from_echos(instances: Sequence[Tuple[bytes, Sequence[Tuple[int, bytes]]]], n: int, f: int) -> List[Restored]:
    """TrySendReadyMessageFromEchos (:201-234) per instance = (the echoes' root, N - 2F echoes as (from, data) in any
    order): DecodeFromEchos, the restored shards' tree, and whether its root is the echoes'"""
    k = n - 2 * f
    off, frm = [0], []
    for _, echos in instances:
        if len(echos) != k:
            raise ValueError("restore_from_echos needs exactly N - 2F echoes per instance")
        off.append(off[-1] + sum(len(d) for _, d in echos))
        frm += [i for i, _ in echos]
    shards, status, root_ok, roots = native.rbc_decode_batch(
        b"".join(d for _, echos in instances for _, d in echos), off, frm, b"".join(r for r, _ in instances), n, f)
    out, at = [], 0
    for b in range(len(instances)):
        s = (off[b + 1] - off[b]) // k
        if status[b]:
            out.append(Restored([shards[at + i * s:at + (i + 1) * s] for i in range(n)], roots[32 * b:32 * b + 32],
                                bool(root_ok[b])))
        else:
            out.append(Restored(None, None, False))
        at += n * s
    return out


def payload_from_restored(shards: Sequence[bytes]) -> bytes:
    """CheckResult's read-back (:269-271): len = int32 LE, then bytes[4 : 4 + len] of the restored data"""
    data = b"".join(shards)
    (length,) = struct.unpack_from("<i", data, 0)
    if length < 0 or 4 + length > len(data):
        raise ValueError("restored data does not hold its length prefix's bytes")
    return data[4:4 + length]


def compute_root(hashes: Sequence[bytes]) -> Optional[bytes]:
    """MerkleTree.ComputeRoot (MerkleTree.cs:183-191): None for no hashes"""
    return native.merkle_root_batch([list(hashes)])[0]

