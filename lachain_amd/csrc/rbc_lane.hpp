// lachain_amd/csrc/rbc_lane.hpp — the per-lane pieces of the reliable-broadcast Merkle layer (k_rbc.hip): Keccak-256 of
// a byte range, the 64-byte node hash, CheckEchoMessage's walk and ComputeRoot's pairing.  One Keccak state per lane
// in registers, no LDS, no barriers, so tools/emul/rbc_emul.cpp (RBC_HOST_EMULATION) runs them lane by lane on the CPU.
//
// Reference: ReliableBroadcast.cs:296-309 (CheckEchoMessage), :375-386 (ConstructMerkleTree), MerkleTree.cs:139-176
// (Build).  A hash is four 64-bit words, little-endian, i.e. the first 32 state bytes after the squeeze.
#pragma once
#ifndef RBC_HOST_EMULATION
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include "keccak.hpp"

// eight message bytes at any alignment as one little-endian word.  Shards of one instance lie S bytes apart with S
// arbitrary, so a lane's pointer has any alignment: an unaligned word is put together from the two aligned words that
// hold it.  Both contain at least one of the eight bytes, so no load touches an aligned word that lies wholly outside
// the range.
SDI u64 rbc_load64(const uint8_t *p) {
    uintptr_t a = (uintptr_t)p;
    unsigned sh = (unsigned)(a & 7) * 8;
    const u64 *q = (const u64 *)(a & ~(uintptr_t)7);
    const u64 lo = q[0], hi = q[sh != 0];              // aligned: the same word again, shifted out below (no branch)
    return (lo >> sh) | ((hi << 1) << (63 - sh));
}
SDI void rbc_load_hash(u64 v[4], const uint8_t *p) {
#pragma unroll
    for (int w = 0; w < 4; w++) v[w] = rbc_load64(p + 8 * w);
}
SDI void rbc_store_hash(uint8_t *p, const u64 v[4]) {
    if ((((uintptr_t)p) & 7) == 0) {
#pragma unroll
        for (int w = 0; w < 4; w++) ((u64 *)p)[w] = v[w];
    } else {
#pragma unroll
        for (int k = 0; k < 32; k++) p[k] = (uint8_t)(v[k / 8] >> (8 * (k % 8)));
    }
}

// Keccak-256 (original padding 0x01 .. 0x80, rate 136) of m[0 .. len): whole words by rbc_load64, bytes only in the
// last, partial word.  len / 136 + 1 permutations.
SDI void rbc_keccak_range(u64 out[4], const uint8_t *m, u64 len) {
    u64 s[25];
#pragma unroll
    for (int l = 0; l < 25; l++) s[l] = 0;
    const u64 blocks = len / 136 + 1;
#pragma unroll 1
    for (u64 b = 0; b < blocks; b++) {
        const u64 base = b * 136;
        if (base + 136 <= len) {
#pragma unroll
            for (int l = 0; l < 17; l++) s[l] ^= rbc_load64(m + base + 8 * l);
        } else {                                       // the last block: the message's tail and the padding
#pragma unroll
            for (int l = 0; l < 17; l++) {
                const u64 g = base + 8 * l;
                u64 v = 0;
                if (g + 8 <= len) v = rbc_load64(m + g);
                else if (g <= len) {
                    const int nb = (int)(len - g);     // 0 .. 7 message bytes, then the domain byte
                    for (int k = 0; k < nb; k++) v |= (u64)m[g + k] << (8 * k);
                    v |= (u64)0x01 << (8 * nb);
                }
                s[l] ^= v;
            }
            s[16] ^= 0x8000000000000000ULL;
        }
        keccak_f1600(s);
    }
#pragma unroll
    for (int w = 0; w < 4; w++) out[w] = s[w];
}

// Keccak-256(l || r): one block, the padding bytes at 64 and 135
SDI void rbc_node_hash(u64 out[4], const u64 l[4], const u64 r[4]) {
    u64 s[25];
#pragma unroll
    for (int w = 0; w < 4; w++) { s[w] = l[w]; s[4 + w] = r[w]; }
    s[8] = 0x01;
#pragma unroll
    for (int w = 9; w < 25; w++) s[w] = 0;
    s[16] = 0x8000000000000000ULL;
    keccak_f1600(s);
#pragma unroll
    for (int w = 0; w < 4; w++) out[w] = s[w];
}

// log2 of the tree size T (the smallest power of two >= n, ReliableBroadcast.cs:41-43)
SDI int rbc_depth(int n) {
    int d = 0;
    while ((1 << d) < n) d++;
    return d;
}

// CheckEchoMessage from the leaf hash on: value climbs from node from + T while i > 1 and proof entries remain; accept
// iff the walk ends at the root's index with the root's value.  from outside [0, n) rejects (the reference never
// passes one).  proof: proof_len hashes, leaf level first; entries beyond the depth are not read.
SDI bool rbc_echo_walk(const u64 leaf[4], int from, int n, const uint8_t *proof, u64 proof_len, const uint8_t *root) {
    if (from < 0 || from >= n) return false;
    const int depth = rbc_depth(n);
    u64 v[4] = {leaf[0], leaf[1], leaf[2], leaf[3]};
    u32 i = (u32)from + (1u << depth);
    u64 j = 0;
#pragma unroll 1
    for (; i > 1 && j < proof_len; i >>= 1, j++) {
        u64 sib[4];
        rbc_load_hash(sib, proof + 32 * j);
        const bool right = i & 1;                      // odd index: we are the right sibling
        u64 a[4], b[4];
#pragma unroll
        for (int w = 0; w < 4; w++) { a[w] = right ? sib[w] : v[w]; b[w] = right ? v[w] : sib[w]; }
        rbc_node_hash(v, a, b);
    }
    u64 r[4];
    rbc_load_hash(r, root);
    return i == 1 && v[0] == r[0] && v[1] == r[1] && v[2] == r[2] && v[3] == r[3];
}

// MerkleTree.Build: the right child of parent i in a level of `count` nodes; an odd last node is paired with itself
SDI u64 rbc_right_child(u64 i, u64 count) { return 2 * i + 1 == count ? 2 * i : 2 * i + 1; }
SDI void rbc_root_pair(u64 out[4], const uint8_t *level, u64 i, u64 count) {
    u64 l[4], r[4];
    rbc_load_hash(l, level + 32 * (2 * i));
    rbc_load_hash(r, level + 32 * rbc_right_child(i, count));
    rbc_node_hash(out, l, r);
}
