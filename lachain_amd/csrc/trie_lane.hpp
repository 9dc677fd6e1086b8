// lachain_amd/csrc/trie_lane.hpp — the per-lane pieces of the state-trie layer (k_trie.hip): HashFragment, the path key
// that orders key hashes by fragments, the leaf hash and the internal-node hash.  One Keccak state per lane in
// registers, no LDS, no barriers, so tools/emul/trie_emul.cpp (RBC_HOST_EMULATION) runs them lane by lane on the CPU.
//
// Reference: Lachain.Storage/Trie/TrieHashMap.cs:307-316 (HashFragment), :213-233 (RecalculateHash), LeafNode.cs:13-18,
// InternalNode.cs:48-59 (GetChildrenLabels, UpdateHash), FastSynchronizerBatch.cs/NodeStorage.cs:85-110 (IsConsistent).
//   leaf     = Keccak-256(int32 LE key_len || key hash || value)
//   internal = Keccak-256(label_0 || child_0 || label_1 || child_1 ...), the labels being the set bits of the mask in
//              ascending order, paired with the child hashes as far as both last (the reference's Zip)
// Both hashes are computed word by word: message word g of a block goes to state word g mod 17, which is a
// compile-time index in the unrolled block loop, so the state is never indexed by a register.  A message word is
// gathered from memory at its own byte phase: whole words by rbc_load64 (two aligned loads and a funnel shift, both
// inside the item), bytes only at an item's two ends.
#pragma once
#include "rbc_lane.hpp"

// lcb_trie_node (include/lachain_bls.h), 16 bytes
#define TRIE_NODE_BYTES 16
#define TRIE_LEAF 0
#define TRIE_INTERNAL 1
#define TRIE_FRAGMENTS 51          // whole 5-bit fragments of a 256-bit key hash; bit 255 is left over

SDI u32 trie_popc(u32 x) {
#ifdef RBC_HOST_EMULATION
    return (u32)__builtin_popcount(x);
#else
    return (u32)__popc(x);
#endif
}
SDI u32 trie_ctz(u32 x) {                              // x != 0
#ifdef RBC_HOST_EMULATION
    return (u32)__builtin_ctz(x);
#else
    return (u32)(__ffs((int)x) - 1);
#endif
}
SDI u32 trie_clz64(u64 x) {
#ifdef RBC_HOST_EMULATION
    return x ? (u32)__builtin_clzll(x) : 64;
#else
    return x ? (u32)__clzll((long long)x) : 64;
#endif
}

// ------------------------------------------------------------------------------------------------ fragments, path keys
// HashFragment(hash, n): bits [5n, 5n + 5) of the hash read as a little-endian bit string, n = 0 .. 50.  h: the hash as
// four little-endian words in memory (indexed by n, so not a register array).
SDI u32 trie_fragment(const u64 *h, int n) {
    const int bit = 5 * n, w = bit >> 6, sh = bit & 63;
    u64 v = h[w] >> sh;
    if (sh > 59 && w < 3) v |= h[w + 1] << (64 - sh);
    return (u32)v & 31;
}
// The path key: fragments 0 .. 50 in order, each as a 5-bit number (most significant bit first), then bit 255.  As a
// 256-bit integer (pk[3] the most significant word) its order is the order of the fragment strings, so sorting by it
// puts shared prefixes together and the children of a node in label order.  Fully unrolled: h may live in registers.
SDI void trie_path_key(u64 pk[4], const u64 h[4]) {
#pragma unroll
    for (int w = 0; w < 4; w++) pk[w] = 0;
#pragma unroll
    for (int n = 0; n < TRIE_FRAGMENTS; n++) {
        const int bit = 5 * n, w = bit >> 6, sh = bit & 63;
        u64 v = h[w] >> sh;
        if (sh > 59 && w < 3) v |= h[w + 1] << (64 - sh);
        v &= 31;
        const int pos = 251 - 5 * n, pw = pos >> 6, ps = pos & 63;       // the fragment's lowest bit in the key
        pk[pw] |= v << ps;
        if (ps > 59) pk[pw + 1] |= v >> (64 - ps);                       // pos <= 251: pw + 1 <= 3 whenever ps > 59
    }
    pk[0] |= h[3] >> 63;
}
// fragment d of a path key in memory
SDI u32 trie_pk_fragment(const u64 *pk, int d) {
    const int pos = 251 - 5 * d, w = pos >> 6, sh = pos & 63;
    u64 v = pk[w] >> sh;
    if (sh > 59) v |= pk[w + 1] << (64 - sh);
    return (u32)v & 31;
}
// common prefix of two path keys in whole fragments: 0 .. 51; 51 for equal keys and for keys that differ in bit 255 only
SDI int trie_pk_lcp(const u64 a[4], const u64 b[4]) {
    u32 z = 0;
    bool run = true;
#pragma unroll
    for (int w = 3; w >= 0; w--) {
        const u32 zw = trie_clz64(a[w] ^ b[w]);
        z += run ? zw : 0;
        run = run && zw == 64;
    }
    return (int)(z / 5);
}

// ------------------------------------------------------------------------------------------------ the leaf hash
// Word h of the stream  c (4 bytes) || m[0 .. len) || 0x01 || 0 ...: bytes m[8h - 4 .. 8h + 4) for h >= 1
SDI u64 trie_body_word(const uint8_t *m, u64 len, u32 c, u64 h) {
    const u64 g = 8 * h;
    if (g >= 4 && g + 4 <= len) return rbc_load64(m + g - 4);
    u64 v = 0;
    if (g == 0) {
        v = c;
        for (u32 k = 0; k < 4; k++)
            if (k < len) v |= (u64)m[k] << (32 + 8 * k);
        if (len < 4) v |= (u64)0x01 << (8 * (4 + len));
        return v;
    }
    if (g - 4 > len) return 0;
    const u32 nb = (u32)(len - (g - 4));               // 0 .. 7 message bytes, then the domain byte
    for (u32 k = 0; k < nb; k++) v |= (u64)m[g - 4 + k] << (8 * k);
    return v | ((u64)0x01 << (8 * nb));
}
// Keccak-256(int32 LE key_len || [kh, 32 bytes, when KH] || m[0 .. len)).  KH = false: the item's bytes are the key
// hash and the value as they lie in memory (any key_len: only its four bytes enter the hash).  KH = true: the key
// hash comes in registers (the root builder has just computed it) and m is the value.
template <bool KH> SDI void trie_leaf_hash(u64 out[4], u32 key_len, const u64 *kh, const uint8_t *m, u64 len) {
    u64 s[25];
#pragma unroll
    for (int l = 0; l < 25; l++) s[l] = 0;
    const u64 G0 = KH ? 4 : 0;                         // whole words before the stream  c || m
    const u32 c = KH ? (u32)(kh[3] >> 32) : key_len;
    const u64 blocks = (8 * G0 + 4 + len) / 136 + 1;
#pragma unroll 1
    for (u64 b = 0; b < blocks; b++) {
        const u64 h0 = 17 * b - G0;                    // b = 0 with KH: words 0 .. 3 come from registers below
        if (b > 0 && 8 * (h0 + 16) + 4 <= len) {       // a whole rate block inside the item
#pragma unroll
            for (int l = 0; l < 17; l++) s[l] ^= rbc_load64(m + 8 * (h0 + l) - 4);
        } else {
#pragma unroll
            for (int l = 0; l < 17; l++) {
                u64 v;
                if (KH && l < 4 && b == 0) v = (l == 0 ? (u64)key_len : kh[l ? l - 1 : 0] >> 32) | (kh[l & 3] << 32);
                else v = trie_body_word(m, len, c, h0 + l);
                s[l] ^= v;
            }
        }
        if (b + 1 == blocks) s[16] ^= 0x8000000000000000ULL;
        keccak_f1600(s);
    }
#pragma unroll
    for (int w = 0; w < 4; w++) out[w] = s[w];
}

// ------------------------------------------------------------------------------------------------ the internal hash
// up to eight bytes of a 32-byte hash from byte x (0 .. 31) on, low byte first, zero above the hash's end; no load
// leaves the hash
SDI u64 trie_hash_bytes(const uint8_t *p, u32 x) {
    const u32 xx = x < 24 ? x : 24;
    return rbc_load64(p + xx) >> (8 * (x - xx));
}
// child hashes that lie back to back (the flat form, and a group of the root builder)
struct trie_children_flat {
    const uint8_t *base;
    SDI const uint8_t *at(u32 j) const { return base + 32 * (size_t)j; }
};
// child hashes by reference (the rehash form): ref >= 0 is node ref's hash in `hashes`, ref < 0 the literal ~ref
struct trie_children_ref {
    const int64_t *ref;
    const uint8_t *hashes, *literals;
    SDI const uint8_t *at(u32 j) const {
        const int64_t r = ref[j];
        return r >= 0 ? hashes + 32 * (size_t)r : literals + 32 * (size_t)~r;
    }
};
// Keccak-256 over min(c, popcount(mask)) pairs label || child.  Child j lies at message byte 33 j; a message word
// starts in child j = 8g / 33 at byte r = 8g mod 33 of it and may run on into child j + 1 (its label, then its hash).
// j, r, the current label and the labels still to come advance with the words; no division.
template <class CH> SDI void trie_internal_hash(u64 out[4], u32 mask, u32 c, const CH &ch) {
    u64 s[25];
#pragma unroll
    for (int l = 0; l < 25; l++) s[l] = 0;
    const u32 pc = trie_popc(mask), cnt = c < pc ? c : pc;
    const u32 blocks = 33 * cnt / 136 + 1;
    u32 j = 0, r = 0;
    u32 rest = mask;                                   // the labels of the children after j
    u32 label = 0;
    if (cnt) { label = trie_ctz(rest); rest &= rest - 1; }
#pragma unroll 1
    for (u32 b = 0; b < blocks; b++) {
#pragma unroll
        for (int l = 0; l < 17; l++) {
            u64 v = 0;
            if (j < cnt) {
                u32 n1;                                // bytes of this word that child j fills
                if (r == 0) {
                    v = (u64)label | (trie_hash_bytes(ch.at(j), 0) << 8);
                    n1 = 8;
                } else {
                    v = trie_hash_bytes(ch.at(j), r - 1);
                    n1 = 33 - r < 8 ? 33 - r : 8;
                }
                if (n1 < 8) {
                    if (j + 1 < cnt) {
                        v |= (u64)trie_ctz(rest) << (8 * n1);
                        if (n1 < 7) v |= trie_hash_bytes(ch.at(j + 1), 0) << (8 * (n1 + 1));
                    } else {
                        v |= (u64)0x01 << (8 * n1);    // the message ends inside this word
                    }
                }
                r += 8;
                if (r >= 33) {
                    r -= 33;
                    j++;
                    if (j < cnt) { label = trie_ctz(rest); rest &= rest - 1; }
                }
            } else if (j == cnt && r == 0) {
                v = 0x01;                              // the message ended on a word boundary
                r = 8;
            }
            s[l] ^= v;
        }
        if (b + 1 == blocks) s[16] ^= 0x8000000000000000ULL;
        keccak_f1600(s);
    }
#pragma unroll
    for (int w = 0; w < 4; w++) out[w] = s[w];
}

SDI bool trie_hash_eq(const u64 a[4], const u64 b[4]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]; }

// Node i of a flat batch: its record, its bytes data[off[i] .. off[i + 1]) (a leaf: key hash || value; an internal
// node: child hashes back to back, whole hashes only)
SDI void trie_node_hash(u64 h[4], const uint8_t *nodes, const uint8_t *data, const u64 *off, size_t i) {
    const u32 *rec = (const u32 *)(nodes + TRIE_NODE_BYTES * i);
    const u64 len = off[i + 1] - off[i];
    if (rec[0] == TRIE_LEAF) {
        trie_leaf_hash<false>(h, rec[2], nullptr, data + off[i], len);
    } else {
        trie_children_flat ch = {data + off[i]};
        trie_internal_hash(h, rec[1], (u32)(len / 32 < 33 ? len / 32 : 33), ch);
    }
}
SDI void trie_node_finish(const u64 h[4], size_t i, uint8_t *out32, const uint8_t *expected32, uint8_t *accept) {
    if (out32) rbc_store_hash(out32 + 32 * i, h);
    if (accept) {
        u64 e[4];
        rbc_load_hash(e, expected32 + 32 * i);
        accept[i] = trie_hash_eq(h, e);
    }
}
