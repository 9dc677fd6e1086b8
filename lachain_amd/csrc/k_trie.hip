// lachain_amd/csrc/k_trie.hip — gfx950 kernels: the state trie's node hashes, consistency checks and roots.
//
// Reference: Lachain.Storage/Trie/TrieHashMap.cs (InsertAllNodes :136-168, CheckAllNodeHashes :170-179, RecalculateHash
// :213-233, ModifyInternalNode :268-289, SplitLeafNode :318-346), LeafNode.cs, InternalNode.cs, NodeStorage.cs:85-110
// (IsConsistent), BlockchainSnapshot.cs:71-80 (StateHash).  The per-lane hashing lives in trie_lane.hpp.
//
// Hashing kernels (one node per lane, the sponge in registers, no LDS, no scratch):
//   k_trie_flat          flat batch: a lane hashes its leaf; an internal node is hashed in place (mixed mode) or its
//                        index is appended to a list (one vector atomic add) for
//   k_trie_flat_listed   the listed internal nodes, packed: an internal node runs up to 8 permutations against a
//                        leaf's 1 - 2, and a wave waits for its slowest lane
//   k_trie_level         rehash by reference: the nodes of one height, children through childRef
//   k_trie_items         roots: per item the key hash (Keccak-256 of the key unless given), its path key, trie and leaf hash
//   k_trie_merge         roots: one depth step, the head of each group hashes its members into an internal node
// Plumbing of the root builder (no hashing): k_trie_sort_key, k_trie_order, k_trie_heads, k_trie_roots_init,
// k_trie_roots_write.  The sort and the scans are hipcub's device-wide radix sort and exclusive sum.
#include "trie_lane.hpp"
#include "gate.hpp"
#include <hipcub/hipcub.hpp>

#define TRIE_BLOCK 256
typedef unsigned long long ull;

// ---------------------------------------------------------------- (a) flat hashing and consistency
// list == null: every lane hashes its node (mixed mode).  Otherwise internal nodes are left to k_trie_flat_listed.
extern "C" __global__ void __launch_bounds__(TRIE_BLOCK) k_trie_flat(const uint8_t *nodes, const uint8_t *data, const ull *off,
                                                                   const uint8_t *expected32, u32 n, uint8_t *out32,
                                                                   uint8_t *accept, u32 *count, u32 *list) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (list && ((const u32 *)(nodes + TRIE_NODE_BYTES * (size_t)i))[0] != TRIE_LEAF) {
        list[atomicAdd(count, 1u)] = i;                // at most n entries: every lane appends at most once
        return;
    }
    u64 h[4];
    trie_node_hash(h, nodes, data, (const u64 *)off, i);
    trie_node_finish(h, i, out32, expected32, accept);
}
// launched over n lanes (the count is known only on the device): lanes past the count leave at once
extern "C" __global__ void __launch_bounds__(TRIE_BLOCK) k_trie_flat_listed(const uint8_t *nodes, const uint8_t *data,
                                                                          const ull *off, const uint8_t *expected32, u32 n,
                                                                          uint8_t *out32, uint8_t *accept, const u32 *count,
                                                                          const u32 *list) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || j >= *count) return;
    const u32 i = list[j];
    if (i >= n) return;
    u64 h[4];
    trie_node_hash(h, nodes, data, (const u64 *)off, i);
    trie_node_finish(h, i, out32, expected32, accept);
}

// ---------------------------------------------------------------- (b) rehash by reference
// lanes t < count: node i = order[t].  A leaf hashes its bytes; an internal node its children childRef[childOff[i] ..
// childOff[i + 1]): hashes of lower levels of this batch (already written to hashes32) or literals.
extern "C" __global__ void __launch_bounds__(TRIE_BLOCK) k_trie_level(uint8_t *hashes32, const uint8_t *nodes,
                                                                    const uint8_t *data, const ull *off, const ull *child_off,
                                                                    const long long *child_ref, const uint8_t *literals32,
                                                                    const ull *order, u32 count) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const size_t i = (size_t)order[t];
    const u32 *rec = (const u32 *)(nodes + TRIE_NODE_BYTES * i);
    u64 h[4];
    if (rec[0] == TRIE_LEAF) {
        trie_leaf_hash<false>(h, rec[2], nullptr, data + off[i], off[i + 1] - off[i]);
    } else {
        const u64 c = child_off[i + 1] - child_off[i];
        trie_children_ref ch = {(const int64_t *)child_ref + child_off[i], hashes32, literals32};
        trie_internal_hash(h, rec[1], (u32)(c < 33 ? c : 33), ch);
    }
    rbc_store_hash(hashes32 + 32 * i, h);
}

// ---------------------------------------------------------------- (c) roots from key/value sets
// item i: its trie (trie_off has B + 1 entries, in items: the last b with trie_off[b] <= i), key hash, path key, leaf hash
extern "C" __global__ void __launch_bounds__(TRIE_BLOCK) k_trie_items(const uint8_t *keys, const ull *key_off,
                                                                    const uint8_t *values, const ull *val_off,
                                                                    const ull *trie_off, u32 B, u32 n, int keys_hashed,
                                                                    u64 *pk, u32 *tid, uint8_t *leaf32) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 lo = 0, hi = B;                                // trie_off[lo] <= i < trie_off[hi]
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (trie_off[mid] <= i) lo = mid; else hi = mid;
    }
    tid[i] = lo;
    u64 kh[4];
    if (keys_hashed) rbc_load_hash(kh, keys + key_off[i]);
    else rbc_keccak_range(kh, keys + key_off[i], key_off[i + 1] - key_off[i]);
    u64 p[4];
    trie_path_key(p, kh);
#pragma unroll
    for (int w = 0; w < 4; w++) pk[4 * (size_t)i + w] = p[w];
    u64 h[4];
    trie_leaf_hash<true>(h, 32, kh, values + val_off[i], val_off[i + 1] - val_off[i]);
    rbc_store_hash(leaf32 + 32 * (size_t)i, h);
}
// the sort key of one stable pass: word `word` of the path key of item perm[s] (perm == null: s itself), or its trie
extern "C" __global__ void __launch_bounds__(TRIE_BLOCK) k_trie_sort_key(const u64 *pk, const u32 *tid, const u32 *perm,
                                                                       int word, u32 n, u64 *key, u32 *perm_out) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const u32 i = perm ? perm[s] : s;
    key[s] = word < 4 ? pk[4 * (size_t)i + word] : (u64)tid[i];
    if (perm_out) perm_out[s] = i;
}
// sorted position s: its path key and trie, the common prefix with its left neighbour (-1 across tries and at 0), the
// tries the reference throws on (equal key hashes: Add's "already present"; key hashes that differ in bit 255 only:
// HashFragment runs past the hash at n = 51), and the first list of live entries: the leaves.  An entry is its hash,
// the sorted position of its first key with bit 31 set once it is an internal node, and its boundary prefix.
extern "C" __global__ void __launch_bounds__(TRIE_BLOCK) k_trie_order(const u64 *pk, const u32 *tid, const u32 *perm,
                                                                    const uint8_t *leaf32, u32 n, u64 *spk, u32 *stid,
                                                                    uint8_t *bad, int *max_lcp, u64 *ehash, u32 *efirst,
                                                                    int *elcp, u32 *count) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const u32 i = perm[s];
    const u32 t = tid[i];
    u64 a[4];
#pragma unroll
    for (int w = 0; w < 4; w++) { a[w] = pk[4 * (size_t)i + w]; spk[4 * (size_t)s + w] = a[w]; }
    stid[s] = t;
    int lcp = -1;
    if (s > 0) {
        const u32 ip = perm[s - 1];
        if (tid[ip] == t) {
            u64 b[4];
#pragma unroll
            for (int w = 0; w < 4; w++) b[w] = pk[4 * (size_t)ip + w];
            lcp = trie_pk_lcp(a, b);
            if (lcp >= TRIE_FRAGMENTS) {               // the trie's result is discarded; keep its construction bounded
                bad[t] = 1;
                lcp = TRIE_FRAGMENTS - 1;
            }
            atomicMax(max_lcp, lcp);
        }
    }
#pragma unroll
    for (int w = 0; w < 4; w++) ehash[4 * (size_t)s + w] = ((const u64 *)leaf32)[4 * (size_t)i + w];
    efirst[s] = s;
    elcp[s] = lcp;
    if (s == 0) *count = n;
}
// depth step d, part 1: head[e] = entry e starts a group (its boundary prefix is not d); zero past the live count
extern "C" __global__ void __launch_bounds__(TRIE_BLOCK) k_trie_heads(const int *elcp, const u32 *count, int d, u32 n,
                                                                    u32 *head) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    head[e] = e < *count && elcp[e] != d;
}
// part 2: the head of each group.  Its members are the entries after it whose boundary prefix is d: subtrees that
// share d fragments and differ in fragment d, at most 32 and in label order.  Two or more members, or one that is an
// internal node already (a single-child chain node), become an internal node at depth d; a lone leaf stays as it is.
// pos: the exclusive sum of head.  The last live entry writes the next count.
extern "C" __global__ void __launch_bounds__(TRIE_BLOCK) k_trie_merge(const u64 *spk, const u64 *ehash, const u32 *efirst,
                                                                    const int *elcp, const u32 *head, const u32 *pos,
                                                                    const u32 *count, int d, u32 n, u64 *ohash, u32 *ofirst,
                                                                    int *olcp, u32 *ocount) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const u32 live = *count;
    if (e >= live) return;
    if (e == live - 1) *ocount = pos[e] + head[e];
    if (!head[e]) return;
    u32 m = 1, mask = 0;
    while (m < 32 && e + m < live && elcp[e + m] == d) m++;
    const u32 first = efirst[e];
    const u32 o = pos[e];
    u64 h[4];
    if (m >= 2 || (first >> 31)) {
        for (u32 k = 0; k < m; k++) mask |= 1u << trie_pk_fragment(spk + 4 * (size_t)(efirst[e + k] & 0x7fffffffu), d);
        trie_children_flat ch = {(const uint8_t *)(ehash + 4 * (size_t)e)};
        trie_internal_hash(h, mask, m, ch);
        ofirst[o] = first | 0x80000000u;
    } else {
#pragma unroll
        for (int w = 0; w < 4; w++) h[w] = ehash[4 * (size_t)e + w];
        ofirst[o] = first;
    }
#pragma unroll
    for (int w = 0; w < 4; w++) ohash[4 * (size_t)o + w] = h[w];
    olcp[o] = elcp[e];
}
// per trie: the zero root; status 1 unless the reference throws on the set (an empty set is GetHash's zero fallback)
extern "C" __global__ void __launch_bounds__(TRIE_BLOCK) k_trie_roots_init(uint8_t *roots32, uint8_t *status,
                                                                         const uint8_t *bad, u32 B) {
    const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const u64 z[4] = {0, 0, 0, 0};
    rbc_store_hash(roots32 + 32 * (size_t)b, z);
    status[b] = bad ? !bad[b] : 1;
}
// after the step at depth 0 one entry is left per non-empty trie
extern "C" __global__ void __launch_bounds__(TRIE_BLOCK) k_trie_roots_write(const u64 *ehash, const u32 *efirst,
                                                                          const u32 *stid, const uint8_t *bad,
                                                                          const u32 *count, u32 n, u32 B, uint8_t *roots32) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || e >= *count) return;
    const u32 t = stid[efirst[e] & 0x7fffffffu];
    if (t >= B || bad[t]) return;
    rbc_store_hash(roots32 + 32 * (size_t)t, ehash + 4 * (size_t)e);
}

// ---------------------------------------------------------------- host launch wrappers
static unsigned trie_blocks(u32 n) { return (n + TRIE_BLOCK - 1) / TRIE_BLOCK; }
// list_ws: a count and n indices, or null for the mixed launch
extern "C" void lcbk_trie_flat(hipStream_t s, const uint8_t *nodes, const uint8_t *data, const uint64_t *off,
                               const uint8_t *expected32, u32 n, uint8_t *out32, uint8_t *accept, uint32_t *list_ws) {
    if (!n) return;
    if (list_ws) (void)hipMemsetAsync(list_ws, 0, 4, s);
    LCB_LAUNCH_GATED(k_trie_flat, dim3(trie_blocks(n)), dim3(TRIE_BLOCK), 0, s, nodes, data, (const ull *)off, expected32, n,
                     out32, accept, list_ws, list_ws ? list_ws + 1 : nullptr);
    if (!list_ws) return;
    LCB_LAUNCH_GATED(k_trie_flat_listed, dim3(trie_blocks(n)), dim3(TRIE_BLOCK), 0, s, nodes, data, (const ull *)off,
                     expected32, n, out32, accept, (const u32 *)list_ws, (const u32 *)(list_ws + 1));
}
extern "C" void lcbk_trie_level(hipStream_t s, uint8_t *hashes32, const uint8_t *nodes, const uint8_t *data,
                                const uint64_t *off, const uint64_t *child_off, const int64_t *child_ref,
                                const uint8_t *literals32, const uint64_t *order, u32 count) {
    if (!count) return;
    LCB_LAUNCH_GATED(k_trie_level, dim3(trie_blocks(count)), dim3(TRIE_BLOCK), 0, s, hashes32, nodes, data, (const ull *)off,
                     (const ull *)child_off, (const long long *)child_ref, literals32, (const ull *)order, count);
}

// The root builder's workspace, carved from one allocation by lcb_trie.cpp; every part 8-byte aligned.
struct trie_root_ws {
    u64 *pk, *spk, *key[2], *ehash[2];
    u32 *tid, *stid, *perm[2], *efirst[2], *head, *pos, *count;     // count: 2 words (ping-pong), then max_lcp
    int *elcp[2];
    uint8_t *leaf32, *bad, *tmp;
    size_t tmp_bytes;
};
static size_t trie_al(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t trie_tmp_bytes(u32 n) {
    size_t a = 0, b = 0;
    hipcub::DoubleBuffer<u64> dk(nullptr, nullptr);
    hipcub::DoubleBuffer<u32> dv(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, dk, dv, (int)n, 0, 64, (hipStream_t)0);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (u32 *)nullptr, (u32 *)nullptr, (int)n, (hipStream_t)0);
    return a > b ? a : b;
}
static size_t trie_carve(trie_root_ws &w, uint8_t *base, u32 n, u32 B) {
    size_t o = 0;
    auto take = [&](size_t bytes) { uint8_t *p = base ? base + o : nullptr; o += trie_al(bytes); return p; };
    const size_t N = n ? n : 1;
    w.pk = (u64 *)take(32 * N);
    w.spk = (u64 *)take(32 * N);
    for (int k = 0; k < 2; k++) w.key[k] = (u64 *)take(8 * N);
    for (int k = 0; k < 2; k++) w.ehash[k] = (u64 *)take(32 * N);
    w.tid = (u32 *)take(4 * N);
    w.stid = (u32 *)take(4 * N);
    for (int k = 0; k < 2; k++) w.perm[k] = (u32 *)take(4 * N);
    for (int k = 0; k < 2; k++) w.efirst[k] = (u32 *)take(4 * N);
    for (int k = 0; k < 2; k++) w.elcp[k] = (int *)take(4 * N);
    w.head = (u32 *)take(4 * N);
    w.pos = (u32 *)take(4 * N);
    w.count = (u32 *)take(16);
    w.leaf32 = take(32 * N);
    w.bad = take(B ? B : 1);
    w.tmp_bytes = trie_tmp_bytes(n);
    w.tmp = take(w.tmp_bytes);
    return o;
}
extern "C" size_t lcbk_trie_root_ws_bytes(u32 n, u32 B) {
    trie_root_ws w;
    return trie_carve(w, nullptr, n, B);
}
// Enqueues the whole construction on s.  Reads the largest common prefix back once (the stream is synchronised) to
// know how many depth steps to launch.  Returns 0, or -1 when a device call failed.
extern "C" int lcbk_trie_roots(hipStream_t s, uint8_t *roots32, uint8_t *status, const uint8_t *keys, const uint64_t *key_off,
                               const uint8_t *values, const uint64_t *val_off, const uint64_t *trie_off, u32 B, u32 n,
                               int keys_hashed, void *ws) {
    if (!B) return 0;
    trie_root_ws w;
    trie_carve(w, (uint8_t *)ws, n, B);
    const dim3 blk(TRIE_BLOCK), gn(trie_blocks(n ? n : 1)), gb(trie_blocks(B));
    if (!n) {
        LCB_LAUNCH_GATED(k_trie_roots_init, gb, blk, 0, s, roots32, status, (const uint8_t *)nullptr, B);
        return 0;
    }
    int *max_lcp = (int *)(w.count + 2);
    (void)hipMemsetAsync(w.bad, 0, B, s);
    (void)hipMemsetAsync(max_lcp, 0xff, 4, s);         // -1
    LCB_LAUNCH_GATED(k_trie_items, gn, blk, 0, s, keys, (const ull *)key_off, values, (const ull *)val_off,
                     (const ull *)trie_off, B, n, keys_hashed, w.pk, w.tid, w.leaf32);
    // stable passes from the least significant word up: path key words 0 .. 3, then the trie
    int cur = 0;
    for (int word = 0; word < (B > 1 ? 5 : 4); word++) {
        LCB_LAUNCH_GATED(k_trie_sort_key, gn, blk, 0, s, (const u64 *)w.pk, (const u32 *)w.tid,
                         word ? (const u32 *)w.perm[cur] : (const u32 *)nullptr, word, n, w.key[0],
                         word ? (u32 *)nullptr : w.perm[cur]);
        hipcub::DoubleBuffer<u64> dk(w.key[0], w.key[1]);
        hipcub::DoubleBuffer<u32> dv(w.perm[cur], w.perm[cur ^ 1]);
        size_t tb = w.tmp_bytes;
        if (hipcub::DeviceRadixSort::SortPairs(w.tmp, tb, dk, dv, (int)n, 0, word < 4 ? 64 : 32, s) != hipSuccess) return -1;
        if (dv.Current() != w.perm[cur]) cur ^= 1;
    }
    LCB_LAUNCH_GATED(k_trie_order, gn, blk, 0, s, (const u64 *)w.pk, (const u32 *)w.tid, (const u32 *)w.perm[cur],
                     (const uint8_t *)w.leaf32, n, w.spk, w.stid, w.bad, max_lcp, w.ehash[0], w.efirst[0], w.elcp[0], w.count);
    int depth = -1;
    if (hipMemcpyAsync(&depth, max_lcp, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
    if (hipStreamSynchronize(s) != hipSuccess) return -1;
    if (depth >= TRIE_FRAGMENTS) depth = TRIE_FRAGMENTS - 1;
    int e = 0;
    for (int d = depth; d >= 0; d--, e ^= 1) {
        LCB_LAUNCH_GATED(k_trie_heads, gn, blk, 0, s, (const int *)w.elcp[e], (const u32 *)(w.count + e), d, n, w.head);
        size_t tb = w.tmp_bytes;
        if (hipcub::DeviceScan::ExclusiveSum(w.tmp, tb, w.head, w.pos, (int)n, s) != hipSuccess) return -1;
        LCB_LAUNCH_GATED(k_trie_merge, gn, blk, 0, s, (const u64 *)w.spk, (const u64 *)w.ehash[e], (const u32 *)w.efirst[e],
                         (const int *)w.elcp[e], (const u32 *)w.head, (const u32 *)w.pos, (const u32 *)(w.count + e), d, n,
                         w.ehash[e ^ 1], w.efirst[e ^ 1], w.elcp[e ^ 1], w.count + (e ^ 1));
    }
    LCB_LAUNCH_GATED(k_trie_roots_init, gb, blk, 0, s, roots32, status, (const uint8_t *)w.bad, B);
    LCB_LAUNCH_GATED(k_trie_roots_write, gn, blk, 0, s, (const u64 *)w.ehash[e], (const u32 *)w.efirst[e],
                     (const u32 *)w.stid, (const uint8_t *)w.bad, (const u32 *)(w.count + e), n, B, roots32);
    return 0;
}
