// lachain_amd/csrc/lcb_trie.cpp — host side of the state-trie layer (include/lachain_bls.h "state trie").
//
// Reference calls: NodeStorage.IsConsistent (FastSynchronizerBatch.cs/NodeStorage.cs:85-110), TrieHashMap.RecalculateHash /
// CheckAllNodeHashes / InsertAllNodes (TrieHashMap.cs:136-179, :213-233), the LeafNode constructor, InternalNode.
// UpdateHash, and the root of a key/value set as AddInternal / SplitLeafNode / ModifyInternalNode leave it
// (TrieHashMap.cs:268-373).  The kernels are k_trie.hip's; the host only checks arguments, orders the rehash levels and
// moves bytes.  No CPU fallback: every hash is computed on the device.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "launch.h"
#include "lcb_internal.hpp"
#include "../../include/lachain_bls.h"

using namespace lcb_int;

static_assert(sizeof(lcb_trie_node) == 16, "lcb_trie_node is the 16-byte record the trie kernels read");

namespace {

const size_t MAX_ITEMS = 0x7fffffffu;

bool fail(const char *what, const char *why) {
    static thread_local char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", what, why);
    set_err(msg);
    return false;
}
unsigned popcount32(uint32_t x) { return (unsigned)__builtin_popcount(x); }

// what the host-pointer forms read and the device forms must trust
bool host_nodes_ok(const lcb_trie_node *nodes, const uint64_t *off, size_t n, const char *what) {
    for (size_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i]) return fail(what, "offsets must not decrease");
        const uint64_t len = off[i + 1] - off[i];
        if (len > MAX_ITEMS) return fail(what, "an item of 2^31 bytes or more");
        if (nodes[i].kind > 1) return fail(what, "kind must be 0 (leaf) or 1 (internal)");
        if (nodes[i].reserved) return fail(what, "reserved must be 0");
        if (nodes[i].kind == 1 && len % 32) return fail(what, "an internal node's bytes must be whole 32-byte hashes");
        if (nodes[i].kind == 0 && nodes[i].key_len > len) return fail(what, "key_len runs past the leaf's bytes");
    }
    return true;
}

int flat_enqueue(lcb_ctx *c, hipStream_t s, uint8_t *out32, uint8_t *accept, const uint8_t *nodes, const uint8_t *data,
                 const uint64_t *off, const uint8_t *expected32, size_t n) {
    if (((uintptr_t)nodes & 3) || ((uintptr_t)off & 7)) {
        set_err("trie node hash: nodes must be 4-byte and data_off 8-byte aligned");
        return -1;
    }
    uint32_t *list = nullptr;
    if (!env_on("LCB_TRIE_MIXED")) {                   // measurement switch: one mixed launch
        list = (uint32_t *)c->trie[TRIE_LIST].get(4 * (n + 1));
        if (!list) { set_err("device allocation failed"); return -1; }
    }
    lcbk_trie_flat(s, nodes, data, off, expected32, (u32)n, out32, accept, list);
    return launch_ok("trie node hash launch") ? 0 : -1;
}

bool flat_args_ok(const void *out32, const void *accept, const void *nodes, const void *data, const void *off,
                  const void *expected32, size_t n) {
    const char *what = "trie node hash";
    if (n > MAX_ITEMS) return fail(what, "batch too large");
    if (n && (!nodes || !data || !off)) return fail(what, "nodes, data and data_off are required");
    if (n && !out32 && !accept) return fail(what, "out32 or accept is required");
    if (accept && !expected32) return fail(what, "accept needs expected32");
    return true;
}

int rehash_enqueue(lcb_ctx *c, hipStream_t s, uint8_t *hashes32, const uint8_t *nodes, const uint8_t *data,
                   const uint64_t *off, const uint64_t *child_off, const int64_t *child_ref, const uint8_t *literals32,
                   const uint64_t *order, const uint64_t *level_off, size_t n_levels) {
    if (((uintptr_t)nodes & 3) || (((uintptr_t)off | (uintptr_t)child_off | (uintptr_t)child_ref | (uintptr_t)order) & 7)) {
        set_err("trie rehash: nodes must be 4-byte aligned, the offset, reference and order arrays 8-byte aligned");
        return -1;
    }
    for (size_t l = 0; l < n_levels; l++)
        lcbk_trie_level(s, hashes32, nodes, data, off, child_off, child_ref, literals32, order + level_off[l],
                        (u32)(level_off[l + 1] - level_off[l]));
    return launch_ok("trie rehash launch") ? 0 : -1;
}

bool root_args_ok(const void *roots32, const void *status, const void *keys, const void *key_off, const void *values,
                  const void *val_off, const void *trie_off, size_t B, size_t n) {
    const char *what = "trie root";
    if (B > MAX_ITEMS || n > MAX_ITEMS) return fail(what, "batch too large");
    if (B && (!roots32 || !status || !trie_off)) return fail(what, "roots32, status and trie_off are required");
    if (n && (!keys || !key_off || !values || !val_off)) return fail(what, "keys, values and their offsets are required");
    return true;
}
int root_enqueue(lcb_ctx *c, hipStream_t s, uint8_t *roots32, uint8_t *status, const uint8_t *keys, const uint64_t *key_off,
                 const uint8_t *values, const uint64_t *val_off, const uint64_t *trie_off, size_t B, size_t n,
                 int keys_hashed) {
    if (((uintptr_t)key_off | (uintptr_t)val_off | (uintptr_t)trie_off) & 7) {
        set_err("trie root: the offset arrays must be 8-byte aligned");
        return -1;
    }
    void *ws = c->trie[TRIE_ROOT_WS].get(lcbk_trie_root_ws_bytes((u32)n, (u32)B));
    if (!ws) { set_err("device allocation failed"); return -1; }
    if (lcbk_trie_roots(s, roots32, status, keys, key_off, values, val_off, trie_off, (u32)B, (u32)n, keys_hashed, ws)) {
        set_err("trie root", hipGetLastError());
        return -1;
    }
    return launch_ok("trie root launch") ? 0 : -1;
}

}  // namespace

namespace lcb_int {
void trie_ctx_release(lcb_ctx *c) {
    for (auto &b : c->trie) b.release();
}
}  // namespace lcb_int

// ------------------------------------------------------------------ (a) flat hashing and consistency
extern "C" int lcb_ctx_trie_node_hash_dev(lcb_ctx *ctx, uint8_t *out32, uint8_t *accept, const lcb_trie_node *nodes,
                                          const uint8_t *data, const uint64_t *data_off, const uint8_t *expected32,
                                          size_t n, void *stream) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    if (!flat_args_ok(out32, accept, nodes, data, data_off, expected32, n)) return -1;
    Enq q(c, (hipStream_t)stream);
    if (!n) return 0;
    return flat_enqueue(c, q.s, out32, accept, (const uint8_t *)nodes, data, data_off, expected32, n);
}
extern "C" int lcb_trie_node_hash_dev(uint8_t *out32, uint8_t *accept, const lcb_trie_node *nodes, const uint8_t *data,
                                      const uint64_t *data_off, const uint8_t *expected32, size_t n, void *stream) {
    return lcb_ctx_trie_node_hash_dev(nullptr, out32, accept, nodes, data, data_off, expected32, n, stream);
}
extern "C" int lcb_trie_node_hash_batch(uint8_t *out32, uint8_t *accept, const lcb_trie_node *nodes, const uint8_t *data,
                                        const uint64_t *data_off, const uint8_t *expected32, size_t n) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!flat_args_ok(out32, accept, nodes, data, data_off, expected32, n)) return -1;
    if (!n) return 0;
    if (!host_nodes_ok(nodes, data_off, n, "trie node hash")) return -1;
    std::vector<uint64_t> rel;
    if (!rebase(rel, data_off, n, "trie node hash: offsets must not decrease")) return -1;
    HostCall h(c, "trie node hash");
    const lcb_trie_node *dn = h.in(nodes, n);
    const uint8_t *dd = h.in(data + data_off[0], (size_t)rel[n]);
    const uint64_t *doff = h.in(rel.data(), n + 1);
    const uint8_t *dexp = accept ? h.in(expected32, 32 * n) : nullptr;
    uint8_t *dout = h.out<uint8_t>(33 * n);
    if (!h.ok()) return -1;
    uint8_t *dh = out32 ? dout : nullptr, *dacc = accept ? dout + 32 * n : nullptr;
    if (flat_enqueue(c, h.s, dh, dacc, (const uint8_t *)dn, dd, doff, dexp, n)) return -1;
    h.back(out32, dh, 32 * n);
    h.back(accept, dacc, n);
    return h.finish();
}

// ------------------------------------------------------------------ (b) rehash by reference
extern "C" int lcb_ctx_trie_rehash_dev(lcb_ctx *ctx, uint8_t *hash_out32, const lcb_trie_node *nodes, const uint8_t *data,
                                       const uint64_t *data_off, const uint64_t *child_off, const int64_t *child_ref,
                                       const uint8_t *literals32, const uint64_t *order, const uint64_t *level_off,
                                       size_t n_levels, size_t n, void *stream) {
    const char *what = "trie rehash";
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    if (n > MAX_ITEMS || n_levels > MAX_ITEMS) { fail(what, "batch too large"); return -1; }
    if (n && (!hash_out32 || !nodes || !data || !data_off || !child_off || !child_ref || !order || !level_off)) {
        fail(what, "hash_out32, nodes, data, the offsets, child_ref, order and level_off are required");
        return -1;
    }
    for (size_t l = 0; n && l < n_levels; l++)         // level_off is host memory: the launches are sized from it
        if (level_off[l + 1] < level_off[l] || level_off[l + 1] > n) { fail(what, "level_off must rise within [0, n]"); return -1; }
    Enq q(c, (hipStream_t)stream);
    if (!n) return 0;
    return rehash_enqueue(c, q.s, hash_out32, (const uint8_t *)nodes, data, data_off, child_off, child_ref, literals32, order,
                          level_off, n_levels);
}
extern "C" int lcb_trie_rehash_dev(uint8_t *hash_out32, const lcb_trie_node *nodes, const uint8_t *data,
                                   const uint64_t *data_off, const uint64_t *child_off, const int64_t *child_ref,
                                   const uint8_t *literals32, const uint64_t *order, const uint64_t *level_off,
                                   size_t n_levels, size_t n, void *stream) {
    return lcb_ctx_trie_rehash_dev(nullptr, hash_out32, nodes, data, data_off, child_off, child_ref, literals32, order,
                                   level_off, n_levels, n, stream);
}
extern "C" int lcb_trie_rehash_batch(uint8_t *hash_out32, const lcb_trie_node *nodes, const uint8_t *data,
                                     const uint64_t *data_off, const uint64_t *child_off, const int64_t *child_ref,
                                     const uint8_t *literals32, size_t n_literals, size_t n) {
    const char *what = "trie rehash";
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (n > MAX_ITEMS) { fail(what, "batch too large"); return -1; }
    if (!n) return 0;
    if (!hash_out32 || !nodes || !data || !data_off || !child_off) {
        fail(what, "hash_out32, nodes, data, data_off and child_off are required");
        return -1;
    }
    if (!host_nodes_ok(nodes, data_off, n, what)) return -1;
    std::vector<uint64_t> rel, crel;
    if (!rebase(rel, data_off, n, "trie rehash: offsets must not decrease") ||
        !rebase(crel, child_off, n, "trie rehash: child offsets must not decrease"))
        return -1;
    const uint64_t base = child_off[0], n_refs = child_off[n] - base;
    if (n_refs && !child_ref) { fail(what, "child_ref is required"); return -1; }
    // heights: a node without in-batch children has height 0, a parent one more than its highest in-batch child.
    // Kahn's order over the child -> parent edges; a node that never runs dry of unprocessed children lies on a cycle.
    std::vector<uint32_t> pending(n, 0), height(n, 0), par_off(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        const uint64_t cnt = child_off[i + 1] - child_off[i];
        if (nodes[i].kind == 0 ? cnt != 0 : cnt != popcount32(nodes[i].mask)) {
            fail(what, "an internal node needs popcount(mask) children, a leaf none");
            return -1;
        }
        for (uint64_t k = child_off[i]; k < child_off[i + 1]; k++) {
            const int64_t r = child_ref[k];
            if (r >= 0 ? (uint64_t)r >= n : (uint64_t)~r >= n_literals) { fail(what, "a child reference is out of range"); return -1; }
            if (r >= 0) { pending[i]++; par_off[(size_t)r + 1]++; }
        }
    }
    if (n_literals && !literals32) { fail(what, "literals32 is required"); return -1; }
    for (size_t i = 0; i < n; i++) par_off[i + 1] += par_off[i];
    std::vector<uint32_t> parents(par_off[n]), fill(par_off.begin(), par_off.end() - 1);
    for (size_t i = 0; i < n; i++)
        for (uint64_t k = child_off[i]; k < child_off[i + 1]; k++)
            if (child_ref[k] >= 0) parents[fill[(size_t)child_ref[k]]++] = (uint32_t)i;
    std::vector<uint64_t> order;
    order.reserve(n);
    for (size_t i = 0; i < n; i++)
        if (!pending[i]) order.push_back(i);
    uint32_t max_h = 0;
    for (size_t q = 0; q < order.size(); q++) {
        const size_t i = (size_t)order[q];
        for (uint32_t k = par_off[i]; k < par_off[i + 1]; k++) {
            const uint32_t p = parents[k];
            if (height[p] < height[i] + 1) height[p] = height[i] + 1;
            if (--pending[p] == 0) { order.push_back(p); max_h = height[p] > max_h ? height[p] : max_h; }
        }
    }
    if (order.size() != n) { fail(what, "the child references form a cycle"); return -1; }
    std::vector<uint64_t> level_off(max_h + 2, 0), by_level(n);
    for (size_t i = 0; i < n; i++) level_off[height[i] + 1]++;
    for (size_t l = 0; l <= max_h; l++) level_off[l + 1] += level_off[l];
    {
        std::vector<uint64_t> at(level_off.begin(), level_off.end() - 1);
        for (size_t i = 0; i < n; i++) by_level[at[height[i]]++] = i;
    }
    HostCall h(c, what);
    const lcb_trie_node *dn = h.in(nodes, n);
    const uint8_t *dd = h.in(data + data_off[0], (size_t)rel[n]);
    const uint64_t *doff = h.in(rel.data(), n + 1);
    const uint8_t *dlit = h.in(literals32, 32 * n_literals);
    uint8_t *dout = h.out<uint8_t>(32 * n);
    const uint64_t *dcoff = h.in(crel.data(), n + 1);
    const int64_t *dref = h.in(n_refs ? child_ref + base : nullptr, (size_t)n_refs);
    const uint64_t *dord = h.in(by_level.data(), n);
    if (!h.ok()) return -1;
    if (rehash_enqueue(c, h.s, dout, (const uint8_t *)dn, dd, doff, dcoff, dref, dlit, dord, level_off.data(), max_h + 1)) return -1;
    h.back(hash_out32, dout, 32 * n);
    return h.finish();
}

// ------------------------------------------------------------------ (c) roots from key/value sets
extern "C" int lcb_ctx_trie_root_dev(lcb_ctx *ctx, uint8_t *roots32, uint8_t *status, const uint8_t *keys,
                                     const uint64_t *key_off, const uint8_t *values, const uint64_t *val_off,
                                     const uint64_t *trie_off, size_t B, size_t n_items, int keys_hashed, void *stream) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    if (!root_args_ok(roots32, status, keys, key_off, values, val_off, trie_off, B, n_items)) return -1;
    Enq q(c, (hipStream_t)stream);
    if (!B) return 0;
    return root_enqueue(c, q.s, roots32, status, keys, key_off, values, val_off, trie_off, B, n_items, keys_hashed);
}
extern "C" int lcb_trie_root_dev(uint8_t *roots32, uint8_t *status, const uint8_t *keys, const uint64_t *key_off,
                                 const uint8_t *values, const uint64_t *val_off, const uint64_t *trie_off, size_t B,
                                 size_t n_items, int keys_hashed, void *stream) {
    return lcb_ctx_trie_root_dev(nullptr, roots32, status, keys, key_off, values, val_off, trie_off, B, n_items, keys_hashed,
                                 stream);
}
extern "C" int lcb_trie_root_batch(uint8_t *roots32, uint8_t *status, const uint8_t *keys, const uint64_t *key_off,
                                   const uint8_t *values, const uint64_t *val_off, const uint64_t *trie_off, size_t B,
                                   int keys_hashed) {
    const char *what = "trie root";
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!B) return 0;
    if (B > MAX_ITEMS || !roots32 || !status || !trie_off) { fail(what, "roots32, status and trie_off are required"); return -1; }
    for (size_t b = 0; b < B; b++)
        if (trie_off[b + 1] < trie_off[b]) { fail(what, "trie offsets must not decrease"); return -1; }
    if (trie_off[0] != 0) { fail(what, "trie_off must start at 0"); return -1; }
    const size_t n = (size_t)trie_off[B];
    if (!root_args_ok(roots32, status, keys, key_off, values, val_off, trie_off, B, n)) return -1;
    for (size_t i = 0; i < n; i++) {
        if (key_off[i + 1] < key_off[i] || val_off[i + 1] < val_off[i]) { fail(what, "offsets must not decrease"); return -1; }
        if (key_off[i + 1] - key_off[i] > MAX_ITEMS || val_off[i + 1] - val_off[i] > MAX_ITEMS) {
            fail(what, "an item of 2^31 bytes or more");
            return -1;
        }
        if (keys_hashed && key_off[i + 1] - key_off[i] != 32) { fail(what, "a key hash is 32 bytes"); return -1; }
    }
    std::vector<uint64_t> krel, vrel;
    if (!rebase(krel, key_off, n, "trie root: offsets must not decrease") ||
        !rebase(vrel, val_off, n, "trie root: offsets must not decrease"))
        return -1;
    HostCall h(c, what);
    const uint8_t *dk = h.in(n ? keys + key_off[0] : keys, (size_t)krel[n]);
    const uint8_t *dv = h.in(n ? values + val_off[0] : values, (size_t)vrel[n]);
    const uint64_t *dko = h.in(krel.data(), n + 1);
    const uint64_t *dvo = h.in(vrel.data(), n + 1);
    uint8_t *dout = h.out<uint8_t>(33 * B);
    const uint64_t *dto = h.in(trie_off, B + 1);
    if (!h.ok()) return -1;
    if (root_enqueue(c, h.s, dout, dout + 32 * B, dk, dko, dv, dvo, dto, B, n, keys_hashed)) return -1;
    h.back(roots32, dout, 32 * B);
    h.back(status, dout + 32 * B, B);
    return h.finish();
}
