// lachain_amd/csrc/lcb_rbc.cpp — host side of the reliable broadcast's Merkle layer, the block transaction root
// (include/lachain_bls.h "reliable broadcast: Merkle layer") and, at the end, the single-instance
// Reed-Solomon encode / decode (lcb_rs_*) on the same k_rs.hip kernels.
//
// Reference calls: ReliableBroadcast.HandleInputMessage -> AugmentInput + ConstructValMessages (ReliableBroadcast.cs:
// 116, 311-338), CheckEchoMessage (:173, :296-309), TrySendReadyMessageFromEchos (:201-234: DecodeFromEchos, rebuild the
// tree, compare the root), MerkleTree.ComputeRoot (MerkleTree.cs:183-191; BlockManager.cs:692).  Each entry point is a
// handful of launches over the whole batch (k_rbc.hip, k_rs.hip); the host only checks arguments, lays out offsets and
// moves bytes.  No CPU fallback: every hash and every code symbol is computed on the device.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>

#include "launch.h"
#include "lcb_internal.hpp"
#include "../../include/lachain_bls.h"

using namespace lcb_int;

namespace {

const size_t MAX_BATCH = 65535;          // instances per call: the grid's y dimension
const size_t MAX_ITEMS = 0x7fffffffu;

bool shards_ok(int n, const char *what) {
    if (n < 1 || n > 256) { set_err(what); return false; }
    return true;
}
int depth_of(int n) {
    int d = 0;
    while ((1 << d) < n) d++;
    return d;
}
void rs_matrix_lds() {
    static bool attr = false;
    if (attr) return;
    (void)hipFuncSetAttribute(lcbk_rs_matrix_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, 65536 * 2);
    (void)hipFuncSetAttribute(lcbk_rs_matrix_batch_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, 65536 * 2);
    attr = true;
}

}  // namespace

// ------------------------------------------------------------------ sizes (host arithmetic, no device)
extern "C" size_t lcb_rbc_shard_size(size_t payload_len, int n, int f) {
    if (n < 1 || n > 256 || f < 0 || n - 2 * f <= 0 || payload_len > 0x7fffffffu - 4) {
        set_err("rbc shard size: need 1 <= n <= 256, 0 <= 2f < n and a payload below 2^31 - 4 bytes");
        return 0;
    }
    size_t k = (size_t)(n - 2 * f);
    return (payload_len + 4 + k - 1) / k;
}
extern "C" int lcb_rbc_tree_depth(int n) {
    if (!shards_ok(n, "rbc tree depth: need 1 <= n <= 256")) return -1;
    return depth_of(n);
}

// ------------------------------------------------------------------ ConstructValMessages
extern "C" int lcb_rbc_val_batch(uint8_t *shards_out, uint8_t *roots_out, uint8_t *proofs_out, const uint8_t *payloads,
                                 const uint64_t *payload_off, size_t B, int n, int f) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (n < 1 || n > 256 || f < 0 || n - 2 * f <= 0) { set_err("rbc val: need 1 <= n <= 256 and 0 <= 2f < n"); return -1; }
    if (!B) return 0;
    if (B > MAX_BATCH) { set_err("rbc val: at most 65535 instances per call"); return -1; }
    std::vector<uint64_t> poff, soff(B + 1);
    if (!rebase(poff, payload_off, B, "rbc val: offsets must not decrease")) return -1;
    const int k = n - 2 * f, m = 2 * f, depth = depth_of(n);
    size_t max_S = 0;
    soff[0] = 0;
    for (size_t b = 0; b < B; b++) {
        uint64_t len = payload_off[b + 1] - payload_off[b];
        if (len > 0x7fffffffu - 4) { set_err("rbc val: payload too long for the int32 length prefix"); return -1; }
        size_t S = (size_t)((len + 4 + k - 1) / k);
        max_S = S > max_S ? S : max_S;
        soff[b + 1] = soff[b] + (uint64_t)n * S;
    }
    HostCall h(c, "rbc val");
    hipStream_t s = h.s;
    const uint8_t *dpay = h.in(payloads + payload_off[0], (size_t)poff[B]);
    const uint64_t *dpoff = h.in(poff.data(), B + 1);
    const uint64_t *dsoff = h.in(soff.data(), B + 1);
    uint8_t *dsh = h.out<uint8_t>((size_t)soff[B]);
    int *dpos = h.out<int>((size_t)n);
    uint8_t *dM = h.out<uint8_t>((size_t)m * k + 16);
    uint8_t *droots = h.out<uint8_t>(32 * B);
    uint8_t *dproofs = h.out<uint8_t>(32 * B * n * (size_t)depth);
    if (!h.ok()) return -1;
    lcbk_rbc_augment(s, dpay, dpoff, dsh, dsoff, n, k, max_S * k, (unsigned)B);
    uint8_t *dok = dM + (size_t)m * k;
    uint8_t ok = 1;
    if (m) {
        rs_matrix_lds();
        std::vector<int> pos(n);
        for (int j = 0; j < m; j++) pos[j] = k + j;          // unknown: the parity positions
        for (int j = 0; j < k; j++) pos[m + j] = j;
        hipMemcpyAsync(dpos, pos.data(), 4 * (size_t)n, hipMemcpyHostToDevice, s);
        lcbk_rs_matrix(s, dpos, m, dpos + m, k, n, dM, dok);
        lcbk_rs_apply_batch(s, dM, 0, dok, 0, m, k, n, dsh, dsoff, dpos, 0, dsh, dsoff, 0, max_S, (unsigned)B);
        hipMemcpyAsync(&ok, dok, 1, hipMemcpyDeviceToHost, s);
    }
    lcbk_rbc_tree(s, dsh, dsoff, n, depth, nullptr, droots, depth ? dproofs : nullptr, (unsigned)B);
    if (!launch_ok("rbc val launch")) return -1;
    h.back(shards_out, dsh, (size_t)soff[B]);
    h.back(roots_out, droots, 32 * B);
    h.back(proofs_out, dproofs, 32 * B * n * (size_t)depth);
    if (h.finish()) return -1;
    if (!ok) { set_err("rbc val: parity positions are not independent"); return -1; }
    return 0;
}

// ------------------------------------------------------------------ CheckEchoMessage
extern "C" int lcb_ctx_rbc_check_echo_dev(lcb_ctx *ctx, uint8_t *accept, const uint8_t *data, const uint64_t *data_off,
                                          const int32_t *from, const uint8_t *roots, const uint8_t *proofs,
                                          const uint64_t *proof_off, size_t n_items, int n_shards, void *stream) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    if (!shards_ok(n_shards, "rbc check echo: need 1 <= n_shards <= 256")) return -1;
    if (n_items > MAX_ITEMS) { set_err("rbc check echo: batch too large"); return -1; }
    Enq q(c, (hipStream_t)stream);
    if (!n_items) return 0;
    lcbk_rbc_echo(q.s, accept, data, data_off, from, roots, proofs, proof_off, (u32)n_items, n_shards);
    return launch_ok("rbc check echo launch") ? 0 : -1;
}
extern "C" int lcb_rbc_check_echo_dev(uint8_t *accept, const uint8_t *data, const uint64_t *data_off, const int32_t *from,
                                      const uint8_t *roots, const uint8_t *proofs, const uint64_t *proof_off,
                                      size_t n_items, int n_shards, void *stream) {
    return lcb_ctx_rbc_check_echo_dev(nullptr, accept, data, data_off, from, roots, proofs, proof_off, n_items, n_shards,
                                      stream);
}
extern "C" int lcb_rbc_check_echo_batch(uint8_t *accept, const uint8_t *data, const uint64_t *data_off, const int32_t *from,
                                        const uint8_t *roots, const uint8_t *proofs, const uint64_t *proof_off,
                                        size_t n_items, int n_shards) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!shards_ok(n_shards, "rbc check echo: need 1 <= n_shards <= 256")) return -1;
    if (!n_items) return 0;
    if (n_items > MAX_ITEMS) { set_err("rbc check echo: batch too large"); return -1; }
    std::vector<uint64_t> doff, poff;
    if (!rebase(doff, data_off, n_items, "rbc check echo: data offsets must not decrease") ||
        !rebase(poff, proof_off, n_items, "rbc check echo: proof offsets must not decrease"))
        return -1;
    HostCall h(c, "rbc check echo");
    const uint8_t *dd = h.in(data + data_off[0], (size_t)doff[n_items]);
    const uint64_t *ddoff = h.in(doff.data(), n_items + 1);
    const uint64_t *dpoff = h.in(poff.data(), n_items + 1);
    const int32_t *dfrom = h.in(from, n_items);
    const uint8_t *dpr = h.in(proofs + 32 * proof_off[0], 32 * (size_t)poff[n_items]);
    const uint8_t *droots = h.in(roots, 32 * n_items);
    uint8_t *dacc = h.out<uint8_t>(n_items);
    if (!h.ok()) return -1;
    if (lcb_ctx_rbc_check_echo_dev(c, dacc, dd, ddoff, dfrom, droots, dpr, dpoff, n_items, n_shards, h.s)) return -1;
    h.back(accept, dacc, n_items);
    return h.finish();
}

// ------------------------------------------------------------------ ConstructMerkleTree
extern "C" int lcb_ctx_rbc_merkle_tree_dev(lcb_ctx *ctx, uint8_t *trees_out, const uint8_t *shards,
                                           const uint64_t *shard_off, size_t B, int n_shards, void *stream) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    if (!shards_ok(n_shards, "rbc merkle tree: need 1 <= n_shards <= 256")) return -1;
    if (B > MAX_ITEMS) { set_err("rbc merkle tree: batch too large"); return -1; }
    if (((uintptr_t)trees_out) & 7) { set_err("rbc merkle tree: trees_out must be 8-byte aligned"); return -1; }
    Enq q(c, (hipStream_t)stream);
    if (!B) return 0;
    lcbk_rbc_tree(q.s, shards, shard_off, n_shards, depth_of(n_shards), trees_out, nullptr, nullptr, (unsigned)B);
    return launch_ok("rbc merkle tree launch") ? 0 : -1;
}
extern "C" int lcb_rbc_merkle_tree_dev(uint8_t *trees_out, const uint8_t *shards, const uint64_t *shard_off, size_t B,
                                       int n_shards, void *stream) {
    return lcb_ctx_rbc_merkle_tree_dev(nullptr, trees_out, shards, shard_off, B, n_shards, stream);
}
extern "C" int lcb_rbc_merkle_tree_batch(uint8_t *trees_out, const uint8_t *shards, const uint64_t *shard_off, size_t B,
                                         int n_shards) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!shards_ok(n_shards, "rbc merkle tree: need 1 <= n_shards <= 256")) return -1;
    if (!B) return 0;
    if (B > MAX_ITEMS) { set_err("rbc merkle tree: batch too large"); return -1; }
    std::vector<uint64_t> off;
    if (!rebase(off, shard_off, B, "rbc merkle tree: offsets must not decrease")) return -1;
    for (size_t b = 0; b < B; b++)
        if ((off[b + 1] - off[b]) % (uint64_t)n_shards) {
            set_err("rbc merkle tree: an instance's bytes are not n_shards equal shards");
            return -1;
        }
    const size_t tree_bytes = 64 * ((size_t)1 << depth_of(n_shards));
    HostCall h(c, "rbc merkle tree");
    const uint8_t *dsh = h.in(shards + shard_off[0], (size_t)off[B]);
    const uint64_t *doff = h.in(off.data(), B + 1);
    uint8_t *dtrees = h.out<uint8_t>(tree_bytes * B);
    if (!h.ok()) return -1;
    if (lcb_ctx_rbc_merkle_tree_dev(c, dtrees, dsh, doff, B, n_shards, h.s)) return -1;
    h.back(trees_out, dtrees, tree_bytes * B);
    return h.finish();
}

// ------------------------------------------------------------------ TrySendReadyMessageFromEchos
extern "C" int lcb_rbc_decode_batch(uint8_t *shards_out, uint8_t *status, uint8_t *root_ok, uint8_t *roots_out,
                                    const uint8_t *echo_data, const uint64_t *echo_off, const int32_t *from,
                                    const uint8_t *expected_roots, size_t B, int n, int f) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (n < 1 || n > 256 || f < 0 || n - 2 * f <= 0) { set_err("rbc decode: need 1 <= n <= 256 and 0 <= 2f < n"); return -1; }
    if (!B) return 0;
    if (B > MAX_BATCH) { set_err("rbc decode: at most 65535 instances per call"); return -1; }
    if (!status) { set_err("rbc decode: status is required"); return -1; }
    std::vector<uint64_t> eoff, soff(B + 1);
    if (!rebase(eoff, echo_off, B, "rbc decode: offsets must not decrease")) return -1;
    const int k = n - 2 * f, m = 2 * f, depth = depth_of(n);
    size_t max_S = 0;
    soff[0] = 0;
    for (size_t b = 0; b < B; b++) {
        uint64_t bytes = eoff[b + 1] - eoff[b];
        if (bytes % (uint64_t)k) { set_err("rbc decode: an instance's bytes are not n - 2f equal echoes"); return -1; }
        size_t S = (size_t)(bytes / k);
        max_S = S > max_S ? S : max_S;
        soff[b + 1] = soff[b] + (uint64_t)n * S;
    }
    // per instance: the erased positions, then the echoes' positions in echo order; an instance with a bad or duplicate
    // index gets the identity (its output is zeroed through valid[b] = 0)
    std::vector<int> pos(B * (size_t)n);
    std::vector<uint8_t> valid(B, 1), have(n);
    for (size_t b = 0; b < B; b++) {
        int *p = &pos[b * (size_t)n];
        memset(have.data(), 0, n);
        for (int e = 0; e < k && valid[b]; e++) {
            int32_t j = from[b * (size_t)k + e];
            if (j < 0 || j >= n || have[j]) valid[b] = 0;
            else { have[j] = 1; p[m + e] = j; }
        }
        if (valid[b]) {
            int w = 0;
            for (int j = 0; j < n; j++) if (!have[j]) p[w++] = j;
        } else {
            for (int j = 0; j < n; j++) p[j] = j;
        }
    }
    HostCall h(c, "rbc decode");
    hipStream_t s = h.s;
    rs_matrix_lds();
    const uint8_t *decho = h.in(echo_data + echo_off[0], (size_t)eoff[B]);
    const uint64_t *deoff = h.in(eoff.data(), B + 1);
    const uint64_t *dsoff = h.in(soff.data(), B + 1);
    uint8_t *dsh = h.out<uint8_t>((size_t)soff[B]);
    const int *dpos = h.in(pos.data(), pos.size());
    uint8_t *dM = h.out<uint8_t>(B * (size_t)m * k + B);
    const uint8_t *dvalid = h.in(valid.data(), B);
    uint8_t *droots = h.out<uint8_t>(32 * B);
    if (!h.ok()) return -1;
    uint8_t *dok = dM + B * (size_t)m * k;
    lcbk_rs_matrix_batch(s, dpos, m, k, n, dvalid, dM, dok, (unsigned)B);
    lcbk_rs_apply_batch(s, dM, (size_t)m * k, dok, 1, m, k, n, decho, deoff, dpos, (size_t)n, dsh, dsoff, k, max_S,
                        (unsigned)B);
    lcbk_rbc_tree(s, dsh, dsoff, n, depth, nullptr, droots, nullptr, (unsigned)B);
    if (!launch_ok("rbc decode launch")) return -1;
    std::vector<uint8_t> roots(32 * B);
    h.back(shards_out, dsh, (size_t)soff[B]);
    h.back(status, dok, B);
    h.back(roots.data(), droots, 32 * B);
    if (h.finish()) return -1;
    for (size_t b = 0; b < B; b++) {
        status[b] = status[b] ? 1 : 0;
        if (!status[b]) memset(&roots[32 * b], 0, 32);
        if (root_ok) root_ok[b] = status[b] && expected_roots && !memcmp(&roots[32 * b], expected_roots + 32 * b, 32);
    }
    if (roots_out) memcpy(roots_out, roots.data(), 32 * B);
    return 0;
}

// ------------------------------------------------------------------ MerkleTree.ComputeRoot
extern "C" int lcb_ctx_merkle_root_dev(lcb_ctx *ctx, uint8_t *roots_out, uint8_t *status, const uint8_t *hashes,
                                       const uint64_t *off, size_t n_trees, size_t n_hashes, void *stream) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    if (n_trees > MAX_ITEMS) { set_err("merkle root: batch too large"); return -1; }
    Enq q(c, (hipStream_t)stream);
    if (!n_trees) return 0;
    uint8_t *ws = (uint8_t *)c->merkle_ws.get(32 * n_hashes);
    if (!ws) { set_err("device allocation failed"); return -1; }
    lcbk_merkle_root(q.s, roots_out, status, hashes, off, ws, (unsigned)n_trees);
    return launch_ok("merkle root launch") ? 0 : -1;
}
extern "C" int lcb_merkle_root_dev(uint8_t *roots_out, uint8_t *status, const uint8_t *hashes, const uint64_t *off,
                                   size_t n_trees, size_t n_hashes, void *stream) {
    return lcb_ctx_merkle_root_dev(nullptr, roots_out, status, hashes, off, n_trees, n_hashes, stream);
}
extern "C" int lcb_merkle_root_batch(uint8_t *roots_out, uint8_t *status, const uint8_t *hashes, const uint64_t *off,
                                     size_t n_trees) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!n_trees) return 0;
    if (n_trees > MAX_ITEMS) { set_err("merkle root: batch too large"); return -1; }
    std::vector<uint64_t> rel;
    if (!rebase(rel, off, n_trees, "merkle root: offsets must not decrease")) return -1;
    HostCall h(c, "merkle root");
    const uint8_t *dh = h.in(hashes + 32 * off[0], 32 * (size_t)rel[n_trees]);
    const uint64_t *doff = h.in(rel.data(), n_trees + 1);
    uint8_t *droots = h.out<uint8_t>(32 * n_trees), *dst = h.out<uint8_t>(n_trees);
    if (!h.ok()) return -1;
    if (lcb_ctx_merkle_root_dev(c, droots, dst, dh, doff, n_trees, (size_t)rel[n_trees], h.s)) return -1;
    h.back(roots_out, droots, 32 * n_trees);
    h.back(status, dst, n_trees);
    return h.finish();
}

// ================================================================== reliable-broadcast Reed-Solomon (k_rs.hip)
// ReliableBroadcast.ErasureCodingShards / DecodeFromEchos (src/Lachain.Consensus/ReliableBroadcast/ReliableBroadcast.cs:
// 393-446): the erased / parity shards are M times the known shards, M = H_E^-1 H_K built on the GPU.  Positions,
// matrix and shards are staging of the one call.
namespace {
int rs_enqueue(HostCall &h, uint8_t *d_out, const uint8_t *d_known, const std::vector<int> &pe,
               const std::vector<int> &pk, int n, size_t S, uint8_t **d_ok) {
    rs_matrix_lds();
    hipStream_t s = h.s;
    int m = (int)pe.size(), k = (int)pk.size();
    std::vector<int> both(pe);
    both.insert(both.end(), pk.begin(), pk.end());
    const int *dpe = h.in(both.data(), both.size());
    uint8_t *M = h.out<uint8_t>((size_t)m * k + 16);
    if (!h.ok()) return -1;
    uint8_t *ok = M + (size_t)m * k;
    lcbk_rs_matrix(s, dpe, m, dpe + m, k, n, M, ok);
    lcbk_rs_apply(s, M, ok, m, k, d_known, S, dpe, d_out);
    *d_ok = ok;
    return launch_ok("rs launch") ? 0 : -1;
}
}  // namespace
extern "C" int lcb_rs_encode(uint8_t *shards_out, const uint8_t *input, size_t input_len, int n_shards, int erasures) {
    SYNC_CTX_OR(c, -1)
    int k = n_shards - erasures;
    if (n_shards <= 0 || erasures < 0 || k <= 0 || input_len % (size_t)k) {
        set_err("rs encode: need 0 <= erasures < shards and input length divisible by the data shards");
        return -1;
    }
    size_t S = input_len / (size_t)k;
    if (erasures == 0 || S == 0) { memcpy(shards_out, input, input_len); return 0; }
    HostCall h(c, "rs encode");
    hipStream_t s = h.s;
    uint8_t *dout = h.out<uint8_t>(S * n_shards);
    if (!h.ok()) return -1;
    hipMemcpyAsync(dout, input, input_len, hipMemcpyHostToDevice, s);   // data shards stay in place (systematic)
    std::vector<int> pe, pk;
    for (int j = k; j < n_shards; j++) pe.push_back(j);
    for (int j = 0; j < k; j++) pk.push_back(j);
    uint8_t *dok;
    if (rs_enqueue(h, dout, dout, pe, pk, n_shards, S, &dok)) return -1;
    uint8_t ok = 0;
    h.back(shards_out, dout, S * n_shards);
    h.back(&ok, dok, 1);
    if (h.finish()) return -1;
    if (!ok) { set_err("rs encode: parity positions are not independent (more than 255 shards)"); return -1; }
    return 0;
}
extern "C" int lcb_rs_decode(uint8_t *out, const uint8_t *echo_data, const int32_t *from, int n_echos, size_t shard_size,
                             int n_shards, int erasures) {
    SYNC_CTX_OR(c, -1)
    int k = n_shards - erasures;
    if (n_shards <= 0 || erasures < 0 || k <= 0 || n_echos != k) {
        set_err("rs decode: need exactly shards - erasures echoes (DecodeFromEchos asserts N - 2F)");
        return -1;
    }
    std::vector<char> have(n_shards, 0);
    std::vector<int> pe, pk;
    for (int e = 0; e < n_echos; e++) {
        if (from[e] < 0 || from[e] >= n_shards || have[from[e]]) { set_err("rs decode: bad or duplicate echo index"); return -1; }
        have[from[e]] = 1;
        pk.push_back(from[e]);
    }
    for (int j = 0; j < n_shards; j++) if (!have[j]) pe.push_back(j);
    size_t S = shard_size;
    if (S == 0) return 0;
    HostCall h(c, "rs decode");
    hipStream_t s = h.s;
    uint8_t *dout = h.out<uint8_t>(S * n_shards);
    const uint8_t *decho = h.in(echo_data, S * (size_t)n_echos);
    if (!h.ok()) return -1;
    for (int e = 0; e < n_echos; e++)
        hipMemcpyAsync(dout + (size_t)from[e] * S, decho + (size_t)e * S, S, hipMemcpyDeviceToDevice, s);
    uint8_t ok = 1;
    if (!pe.empty()) {
        uint8_t *dok;
        if (rs_enqueue(h, dout, decho, pe, pk, n_shards, S, &dok)) return -1;
        h.back(&ok, dok, 1);
    }
    h.back(out, dout, S * n_shards);
    if (h.finish()) return -1;
    if (!ok) { set_err("rs decode: erased positions share an evaluation point (more than 255 shards)"); return -1; }
    return 0;
}
