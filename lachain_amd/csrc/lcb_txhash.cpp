// lachain_amd/csrc/lcb_txhash.cpp — host side of the device transaction hashing and receipt verification
// (include/lachain_bls.h "transaction hashing and receipt verification").
//
// Reference calls: TransactionUtils.RawHash / FullHash (TransactionUtils.cs:92-105), TransactionVerifier.
// VerifyTransactionImmediately(receipt, useNewChainId, cacheEnabled: false) (TransactionVerifier.cs:109-143) and the
// block's transaction root (BlockManager.cs:690-694).  A receipts call is k_tx_hash (k_txhash.hip), the recovery chain
// of lcb_ecdsa.cpp on the raw hashes it left on the device, and k_tx_detail; a blocks call adds k_merkle_root and
// k_tx_root_ok.  The host only checks arguments and moves bytes.  No CPU fallback: every hash is computed on the device.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "launch.h"
#include "lcb_internal.hpp"
#include "../../include/lachain_bls.h"

using namespace lcb_int;

static_assert(sizeof(lcb_tx_fields) == 104, "lcb_tx_fields is the 104-byte record k_tx_hash reads");

namespace {

const size_t MAX_ITEMS = 0x7fffffffu;
const uint64_t MAX_INVOCATION = 0x7fffffffu;     // an item of 2^31 bytes or more fails the call

bool events_ready(lcb_ctx *c) {
    if (c->tx_ev_ready) return true;
    for (auto &e : c->tx_ev)
        if (hipEventCreate(&e) != hipSuccess) { set_err("event creation"); return false; }
    c->tx_ev_ready = true;
    return true;
}
// what every form checks: the signature width goes with the chain id's kind (DefaultCrypto.cs:26-29)
bool common_ok(size_t n, const void *txs, const void *inv, const void *off, size_t sig_len, bool sigs_given,
               int use_new_chain_id, int32_t chain_id, const char *what) {
    static thread_local char msg[160];
    const char *why = nullptr;
    if (n > MAX_ITEMS) why = "batch too large";
    else if (chain_id < 0) why = "the chain id must not be negative";
    else if (n && (!txs || !inv || !off)) why = "txs, invocations and inv_off are required";
    else if (sigs_given && sig_len != (use_new_chain_id ? 66u : 65u)) why = "sig_len must be 65 (old chain id) or 66 (new)";
    if (!why) return true;
    snprintf(msg, sizeof msg, "%s: %s", what, why);
    set_err(msg);
    return false;
}
// the host-pointer forms also read what the device forms must trust: offsets and To lengths
bool host_items_ok(const lcb_tx_fields *txs, const uint64_t *off, size_t n, const char *what) {
    static thread_local char msg[160];
    const char *why = nullptr;
    for (size_t i = 0; i < n && !why; i++) {
        if (off[i + 1] < off[i]) why = "offsets must not decrease";
        else if (off[i + 1] - off[i] > MAX_INVOCATION) why = "an invocation of 2^31 bytes or more";
        else if (txs[i].to_len != 0 && txs[i].to_len != 20) why = "to_len must be 0 or 20";
    }
    if (!why) return true;
    snprintf(msg, sizeof msg, "%s: %s", what, why);
    set_err(msg);
    return false;
}

// hashing alone, device pointers; the events of a later phase collapse onto the hashing's end
int hash_enqueue(lcb_ctx *c, hipStream_t s, uint8_t *raw32, uint8_t *full32, uint8_t *match, const uint8_t *txs,
                 const uint8_t *inv, const uint64_t *off, const uint8_t *sigs, size_t sig_len, const uint8_t *claimed,
                 size_t n, int32_t chain_id, bool last_phase) {
    if (((uintptr_t)txs | (uintptr_t)off) & 7) { set_err("tx hash: txs and inv_off must be 8-byte aligned"); return -1; }
    if (!events_ready(c)) return -1;
    uint32_t *long_ws = (uint32_t *)c->tx[TX_LONG].get(4 * (n + 1));    // k_tx_hash's list of long items
    if (!long_ws) { set_err("device allocation failed"); return -1; }
    (void)hipEventRecord(c->tx_ev[0], s);
    lcbk_tx_hash(s, txs, inv, off, sigs, (u32)sig_len, claimed, (u32)chain_id, (u32)n, raw32, full32, match, long_ws);
    (void)hipEventRecord(c->tx_ev[1], s);
    if (last_phase) {
        (void)hipEventRecord(c->tx_ev[2], s);
        (void)hipEventRecord(c->tx_ev[3], s);
    }
    c->tx_ran = true;
    return launch_ok("tx hash launch") ? 0 : -1;
}

// VerifyTransactionImmediately over n receipts and, with n_blocks, the blocks' roots; device pointers
int receipts_enqueue(lcb_ctx *c, hipStream_t s, uint8_t *accept, uint8_t *detail, uint8_t *root_ok, const uint8_t *txs,
                     const uint8_t *inv, const uint64_t *off, const uint8_t *sigs, size_t sig_len, const uint8_t *claimed,
                     size_t n, const uint64_t *tx_off, const uint8_t *expected_roots, size_t n_blocks,
                     int use_new_chain_id, int32_t chain_id) {
    if (n) {
        uint8_t *raw = (uint8_t *)c->tx[TX_RAW].get(32 * n), *flags = (uint8_t *)c->tx[TX_FLAGS].get(2 * n);
        uint8_t *addr = (uint8_t *)c->tx[TX_ADDR].get(20 * n);
        if (!raw || !flags || !addr) { set_err("device allocation failed"); return -1; }
        uint8_t *match = flags, *rec_ok = flags + n;
        if (hash_enqueue(c, s, raw, nullptr, match, txs, inv, off, sigs, sig_len, claimed, n, chain_id, false)) return -1;
        if (lcb_ctx_ecdsa_recover_hashed_dev(c, nullptr, addr, rec_ok, raw, sigs, sig_len, n, use_new_chain_id, chain_id, s))
            return -1;
        lcbk_tx_detail(s, match, rec_ok, addr, txs, (u32)n, accept, detail);
    } else {
        if (!events_ready(c)) return -1;
        (void)hipEventRecord(c->tx_ev[0], s);
        (void)hipEventRecord(c->tx_ev[1], s);
        c->tx_ran = true;
    }
    (void)hipEventRecord(c->tx_ev[2], s);
    if (n_blocks) {
        uint8_t *roots = (uint8_t *)c->tx[TX_ROOTS].get(33 * n_blocks);
        if (!roots) { set_err("device allocation failed"); return -1; }
        if (lcb_ctx_merkle_root_dev(c, roots, roots + 32 * n_blocks, claimed, tx_off, n_blocks, n, s)) return -1;
        lcbk_tx_root_ok(s, roots, expected_roots, (u32)n_blocks, root_ok);
    }
    (void)hipEventRecord(c->tx_ev[3], s);
    return launch_ok("receipts verify launch") ? 0 : -1;
}

int receipts_dev(lcb_ctx *ctx, uint8_t *accept, uint8_t *detail, uint8_t *root_ok, const lcb_tx_fields *txs,
                 const uint8_t *inv, const uint64_t *off, const uint8_t *sigs, size_t sig_len, const uint8_t *claimed,
                 size_t n, const uint64_t *tx_off, const uint8_t *expected_roots, size_t n_blocks, bool blocks,
                 int use_new_chain_id, int32_t chain_id, void *stream) {
    const char *what = blocks ? "block txs verify" : "receipts verify";
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    if (!common_ok(n, txs, inv, off, sig_len, true, use_new_chain_id, chain_id, what)) return -1;
    if (n && (!accept || !sigs || !claimed)) { set_err("receipts verify: accept, sigs and hashes32 are required"); return -1; }
    if (blocks && (n_blocks > MAX_ITEMS || (n_blocks && (!tx_off || !expected_roots || !root_ok)))) {
        set_err("block txs verify: tx_off, expected_roots and root_ok are required (at most 2^31 - 1 blocks)");
        return -1;
    }
    Enq q(c, (hipStream_t)stream);
    return receipts_enqueue(c, q.s, accept, detail, root_ok, (const uint8_t *)txs, inv, off, sigs, sig_len, claimed, n,
                            tx_off, expected_roots, blocks ? n_blocks : 0, use_new_chain_id, chain_id);
}

int receipts_host(uint8_t *accept, uint8_t *detail, uint8_t *root_ok, const lcb_tx_fields *txs, const uint8_t *inv,
                  const uint64_t *off, const uint8_t *sigs, size_t sig_len, const uint8_t *claimed, size_t n,
                  const uint64_t *tx_off, const uint8_t *expected_roots, size_t n_blocks, bool blocks,
                  int use_new_chain_id, int32_t chain_id) {
    const char *what = blocks ? "block txs verify" : "receipts verify";
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!common_ok(n, txs, inv, off, sig_len, true, use_new_chain_id, chain_id, what)) return -1;
    if (n && (!accept || !sigs || !claimed)) { set_err("receipts verify: accept, sigs and hashes32 are required"); return -1; }
    if (!host_items_ok(txs, off, n, what)) return -1;
    if (!blocks) n_blocks = 0;
    if (n_blocks) {
        if (n_blocks > MAX_ITEMS || !tx_off || !expected_roots || !root_ok) {
            set_err("block txs verify: tx_off, expected_roots and root_ok are required (at most 2^31 - 1 blocks)");
            return -1;
        }
        for (size_t b = 0; b < n_blocks; b++)
            if (tx_off[b + 1] < tx_off[b]) { set_err("block txs verify: block offsets must not decrease"); return -1; }
        if (tx_off[0] != 0 || tx_off[n_blocks] != n) {
            set_err("block txs verify: tx_off must run from 0 to n");
            return -1;
        }
    }
    if (!n && !n_blocks) return 0;
    std::vector<uint64_t> rel;
    if (!rebase(rel, off, n, "receipts verify: offsets must not decrease")) return -1;
    HostCall h(c, what);
    const lcb_tx_fields *dtx = h.in(txs, n);
    const uint8_t *dinv = h.in(n ? inv + off[0] : inv, (size_t)rel[n]);
    const uint64_t *doff = h.in(rel.data(), n + 1);
    const uint8_t *dsig = h.in(sigs, sig_len * n);
    const uint8_t *dclaim = h.in(claimed, 32 * n);
    uint8_t *dout = h.out<uint8_t>(2 * n + n_blocks);
    const uint64_t *dtoff = n_blocks ? h.in(tx_off, n_blocks + 1) : nullptr;
    const uint8_t *dexp = n_blocks ? h.in(expected_roots, 32 * n_blocks) : nullptr;
    if (!h.ok()) return -1;
    uint8_t *dacc = dout, *ddet = dout + n, *drok = dout + 2 * n;
    if (receipts_enqueue(c, h.s, dacc, ddet, drok, (const uint8_t *)dtx, dinv, doff, dsig, sig_len, dclaim, n, dtoff, dexp,
                         n_blocks, use_new_chain_id, chain_id))
        return -1;
    h.back(accept, dacc, n);
    h.back(detail, ddet, n);
    h.back(root_ok, drok, n_blocks);
    return h.finish();
}

}  // namespace

namespace lcb_int {
void txhash_ctx_release(lcb_ctx *c) {
    if (c->tx_ev_ready) for (auto &e : c->tx_ev) (void)hipEventDestroy(e);
    c->tx_ev_ready = false;
    for (auto &b : c->tx) b.release();
}
}  // namespace lcb_int

// ------------------------------------------------------------------ RawHash / FullHash
extern "C" int lcb_ctx_tx_hash_dev(lcb_ctx *ctx, uint8_t *raw32_out, uint8_t *full32_out, const lcb_tx_fields *txs,
                                   const uint8_t *invocations, const uint64_t *inv_off, const uint8_t *sigs,
                                   size_t sig_len, size_t n, int use_new_chain_id, int32_t chain_id, void *stream) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    if (!common_ok(n, txs, invocations, inv_off, sig_len, sigs != nullptr, use_new_chain_id, chain_id, "tx hash")) return -1;
    Enq q(c, (hipStream_t)stream);
    if (!n) return 0;
    return hash_enqueue(c, q.s, raw32_out, sigs ? full32_out : nullptr, nullptr, (const uint8_t *)txs, invocations, inv_off,
                        sigs, sig_len, nullptr, n, chain_id, true);
}
extern "C" int lcb_tx_hash_dev(uint8_t *raw32_out, uint8_t *full32_out, const lcb_tx_fields *txs, const uint8_t *invocations,
                               const uint64_t *inv_off, const uint8_t *sigs, size_t sig_len, size_t n,
                               int use_new_chain_id, int32_t chain_id, void *stream) {
    return lcb_ctx_tx_hash_dev(nullptr, raw32_out, full32_out, txs, invocations, inv_off, sigs, sig_len, n,
                               use_new_chain_id, chain_id, stream);
}
extern "C" int lcb_tx_hash_batch(uint8_t *raw32_out, uint8_t *full32_out, const lcb_tx_fields *txs,
                                 const uint8_t *invocations, const uint64_t *inv_off, const uint8_t *sigs, size_t sig_len,
                                 size_t n, int use_new_chain_id, int32_t chain_id) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!common_ok(n, txs, invocations, inv_off, sig_len, sigs != nullptr, use_new_chain_id, chain_id, "tx hash")) return -1;
    if (!n) return 0;
    if (!host_items_ok(txs, inv_off, n, "tx hash")) return -1;
    std::vector<uint64_t> rel;
    if (!rebase(rel, inv_off, n, "tx hash: offsets must not decrease")) return -1;
    HostCall h(c, "tx hash");
    const lcb_tx_fields *dtx = h.in(txs, n);
    const uint8_t *dinv = h.in(invocations + inv_off[0], (size_t)rel[n]);
    const uint64_t *doff = h.in(rel.data(), n + 1);
    const uint8_t *dsig = sigs ? h.in(sigs, sig_len * n) : nullptr;
    uint8_t *dout = h.out<uint8_t>(64 * n);
    if (!h.ok()) return -1;
    uint8_t *draw = raw32_out ? dout : nullptr, *dfull = sigs && full32_out ? dout + 32 * n : nullptr;
    if (hash_enqueue(c, h.s, draw, dfull, nullptr, (const uint8_t *)dtx, dinv, doff, dsig, sig_len, nullptr, n, chain_id, true))
        return -1;
    h.back(raw32_out, draw, 32 * n);
    h.back(full32_out, dfull, 32 * n);
    return h.finish();
}

// ------------------------------------------------------------------ VerifyTransactionImmediately
extern "C" int lcb_ctx_receipts_verify_dev(lcb_ctx *ctx, uint8_t *accept, uint8_t *detail, const lcb_tx_fields *txs,
                                           const uint8_t *invocations, const uint64_t *inv_off, const uint8_t *sigs,
                                           size_t sig_len, const uint8_t *hashes32, size_t n, int use_new_chain_id,
                                           int32_t chain_id, void *stream) {
    return receipts_dev(ctx, accept, detail, nullptr, txs, invocations, inv_off, sigs, sig_len, hashes32, n, nullptr,
                        nullptr, 0, false, use_new_chain_id, chain_id, stream);
}
extern "C" int lcb_receipts_verify_dev(uint8_t *accept, uint8_t *detail, const lcb_tx_fields *txs,
                                       const uint8_t *invocations, const uint64_t *inv_off, const uint8_t *sigs,
                                       size_t sig_len, const uint8_t *hashes32, size_t n, int use_new_chain_id,
                                       int32_t chain_id, void *stream) {
    return lcb_ctx_receipts_verify_dev(nullptr, accept, detail, txs, invocations, inv_off, sigs, sig_len, hashes32, n,
                                       use_new_chain_id, chain_id, stream);
}
extern "C" int lcb_receipts_verify_batch(uint8_t *accept, uint8_t *detail, const lcb_tx_fields *txs,
                                         const uint8_t *invocations, const uint64_t *inv_off, const uint8_t *sigs,
                                         size_t sig_len, const uint8_t *hashes32, size_t n, int use_new_chain_id,
                                         int32_t chain_id) {
    return receipts_host(accept, detail, nullptr, txs, invocations, inv_off, sigs, sig_len, hashes32, n, nullptr, nullptr,
                         0, false, use_new_chain_id, chain_id);
}

// ------------------------------------------------------------------ the same for B blocks, with their transaction roots
extern "C" int lcb_ctx_block_txs_verify_dev(lcb_ctx *ctx, uint8_t *accept, uint8_t *detail, uint8_t *root_ok,
                                            const lcb_tx_fields *txs, const uint8_t *invocations, const uint64_t *inv_off,
                                            const uint8_t *sigs, size_t sig_len, const uint8_t *hashes32, size_t n,
                                            const uint64_t *tx_off, const uint8_t *expected_roots, size_t n_blocks,
                                            int use_new_chain_id, int32_t chain_id, void *stream) {
    return receipts_dev(ctx, accept, detail, root_ok, txs, invocations, inv_off, sigs, sig_len, hashes32, n, tx_off,
                        expected_roots, n_blocks, true, use_new_chain_id, chain_id, stream);
}
extern "C" int lcb_block_txs_verify_dev(uint8_t *accept, uint8_t *detail, uint8_t *root_ok, const lcb_tx_fields *txs,
                                        const uint8_t *invocations, const uint64_t *inv_off, const uint8_t *sigs,
                                        size_t sig_len, const uint8_t *hashes32, size_t n, const uint64_t *tx_off,
                                        const uint8_t *expected_roots, size_t n_blocks, int use_new_chain_id,
                                        int32_t chain_id, void *stream) {
    return lcb_ctx_block_txs_verify_dev(nullptr, accept, detail, root_ok, txs, invocations, inv_off, sigs, sig_len,
                                        hashes32, n, tx_off, expected_roots, n_blocks, use_new_chain_id, chain_id, stream);
}
extern "C" int lcb_block_txs_verify_batch(uint8_t *accept, uint8_t *detail, uint8_t *root_ok, const lcb_tx_fields *txs,
                                          const uint8_t *invocations, const uint64_t *inv_off, const uint8_t *sigs,
                                          size_t sig_len, const uint8_t *hashes32, size_t n, const uint64_t *tx_off,
                                          const uint8_t *expected_roots, size_t n_blocks, int use_new_chain_id,
                                          int32_t chain_id) {
    return receipts_host(accept, detail, root_ok, txs, invocations, inv_off, sigs, sig_len, hashes32, n, tx_off,
                         expected_roots, n_blocks, true, use_new_chain_id, chain_id);
}

// kernel milliseconds of the context's last transaction call: hashing, recovery (with the decision), roots
extern "C" int lcb_ctx_tx_phase_ms(lcb_ctx *ctx, float ms[3]) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!c->tx_ran) { set_err("no transaction hashing has run in this context"); return -1; }
    for (int k = 0; k < 3; k++) {
        hipError_t e = hipEventSynchronize(c->tx_ev[k + 1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[k], c->tx_ev[k], c->tx_ev[k + 1]);
        if (e != hipSuccess) { set_err("tx phase timing", e); return -1; }
    }
    return 0;
}
extern "C" int lcb_tx_phase_ms(float ms[3]) { return lcb_ctx_tx_phase_ms(nullptr, ms); }
