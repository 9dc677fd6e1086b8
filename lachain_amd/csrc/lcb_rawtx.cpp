// lachain_amd/csrc/lcb_rawtx.cpp — host side of the raw-transaction ingress (include/lachain_bls.h "raw-transaction
// ingress").
//
// Reference calls: TransactionServiceWeb3.SendRawTransaction and its batch forms (TransactionServiceWeb3.cs:184-254)
// down to TransactionPool.Add's signature check (TransactionPool.cs:130-143).  A call is k_rawtx_decode with
// k_rawtx_long (k_rawtx.hip: decode, outputs, RawHash and FullHash), the recovery chain of lcb_ecdsa.cpp over the raw
// hashes and decoded signatures left on the device, and k_rawtx_finish.  The host only checks arguments and moves
// bytes; it never looks inside an item.  No CPU fallback: every item is decoded and hashed on the device.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "launch.h"
#include "lcb_internal.hpp"
#include "../../include/lachain_bls.h"

using namespace lcb_int;

namespace {

const size_t MAX_ITEMS = 0x7fffffffu;
const uint64_t MAX_ITEM_BYTES = 0x7fffffffu;     // the host form: an item of 2^31 bytes or more fails the call

bool events_ready(lcb_ctx *c) {
    if (c->rawtx_ev_ready) return true;
    for (auto &e : c->rawtx_ev)
        if (hipEventCreate(&e) != hipSuccess) { set_err("event creation"); return false; }
    c->rawtx_ev_ready = true;
    return true;
}
// what every form checks.  v = 2 chain_id + 35 or 36 must fit the signature's tail (sig_len - 64 bytes), or no item
// could pass the chain check
bool common_ok(size_t n, const void *status, const void *raw, const void *off, int use_new_chain_id, int32_t chain_id) {
    const char *why = nullptr;
    if (n > MAX_ITEMS) why = "raw txs ingest: batch too large";
    else if (!status) why = "raw txs ingest: status is required";
    else if (!raw || !off) why = "raw txs ingest: raw and raw_off are required";
    else if (chain_id <= 0) why = "raw txs ingest: the chain id must be positive";
    else if (2 * (int64_t)chain_id + 36 > (use_new_chain_id ? 0xffff : 0xff))
        why = "raw txs ingest: 2 * chain_id + 36 does not fit the signature's v (chain id <= 109 old, <= 32749 new)";
    if (why) set_err(why);
    return !why;
}

// device pointers; span_base: what the caller's raw lies behind the staged one (the host form's rebased offsets)
int ingest_enqueue(lcb_ctx *c, hipStream_t s, uint8_t *accept, uint8_t *status, uint8_t *detail, uint8_t *txs,
                   uint64_t *span, uint8_t *sigs, uint8_t *raw32, uint8_t *full32, const uint8_t *raw,
                   const uint64_t *off, uint64_t span_base, size_t n, int use_new_chain_id, int32_t chain_id) {
    if (((uintptr_t)txs | (uintptr_t)off | (uintptr_t)span) & 7) {
        set_err("raw txs ingest: txs_out, inv_span_out and raw_off must be 8-byte aligned");
        return -1;
    }
    if (!events_ready(c)) return -1;
    const size_t sig_len = use_new_chain_id ? 66 : 65;
    uint32_t *long_ws = (uint32_t *)c->rawtx[RAWTX_LONG_LIST].get(4 * (n + 1));
    uint8_t *rec_ok = nullptr, *addr = nullptr;
    bool good = long_ws != nullptr;
    if (accept) {                                  // the recovery reads raw hashes and signatures: the caller's, or ours
        if (!raw32) good = good && (raw32 = (uint8_t *)c->rawtx[RAWTX_HASH].get(32 * n));
        if (!sigs) good = good && (sigs = (uint8_t *)c->rawtx[RAWTX_SIGS].get(sig_len * n));
        if (!detail) good = good && (detail = (uint8_t *)c->rawtx[RAWTX_DETAIL].get(n));
        good = good && (rec_ok = (uint8_t *)c->rawtx[RAWTX_REC_OK].get(n));
        good = good && (addr = (uint8_t *)c->rawtx[RAWTX_ADDR].get(20 * n));
    }
    if (!good) { set_err("device allocation failed"); return -1; }
    (void)hipEventRecord(c->rawtx_ev[0], s);
    lcbk_rawtx_decode(s, raw, off, span_base, (u32)sig_len, (u32)chain_id, (u32)n, status, detail, txs, span, sigs, raw32,
                      full32, long_ws);
    (void)hipEventRecord(c->rawtx_ev[1], s);
    c->rawtx_ran = true;
    if (accept) {
        // refused items carry a zero signature and do not recover
        if (lcb_ctx_ecdsa_recover_hashed_dev(c, nullptr, addr, rec_ok, raw32, sigs, sig_len, n, use_new_chain_id, chain_id, s))
            return -1;
        (void)hipEventRecord(c->rawtx_ev[2], s);
        lcbk_rawtx_finish(s, status, rec_ok, addr, detail, (u32)n, accept, detail, txs);
    } else {
        (void)hipEventRecord(c->rawtx_ev[2], s);
    }
    (void)hipEventRecord(c->rawtx_ev[3], s);
    return launch_ok("raw txs ingest launch") ? 0 : -1;
}

}  // namespace

namespace lcb_int {
void rawtx_ctx_release(lcb_ctx *c) {
    if (c->rawtx_ev_ready) for (auto &e : c->rawtx_ev) (void)hipEventDestroy(e);
    c->rawtx_ev_ready = false;
    for (auto &b : c->rawtx) b.release();
}
}  // namespace lcb_int

extern "C" int lcb_ctx_raw_txs_ingest_dev(lcb_ctx *ctx, uint8_t *accept, uint8_t *status, uint8_t *detail,
                                          lcb_tx_fields *txs_out, uint64_t *inv_span_out, uint8_t *sigs_out,
                                          uint8_t *raw32_out, uint8_t *full32_out, const uint8_t *raw,
                                          const uint64_t *raw_off, size_t n, int use_new_chain_id, int32_t chain_id,
                                          void *stream) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    if (!common_ok(n, status, raw, raw_off, use_new_chain_id, chain_id)) return -1;
    Enq q(c, (hipStream_t)stream);
    if (!n) return 0;
    return ingest_enqueue(c, q.s, accept, status, detail, (uint8_t *)txs_out, inv_span_out, sigs_out, raw32_out, full32_out,
                          raw, raw_off, 0, n, use_new_chain_id, chain_id);
}
extern "C" int lcb_raw_txs_ingest_dev(uint8_t *accept, uint8_t *status, uint8_t *detail, lcb_tx_fields *txs_out,
                                      uint64_t *inv_span_out, uint8_t *sigs_out, uint8_t *raw32_out, uint8_t *full32_out,
                                      const uint8_t *raw, const uint64_t *raw_off, size_t n, int use_new_chain_id,
                                      int32_t chain_id, void *stream) {
    return lcb_ctx_raw_txs_ingest_dev(nullptr, accept, status, detail, txs_out, inv_span_out, sigs_out, raw32_out,
                                      full32_out, raw, raw_off, n, use_new_chain_id, chain_id, stream);
}
extern "C" int lcb_raw_txs_ingest_batch(uint8_t *accept, uint8_t *status, uint8_t *detail, lcb_tx_fields *txs_out,
                                        uint64_t *inv_span_out, uint8_t *sigs_out, uint8_t *raw32_out, uint8_t *full32_out,
                                        const uint8_t *raw, const uint64_t *raw_off, size_t n, int use_new_chain_id,
                                        int32_t chain_id) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!common_ok(n, status, raw, raw_off, use_new_chain_id, chain_id)) return -1;
    if (!n) return 0;
    for (size_t i = 0; i < n; i++) {
        if (raw_off[i + 1] < raw_off[i]) { set_err("raw txs ingest: offsets must not decrease"); return -1; }
        if (raw_off[i + 1] - raw_off[i] > MAX_ITEM_BYTES) { set_err("raw txs ingest: an item of 2^31 bytes or more"); return -1; }
    }
    std::vector<uint64_t> rel;
    if (!rebase(rel, raw_off, n, "raw txs ingest: offsets must not decrease")) return -1;
    const size_t sig_len = use_new_chain_id ? 66 : 65;
    HostCall h(c, "raw txs ingest");
    const uint8_t *draw = h.in(raw + raw_off[0], (size_t)rel[n]);
    const uint64_t *doff = h.in(rel.data(), n + 1);
    uint8_t *dflags = h.out<uint8_t>(3 * n);       // status, accept, detail
    uint8_t *dtx = txs_out ? h.out<uint8_t>(sizeof(lcb_tx_fields) * n) : nullptr;
    uint64_t *dspan = inv_span_out ? h.out<uint64_t>(2 * n) : nullptr;
    uint8_t *dsig = sigs_out ? h.out<uint8_t>(sig_len * n) : nullptr;
    uint8_t *dhash = raw32_out || full32_out ? h.out<uint8_t>(64 * n) : nullptr;
    if (!h.ok()) return -1;
    uint8_t *dst = dflags, *dacc = accept ? dflags + n : nullptr, *ddet = detail ? dflags + 2 * n : nullptr;
    uint8_t *dr = raw32_out ? dhash : nullptr, *df = full32_out ? dhash + 32 * n : nullptr;
    if (ingest_enqueue(c, h.s, dacc, dst, ddet, dtx, dspan, dsig, dr, df, draw, doff, raw_off[0], n, use_new_chain_id,
                       chain_id))
        return -1;
    h.back(status, dst, n);
    h.back(accept, dacc, n);
    h.back(detail, ddet, n);
    h.back(txs_out, dtx, sizeof(lcb_tx_fields) * n);
    h.back(inv_span_out, dspan, 16 * n);
    h.back(sigs_out, dsig, sig_len * n);
    h.back(raw32_out, dr, 32 * n);
    h.back(full32_out, df, 32 * n);
    return h.finish();
}

// kernel milliseconds of the context's last ingress: decode and hashing, recovery, finish
extern "C" int lcb_ctx_rawtx_phase_ms(lcb_ctx *ctx, float ms[3]) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!c->rawtx_ran) { set_err("no raw-transaction ingress has run in this context"); return -1; }
    for (int k = 0; k < 3; k++) {
        hipError_t e = hipEventSynchronize(c->rawtx_ev[k + 1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[k], c->rawtx_ev[k], c->rawtx_ev[k + 1]);
        if (e != hipSuccess) { set_err("rawtx phase timing", e); return -1; }
    }
    return 0;
}
extern "C" int lcb_rawtx_phase_ms(float ms[3]) { return lcb_ctx_rawtx_phase_ms(nullptr, ms); }
