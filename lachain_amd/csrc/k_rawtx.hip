// lachain_amd/csrc/k_rawtx.hip — gfx950 kernels of the raw-transaction ingress: a batch of signed wire transactions
// (RLP) goes in; the decoded records, signatures, invocation spans, RawHash, FullHash and the pool's signature decision
// come out.  The inverse of k_txhash.hip, whose sponge does the hashing here too.
//
// Reference: TransactionServiceWeb3.cs:184-254 (SendRawTransaction and its batch forms), TransactionPool.cs:130-143
// (Add).  rawtx_lane.hpp holds the lane; DESIGN.md §24 the rules and why decode and hashing are one kernel.
//
//   k_rawtx_decode     one item per lane: decode, outputs, then the two hashes of the decoded fields; no LDS, no
//                      barriers.  A lane whose invocation has RAWTX_LONG bytes or more writes its decoded outputs but
//                      does not hash: it appends its index to a list (one vector atomic add) and leaves
//   k_rawtx_long       the listed items, one per lane, packed (k_tx_hash_long's reason: a sponge is serial, and a long
//                      item among short ones would hold its wave on one active lane); the lane runs whole again, so
//                      nothing but the wire bytes is read back
//   k_rawtx_finish     one item per lane after the recovery: detail bit 2, accept, From
#include "rawtx_lane.hpp"
#include "gate.hpp"

#define RAWTX_BLOCK 256
typedef unsigned long long ull;

extern "C" __global__ void __launch_bounds__(RAWTX_BLOCK) k_rawtx_decode(const uint8_t *raw, const ull *off, ull span_base,
                                                                        u32 sig_len, u32 chain_id, u32 n, uint8_t *status,
                                                                        uint8_t *detail, uint8_t *txs, ull *span,
                                                                        uint8_t *sigs, uint8_t *raw32, uint8_t *full32,
                                                                        u32 *long_count, u32 *long_list) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (rawtx_lane(i, raw, (const u64 *)off, span_base, sig_len, chain_id, raw32 || full32, status, detail, txs,
                   (u64 *)span, sigs, raw32, full32))
        long_list[atomicAdd(long_count, 1u)] = i;      // at most n entries: every lane appends at most once
}
// launched over n lanes (the count is known only on the device): lanes past the count leave at once
extern "C" __global__ void __launch_bounds__(RAWTX_BLOCK) k_rawtx_long(const uint8_t *raw, const ull *off, ull span_base,
                                                                      u32 sig_len, u32 chain_id, u32 n, uint8_t *status,
                                                                      uint8_t *detail, uint8_t *txs, ull *span,
                                                                      uint8_t *sigs, uint8_t *raw32, uint8_t *full32,
                                                                      const u32 *long_count, const u32 *long_list) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || j >= *long_count) return;
    const u32 i = long_list[j];
    if (i >= n) return;
    rawtx_lane(i, raw, (const u64 *)off, span_base, sig_len, chain_id, false, status, detail, txs, (u64 *)span, sigs, raw32,
               full32);
}

extern "C" __global__ void __launch_bounds__(RAWTX_BLOCK) k_rawtx_finish(const uint8_t *status, const uint8_t *rec_ok,
                                                                        const uint8_t *addr20, const uint8_t *det_in, u32 n,
                                                                        uint8_t *accept, uint8_t *detail, uint8_t *txs) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rawtx_finish(i, status, rec_ok, addr20, det_in, accept, detail, txs);
}

// ---------------------------------------------------------------- host launch wrappers
static unsigned rawtx_blocks(u32 n) { return (n + RAWTX_BLOCK - 1) / RAWTX_BLOCK; }
extern "C" void lcbk_rawtx_decode(hipStream_t s, const uint8_t *raw, const uint64_t *off, uint64_t span_base, u32 sig_len,
                                  u32 chain_id, u32 n, uint8_t *status, uint8_t *detail, uint8_t *txs, uint64_t *span,
                                  uint8_t *sigs, uint8_t *raw32, uint8_t *full32, uint32_t *long_ws) {
    if (!n) return;
    (void)hipMemsetAsync(long_ws, 0, 4, s);           // long_ws: the count, then n indices
    LCB_LAUNCH_GATED(k_rawtx_decode, dim3(rawtx_blocks(n)), dim3(RAWTX_BLOCK), 0, s, raw, (const ull *)off, (ull)span_base,
                     sig_len, chain_id, n, status, detail, txs, (ull *)span, sigs, raw32, full32, long_ws, long_ws + 1);
    if (!raw32 && !full32) return;                     // nothing to hash, nothing listed
    LCB_LAUNCH_GATED(k_rawtx_long, dim3(rawtx_blocks(n)), dim3(RAWTX_BLOCK), 0, s, raw, (const ull *)off, (ull)span_base,
                     sig_len, chain_id, n, status, detail, txs, (ull *)span, sigs, raw32, full32, (const u32 *)long_ws,
                     (const u32 *)(long_ws + 1));
}
extern "C" void lcbk_rawtx_finish(hipStream_t s, const uint8_t *status, const uint8_t *rec_ok, const uint8_t *addr20,
                                  const uint8_t *det_in, u32 n, uint8_t *accept, uint8_t *detail, uint8_t *txs) {
    if (!n) return;
    LCB_LAUNCH_GATED(k_rawtx_finish, dim3(rawtx_blocks(n)), dim3(RAWTX_BLOCK), 0, s, status, rec_ok, addr20, det_in, n,
                     accept, detail, txs);
}
