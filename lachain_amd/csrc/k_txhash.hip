// lachain_amd/csrc/k_txhash.hip — gfx950 kernels: a transaction's RawHash and FullHash from its fields (RLP encoded in
// registers and absorbed into Keccak-256, never materialised) and the receipt decision that rides on them.
//
// Reference: TransactionUtils.cs:30-105 (the encoding; txhash_lane.hpp holds the lane), TransactionVerifier.cs:109-143
// (VerifyTransactionImmediately), BlockManager.cs:690-694 (the block's transaction root).
//
//   k_tx_hash          one transaction per lane: RawHash, FullHash, FullHash == claimed hash; one sponge per lane in
//                      registers, one pass per hash, no LDS, no barriers.  A lane whose invocation has TXH_LONG bytes or
//                      more does not hash it: it appends its index to a list (one vector atomic add) and leaves
//   k_tx_hash_long     the listed items, one per lane, packed: a sponge is serial, so a long item among short ones would
//                      hold its wave for hundreds of permutations on one active lane
//   k_tx_detail        one receipt per lane: detail = hash bit | recovered << 1 | address is From << 2, accept = all three
//   k_tx_root_ok       one block per lane: computed root (zero for an empty block) == expected root
#include "txhash_lane.hpp"
#include "gate.hpp"

#define TXH_BLOCK 256
typedef unsigned long long ull;

#define TXH_LONG 1024
extern "C" __global__ void __launch_bounds__(TXH_BLOCK) k_tx_hash(const uint8_t *txs, const uint8_t *inv, const ull *off,
                                                                 const uint8_t *sigs, u32 sig_len, const uint8_t *claimed,
                                                                 u32 chain_id, u32 n, uint8_t *raw32, uint8_t *full32,
                                                                 uint8_t *match, u32 *long_count, u32 *long_list) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (off[i + 1] - off[i] >= TXH_LONG) {             // at most n entries: every lane appends at most once
        long_list[atomicAdd(long_count, 1u)] = i;
        return;
    }
    tx_lane(i, txs, inv, (const u64 *)off, sigs, sig_len, claimed, chain_id, raw32, full32, match);
}
// launched over n lanes (the count is known only on the device): lanes past the count leave at once
extern "C" __global__ void __launch_bounds__(TXH_BLOCK) k_tx_hash_long(const uint8_t *txs, const uint8_t *inv,
                                                                      const ull *off, const uint8_t *sigs, u32 sig_len,
                                                                      const uint8_t *claimed, u32 chain_id, u32 n,
                                                                      uint8_t *raw32, uint8_t *full32, uint8_t *match,
                                                                      const u32 *long_count, const u32 *long_list) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n || j >= *long_count) return;
    const u32 i = long_list[j];
    if (i >= n) return;
    tx_lane(i, txs, inv, (const u64 *)off, sigs, sig_len, claimed, chain_id, raw32, full32, match);
}

// match / rec_ok: one byte per receipt; addr20: the recovered addresses (zero where nothing recovered); From is read
// from the receipt's record
extern "C" __global__ void __launch_bounds__(TXH_BLOCK) k_tx_detail(const uint8_t *match, const uint8_t *rec_ok,
                                                                   const uint8_t *addr20, const uint8_t *txs, u32 n,
                                                                   uint8_t *accept, uint8_t *detail) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool rec = rec_ok[i] != 0;
    bool same = rec;
    for (int b = 0; b < 20; b++) same = same && addr20[20 * (size_t)i + b] == txs[TX_REC_BYTES * (size_t)i + TX_REC_FROM + b];
    const uint8_t d = (uint8_t)((match[i] != 0) | (rec << 1) | (same << 2));
    accept[i] = d == 7;
    if (detail) detail[i] = d;
}

// roots / status: k_merkle_root's outputs (a block without transactions has status 0 and a zero root, the
// reference's `?? UInt256Utils.Zero`)
extern "C" __global__ void __launch_bounds__(TXH_BLOCK) k_tx_root_ok(const uint8_t *roots, const uint8_t *expected, u32 n,
                                                                    uint8_t *root_ok) {
    const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    u64 a[4], e[4];
    rbc_load_hash(a, roots + 32 * (size_t)b);
    rbc_load_hash(e, expected + 32 * (size_t)b);
    root_ok[b] = a[0] == e[0] && a[1] == e[1] && a[2] == e[2] && a[3] == e[3];
}

// ---------------------------------------------------------------- host launch wrappers
static unsigned txh_blocks(u32 n) { return (n + TXH_BLOCK - 1) / TXH_BLOCK; }
extern "C" void lcbk_tx_hash(hipStream_t s, const uint8_t *txs, const uint8_t *inv, const uint64_t *off,
                             const uint8_t *sigs, u32 sig_len, const uint8_t *claimed, u32 chain_id, u32 n,
                             uint8_t *raw32, uint8_t *full32, uint8_t *match, uint32_t *long_ws) {
    if (!n) return;
    (void)hipMemsetAsync(long_ws, 0, 4, s);           // long_ws: the count, then n indices
    LCB_LAUNCH_GATED(k_tx_hash, dim3(txh_blocks(n)), dim3(TXH_BLOCK), 0, s, txs, inv, (const ull *)off, sigs, sig_len,
                     claimed, chain_id, n, raw32, full32, match, long_ws, long_ws + 1);
    LCB_LAUNCH_GATED(k_tx_hash_long, dim3(txh_blocks(n)), dim3(TXH_BLOCK), 0, s, txs, inv, (const ull *)off, sigs, sig_len,
                     claimed, chain_id, n, raw32, full32, match, (const u32 *)long_ws, (const u32 *)(long_ws + 1));
}
extern "C" void lcbk_tx_detail(hipStream_t s, const uint8_t *match, const uint8_t *rec_ok, const uint8_t *addr20,
                               const uint8_t *txs, u32 n, uint8_t *accept, uint8_t *detail) {
    if (!n) return;
    LCB_LAUNCH_GATED(k_tx_detail, dim3(txh_blocks(n)), dim3(TXH_BLOCK), 0, s, match, rec_ok, addr20, txs, n, accept,
                     detail);
}
extern "C" void lcbk_tx_root_ok(hipStream_t s, const uint8_t *roots, const uint8_t *expected, u32 n, uint8_t *root_ok) {
    if (!n) return;
    LCB_LAUNCH_GATED(k_tx_root_ok, dim3(txh_blocks(n)), dim3(TXH_BLOCK), 0, s, roots, expected, n, root_ok);
}
