// lachain_amd/csrc/lcb_ctx.hpp — the library's per-caller execution context (host side, internal).
//
// An lcb_ctx owns every device workspace a batch call needs, so concurrent callers never share one: the TPKE
// and threshold-signature line sets are separate, and a *_prepared call checks the exact shape (keys,
// ciphertexts / messages) and generation its prepare recorded instead of a buffer capacity.  Work of one
// context is ordered by an event chain: every enqueue waits on the context's previous work and records a new
// event, so a workspace is never rewritten while a kernel on another stream still reads it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <vector>
#include <string>
#include <unordered_map>

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    void *get(size_t n) {
        if (n == 0) n = 16;
        if (n > cap) {
            if (p) (void)hipFree(p);
            p = nullptr;
            if (hipMalloc(&p, n) != hipSuccess) { cap = 0; p = nullptr; return nullptr; }
            cap = n;
        }
        return p;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// The device buffers of the randomized batch check (lcb_batch.cpp), grown on demand (DevBuf::get) by the function named
// last in each line.  n: the call's shares; a level's entries: its groups or singles.
enum RlcBuf {
    RLC_REC_A,        // per share, its exponent's multiple of U_i (TPKE) / of the key (CommonCoin): n Jacobian G1 records; rlc_ws
    RLC_REC_B,        // per share, the multiple of Y_i (G1) / of the signature share (G2): n Jacobian records; rlc_ws
    RLC_DESC_A,       // the current level's entry list, 16 B per entry, n entries; rlc_ws (swapped with DESC_B per level)
    RLC_DESC_B,       // the next level's list (k_rlc_resolve / search append to it); the census's singles first; rlc_ws
    RLC_CNT,          // the device counter block (RlcCnt words, 32 B); rlc_ws
    RLC_GPTS,         // a level's summed points, one record per entry (RlcKindInfo::rec bytes); rlc_census / rlc_levels
    RLC_GACC,         // a level's decisions, one byte per entry: Miller pre-flag, then the check's result; the same
    RLC_GEX,          // per entry: its shares need exact single checks (W outside G2), set by the sums; the same
    RLC_SDESC,        // level 2's descriptors of the failed level-1 groups, 16 B each (TPKE: twice as many, the open
                      // groups' go behind them); rlc_levels at level 1
    RLC_GAMMA,        // the level-1 groups' final-exponentiation values (gamma_0), 576 B per group; rlc_levels at level 1
    RLC_WSUM,         // CommonCoin: the level-1 groups' weighted sums for level 2 (RlcKindInfo::wrec bytes); the same
    RLC_KTAB,         // the keys' fixed-base tables and their workspace (lcbk_key_table_bytes); rlc_key_tables
    RLC_SUSP,         // the suspect-key bitmap, one bit per key; rlc_ws when the call has a census
    RLC_CVAL,         // per census share: its single was a valid check (feeds k_rlc_census_stats); rlc_census
    RLC_MFB,          // the cooperative Miller kernel's fallback flags, one byte per check of a chunk; rlc_checks
    RLC_G12,          // TPKE level 2: gamma_c rows, then gamma_t rows, 576 B per failed group each; rlc_levels
    RLC_OPEN,         // TPKE level 2: the count (4 words) and list of groups the one-error search leaves open; rlc_levels
    RLC_HOK,          // split preparation: H's hash validity per ciphertext, merged into t_ctok; the fused TPKE call
    RLC_S2B_PARK,     // the two-error search's Fp12 slots (lcbk_tpke_rlc_search2b_asm_park_bytes); rlc_levels
    RLC_PAIR_PARK,    // the level-1 pair stage's two park buffers (products + solos, then pass 2); rlc_fe_pairs
    RLC_PAIR_LISTS,   // its job lists (FePairWs); rlc_fe_pairs
    RLC_POS_BIN,      // TPKE: per share, its exponent's bin (32 set + pos), one byte; rlc_points_enqueue
    RLC_POS_PERM,     // TPKE: the shares behind the census sorted by bin, 4 B each; the same
    RLC_POS_BINS,     // TPKE: the counting sort's histogram and cursors (lcbk_rlc_pos_bins_bytes); the same
    RLC_POS_TABLE,    // TPKE: P[bin][key] = t[bin] Y_key and its flags (lcbk_rlc_pos_table_bytes); the same
    RLC_N
};
// The words of the device counter block RLC_CNT (the kernels take pointers to single words)
enum RlcCnt {
    CNT_GROUPS,       // the current level's entries (k_rlc_groups counts level 1's)
    CNT_NEXT,         // the next level's entries (k_rlc_resolve and the searches)
    CNT_SEARCH,       // failed level-1 groups handed to level 2 (k_rlc_resolve)
    CNT_SUSPECTS,     // suspect keys (k_rlc_census_stats)
    CNT_SPLIT,        // level-1 entries after the suspect split (k_rlc_suspect_split)
    CNT_N
};
// Host-side names of the last batched call's statistics; the C ABI returns each array in this order
enum RlcCensusStat {  // lcb_ctx::rlc_census
    CENSUS_SHARES,    // shares the census checked one by one
    CENSUS_SUSPECTS,  // keys it marked suspect
    CENSUS_GROUPS,    // level-1 groups before the suspect split
    CENSUS_ENTRIES,   // level-1 entries after it
    CENSUS_N
};
enum FePairStat {     // lcb_ctx::fe_pair, the level-1 pair stage
    FE_PAIRS_FORMED,
    FE_PAIRS_FAILED,
    FE_PASS1_JOBS,    // final exponentiations of pass 1
    FE_PASS2_JOBS,    // and of pass 2
    FE_PAIR_N
};
enum LvlKernelStat {  // lcb_ctx::lvl_kernel, the levels' final-exponentiation dispatches
    LVL_ONE_LANE,     // on the one-lane kernel
    LVL_NINE_LANE,    // on the nine-lane kernel
    LVL_MOVED_BUSY,   // one-lane only because the call was overlapped
    LVL_MAX_INFLIGHT, // the largest in-flight count seen
    LVL_KERNEL_N
};
enum RlcMsStat {      // lcb_ctx::rlc_ms, accumulated over the levels
    MS_SUMS,
    MS_MILLER,
    MS_FINAL_EXP,     // with the resolve / search behind it
    MS_PREP,          // the fused call's preparation chain (0 for other calls)
    RLC_MS_N
};


// The named workspaces below belong to device-path code (what the *_dev forms reach), each grown on demand by the function
// named last in its line.  What a host-pointer form itself uploads, receives or scratches in has no name: HostCall
// (host_call.hpp) hands it slots of lcb_ctx::stage[] in request order.
enum { STAGE_SLOTS = 20 };
enum CoopBuf {        // lcb_ctx::t_coop, small exact TPKE batches on the cooperative kernels (n: the call's shares)
    COOP_PTS,         // per share, its two G1 points (U_i, Y_i), 2 n affine records; tpke_verify_core
    COOP_DESC,        // per share, the check's descriptor, 16 B; the same
    COOP_FLAGS,       // the cooperative Miller kernel's two flag bytes per share, 2 n B; the same
    COOP_N
};
enum LagBuf {         // lcb_ctx::lag, Lagrange interpolation at 0 (ne: entries over all problems)
    LAG_LAMBDA,       // the coefficients, ne Fr values; lagrange_enqueue
    LAG_PARTS,        // lambda_i y_i, ne Jacobian G1 / G2 records; the same
    LAG_PARTS_OK,     // their validity, ne B; the same
    LAG_LANES_WS,     // the persistent multiplication grid's workspace (lcbk_lanes_ws_bytes); the same
    LAG_PREFIX,       // the batch inversion's prefix products, ne Fr values; the same
    LAG_N
};
enum SelBuf {         // lcb_ctx::sel, the first k valid shares of every group (ne = groups x k)
    SEL_XS,           // their evaluation points, 32 ne B; assemble_enqueue
    SEL_YS,           // their wire points, 48 / 96 ne B; the same
    SEL_OFF,          // the problems' entry offsets, groups + 1 words; the same
    SEL_SRC,          // G2: each entry's share index into s_dec, ne words; the same
    SEL_N
};
enum MsmBuf {         // lcb_ctx::msm, the Pippenger MSM (m = points x windows digit records, nb buckets)
    MSM_KEYS,         // the records' bucket keys, m words; msm_enqueue
    MSM_KEYS2,        // the radix sort's second key buffer, m words; the same
    MSM_VALS,         // the records' point indices, m words; the same
    MSM_VALS2,        // the sort's second value buffer, m words; the same
    MSM_START,        // per bucket, its first record, nb words; the same
    MSM_END,          // per bucket, one past its last record, nb words; the same
    MSM_BUCKETS,      // the bucket sums, nb Jacobian records; the same
    MSM_SEGS,         // the bucket reduction's segment sums, n_seg Jacobian records; the same
    MSM_L1,           // the per-window tree reduction's other buffer, n_l1 Jacobian records; the same
    MSM_WINS,         // the window sums, one Jacobian record per key window; the same
    MSM_SORT_TMP,     // the radix sort's temporary storage (lcbk_sort_pairs' query); the same
    MSM_PHI,          // GLV form: phi(P) of every point, 96 n B; the same
    MSM_CHUNK_HEAD,   // record-balanced accumulation: each chunk's head partial, one Jacobian record; the same
    MSM_CHUNK_TAIL,   // and its tail partial; the same
    MSM_JAC_SUM,      // the sum of the ranks' partial results, one Jacobian record; lcb_ctx_g1_jac_sum_dev
    MSM_N
};
enum EcBuf {          // lcb_ctx::ec, ECDSA verification (n signatures)
    EC_JOBS,          // the job records, lcbk_secp_job_bytes() n; verify_enqueue
    EC_HASH,          // the header hashes when the call hashes first, 32 n B; the same
    EC_HASH_OK,       // their validity, n B; the same
    EC_N
};
enum ErBuf {          // lcb_ctx::er, public-key recovery (n signatures)
    ER_JOBS,          // the job records, lcbk_secp_rjob_bytes() n; recover_enqueue
    ER_PTS,           // the Jacobian results, lcbk_secp_rpoint_bytes() n; the same
    ER_N
};
enum EciesBuf {       // lcb_ctx::ecies, the ECIES envelope (n items); the secret-bearing ones are cleared after use
    ECIES_JOBS,       // the ECDH job records (the scalars' digits), lcbk_ecdh_job_bytes() n; ecdh_core
    ECIES_PTS,        // the Jacobian results, lcbk_ecdh_point_bytes() n; the same
    ECIES_KEYS,       // the session keys of the fused envelope calls, 32 n B; envelope_encrypt_dev / envelope_decrypt_dev
    ECIES_EOK,        // the ECDH validity, n B; the same two
    ECIES_EPH,        // the ephemeral public keys, 33 n B; envelope_encrypt_dev
    ECIES_POK,        // their validity, n B; the same
    ECIES_OFF,        // the plaintext offsets of a decryption, n + 1 u64; gcm_decrypt_dev / envelope_decrypt_dev
    ECIES_N
};
enum TxBuf {          // lcb_ctx::tx, transaction hashing and receipts (n transactions)
    TX_RAW,           // the raw hashes, 32 n B; receipts_enqueue
    TX_FLAGS,         // hash-match, then recovered flags, 2 n B; the same
    TX_ADDR,          // the recovered addresses, 20 n B; the same
    TX_ROOTS,         // the blocks' roots and their status, 33 B per block; the same
    TX_LONG,          // the count and list of long items k_tx_hash leaves to k_tx_hash_long, n + 1 words; hash_enqueue
    TX_N
};
enum RawTxBuf {       // lcb_ctx::rawtx, the raw-transaction ingress (n items)
    RAWTX_HASH,       // the raw hashes the recovery reads when the caller takes none, 32 n B; ingest_enqueue
    RAWTX_SIGS,       // the decoded signatures when the caller takes none, sig_len n B; the same
    RAWTX_DETAIL,     // detail bits 0 and 1 when the caller takes no detail, n B; the same
    RAWTX_REC_OK,     // the recovery's validity, n B; the same
    RAWTX_ADDR,       // the recovered addresses, 20 n B; the same
    RAWTX_LONG_LIST,  // the count and list of long items k_rawtx_decode leaves to k_rawtx_long, n + 1 words; the same
    RAWTX_N
};
enum TrieBuf {        // lcb_ctx::trie, the state trie
    TRIE_LIST,        // the flat call's count and list of internal nodes, n + 1 words; flat_enqueue
    TRIE_ROOT_WS,     // the root builder's workspace (lcbk_trie_root_ws_bytes); root_enqueue
    TRIE_N
};
enum KdfBuf {         // lcb_ctx::kdf, the TPKE keystream and its compositions (n items; ne entries of the literal form)
    KDF_T,            // Encrypt: T = r Y per item, the keystream's seeds, 48 n B, cleared after use; encrypt_enqueue
    KDF_OK1,          // Encrypt: the first phase's validity when the caller passes no ok, n B; lcb_ctx_tpke_encrypt_dev
    KDF_OK2,          // Encrypt: the second phase's validity, merged into the caller's ok, n B; the same
    KDF_U,            // FullDecrypt: u = sum lambda_i U_i per ciphertext, the seeds, 48 n B, cleared after use;
                      // lcb_ctx_tpke_full_decrypt_dev / literal_enqueue
    KDF_XS,           // FullDecrypt, literal form: the evaluation points ids + 1 as Fr values, 32 ne B; literal_enqueue
    KDF_N
};
struct lcb_ctx {
    std::recursive_mutex mu;      // one enqueue at a time per context (contexts may be shared by threads)
    int device = 0;
    hipStream_t stream = nullptr;   // for the synchronous host-pointer entry points
    hipEvent_t order = nullptr;     // completion of the last work enqueued in this context
    bool order_valid = false;
    int enq_depth = 0;              // nesting of Enq scopes held by the owning thread
    size_t chunk = (size_t)1 << 21; // lcb_set_verify_chunk's value, read once per outermost enqueue (LCB_VERIFY_CHUNK)
    // TPKE workspace (lcb_*tpke_prepare_dev): line sets of H and W per ciphertext, validity, decompressed keys
    DevBuf t_lines, t_ctok, t_keys, t_f;
    DevBuf t_ctg2;                    // per ciphertext: W in G2, decided from its line set; written by every TPKE
                                      // preparation (tpke_prepare, the fused batched call), read by the batch check's sums
    DevBuf t_coop[COOP_N];           // small exact batches on the cooperative kernels
    // prepared-ciphertext cache of lcb_tpke_verify_shares_cached (line sets + validity per slot, keyed by the bytes)
    DevBuf cc_lines, cc_ok;
    std::unordered_map<std::string, uint32_t> cc_map;
    std::vector<std::string> cc_keys;
    std::vector<uint64_t> cc_used;
    uint64_t cc_tick = 0;
    int cc_flags = -1;
    // decompressed-key cache of the same entry point (an epoch's verification keys recur in every flush): one slot per
    // 48-byte key, filled in order; a call that would overflow it starts it afresh
    DevBuf kc_pts;
    std::unordered_map<std::string, uint32_t> kc_map;
    uint32_t kc_n = 0;
    size_t t_n_cts = 0, t_n_keys = 0;
    uint64_t t_gen = 0;
    bool t_ready = false;
    // threshold-signature workspace (lcb_*ts_prepare_dev): line sets of H(m) per message, keys
    DevBuf s_lines, s_mok, s_keys, s_f;
    DevBuf s_dec;                     // decoded shares of the batched CommonCoin checks (ts_share_st), for the assembly
    size_t s_dec_n = 0;
    size_t s_n_msgs = 0, s_n_pks = 0;
    uint64_t s_gen = 0;
    bool s_ready = false;
    // the host-pointer forms' transient buffers, handed out by HostCall (host_call.hpp) in request order.  The largest
    // taker at present is lcb_dkg_commitment_eval's exact form with 15 (5 inputs, 2 outputs, 8 of scratch; 14 distinct
    // buffers before there was a HostCall); next come lcb_tpke_verify_shares_cached (11) and lcb_debug_tpke_miller (10).  The rest is headroom; one request too many
    // fails the call
    DevBuf stage[STAGE_SLOTS];
    int stage_next = 0;               // HostCall's cursor: the first free slot
    // Lagrange / assembly / MSM
    DevBuf lag[LAG_N], sel[SEL_N], msm[MSM_N];
    DevBuf lws;                       // lanetab.hpp workspaces of the persistent scalar-multiplication grids (HostCall::lws)
    DevBuf merkle_ws;                 // MerkleTree.ComputeRoot's level workspace, 32 B per hash; lcb_ctx_merkle_root_dev
    // mclBn_pairing's cache of G2 line sets (pc_lines: slot k = Q_k's set and the infinity set), least recently used
    // slot replaced: the protocol pairs every share of a ciphertext / coin with the same H, W (TPKE/PublicKey.cs:91).
    // A buffer of its own: no other call's staging may overwrite cached sets between pairings
    DevBuf pc_lines;
    std::vector<uint32_t> pc_keys;    // 72 words (the mclBnG2 record) per slot
    std::vector<uint64_t> pc_used;    // last use (0: empty)
    uint64_t pc_tick = 0;
    hipEvent_t ver_ev[3] = {};
    bool ver_ev_ready = false, ver_ran = false;
    // randomized batch verification (k_batch.hip, lcb_batch.cpp)
    DevBuf rlc[RLC_N];
    uint32_t fe_pair[FE_PAIR_N] = {};         // last call's pair stage
    uint32_t lvl_kernel[LVL_KERNEL_N] = {};   // last call's level final exponentiations
    bool rlc_pos_exp = false;         // the TPKE call in progress draws its exponents per group position (pair stage: by set)
    bool lvl_counted = false;         // this call holds a count in the device's in-flight counter (BatchedInflight)
    hipEvent_t rlc_ev[3] = {};
    hipEvent_t rlc_lev_ev[4] = {};    // per level: before sum / Miller / final exp / resolve
    float rlc_ms[RLC_MS_N] = {};      // last call's phase times
    bool rlc_ev_ready = false, rlc_ran = false;
    uint32_t rlc_levels[8] = {};
    uint32_t rlc_census[CENSUS_N] = {};
    int rlc_nlev = 0;
    uint64_t rlc_calls = 0;
    // what the last batched call's randomisation wrote into rlc[RLC_REC_A / RLC_REC_B], for lcb_debug_rlc_records (test
    // hook): its shares, its census prefix (shares [0, i0) have no records) and its kind (-1: none yet, 0 TPKE, 1 TS)
    size_t rlc_last_n = 0, rlc_last_i0 = 0;
    int rlc_last_kind = -1;
    // which prepared line sets are not normalised (adversarial W): [0] the census's ciphertexts, [1] all; the one-lane
    // Miller fallback is dispatched only when the flag is set (round 5: an idle fallback dispatch waited ~15 ms for a
    // SIMD with 360 free registers behind the randomisation).  Device words, pinned copies, events after the copies.
    DevBuf unn;
    uint32_t *unn_pin = nullptr;
    hipEvent_t unn_ev[2] = {};
    bool unn_set[2] = {false, false};
    int unn_census = 1;               // the flag the census reads: 0 when its ciphertexts were prepared first (split)
    hipStream_t aux = nullptr;        // second stream of the fused batched verify (randomisation beside preparation)
    hipStream_t hi = nullptr;         // high-priority stream: the latency-bound preparation chain (lcb_set_fork_mode 1)
    hipStream_t hi2 = nullptr;        // second high-priority stream: U / W decompression + W's line sets (fork mode 3)
    hipStream_t hi3 = nullptr;        // third: the bulk of the split preparation when the census ciphertexts go first
    hipEvent_t fork_ev[5] = {};
    hipEvent_t prep_ev[3] = {};       // timed: the fused call's preparation chain (stats ms[5]); [2] after the hashing
    bool prep_timed = false;
    bool fork_ready = false;
    hipEvent_t msm_ev[7] = {};
    bool msm_ev_ready = false, msm_ran = false;
    // secp256k1 ECDSA (lcb_ecdsa.cpp): job records and header hashes, and the host API's cached key set
    DevBuf ec[EC_N];
    hipEvent_t ec_ev[4] = {};         // around header hash / scalars / verify of the last verification
    bool ec_ev_ready = false, ec_ran = false, ec_hashed = false;
    struct lcb_ecdsa_keyset *ec_cache = nullptr;
    std::vector<uint8_t> ec_cache_keys;
    size_t ec_cache_pk_len = 0;
    // public-key recovery (lcb_ecdsa.cpp): job records and Jacobian results
    DevBuf er[ER_N];
    hipEvent_t er_ev[4] = {};         // around scalars / recovery / finish of the last recovery
    bool er_ev_ready = false, er_ran = false;
    // secp256k1 ECIES (lcb_ecies.cpp)
    DevBuf ecies[ECIES_N];
    hipEvent_t ecies_ev[5] = {};      // around scalars / multiplication / finish / GCM of the last call
    bool ecies_ev_ready = false, ecies_ran = false;
    // transaction hashing and receipt verification (lcb_txhash.cpp)
    DevBuf tx[TX_N];
    hipEvent_t tx_ev[4] = {};         // around hashing / recovery and decision / roots of the last call
    bool tx_ev_ready = false, tx_ran = false;
    // raw-transaction ingress (lcb_rawtx.cpp)
    DevBuf rawtx[RAWTX_N];
    hipEvent_t rawtx_ev[4] = {};      // around decode and hashing / recovery / finish of the last call
    bool rawtx_ev_ready = false, rawtx_ran = false;
    // state trie (lcb_trie.cpp)
    DevBuf trie[TRIE_N];
    // TPKE keystream and the one-call Encrypt / FullDecrypt (lcb_kdf.cpp)
    DevBuf kdf[KDF_N];
    hipEvent_t kdf_ev[2] = {};        // around k_kdf_xor of the last call
    bool kdf_ev_ready = false, kdf_ran = false;
};

// Enqueue scope: exclusive use of the context, stream ordered after the context's previous work, and the
// context's order event recorded after this call's work.  The outermost scope snapshots the verify chunk, so a call
// sizes its park buffers and steps its chunk loops with one value even if lcb_set_verify_chunk runs meanwhile.
size_t lcb_verify_chunk_now();
struct Enq {
    lcb_ctx *c;
    hipStream_t s;
    std::unique_lock<std::recursive_mutex> lk;
    Enq(lcb_ctx *c_, hipStream_t s_) : c(c_), s(s_), lk(c_->mu) {
        if (c->enq_depth++ == 0) c->chunk = lcb_verify_chunk_now();
        if (c->order_valid) (void)hipStreamWaitEvent(s, c->order, 0);
    }
    ~Enq() {
        if (hipEventRecord(c->order, s) == hipSuccess) c->order_valid = true;
        --c->enq_depth;
    }
};
