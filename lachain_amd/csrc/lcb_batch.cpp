// lachain_amd/csrc/lcb_batch.cpp — host driver of the randomized batch check (include/lachain_bls.h "*_batched";
// kernels: k_batch.hip, k_rlc_rand.hip, k_tpke.hip, k_prep.hip, k_coop.hip).
//
// One call: the census (exact checks of a prefix of the shares, which marks suspect keys), the randomisation (per-share
// exponent multiples and the level-1 groups), then the level loop (sums, Miller, final exponentiation, resolve) with
// the TPKE level-1 pair stage and the level-2 searches.  The fused calls also prepare the batch (keys, hashing, line
// sets) beside the randomisation on forked streams.  The exact paths, the preparations they share with the prepared
// forms (tpke_prepare, ts_prepare) and the host-pointer entry points are in lcb_host.cpp; lcb_internal.hpp lists what
// the two files use of each other.  The device buffers are lcb_ctx::rlc[RlcBuf] (lcb_ctx.hpp).
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <mutex>
#include <atomic>
#include <vector>
#include <algorithm>
#include <sys/random.h>

#include "launch.h"
#include "lcb_internal.hpp"
#include "../../include/lachain_bls.h"

using namespace lcb_int;

#define LCB_RLC_GROUP_CAP 32                  // shares per TPKE level-1 group (k_rlc_groups)
#define LCB_VERIFY_CHUNK (c->chunk)             // lcb_set_verify_chunk's value for this call (lcb_ctx.hpp Enq)
// level-2 two-error search on the assembly Fp12 products (k_tpke.hip k_tpke_rlc_search2b_asm, round 6)
#ifndef LCB_SEARCH2B_ASM
#define LCB_SEARCH2B_ASM 1
#endif

std::atomic<uint32_t> lcb_int::g_coop_max{32768};    // lcb_set_coop_max: batches / levels of <= this many checks use the 9-lane kernels

namespace {

std::atomic<int> g_fork_mode{4};            // lcb_set_fork_mode: stream layout of the fused batched verify (1: measured
                                            // 104.8 vs 117.8 ms per 1M-share TPKE step, profiles/r03/ab1; 3, the split
                                            // preparation: 99.6 vs 103.2 ms, profiles/r03/ab8; 4, the split preparation
                                            // in one dispatch on one high-priority stream: DESIGN.md §14.2)
std::atomic<uint32_t> g_coop_miller_max{65536};   // lcb_set_coop_miller_max: as g_coop_max for the group Miller loops only
                                                  // (65536: level 1 too, 105.5 vs 106.1 ms, profiles/r03/ab2)
// The kernel form of a TPKE level's final exponentiation when batches overlap.  The nine-lane kernel
// issues about 50 % more wave instructions per check than the one-lane kernel; they buy latency while a level is below
// one wave per SIMD and nothing while other batches keep the SIMDs full.  g_batched_inflight counts, per device, the
// batched TPKE verify calls between entry and return; a call that sees another one counted when it enqueues a level's
// final exponentiation is overlapped, and then lcb_set_busy_coop_max's value decides instead of lcb_set_coop_max's.
// Default 20,000: pass 1 of the headline batch's pair stage (23.8 K jobs) moves, pass 2 and level 2 (8.5 K and 9.4 K
// checks, under one one-lane wave per SIMD) stay: moving them too measured no better than moving nothing (§18).
#ifndef LCB_BUSY_COOP_MAX
#define LCB_BUSY_COOP_MAX 20000u
#endif
static_assert(LCB_BUSY_COOP_MAX >= 1024u, "the aggregation queue's overlapping small flushes keep the nine-lane kernel");
std::atomic<uint32_t> g_busy_coop_max{LCB_BUSY_COOP_MAX};   // UINT32_MAX: the rule is off
std::atomic<int> g_level_mode{0};                 // lcb_set_level_mode: 0 by the count, 1 never overlapped, 2 always
std::atomic<uint32_t> g_batched_inflight[64];
struct BatchedInflight {                          // scope guard: every return of the counted call releases its count
    lcb_ctx *c;
    std::atomic<uint32_t> *a;
    explicit BatchedInflight(lcb_ctx *c_)
        : c(c_), a(c_->device >= 0 && c_->device < 64 && !c_->lvl_counted ? &g_batched_inflight[c_->device] : nullptr) {
        if (a) { a->fetch_add(1); c->lvl_counted = true; }
    }
    ~BatchedInflight() {
        if (a) { c->lvl_counted = false; a->fetch_sub(1); }
    }
    BatchedInflight(const BatchedInflight &) = delete;
    BatchedInflight &operator=(const BatchedInflight &) = delete;
};
// the kernel of a final-exponentiation dispatch of m checks in the level driver: true = one-lane.  ruled: a TPKE level
// (not CommonCoin, not a census chain), where the overlap rule may replace lcb_set_coop_max's
bool fe_one_lane(lcb_ctx *c, size_t m, bool ruled) {
    const bool lat_one = m > g_coop_max.load();
    bool one = lat_one;
    const uint32_t bm = g_busy_coop_max.load();
    if (ruled) {
        const int mode = g_level_mode.load();
        uint32_t nfl = 0;
        if (c->device >= 0 && c->device < 64) nfl = g_batched_inflight[c->device].load();
        if (nfl > c->lvl_kernel[LVL_MAX_INFLIGHT]) c->lvl_kernel[LVL_MAX_INFLIGHT] = nfl;
        const bool busy = mode == 2 || (mode == 0 && c->lvl_counted && nfl >= 2);
        if (busy && bm != UINT32_MAX) {
            one = m > bm;
            if (one && !lat_one) c->lvl_kernel[LVL_MOVED_BUSY]++;
        }
    }
    c->lvl_kernel[one ? LVL_ONE_LANE : LVL_NINE_LANE]++;
    return one;
}
// the final exponentiation of m checks (f: their Miller values, acc: their flags) on the kernel fe_one_lane selects.
// The nine-lane form is the one at 248 registers (k_prep.hip): it shares a SIMD with a randomisation wave of the
// batches in flight (three TPKE batches: 15.50-15.78 vs 15.26-15.46 M/s, profiles/r05/abfe2w)
void fe_dispatch(lcb_ctx *c, hipStream_t s, u32 *f, size_t m, uint8_t *acc, bool ruled) {
    if (!fe_one_lane(c, m, ruled)) lcbk_coop_final_exp_check_2w(s, f, (u32)m, acc);
    else lcbk_final_exp_check(dim3(nblk(m)), s, f, (u32)m, acc);
}

// Randomized batch verification (k_batch.hip header): the same accept / reject decisions as the exact per-share
// checks, except with probability <= 2^-64 per group decision (the exponents are secret).  Groups are runs of shares
// of one ciphertext (TPKE) / message (threshold signatures) in the caller's order: ciphertext- / message-major batches
// give one group per ciphertext / message.  A level's group count comes back to the host (one 8-byte read per level).
std::mutex g_seed_mu;                       // lcb_set_batch_seed (test hook) vs. the callers' key fills
uint8_t g_rlc_seed[32];
bool g_rlc_seed_set = false;
std::atomic<size_t> g_census_min{16384};    // lcb_set_batch_census: batches of at least this many shares get a census
enum RlcKind { RLC_TPKE = 0, RLC_TS = 1 };
struct RlcStats {
    bool valid = false;
    int nlev = 0;
    uint32_t levels[8] = {};
    float ms[2 + RLC_MS_N] = {};
    uint32_t census[CENSUS_N] = {};
    uint32_t fe_pair[FE_PAIR_N] = {};
};
thread_local RlcStats t_rlc_stats;
// cnt: the device counter block (RlcCnt); susp: the suspect-key bitmap; m: census shares [0, m)
struct RlcWs {
    u32 *rA, *rB;
    uint8_t *dA, *dB;
    u32 *cnt;
    u32 *susp;
    u32 m;
    u32 *ktab = nullptr;               // the keys' fixed-base tables when built ahead of the fork (keys_first_tables)
    uint8_t *kok = nullptr;
    bool ktab_pre = false;
};
// the fused batched calls build the keys' fixed-base tables on the caller's stream BEFORE forking the preparation: a
// key-table wave (277 registers) cannot be placed beside a preparation wave (346), so launched beside them the tables
// (and the randomisation behind them) waited up to ~20 ms for the preparation to drain (profiles/r04/ab1)
std::atomic<int> g_keys_first{1};
u32 *rlc_key_tables(lcb_ctx *c, const void *keys, size_t n_keys, hipStream_t s, uint8_t **ktab_ok);
void keys_first_tables(lcb_ctx *c, RlcWs &w, const void *keys, size_t n_keys, size_t n, hipStream_t s) {
    if (!g_keys_first.load() || w.m >= n) return;
    w.ktab = rlc_key_tables(c, keys, n_keys, s, &w.kok);
    w.ktab_pre = true;
}
bool rlc_key_fill(lcb_ctx *c, u32 key[10]) {
    bool fixed;
    {
        std::lock_guard<std::mutex> lk(g_seed_mu);
        fixed = g_rlc_seed_set;
        if (fixed) memcpy(key, g_rlc_seed, 32);
    }
    if (!fixed && getrandom(key, 32, 0) != 32) { set_err("batched verify: getrandom failed"); return false; }
    c->rlc_calls++;
    key[8] = (u32)c->rlc_calls;
    key[9] = (u32)(c->rlc_calls >> 32);
    return true;
}
// what the call's points kernel is about to store in RLC_REC_A / RLC_REC_B (lcb_debug_rlc_records reads it back)
void rlc_note_records(lcb_ctx *c, int kind, size_t n, size_t m) {
    c->rlc_last_kind = kind;
    c->rlc_last_n = n;
    c->rlc_last_i0 = m < n ? m : n;
}
// census size: a prefix of the batch large enough to sample every key a few times (>= 8 shares per key on average,
// 512 .. 2048 shares), at most a quarter of the batch; 0 = no census (small batches, or disabled)
u32 census_size(size_t n, size_t n_keys) {
    const size_t min_n = g_census_min.load();
    if (!min_n || n < min_n || n_keys < 2 || n_keys > 4096) return 0;
    size_t m = std::min<size_t>(std::max<size_t>(512, 8 * n_keys), 2048);
    m = std::min(m, n / 4);
    return m < 16 ? 0 : (u32)m;
}
bool rlc_ws(lcb_ctx *c, RlcWs &w, size_t n, size_t rec_a, size_t rec_b, size_t n_keys, u32 m, hipStream_t s) {
    w.rA = (u32 *)c->rlc[RLC_REC_A].get(n * rec_a);
    w.rB = (u32 *)c->rlc[RLC_REC_B].get(n * rec_b);
    w.dA = (uint8_t *)c->rlc[RLC_DESC_A].get(n * 16);
    w.dB = (uint8_t *)c->rlc[RLC_DESC_B].get(n * 16);
    w.cnt = (u32 *)c->rlc[RLC_CNT].get(32);
    const size_t sw = (n_keys + 31) / 32;
    w.susp = m ? (u32 *)c->rlc[RLC_SUSP].get(4 * sw) : nullptr;
    w.m = m;
    if (!w.rA || !w.rB || !w.dA || !w.dB || !w.cnt || (m && !w.susp)) { set_err("device allocation failed"); return false; }
    if (!c->rlc_ev_ready) {
        for (auto &e : c->rlc_ev) hipEventCreate(&e);
        for (auto &e : c->rlc_lev_ev) hipEventCreate(&e);
        c->rlc_ev_ready = true;
    }
    // zeroed on the calling stream before any kernel of the call (the randomisation on the second stream reads
    // the bitmap while the census writes it)
    hipMemsetAsync(w.cnt, 0, 32, s);
    if (m) hipMemsetAsync(w.susp, 0, 4 * sw, s);
    c->rlc_census[CENSUS_SHARES] = m;
    c->prep_timed = false;
    c->rlc_census[CENSUS_SUSPECTS] = c->rlc_census[CENSUS_GROUPS] = c->rlc_census[CENSUS_ENTRIES] = 0;
    return true;
}
// fixed-base tables of the batch's keys (k_rlc_key_tables), when the batch is large enough to repay them
// (4 x 255 points per key, 64 lanes per key, ~24 additions of latency); nullptr: the points kernel multiplies the keys directly
u32 *rlc_key_tables(lcb_ctx *c, const void *keys, size_t n_keys, hipStream_t s, uint8_t **ktab_ok) {
    *ktab_ok = nullptr;
    if (!n_keys || n_keys > 4096) return nullptr;
    u32 *ws = (u32 *)c->rlc[RLC_KTAB].get(lcbk_key_table_bytes((u32)n_keys));
    if (!ws) return nullptr;
    u32 *tab = nullptr;
    lcbk_rlc_key_tables(dim3(1), s, keys, (u32)n_keys, ws, &tab, ktab_ok);
    return tab;
}
// The TPKE exponents (k_batch.hip header).  lcb_set_rlc_share_exponents(1): one exponent per share, from
// its index (the form before the position exponents); 0 (default): per group position, t[set][pos].
// lcb_set_rlc_lane_permutation(0): lane t of the randomisation handles share m + t; 1 (default): the shares sorted by
// bin, so that a wave holds one exponent and skips its zero columns as a wave.  Each half can be measured alone.
// (LCB_RLC_SHARE_EXP, LCB_RLC_LANE_PERM, LCB_RLC_SIGNED_DIGITS and LCB_RLC_POS_TABLE_MIN, with LCB_ALLOW_TUNING=1, set the starting values: A/B
// runs of programs that do not call the setters)
long tuning_env(const char *name, long dflt) {
    const char *e = getenv(name);
    return (e && *e && env_on("LCB_ALLOW_TUNING")) ? atol(e) : dflt;
}
std::atomic<int> g_share_exp{tuning_env("LCB_RLC_SHARE_EXP", 0) ? 1 : 0};
std::atomic<int> g_lane_perm{tuning_env("LCB_RLC_LANE_PERM", 1) ? 1 : 0};
// lcb_set_rlc_signed_digits(1) (default; LCB_RLC_SIGNED_DIGITS): a wave of the randomisation that holds one exponent
// walks its Joint Sparse Form, ~16.5 additions instead of ~24 (rlc_common.hpp g1_mul_ab_jsf); 0: the binary columns.
// The exponents, the records' points and the decisions are the same either way.
std::atomic<int> g_signed_digits{tuning_env("LCB_RLC_SIGNED_DIGITS", 1) ? 1 : 0};
// P = t[bin] Y_d for 128 bins x n_keys keys replaces the key side's eight table additions per share: an entry costs
// about 200 Fp products (eight mixed additions and one inversion), 25,600 per key; a share saves about 88, so the
// table repays itself from 291 shares per key.  512 leaves room for the table's latency ahead of the randomisation
// (a launch of 2 n_keys waves).  lcb_set_rlc_pos_table_min overrides the figure (UINT32_MAX: never).
#ifndef LCB_POS_TABLE_MIN
#define LCB_POS_TABLE_MIN 512u
#endif
std::atomic<uint32_t> g_pos_table_min{(uint32_t)tuning_env("LCB_RLC_POS_TABLE_MIN", LCB_POS_TABLE_MIN)};
// phase 1 (needs the decompressed keys only): per-share exponent multiples of shares [m, n) + level-1 groups (count
// left on device in the CNT_GROUPS word)
int rlc_points_enqueue(lcb_ctx *c, RlcWs &w, uint8_t *d_accept, size_t n, size_t n_keys, size_t n_cts,
                       const uint32_t *d_ct, const uint32_t *d_dec, const uint8_t *d_ui, hipStream_t s) {
    u32 key[10];
    if (!rlc_key_fill(c, key)) return -1;
    rlc_note_records(c, RLC_TPKE, n, w.m);
    const bool pos = !g_share_exp.load(), permute = g_lane_perm.load() != 0;
    c->rlc_pos_exp = pos;
    hipEventRecord(c->rlc_ev[0], s);
    if (w.m < n) {
        uint8_t *kok = w.kok;
        u32 *ktab = w.ktab_pre ? w.ktab : rlc_key_tables(c, c->t_keys.p, n_keys, s, &kok);
        // positions -> bins -> the lane permutation, and the keys' multiples per bin: all on this stream, no host read
        uint8_t *bin = nullptr, *pinf = nullptr;
        u32 *perm = nullptr, *P = nullptr;
        if (pos || permute) {
            bin = (uint8_t *)c->rlc[RLC_POS_BIN].get(n);
            u32 *bins = (u32 *)c->rlc[RLC_POS_BINS].get(lcbk_rlc_pos_bins_bytes());
            if (permute) perm = (u32 *)c->rlc[RLC_POS_PERM].get(4 * (n - w.m));
            if (!bin || !bins || (permute && !perm)) { set_err("device allocation failed (positions)"); return -1; }
            lcbk_rlc_positions(s, d_ct, w.m, (u32)n, (u32)n_cts, bin, bins, perm);
        }
        const uint32_t tmin = g_pos_table_min.load();
        if (pos && ktab && tmin != UINT32_MAX && n - w.m >= (size_t)tmin * n_keys) {
            u32 *pws = (u32 *)c->rlc[RLC_POS_TABLE].get(lcbk_rlc_pos_table_bytes((u32)n_keys));
            if (!pws) { set_err("device allocation failed (position table)"); return -1; }
            lcbk_rlc_pos_table(s, c->t_keys.p, (u32)n_keys, key, ktab, kok, pws, &P, &pinf);
        }
        lcbk_tpke_rlc_points(s, (u32)n_cts, c->t_keys.p, (u32)n_keys, d_ct, d_dec, d_ui, w.m, (u32)n, key, w.rA, w.rB,
                             d_accept, ktab, kok, w.susp, perm, pos ? bin : nullptr, P, pinf, g_signed_digits.load());
        static_assert(LCB_RLC_GROUP_CAP == 32, "the position bins hold the level-1 groups' cap (rlc_common.hpp RLC_POS_CAP)");
        lcbk_rlc_groups(s, d_ct, w.m, (u32)n, (u32)n_cts, LCB_RLC_GROUP_CAP, w.dA, w.cnt + CNT_GROUPS);
    }
    hipEventRecord(c->rlc_ev[1], s);
    return launch_ok("tpke batched verify launch") ? 0 : -1;
}
int ts_rlc_points_enqueue(lcb_ctx *c, RlcWs &w, uint8_t *d_accept, size_t n, size_t n_pks, size_t n_msgs,
                          const uint8_t *d_sigs, const uint32_t *d_midx, const uint32_t *d_pidx, hipStream_t s) {
    u32 key[10];
    if (!rlc_key_fill(c, key)) return -1;
    rlc_note_records(c, RLC_TS, n, w.m);
    hipEventRecord(c->rlc_ev[0], s);
    if (w.m < n) {
        uint8_t *kok = w.kok;
        u32 *ktab = w.ktab_pre ? w.ktab : rlc_key_tables(c, c->s_keys.p, n_pks, s, &kok);
        // decoded-share records for the assembly (optional: without the buffer the assembly decodes the shares)
        const size_t rec = n * (size_t)LCB_TS_SHARE_REC_BYTES;
        const bool grow = c->s_dec.cap < rec;
        void *dec = c->s_dec.get(rec);
        if (dec && grow) hipMemsetAsync(dec, 0, c->s_dec.cap, s);   // no record is valid until written
        c->s_dec_n = dec ? c->s_dec.cap / LCB_TS_SHARE_REC_BYTES : 0;
        lcbk_ts_rlc_points(s, (u32)n_msgs, c->s_keys.p, (u32)n_pks, d_midx, d_pidx, d_sigs, w.m, (u32)n, key, w.rA,
                           w.rB, d_accept, w.dA, w.cnt + CNT_GROUPS, ktab, kok, w.susp, dec);
        lcbk_rlc_groups(s, d_midx, w.m, (u32)n, (u32)n_msgs, 128, w.dA, w.cnt + CNT_GROUPS);
    }
    hipEventRecord(c->rlc_ev[1], s);
    return launch_ok("ts batched verify launch") ? 0 : -1;
}
bool read_counts(u32 *v, const u32 *d, int k, hipStream_t s) {
    if (hipMemcpyAsync(v, d, 4 * k, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        set_err("batched verify: group count");
        return false;
    }
    return true;
}
struct RlcIo {                     // the per-share inputs the exact singles re-read
    const uint32_t *d_key;         // dec_idx (TPKE) / pk_idx (TS)
    const uint8_t *d_pts;          // ui (TPKE) / sigs (TS)
    const uint32_t *d_grp;         // ct_idx (TPKE) / msg_idx (TS): the census singles' groups
};
struct RlcKindInfo {
    bool ts;
    bool fb = true;                   // TPKE: some line set the checks use may be un-normalised (dispatch the fallback)
    const u32 *lines;
    const uint8_t *okv, *ctg2;
    const void *keys;
    size_t n_keys, n_grp, rec, wrec;
};
RlcKindInfo rlc_kind(lcb_ctx *c, RlcKind kind) {
    RlcKindInfo k;
    k.ts = kind == RLC_TS;
    k.lines = (const u32 *)(k.ts ? c->s_lines.p : c->t_lines.p);
    k.okv = (const uint8_t *)(k.ts ? c->s_mok.p : c->t_ctok.p);
    k.ctg2 = (const uint8_t *)c->t_ctg2.p;
    k.keys = k.ts ? c->s_keys.p : c->t_keys.p;
    k.n_keys = k.ts ? c->s_n_pks : c->t_n_keys;
    k.n_grp = k.ts ? c->s_n_msgs : c->t_n_cts;
    k.rec = k.ts ? lcbk_ts_grp_bytes() : 2 * LCB_G1A_ST_BYTES;
    k.wrec = k.ts ? LCB_G1_JAC_BYTES + LCB_G2_JAC_BYTES : 2 * LCB_G1_JAC_BYTES;
    return k;
}
// the buffers of one level (or of the census, or of a level-2 re-check): what the sums write and the checks read.
// A caller sets the ones its stage uses; the rest stay null
struct RlcBufs {
    const uint8_t *desc = nullptr;     // the entries: 16 B each
    void *gpts = nullptr;              // their summed points
    uint8_t *gacc = nullptr;           // their decisions
    uint8_t *gex = nullptr;            // "needs exact singles", from the sums to the resolve
    u32 *f = nullptr;                  // a chunk's Miller values and final-exponentiation slots
    uint4 *sdesc = nullptr;            // resolve: level 2's descriptors, out; search / copy: the entries' own, in
    u32 *gamma = nullptr;              // resolve: the failed groups' values, out; search: in; copy: the rows to fill
    u32 *wsum = nullptr;               // the weighted sums for level 2, out (CommonCoin at level 1)
    uint8_t *cval = nullptr;           // the census singles' validity, out
};
// the group sums / singles of a level's desc list -> gpts (k_*_rlc_sum)
// the CommonCoin level sums on two lanes per group (1) or one (0: k_batch.hip); LCB_TS_SUM2 (with LCB_ALLOW_TUNING=1)
// overrides it for A/B runs
std::atomic<int> g_ts_sum2{[] {
    const char *e = getenv("LCB_TS_SUM2");
    return (e && env_on("LCB_ALLOW_TUNING")) ? atoi(e) : 1;
}()};
// (census: the CommonCoin census's 256-register copies, k_prep.hip)
void rlc_sum_enqueue(const RlcKindInfo &K, RlcWs &w, const RlcBufs &L, u32 groups, bool first, uint8_t *d_accept,
                     size_t n, RlcIo io, hipStream_t s, bool census = false) {
    const u32 *susp = w.susp;
    if (K.ts && census)
        lcbk_ts_rlc_sum_census(dim3(nblk(groups)), s, L.desc, groups, first, K.okv, K.keys, (u32)K.n_keys, io.d_key,
                               io.d_pts, w.rA, w.rB, (u32)n, L.gpts, d_accept, L.gex, L.wsum, susp, L.cval);
    else if (K.ts && g_ts_sum2.load())          // two lanes per group (k_prep.hip)
        lcbk_ts_rlc_sum2(s, L.desc, groups, first, K.okv, K.keys, (u32)K.n_keys, io.d_key, io.d_pts, w.rA, w.rB, (u32)n,
                         L.gpts, d_accept, L.gex, L.wsum, susp, L.cval);
    else if (K.ts)
        lcbk_ts_rlc_sum(dim3(nblk(groups)), s, L.desc, groups, first, K.okv, K.keys, (u32)K.n_keys, io.d_key, io.d_pts,
                        w.rA, w.rB, (u32)n, L.gpts, d_accept, L.gex, L.wsum, susp, L.cval);
    else
        // four lanes per group while the level is latency-bound, one when it is large (e.g. all singles)
        lcbk_tpke_rlc_sum(dim3(nblk((groups <= 262144 ? 4 : 1) * (size_t)groups)), s, L.desc, groups,
                          groups <= 262144 ? 4u : 1u, K.okv, K.ctg2, K.keys, (u32)K.n_keys, io.d_key,
                          io.d_pts, w.rA, w.rB, (u32)n, L.gpts, d_accept, L.gex, L.wsum, susp, L.cval);
}
// Stage dump of the TPKE two-error search (test hook, LCB_ALLOW_TEST_HOOKS=1 and LCB_DUMP_SEARCH2B=<path prefix>):
// before ("in") and after ("out") k_tpke_rlc_search2b, the open list, gamma_0 rows, gamma_c / gamma_t rows and the accept
// bytes go to <prefix>.<stage>.<call>.bin — the header {ns, n_open, n, by_position} then the four arrays
std::atomic<int> g_dump_calls{0};
// Diagnostic builds (-DLCB_SEARCH2B_DEBUG=1) also record per (open check, lane) fingerprints inside the kernel: the
// "in" stage returns the record buffer (set on the kernel), the "out" stage appends it to its file and frees it.
void *search2b_dump(hipStream_t s, const char *stage, u32 ns, u32 no, const u32 *gamma, const u32 *g12, const u32 *open,
                    const uint8_t *d_accept, size_t n, void *dbg = nullptr) {
    const char *pre = getenv("LCB_DUMP_SEARCH2B");
    if (!pre || !*pre || !env_on("LCB_ALLOW_TEST_HOOKS")) return nullptr;
    if (hipStreamSynchronize(s) != hipSuccess) return nullptr;
    std::vector<u32> rec;
    if (stage[0] == 'o' && dbg) {
        rec.resize((size_t)no * 32 * 8);
        hipMemcpy(rec.data(), dbg, 4 * rec.size(), hipMemcpyDeviceToHost);
        lcbk_search2b_debug(nullptr);
        hipFree(dbg);
    }
    std::vector<u32> op(no + 4), g0((size_t)ns * 144), gg(2 * (size_t)ns * 144);
    std::vector<uint8_t> acc(n);
    hipMemcpy(op.data(), open, 4 * (no + 4), hipMemcpyDeviceToHost);
    hipMemcpy(g0.data(), gamma, 4 * g0.size(), hipMemcpyDeviceToHost);
    hipMemcpy(gg.data(), g12, 4 * gg.size(), hipMemcpyDeviceToHost);
    hipMemcpy(acc.data(), d_accept, n, hipMemcpyDeviceToHost);
    const int call = stage[0] == 'i' ? g_dump_calls.fetch_add(1) : g_dump_calls.load() - 1;
    char path[512];
    snprintf(path, sizeof path, "%s.%s.%d.bin", pre, stage, call);
    FILE *fh = fopen(path, "wb");
    if (!fh) return nullptr;
    const u32 hdr[4] = {ns, no, (u32)n, (u32)lcbk_search2b_by_position()};
    fwrite(hdr, 4, 4, fh);
    fwrite(op.data(), 4, op.size(), fh);
    fwrite(g0.data(), 4, g0.size(), fh);
    fwrite(gg.data(), 4, gg.size(), fh);
    fwrite(acc.data(), 1, acc.size(), fh);
    if (!rec.empty()) fwrite(rec.data(), 4, rec.size(), fh);
    fclose(fh);
    void *buf = nullptr;
    if (stage[0] == 'i' && hipMalloc(&buf, (size_t)no * 32 * 8 * 4) == hipSuccess) {
        hipMemset(buf, 0xff, (size_t)no * 32 * 8 * 4);
        if (lcbk_search2b_debug(buf) != 0) { hipFree(buf); buf = nullptr; }
    }
    return buf;
}
// The level-1 pair stage of the TPKE batch check (k_tpke.hip "level-1 pair stage"): one final exponentiation per pair
// of randomized groups instead of one per group.  lcb_set_fe_pair_min: chunks of at least this many entries take it;
// 0 = never, UINT32_MAX (the default) = more entries than lcb_set_coop_max's value, the chunks that would otherwise
// take the one-lane final-exponentiation kernel (smaller, latency-bound levels keep their single pass).
std::atomic<uint32_t> g_fe_pair_min{UINT32_MAX};
bool fe_pair_wanted(size_t m) {
    const uint32_t v = g_fe_pair_min.load(), cm = g_coop_max.load();
    if (v == 0 || m < 2) return false;
    if (v != UINT32_MAX) return m >= v;
    return cm != UINT32_MAX && m > cm;
}
// the final exponentiations of a chunk's m entries (f: their Miller values, gacc: their pre-flags) in two passes: the
// products of the pairs and the other entries, then, after one read of the count, the first member of every pair that
// failed; leaves gacc and the failed entries' rows of f as the single pass does.  Each pass runs on the kernel its own
// count selects (lcb_set_coop_max's rule, or lcb_set_busy_coop_max's when the call is overlapped: fe_one_lane).
struct FePairWs {                  // the job lists in RLC_PAIR_LISTS: one allocation, the u32 arrays first
    u32 *cnt, *list, *p2idx;       // k_fe_pair_list's four counters, pass 2's jobs, each job's place among them
    uint8_t *kind, *pacc, *pacc2;  // per job: its kind and pass 1's flag; per pass-2 entry: its flag
    static size_t bytes(u32 jobs) { return 16 + (size_t)jobs * (4 + 4 + 1 + 1 + 1); }
    explicit FePairWs(void *p, u32 jobs)
        : cnt((u32 *)p), list(cnt + 4), p2idx(list + jobs), kind((uint8_t *)(p2idx + jobs)), pacc(kind + jobs),
          pacc2(pacc + jobs) {}
};
bool rlc_fe_pairs(lcb_ctx *c, const uint8_t *desc, u32 *f, u32 m, uint8_t *gacc, hipStream_t s) {
    const u32 jobs = (m + 1) / 2;
    const size_t park_words = (size_t)jobs * 144 * (size_t)lcbk_fe_slots();
    // pass 1's slots, then pass 2's: sized for the worst case (every job listed) so that no allocation follows the
    // count's read
    u32 *park = (u32 *)c->rlc[RLC_PAIR_PARK].get(2 * park_words * 4);
    void *lists = c->rlc[RLC_PAIR_LISTS].get(FePairWs::bytes(jobs));
    if (!park || !lists) { set_err("device allocation failed (pair stage)"); return false; }
    u32 *park2 = park + park_words;
    const FePairWs ws(lists, jobs);
    hipMemsetAsync(ws.cnt, 0, 16, s);
    lcbk_fe_pair_pack(s, desc, f, m, park, jobs, ws.kind, ws.pacc, c->rlc_pos_exp ? 1u : 0u);
    fe_dispatch(c, s, park, jobs, ws.pacc, true);
    lcbk_fe_pair_list(s, ws.kind, ws.pacc, jobs, ws.list, ws.p2idx, ws.cnt);
    enum { H_PASS2, H_FORMED, H_FAILED, H_N };    // the counters read back
    u32 h[H_N] = {};
    if (!launch_ok("batched verify launch") || !read_counts(h, ws.cnt, H_N, s)) return false;
    const u32 n2 = h[H_PASS2];
    if (n2 > jobs) { set_err("batched verify: pair stage count"); return false; }
    if (n2) {
        lcbk_fe_pair_gather(s, f, m, ws.list, n2, park2, ws.pacc2);
        fe_dispatch(c, s, park2, n2, ws.pacc2, true);
    }
    lcbk_fe_pair_finish(s, f, m, park, jobs, ws.kind, ws.pacc, ws.p2idx, park2, n2, gacc);
    c->fe_pair[FE_PAIRS_FORMED] += h[H_FORMED];
    c->fe_pair[FE_PAIRS_FAILED] += h[H_FAILED];
    c->fe_pair[FE_PASS1_JOBS] += jobs;
    c->fe_pair[FE_PASS2_JOBS] += n2;
    return true;
}
// Miller + final exponentiation (+ resolve / search) over the `count` entries of L.desc in chunks; L.gpts holds their
// points.  RLC_COPY parks the values in L.gamma's rows (copy_map: the rows, or entry order)
enum RlcStage { RLC_RESOLVE = 0, RLC_SEARCH = 1, RLC_COPY = 2 };   // after a chunk's checks: resolve / search / copy out
bool rlc_checks(lcb_ctx *c, const RlcKindInfo &K, RlcWs &w, const RlcBufs &L, u32 count, RlcStage stage, bool first,
                uint8_t *d_accept, RlcIo io, hipStream_t s, const u32 *copy_map = nullptr, bool census = false) {
    hipEvent_t *ev = c->rlc_lev_ev;
    const bool tsc = census && K.ts;      // the CommonCoin census: the 256-register copies (k_prep.hip)
    // small levels (below one wave per SIMD as one check per lane): nine lanes per check (k_coop.hip).  A TPKE chunk of
    // at most coop_ml_max checks takes the cooperative Miller kernel; every chunk but the last is a full one, so the
    // last is the smallest.  The kernel's fallback flags: one buffer for the call, sized for the largest such chunk
    const u32 coop_ml_max = g_coop_miller_max.load();
    const size_t full = std::min<size_t>(count, LCB_VERIFY_CHUNK);
    const size_t last = count % LCB_VERIFY_CHUNK ? count % LCB_VERIFY_CHUNK : full;
    uint8_t *mfb = nullptr;
    if (!K.ts && last <= coop_ml_max) {
        mfb = (uint8_t *)c->rlc[RLC_MFB].get(std::min<size_t>(full, coop_ml_max));
        if (!mfb) { set_err("device allocation failed (Miller fallback flags)"); return false; }
    }
    float t;
    for (size_t o = 0; o < count; o += LCB_VERIFY_CHUNK) {
        const size_t m = count - o < LCB_VERIFY_CHUNK ? count - o : LCB_VERIFY_CHUNK;
        const uint8_t *desc = L.desc + 16 * o, *gpts = (const uint8_t *)L.gpts + K.rec * o;
        hipEventRecord(ev[1], s);
        // (the final exponentiation's form also depends on the batches in flight: fe_one_lane)
        const bool pairs = stage == RLC_RESOLVE && first && !K.ts && !census && fe_pair_wanted(m);
        if (tsc)
            lcbk_ts_rlc_miller_census(dim3(nblk(m)), s, K.lines, desc, gpts, (u32)m, L.f, L.gacc + o);
        else if (K.ts)
            lcbk_ts_rlc_miller(dim3(nblk(m)), s, K.lines, desc, gpts, (u32)m, L.f, L.gacc + o);
        else if (m <= coop_ml_max)
            lcbk_coop_tpke_miller(s, K.lines, desc, gpts, (u32)m, L.f, L.gacc + o, mfb, 2, K.fb ? 1 : 0);
        else
            lcbk_tpke_rlc_miller(dim3(nblk(m)), s, K.lines, desc, gpts, (u32)m, L.f, L.gacc + o);
        hipEventRecord(ev[2], s);
        if (pairs) {                      // (the time of both passes, with the count's read between them)
            if (!rlc_fe_pairs(c, desc, L.f, (u32)m, L.gacc + o, s)) return false;
        } else {
            fe_dispatch(c, s, L.f, m, L.gacc + o, !K.ts && !census);
        }
        hipEventRecord(ev[3], s);
        if (stage == RLC_COPY)
            lcbk_rlc_park_copy(s, L.f, (u32)o, (u32)m, L.gamma, copy_map);
        else if (stage == RLC_SEARCH)
            lcbk_rlc_search(dim3(nblk(m)), s, L.sdesc, (u32)o, (u32)m, L.gamma, L.f, d_accept, w.dB, w.cnt + CNT_NEXT,
                            io.d_key, (u32)K.n_keys, w.susp);
        else
            lcbk_rlc_resolve(dim3(nblk(m)), s, L.desc, (u32)o, (u32)m, L.gacc, L.gex, L.f, first ? 1u : 0u, d_accept,
                             w.dB, w.cnt + CNT_NEXT, L.sdesc, w.cnt + CNT_SEARCH, L.gamma, io.d_key, (u32)K.n_keys,
                             w.susp);
        if (hipEventSynchronize(ev[3]) == hipSuccess) {
            if (hipEventElapsedTime(&t, ev[1], ev[2]) == hipSuccess) c->rlc_ms[MS_MILLER] += t;
            if (hipEventElapsedTime(&t, ev[2], ev[3]) == hipSuccess) c->rlc_ms[MS_FINAL_EXP] += t;
        }
    }
    return true;
}
// the census (SURVEY-style Byzantine validators, k_batch.hip "suspect keys"): exact single checks of shares [0, m),
// then the suspect-key bitmap and its count (the CNT_SUSPECTS word); everything stays on the device (no host read)
int rlc_census(lcb_ctx *c, RlcKind kind, RlcWs &w, uint8_t *d_accept, RlcIo io, hipStream_t s) {
    if (!w.m) return 0;
    RlcKindInfo K = rlc_kind(c, kind);
    if (!K.ts) K.fb = lines_unnormalised(c, c->unn_census);    // waits for the census ciphertexts' line sets
    const u32 m = w.m;
    // the census uses dB as its desc list (dA is the level-1 list being built on the second stream)
    RlcBufs L;
    L.desc = w.dB;
    L.gpts = c->rlc[RLC_GPTS].get((size_t)m * K.rec);
    L.gacc = (uint8_t *)c->rlc[RLC_GACC].get(m);
    L.gex = (uint8_t *)c->rlc[RLC_GEX].get(m);
    L.cval = (uint8_t *)c->rlc[RLC_CVAL].get(m);
    L.f = (u32 *)c->t_f.get((size_t)m * 576 * (size_t)lcbk_fe_slots());
    if (!L.gpts || !L.gacc || !L.gex || !L.cval || !L.f) { set_err("device allocation failed"); return -1; }
    lcbk_rlc_census_desc(s, io.d_grp, io.d_key, m, (u32)K.n_grp, (u32)K.n_keys, w.dB, d_accept);
    RlcWs cw = w;
    cw.susp = nullptr;                  // the census singles are exact checks whatever the bitmap says
    rlc_sum_enqueue(K, cw, L, m, false, d_accept, m, io, s, true);
    if (!rlc_checks(c, K, cw, L, m, RLC_RESOLVE, false, d_accept, io, s, nullptr, true)) return -1;
    lcbk_rlc_census_stats(s, io.d_key, m, (u32)K.n_keys, L.cval, d_accept, w.susp, w.cnt + CNT_SUSPECTS);
    return launch_ok("batched verify census launch") ? 0 : -1;
}
// a level's sums: `enqueue` between the level events 0 and 1, then the wait and their time into the statistics
template <class F> void timed_sums(lcb_ctx *c, hipStream_t s, F enqueue) {
    hipEvent_t *ev = c->rlc_lev_ev;
    float t;
    hipEventRecord(ev[0], s);
    enqueue();
    hipEventRecord(ev[1], s);
    if (hipEventSynchronize(ev[1]) == hipSuccess && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess)
        c->rlc_ms[MS_SUMS] += t;
}
// the next level opens with `size` entries: its statistics slot and the level count
void level_open(lcb_ctx *c, int &lev, u32 size) {
    if (++lev < 8) c->rlc_levels[lev] = size;
    c->rlc_nlev = lev + 1;
}
// phase 2 (after the preparation and the randomisation): level 1 group checks (with suspect keys: the groups summed
// over the other keys, every share of a suspect key as an exact single); level 2: weighted re-check + search of the
// failed groups; then single checks
int rlc_levels(lcb_ctx *c, RlcKind kind, RlcWs &w, uint8_t *d_accept, size_t n, RlcIo io, hipStream_t s) {
    RlcKindInfo K = rlc_kind(c, kind);
    u32 cnt[CNT_N] = {};
    for (auto &m : c->rlc_ms) m = 0.0f;
    for (auto &v : c->fe_pair) v = 0;
    for (auto &v : c->lvl_kernel) v = 0;
    if (!read_counts(cnt, w.cnt, CNT_SUSPECTS + 1, s)) return -1;
    if (!K.ts) K.fb = lines_unnormalised(c, 1) || (c->unn_census == 0 && lines_unnormalised(c, 0));
    u32 groups = cnt[CNT_GROUPS];
    c->rlc_census[CENSUS_SUSPECTS] = cnt[CNT_SUSPECTS];
    c->rlc_census[CENSUS_GROUPS] = c->rlc_census[CENSUS_ENTRIES] = groups;
    if (cnt[CNT_SUSPECTS] && groups) {  // suspect keys: split their shares out of the level-1 groups
        lcbk_rlc_suspect_split(s, w.dA, groups, io.d_key, (u32)K.n_keys, w.susp, d_accept, w.dB, w.cnt + CNT_SPLIT);
        if (!launch_ok("batched verify launch") || !read_counts(cnt + CNT_SPLIT, w.cnt + CNT_SPLIT, 1, s)) return -1;
        groups = cnt[CNT_SPLIT];
        c->rlc_census[CENSUS_ENTRIES] = groups;
        std::swap(w.dA, w.dB);
    } else {
        w.susp = nullptr;               // no suspect key: the sums need not test the bitmap
    }
    for (int lev = -1; groups;) {
        if (lev + 1 > 40) { set_err("batched verify: group splitting did not terminate"); return -1; }
        level_open(c, lev, groups);
        const bool first = lev == 0;
        const size_t nf = groups < LCB_VERIFY_CHUNK ? groups : LCB_VERIFY_CHUNK;
        RlcBufs L;
        L.desc = w.dA;
        L.gpts = c->rlc[RLC_GPTS].get((size_t)groups * K.rec);
        L.gacc = (uint8_t *)c->rlc[RLC_GACC].get(groups);
        L.gex = (uint8_t *)c->rlc[RLC_GEX].get(groups);
        L.f = (u32 *)c->t_f.get(nf * 576 * (size_t)lcbk_fe_slots());
        if (first) {
            L.sdesc = (uint4 *)c->rlc[RLC_SDESC].get((size_t)groups * 16 * (K.ts ? 1 : 2));
            L.gamma = (u32 *)c->rlc[RLC_GAMMA].get((size_t)groups * 576);
            if (K.ts) L.wsum = (u32 *)c->rlc[RLC_WSUM].get((size_t)groups * K.wrec);   // (TPKE: formed at level 2)
        }
        if (!L.gpts || !L.gacc || !L.gex || !L.f || (first && (!L.sdesc || !L.gamma || (K.ts && !L.wsum)))) {
            set_err("device allocation failed");
            return -1;
        }
        uint4 *const sdesc = L.sdesc;
        u32 *const gamma = L.gamma;
        hipMemsetAsync(w.cnt + CNT_NEXT, 0, 8, s);      // CNT_NEXT and CNT_SEARCH
        timed_sums(c, s, [&] { rlc_sum_enqueue(K, w, L, groups, first, d_accept, n, io, s); });
        if (!rlc_checks(c, K, w, L, groups, RLC_RESOLVE, first, d_accept, io, s)) return -1;
        if (!launch_ok("batched verify launch")) return -1;
        if (!read_counts(cnt, w.cnt, CNT_SEARCH + 1, s)) return -1;
        if (first && cnt[CNT_SEARCH] && !K.ts) {  // TPKE level 2: weighted re-check per failed group, one-error search,
            // then for the groups it leaves open a second weighted check and the two-error location
            const u32 ns = cnt[CNT_SEARCH];
            level_open(c, lev, ns);
            const size_t nf2 = ns < LCB_VERIFY_CHUNK ? ns : LCB_VERIFY_CHUNK;
            RlcBufs L2;
            L2.desc = (const uint8_t *)sdesc;
            L2.sdesc = sdesc;
            L2.gpts = c->rlc[RLC_GPTS].get((size_t)ns * K.rec);
            L2.gacc = (uint8_t *)c->rlc[RLC_GACC].get(ns);
            u32 *g12 = (u32 *)c->rlc[RLC_G12].get(2 * (size_t)ns * 576);
            L2.gamma = g12;                             // this pass fills the gamma_c rows
            L2.f = (u32 *)c->t_f.get(nf2 * 576 * (size_t)lcbk_fe_slots());
            u32 *open = (u32 *)c->rlc[RLC_OPEN].get((size_t)ns * 4 + 16);
            if (!L2.gpts || !L2.gacc || !g12 || !L2.f || !open) { set_err("device allocation failed"); return -1; }
            timed_sums(c, s, [&] {
                lcbk_tpke_rlc_wsum2(s, sdesc, ns, nullptr, w.rA, w.rB, (u32)n, io.d_key, (u32)K.n_keys, w.susp, L2.gpts,
                                    nullptr);
            });
            if (!rlc_checks(c, K, w, L2, ns, RLC_COPY, false, d_accept, io, s)) return -1;
            lcbk_tpke_rlc_search2a(s, sdesc, ns, gamma, g12, d_accept, open + 4, open);
            u32 no = 0;
            if (!launch_ok("batched verify launch") || !read_counts(&no, open, 1, s)) return -1;
            if (no) {
                level_open(c, lev, no);
                // sdesc[ns, 2 ns) is free (sized for two entries per level-1 group): the open groups' descriptors
                timed_sums(c, s, [&] {
                    lcbk_tpke_rlc_wsum2(s, sdesc, no, open + 4, w.rA, w.rB, (u32)n, io.d_key, (u32)K.n_keys, w.susp,
                                        L2.gpts, sdesc + ns);
                });
                L2.desc = (const uint8_t *)(sdesc + ns);
                L2.sdesc = sdesc + ns;
                L2.gamma = g12 + (size_t)ns * 144;      // gamma_t of open group g -> row ns + g
                if (!rlc_checks(c, K, w, L2, no, RLC_COPY, false, d_accept, io, s,
                                lcbk_search2b_by_position() ? nullptr : open + 4))
                    return -1;
                void *dbg = search2b_dump(s, "in", ns, no, gamma, g12, open, d_accept, n);
#if LCB_SEARCH2B_ASM
                u32 *s2b_park = (u32 *)c->rlc[RLC_S2B_PARK].get(lcbk_tpke_rlc_search2b_asm_park_bytes(no));
                if (!s2b_park) { set_err("device allocation failed (level-2 search slots)"); return -1; }
                lcbk_tpke_rlc_search2b_asm(s, sdesc, ns, no, gamma, g12, open + 4, open, d_accept, w.dB,
                                           w.cnt + CNT_NEXT, io.d_key, (u32)K.n_keys, w.susp, s2b_park);
#else
                lcbk_tpke_rlc_search2b(s, sdesc, ns, no, gamma, g12, open + 4, open, d_accept, w.dB, w.cnt + CNT_NEXT,
                                       io.d_key, (u32)K.n_keys, w.susp);
#endif
                search2b_dump(s, "out", ns, no, gamma, g12, open, d_accept, n, dbg);
            }
            if (!launch_ok("batched verify launch")) return -1;
            if (!read_counts(cnt + CNT_NEXT, w.cnt + CNT_NEXT, 1, s)) return -1;
        } else if (first && cnt[CNT_SEARCH]) {    // level 2: weighted re-check of the failed groups, then the search
            const u32 ns = cnt[CNT_SEARCH];
            level_open(c, lev, ns);
            RlcBufs L2 = L;                       // (ns <= groups: the level-1 buffers are large enough)
            L2.desc = (const uint8_t *)sdesc;
            L2.gex = nullptr;
            L2.gpts = c->rlc[RLC_GPTS].get((size_t)ns * K.rec);
            timed_sums(c, s, [&] {
                if (K.ts) lcbk_ts_rlc_wsum(dim3(nblk(ns)), s, sdesc, ns, L.wsum, groups, L2.gpts);
                else lcbk_tpke_rlc_wsum(dim3(nblk(ns)), s, sdesc, ns, L.wsum, groups, L2.gpts);
            });
            if (!rlc_checks(c, K, w, L2, ns, RLC_SEARCH, false, d_accept, io, s)) return -1;
            if (!launch_ok("batched verify launch")) return -1;
            if (!read_counts(cnt + CNT_NEXT, w.cnt + CNT_NEXT, 1, s)) return -1;
        }
        groups = cnt[CNT_NEXT];
        std::swap(w.dA, w.dB);            // the next level's groups
    }
    hipEventRecord(c->rlc_ev[2], s);
    c->rlc_ran = true;
    // the calling thread's copy of the statistics (lcb_tpke_batched_stats without a context)
    RlcStats &st = t_rlc_stats;
    st.valid = hipEventSynchronize(c->rlc_ev[2]) == hipSuccess;
    if (st.valid && c->prep_timed && hipEventElapsedTime(&c->rlc_ms[MS_PREP], c->prep_ev[0], c->prep_ev[1]) != hipSuccess)
        c->rlc_ms[MS_PREP] = -1.0f;
    if (st.valid && c->prep_timed && getenv("LCB_PREP_TRACE")) {       // diagnostics: hashing / line sets + census
        float a = -1.0f, b = -1.0f;
        hipEventElapsedTime(&a, c->prep_ev[0], c->prep_ev[2]);
        hipEventElapsedTime(&b, c->prep_ev[2], c->prep_ev[1]);
        fprintf(stderr, "prep_trace hash %.2f lines+census %.2f ms\n", a, b);
    }
    st.nlev = c->rlc_nlev;
    for (int i = 0; i < 8; i++) st.levels[i] = i < c->rlc_nlev ? c->rlc_levels[i] : 0;
    for (int i = 0; i < 2; i++)
        if (!st.valid || hipEventElapsedTime(&st.ms[i], c->rlc_ev[i], c->rlc_ev[i + 1]) != hipSuccess) st.ms[i] = -1.0f;
    for (int i = 0; i < RLC_MS_N; i++) st.ms[2 + i] = c->rlc_ms[i];
    for (int i = 0; i < CENSUS_N; i++) st.census[i] = c->rlc_census[i];
    for (int i = 0; i < FE_PAIR_N; i++) st.fe_pair[i] = c->fe_pair[i];
    return launch_ok("batched verify launch") ? 0 : -1;
}
int tpke_verify_prepared_rlc(lcb_ctx *c, uint8_t *d_accept, size_t n, size_t n_keys, size_t n_cts, const uint32_t *d_ct,
                             const uint32_t *d_dec, const uint8_t *d_ui, hipStream_t s) {
    if (!tpke_shape_ok(c, n_keys, n_cts, "tpke batched verify")) return -1;
    if (n > 0xffffffffu) { set_err("tpke batched verify: batch too large"); return -1; }
    c->rlc_nlev = 0;
    if (!n) return 0;
    RlcWs w;
    const RlcIo io{d_dec, d_ui, d_ct};
    if (!rlc_ws(c, w, n, LCB_G1_JAC_BYTES, LCB_G1_JAC_BYTES, n_keys, census_size(n, n_keys), s)) return -1;
    if (rlc_census(c, RLC_TPKE, w, d_accept, io, s)) return -1;   // before the randomisation: suspects skip it
    if (rlc_points_enqueue(c, w, d_accept, n, n_keys, n_cts, d_ct, d_dec, d_ui, s)) return -1;
    return rlc_levels(c, RLC_TPKE, w, d_accept, n, io, s);
}
bool fork_ready(lcb_ctx *c) {
    if (c->fork_ready) return true;
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->hi, hipStreamNonBlocking, greatest);
    for (auto &ev : c->fork_ev)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    for (auto &ev : c->prep_ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e != hipSuccess) { set_err("batched verify: stream creation", e); return false; }
    c->fork_ready = true;
    return true;
}
// fork mode 0's second normal-priority stream, created on first use
bool aux_ready(lcb_ctx *c) {
    if (c->aux) return true;
    hipError_t e = hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking);
    if (e != hipSuccess) { c->aux = nullptr; set_err("batched verify: stream creation", e); return false; }
    return true;
}
// fork mode 3's two more preparation streams, created on first use: HIP hands every stream a hardware queue when it
// is created (GPU_MAX_HW_QUEUES per priority, shared round-robin beyond that), so streams a context never uses would
// still crowd the other contexts' queues
bool split_ready(lcb_ctx *c) {
    if (c->hi2) return true;
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->hi2, hipStreamNonBlocking, greatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&c->hi3, hipStreamNonBlocking, greatest);
    if (e != hipSuccess) { set_err("batched verify: stream creation", e); return false; }
    return true;
}
// The stream layout of the fused calls (lcb_set_fork_mode).  Mode 0: randomisation on the second stream, preparation +
// census on the caller's; mode >= 1 (hp): the latency-bound preparation chain (one lane per ciphertext / message / line
// set, < 1.5 waves per SIMD) on a high-priority stream, so its waves are dispatched ahead of the randomisation's 16 K
// waves, which run on the caller's stream (s: the caller's stream, sr: the randomisation's, sp: the preparation's).
// Fork from the caller's stream: the other stream starts behind everything enqueued on s so far; timed: the stream
// on which the preparation chain's time starts here (null: not timed, or the fused TPKE call started it earlier)
void fork_from_caller(lcb_ctx *c, hipStream_t s, hipStream_t other, hipStream_t timed) {
    hipEventRecord(c->fork_ev[0], s);
    hipStreamWaitEvent(other, c->fork_ev[0], 0);
    if (timed) hipEventRecord(c->prep_ev[0], timed);
}
// join back: the caller's stream continues behind the preparation chain (hp; its time ends here) or behind the
// randomisation (fork_ev[1], recorded by the caller after it; only a call with shares has one)
void join_caller(lcb_ctx *c, hipStream_t s, hipStream_t sp, bool hp, bool shares) {
    if (hp) {
        hipEventRecord(c->prep_ev[1], sp);
        c->prep_timed = true;
        hipEventRecord(c->fork_ev[1], sp);
    }
    if (hp || shares) hipStreamWaitEvent(s, c->fork_ev[1], 0);
}
// randomized batch form of ts_verify_prepared (k_batch.hip): groups = runs of one message (<= 128 shares)
int ts_verify_prepared_rlc(lcb_ctx *c, uint8_t *d_accept, size_t n, size_t n_pks, size_t n_msgs, const uint8_t *d_sigs,
                           const uint32_t *d_midx, const uint32_t *d_pidx, hipStream_t s) {
    if (!ts_shape_ok(c, n_pks, n_msgs, "ts batched verify")) return -1;
    if (n > 0xffffffffu) { set_err("ts batched verify: batch too large"); return -1; }
    c->rlc_nlev = 0;
    if (!n) return 0;
    RlcWs w;
    const RlcIo io{d_pidx, d_sigs, d_midx};
    if (!rlc_ws(c, w, n, LCB_G1_JAC_BYTES, LCB_G2_JAC_BYTES, n_pks, census_size(n, n_pks), s)) return -1;
    if (rlc_census(c, RLC_TS, w, d_accept, io, s)) return -1;
    if (ts_rlc_points_enqueue(c, w, d_accept, n, n_pks, n_msgs, d_sigs, d_midx, d_pidx, s)) return -1;
    return rlc_levels(c, RLC_TS, w, d_accept, n, io, s);
}

}  // namespace

// prepare + batched verify in one call: the randomisation (needs only the keys) runs on the context's second
// stream beside the per-ciphertext hashing / line sets and the census (latency-bound: < 1 wave per SIMD for 50 K
// ciphertexts); a key the census marks suspect before the randomisation reaches its shares skips them
int lcb_int::tpke_verify_shares_rlc_fused(lcb_ctx *c, uint8_t *d_accept, size_t n, const uint8_t *d_y, size_t n_keys,
                                          const uint8_t *d_u, const uint8_t *d_w, const uint8_t *d_v,
                                          const uint32_t *d_voff, size_t n_cts, const uint32_t *d_ct,
                                          const uint32_t *d_dec, const uint8_t *d_ui, hipStream_t s) {
    const BatchedInflight counted(c);          // until this call returns: the level driver's overlap rule (fe_one_lane)
    if (n_cts > 0xffffffffu || n_keys > 0xffffffffu || n > 0xffffffffu) { set_err("tpke batched verify: batch too large"); return -1; }
    c->t_ready = false;
    c->unn_set[0] = c->unn_set[1] = false;     // the fallback flags describe the line sets prepared below
    c->rlc_nlev = 0;
    u32 *lines = (u32 *)c->t_lines.get((size_t)n_cts * 2 * LCB_LINESET_BYTES);
    uint8_t *ctok = (uint8_t *)c->t_ctok.get(n_cts);
    void *keys = c->t_keys.get(n_keys * LCB_G1A_ST_BYTES);
    uint8_t *ctg2 = (uint8_t *)c->t_ctg2.get(n_cts);     // from the line sets (k_lineset_fill)
    if (!lines || !ctok || !keys || !ctg2) { set_err("device allocation failed"); return -1; }
    if (!fork_ready(c)) return -1;
    const int fm = g_fork_mode.load();
    const bool hp = fm >= 1, prep_first = fm >= 2 && n_cts, split = fm >= 3, one_hi = fm == 4;
    // split mode with a census: the ciphertexts of the census shares [0, m) (indices read to the host before this call
    // launches anything; used when they all lie below a small bound c_early) are prepared first, on the preparation
    // stream, so the census runs while the bulk is prepared
    u32 c_early = 0;
    const u32 m_census = n ? census_size(n, n_keys) : 0;
    if (n_cts && split && !one_hi && m_census) {
        std::vector<uint32_t> ci(m_census);
        if (hipMemcpyAsync(ci.data(), d_ct, 4 * (size_t)m_census, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) { set_err("tpke batched verify: census index read"); return -1; }
        u32 mx = 0;
        for (uint32_t x : ci) mx = std::max(mx, x);
        if ((size_t)mx + 1 < n_cts && mx < 4096u) c_early = mx + 1;
    }
    const int fl = prepare_flags();
    // the census ciphertexts' decode + hash needs no key: it starts before the keys' decompression and tables (≈ 2 ms
    // on an otherwise idle device in a single batch), ordered after the context's earlier work like the caller's stream
    // (c_early is set in split mode only, whose preparation stream is c->hi)
    const bool early = c_early != 0;
    if (early) {
        hipEventRecord(c->fork_ev[4], s);
        hipStreamWaitEvent(c->hi, c->fork_ev[4], 0);
        hipEventRecord(c->prep_ev[0], c->hi);
        lcbk_tpke_ct_prepare_w64(c->hi, d_u, d_w, d_v, d_voff, c_early, lines, ctok, fl);
    }
    if (n_keys) lcbk_g1_decompress(dim3(nblk(n_keys)), s, d_y, (u32)n_keys, keys);
    RlcWs w;
    const RlcIo io{d_dec, d_ui, d_ct};
    if (!hp && !aux_ready(c)) return -1;
    const hipStream_t sr = hp ? s : c->aux, sp = hp ? c->hi : s;
    if (n) {
        if (!rlc_ws(c, w, n, LCB_G1_JAC_BYTES, LCB_G1_JAC_BYTES, n_keys, m_census, s)) return -1;
        keys_first_tables(c, w, keys, n_keys, n, s);
    }
    if (n || hp) fork_from_caller(c, s, hp ? sp : sr, hp && !early ? sp : nullptr);
    if (n) {
        if (!prep_first && rlc_points_enqueue(c, w, d_accept, n, n_keys, n_cts, d_ct, d_dec, d_ui, sr)) return -1;
        if (!hp) hipEventRecord(c->fork_ev[1], sr);
    }
    if (n_cts && split) {
        // split preparation: hash + H's line set per lane, U / W decompression + W's line set (and its G2 flag) per
        // lane, on separate high-priority streams; each lane keeps its SIMD from the hash to the last line, so no
        // second dispatch waits behind the randomisation's waves.  With c_early: ciphertexts [0, c_early) first
        // (one decode + hash lane each, then their line sets on the five-lane kernel, then the census, all on the
        // preparation stream), the rest [c_early, n_cts) beside them on the second and third streams.
        uint8_t *hok = (uint8_t *)c->rlc[RLC_HOK].get(n_cts);
        if (!hok) { set_err("device allocation failed"); return -1; }
        const u32 nc = (u32)n_cts;
        if (one_hi) {
            // fork mode 4: both lane kinds in one dispatch on the context's one high-priority stream, then the census
            // behind it on the same stream; a context holds one queue per priority, so three batches in flight fit
            // the box's GPU_MAX_HW_QUEUES = 4
            lcbk_tpke_ct_prepare_hw(sp, d_u, d_w, d_v, d_voff, nc, lines, hok, ctok, ctg2, fl);
            hipEventRecord(c->prep_ev[2], sp);
            if (n && rlc_points_enqueue(c, w, d_accept, n, n_keys, n_cts, d_ct, d_dec, d_ui, sr)) return -1;
            lcbk_ct_ok_merge(sp, ctok, hok, 0, nc);
            lines_flag_enqueue(c, 1, lines, 0, nc, sp);
            c->unn_census = 1;
        } else {
        if (!split_ready(c)) return -1;
        hipStreamWaitEvent(c->hi2, c->fork_ev[0], 0);
        hipStreamWaitEvent(c->hi3, c->fork_ev[0], 0);
        const u32 ce = c_early;
        c->unn_census = ce ? 0 : 1;
        if (ce) {                    // the census's ciphertexts (decode + hash per lane launched above): their
                                     // line sets on the five-lane kernel
            lcbk_lineset_coop_2w(sp, lines, 2 * ce, nullptr, ctg2);   // (2 ce <= 8192 sets: lines_fill's coop range)
            lines_flag_enqueue(c, 0, lines, 0, ce, sp);
        }
        lcbk_tpke_ct_prepare_h(c->hi2, d_u, d_v, d_voff, ce, nc, lines, hok, fl);
        lcbk_tpke_ct_prepare_w(c->hi3, d_u, d_w, ce, nc, lines, ctok, ctg2, fl);
        hipEventRecord(c->prep_ev[2], c->hi2);
        if (n && rlc_points_enqueue(c, w, d_accept, n, n_keys, n_cts, d_ct, d_dec, d_ui, sr)) return -1;
        hipEventRecord(c->fork_ev[2], c->hi2);
        hipStreamWaitEvent(c->hi3, c->fork_ev[2], 0);
        lcbk_ct_ok_merge(c->hi3, ctok, hok, ce, nc);
        lines_flag_enqueue(c, 1, lines, ce, nc, c->hi3);
        hipEventRecord(c->fork_ev[3], c->hi3);
        if (!ce) hipStreamWaitEvent(sp, c->fork_ev[3], 0);     // the census (below) needs every ciphertext
        }
    } else if (n_cts) {
        lcbk_tpke_ct_prepare(dim3(nblk(n_cts)), sp, d_u, d_w, d_v, d_voff, (u32)n_cts, lines, ctok, fl, nullptr);
        if (hp) hipEventRecord(c->prep_ev[2], sp);
        if (prep_first && n && rlc_points_enqueue(c, w, d_accept, n, n_keys, n_cts, d_ct, d_dec, d_ui, sr)) return -1;
        lines_fill(sp, lines, 2 * n_cts, nullptr, ctg2);
        c->unn_census = 1;
        lines_flag_enqueue(c, 1, lines, 0, (u32)n_cts, sp);
    }
    if (!launch_ok("tpke prepare launch")) return -1;
    c->t_n_cts = n_cts;
    c->t_n_keys = n_keys;
    c->t_gen++;
    c->t_ready = true;
    if (n && rlc_census(c, RLC_TPKE, w, d_accept, io, sp)) return -1;
    if (n_cts && split && c_early) hipStreamWaitEvent(sp, c->fork_ev[3], 0);   // the bulk's preparation
    join_caller(c, s, sp, hp, n != 0);
    if (!n) return 0;
    return rlc_levels(c, RLC_TPKE, w, d_accept, n, io, s);
}
// prepare + batched verify: the randomisation (keys only) beside the message hashing and the census on the second
// stream
int lcb_int::ts_verify_shares_rlc_fused(lcb_ctx *c, uint8_t *d_accept, size_t n, const uint8_t *d_pks, size_t n_pks,
                                        const uint8_t *d_sigs, const uint8_t *d_msg, const uint32_t *d_moff,
                                        size_t n_msgs, const uint32_t *d_midx, const uint32_t *d_pidx, hipStream_t s) {
    if (n_msgs > 0xffffffffu || n_pks > 0xffffffffu || n > 0xffffffffu) { set_err("ts batched verify: batch too large"); return -1; }
    c->s_ready = false;
    c->rlc_nlev = 0;
    u32 *lines = (u32 *)c->s_lines.get((size_t)n_msgs * LCB_LINESET_BYTES);
    uint8_t *mok = (uint8_t *)c->s_mok.get(n_msgs);
    void *keys = c->s_keys.get(n_pks * LCB_G1A_ST_BYTES);
    if (!lines || !mok || !keys) { set_err("device allocation failed"); return -1; }
    if (!fork_ready(c)) return -1;
    if (n_pks) lcbk_g1_decompress(dim3(nblk(n_pks)), s, d_pks, (u32)n_pks, keys);
    RlcWs w;
    const RlcIo io{d_pidx, d_sigs, d_midx};
    // stream layout as in tpke_verify_shares_rlc_fused (lcb_set_fork_mode; 2 acts as 1 here)
    const bool hp = g_fork_mode.load() >= 1;
    if (!hp && !aux_ready(c)) return -1;
    const hipStream_t sr = hp ? s : c->aux, sp = hp ? c->hi : s;
    if (n) {
        if (!rlc_ws(c, w, n, LCB_G1_JAC_BYTES, LCB_G2_JAC_BYTES, n_pks, census_size(n, n_pks), s)) return -1;
        keys_first_tables(c, w, keys, n_pks, n, s);
    }
    if (n || hp) fork_from_caller(c, s, hp ? sp : sr, hp ? sp : nullptr);
    // the message preparation (latency-bound, one lane per message) is enqueued ahead of the randomisation, so its
    // waves take their SIMD slots before the randomisation's fill the device (round 5: enqueued after it, the
    // preparation ran 462 ms beside a 447 ms randomisation and the census chain waited for it)
    if (n_msgs) lcbk_ts_msg_prepare(dim3(nblk(n_msgs)), sp, d_msg, d_moff, (u32)n_msgs, lines, mok, prepare_flags());
    if (n) {
        if (ts_rlc_points_enqueue(c, w, d_accept, n, n_pks, n_msgs, d_sigs, d_midx, d_pidx, sr)) return -1;
        if (!hp) hipEventRecord(c->fork_ev[1], sr);
    }
    if (!launch_ok("ts prepare launch")) return -1;
    c->s_n_msgs = n_msgs;
    c->s_n_pks = n_pks;
    c->s_gen++;
    c->s_ready = true;
    if (n && rlc_census(c, RLC_TS, w, d_accept, io, sp)) return -1;
    join_caller(c, s, sp, hp, n != 0);
    if (!n) return 0;
    return rlc_levels(c, RLC_TS, w, d_accept, n, io, s);
}

// ================================================================== C ABI: the batched entry points on device
// pointers, their statistics and their knobs (the host-pointer forms are in lcb_host.cpp)
extern "C" int lcb_ctx_tpke_verify_prepared_batched_dev(lcb_ctx *ctx, uint8_t *accept, size_t n, size_t n_keys,
                                                        size_t n_cts, const uint32_t *ct_idx, const uint32_t *dec_idx,
                                                        const uint8_t *ui, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return tpke_verify_prepared_rlc(c, accept, n, n_keys, n_cts, ct_idx, dec_idx, ui, q.s);
}
extern "C" int lcb_ctx_tpke_verify_shares_batched_dev(lcb_ctx *ctx, uint8_t *accept, size_t n, const uint8_t *y_keys,
                                                      size_t n_keys, const uint8_t *cts_u, const uint8_t *cts_w,
                                                      const uint8_t *v_data, const uint32_t *v_off, size_t n_cts,
                                                      const uint32_t *ct_idx, const uint32_t *dec_idx,
                                                      const uint8_t *ui, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return tpke_verify_shares_rlc_fused(c, accept, n, y_keys, n_keys, cts_u, cts_w, v_data, v_off, n_cts, ct_idx,
                                        dec_idx, ui, q.s);
}
extern "C" int lcb_tpke_verify_shares_batched_dev(uint8_t *accept, size_t n, const uint8_t *y_keys, size_t n_keys,
                                                  const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data,
                                                  const uint32_t *v_off, size_t n_cts, const uint32_t *ct_idx,
                                                  const uint32_t *dec_idx, const uint8_t *ui, void *stream) {
    return lcb_ctx_tpke_verify_shares_batched_dev(nullptr, accept, n, y_keys, n_keys, cts_u, cts_w, v_data, v_off,
                                                  n_cts, ct_idx, dec_idx, ui, stream);
}
extern "C" int lcb_tpke_verify_prepared_batched_dev(uint8_t *accept, size_t n, size_t n_keys, size_t n_cts,
                                                    const uint32_t *ct_idx, const uint32_t *dec_idx, const uint8_t *ui,
                                                    void *stream) {
    return lcb_ctx_tpke_verify_prepared_batched_dev(nullptr, accept, n, n_keys, n_cts, ct_idx, dec_idx, ui, stream);
}
extern "C" int lcb_ctx_ts_verify_prepared_batched_dev(lcb_ctx *ctx, uint8_t *accept, size_t n, size_t n_pks,
                                                      size_t n_msgs, const uint8_t *sigs, const uint32_t *msg_idx,
                                                      const uint32_t *pk_idx, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return ts_verify_prepared_rlc(c, accept, n, n_pks, n_msgs, sigs, msg_idx, pk_idx, q.s);
}
extern "C" int lcb_ts_verify_prepared_batched_dev(uint8_t *accept, size_t n, size_t n_pks, size_t n_msgs,
                                                  const uint8_t *sigs, const uint32_t *msg_idx, const uint32_t *pk_idx,
                                                  void *stream) {
    return lcb_ctx_ts_verify_prepared_batched_dev(nullptr, accept, n, n_pks, n_msgs, sigs, msg_idx, pk_idx, stream);
}
extern "C" int lcb_ctx_ts_verify_shares_batched_dev(lcb_ctx *ctx, uint8_t *accept, size_t n, const uint8_t *pks,
                                                    size_t n_pks, const uint8_t *sigs, const uint8_t *msg_data,
                                                    const uint32_t *msg_off, size_t n_msgs, const uint32_t *msg_idx,
                                                    const uint32_t *pk_idx, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return ts_verify_shares_rlc_fused(c, accept, n, pks, n_pks, sigs, msg_data, msg_off, n_msgs, msg_idx, pk_idx, q.s);
}
extern "C" int lcb_ts_verify_shares_batched_dev(uint8_t *accept, size_t n, const uint8_t *pks, size_t n_pks,
                                                const uint8_t *sigs, const uint8_t *msg_data, const uint32_t *msg_off,
                                                size_t n_msgs, const uint32_t *msg_idx, const uint32_t *pk_idx,
                                                void *stream) {
    return lcb_ctx_ts_verify_shares_batched_dev(nullptr, accept, n, pks, n_pks, sigs, msg_data, msg_off, n_msgs,
                                                msg_idx, pk_idx, stream);
}
// ---- statistics of the last batched call: of a context, or (without one) of the calling thread
extern "C" int lcb_ctx_tpke_batched_stats(lcb_ctx *ctx, uint32_t levels[8], float ms[6]) {
    CTX_OR(c, ctx, -1)
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!c->rlc_ran) { set_err("tpke batched verify: none has run in this context"); return -1; }
    if (hipEventSynchronize(c->rlc_ev[2]) != hipSuccess) { set_err("tpke batched verify: event sync"); return -1; }
    for (int i = 0; i < 8; i++) levels[i] = i < c->rlc_nlev ? c->rlc_levels[i] : 0;
    for (int i = 0; i < 2; i++)
        if (hipEventElapsedTime(&ms[i], c->rlc_ev[i], c->rlc_ev[i + 1]) != hipSuccess) ms[i] = -1.0f;
    for (int i = 0; i < RLC_MS_N; i++) ms[2 + i] = c->rlc_ms[i];
    return c->rlc_nlev;
}
extern "C" int lcb_tpke_batched_stats(uint32_t levels[8], float ms[6]) {
    const RlcStats &st = t_rlc_stats;
    if (!st.valid) { set_err("batched verify: none has completed on this thread"); return -1; }
    for (int i = 0; i < 8; i++) levels[i] = st.levels[i];
    for (int i = 0; i < 6; i++) ms[i] = st.ms[i];
    return st.nlev;
}
extern "C" int lcb_ctx_tpke_level_kernel_stats(lcb_ctx *ctx, uint32_t out[4]) {
    CTX_OR(c, ctx, -1)
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!c->rlc_ran) { set_err("tpke batched verify: none has run in this context"); return -1; }
    for (int i = 0; i < LVL_KERNEL_N; i++) out[i] = c->lvl_kernel[i];
    return 0;
}
extern "C" int lcb_ctx_tpke_fe_pair_stats(lcb_ctx *ctx, uint32_t out[4]) {
    CTX_OR(c, ctx, -1)
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!c->rlc_ran) { set_err("tpke batched verify: none has run in this context"); return -1; }
    for (int i = 0; i < FE_PAIR_N; i++) out[i] = c->fe_pair[i];
    return 0;
}
extern "C" int lcb_tpke_fe_pair_stats(uint32_t out[4]) {
    const RlcStats &st = t_rlc_stats;
    if (!st.valid) { set_err("batched verify: none has completed on this thread"); return -1; }
    for (int i = 0; i < FE_PAIR_N; i++) out[i] = st.fe_pair[i];
    return 0;
}
extern "C" int lcb_ctx_batched_census(lcb_ctx *ctx, uint32_t out[4]) {
    CTX_OR(c, ctx, -1)
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!c->rlc_ran) { set_err("batched verify: none has run in this context"); return -1; }
    for (int i = 0; i < CENSUS_N; i++) out[i] = c->rlc_census[i];
    return 0;
}
extern "C" int lcb_batched_census(uint32_t out[4]) {
    const RlcStats &st = t_rlc_stats;
    if (!st.valid) { set_err("batched verify: none has completed on this thread"); return -1; }
    for (int i = 0; i < CENSUS_N; i++) out[i] = st.census[i];
    return 0;
}
extern "C" int lcb_batched_inflight(int device) {
    if (device < 0 || device >= 64) { set_err("lcb_batched_inflight: device out of range"); return -1; }
    return (int)g_batched_inflight[device].load();
}
// ---- test hooks of the batch exponents (LCB_ALLOW_TEST_HOOKS=1: with a secret key they would expose material of it)
// rlc_scalar_dom (rlc_common.hpp) on n items: key10 = eight key words and two nonce words per item
extern "C" int lcb_debug_rlc_scalars(const uint32_t *key10, const uint32_t *ctr, const uint32_t *dom, size_t n,
                                     uint32_t *ab_out) {
    if (!env_on("LCB_ALLOW_TEST_HOOKS")) { set_err("lcb_debug_rlc_scalars: needs LCB_ALLOW_TEST_HOOKS=1"); return -1; }
    if (!n || n > 65536 || !key10 || !ctr || !dom || !ab_out) { set_err("lcb_debug_rlc_scalars: 1..65536 items"); return -1; }
    SYNC_CTX_OR(c, -1)
    HostCall h(c, "lcb_debug_rlc_scalars");
    const u32 *dk = h.in(key10, 10 * n), *dc = h.in(ctr, n), *dd = h.in(dom, n);
    u32 *dab = h.out<u32>(2 * n);
    if (!h.ok()) return -1;
    lcbk_rlc_scalars_debug(h.s, dk, dc, dd, (u32)n, dab);
    h.back(ab_out, dab, 8 * n);
    return h.finish();
}
// the records the last batched call of the context stored per share (RLC_REC_A, RLC_REC_B), as wire bytes, with the
// call's nonce and kind.  The levels only read the records, so they are what the group sums were formed from.
extern "C" int lcb_debug_rlc_records(lcb_ctx *ctx, uint8_t *rec_a, uint8_t *rec_b, size_t n, uint64_t *nonce, int *kind) {
    if (!env_on("LCB_ALLOW_TEST_HOOKS")) { set_err("lcb_debug_rlc_records: needs LCB_ALLOW_TEST_HOOKS=1"); return -1; }
    CTX_OR(c, ctx, -1)
    HostCall h(c, "lcb_debug_rlc_records");      // ordered behind the context's work; finish() waits for it
    if (c->rlc_last_kind < 0) { set_err("lcb_debug_rlc_records: no batched call has run in this context"); return -1; }
    if (!n || n != c->rlc_last_n || !rec_a || !rec_b) {
        set_err("lcb_debug_rlc_records: n is not the last batched call's share count");
        return -1;
    }
    const bool ts = c->rlc_last_kind == RLC_TS;
    const size_t wb = ts ? 96 : 48;
    const u32 *rA = (const u32 *)c->rlc[RLC_REC_A].p, *rB = (const u32 *)c->rlc[RLC_REC_B].p;
    if (!rA || !rB || c->rlc[RLC_REC_A].cap < n * LCB_G1_JAC_BYTES ||
        c->rlc[RLC_REC_B].cap < n * (ts ? LCB_G2_JAC_BYTES : LCB_G1_JAC_BYTES)) {
        set_err("lcb_debug_rlc_records: the context holds no records");
        return -1;
    }
    uint8_t *da = h.out<uint8_t>(48 * n), *db = h.out<uint8_t>(wb * n);
    if (!h.ok()) return -1;
    lcbk_rlc_records_debug(h.s, rA, rB, (u32)c->rlc_last_i0, (u32)n, ts ? 1 : 0, da, db);
    h.back(rec_a, da, 48 * n);
    h.back(rec_b, db, wb * n);
    if (h.finish()) return -1;
    if (nonce) *nonce = c->rlc_calls;
    if (kind) *kind = c->rlc_last_kind;
    return 0;
}
// ---- knobs
extern "C" void lcb_set_batch_seed(const uint8_t *seed32) {
    // test hook: a fixed ChaCha key makes the batch exponents predictable, so it is honoured only when the process
    // opted in (LCB_ALLOW_FIXED_BATCH_SEED=1); otherwise the call is ignored and the exponents stay secret
    std::lock_guard<std::mutex> lk(g_seed_mu);
    if (seed32 && env_on("LCB_ALLOW_FIXED_BATCH_SEED")) { memcpy(g_rlc_seed, seed32, 32); g_rlc_seed_set = true; }
    else g_rlc_seed_set = false;
}
extern "C" void lcb_set_batch_census(size_t min_shares) { g_census_min.store(min_shares); }
extern "C" int lcb_set_coop_max(uint32_t max_checks) {
    if (!tuning_allowed("lcb_set_coop_max")) return -1;
    g_coop_max.store(max_checks);
    g_coop_miller_max.store(max_checks);
    return 0;
}
extern "C" int lcb_set_coop_miller_max(uint32_t max_checks) {
    if (!tuning_allowed("lcb_set_coop_miller_max")) return -1;
    g_coop_miller_max.store(max_checks);
    return 0;
}
extern "C" int lcb_set_fe_pair_min(uint32_t min_entries) {
    if (!tuning_allowed("lcb_set_fe_pair_min")) return -1;
    g_fe_pair_min.store(min_entries);
    return 0;
}
extern "C" int lcb_set_busy_coop_max(uint32_t max_checks) {
    if (!tuning_allowed("lcb_set_busy_coop_max")) return -1;
    g_busy_coop_max.store(max_checks);
    return 0;
}
extern "C" uint32_t lcb_busy_coop_max(void) { return g_busy_coop_max.load(); }
extern "C" int lcb_set_level_mode(int mode) {
    if (!tuning_allowed("lcb_set_level_mode")) return -1;
    if (mode < 0 || mode > 2) { set_err("lcb_set_level_mode: 0 (by the count), 1 (never busy), 2 (always busy)"); return -1; }
    g_level_mode.store(mode);
    return 0;
}
extern "C" int lcb_set_fork_mode(int mode) {
    if (!tuning_allowed("lcb_set_fork_mode")) return -1;
    g_fork_mode.store(mode >= 1 && mode <= 4 ? mode : 0);
    return 0;
}
extern "C" int lcb_set_rlc_share_exponents(int on) {
    if (!tuning_allowed("lcb_set_rlc_share_exponents")) return -1;
    g_share_exp.store(on ? 1 : 0);
    return 0;
}
extern "C" int lcb_set_rlc_lane_permutation(int on) {
    if (!tuning_allowed("lcb_set_rlc_lane_permutation")) return -1;
    g_lane_perm.store(on ? 1 : 0);
    return 0;
}
extern "C" int lcb_set_rlc_signed_digits(int on) {
    if (!tuning_allowed("lcb_set_rlc_signed_digits")) return -1;
    g_signed_digits.store(on ? 1 : 0);
    return 0;
}
extern "C" int lcb_set_rlc_pos_table_min(uint32_t shares_per_key) {
    if (!tuning_allowed("lcb_set_rlc_pos_table_min")) return -1;
    g_pos_table_min.store(shares_per_key);
    return 0;
}
extern "C" int lcb_set_keys_first(int on) {
    if (!tuning_allowed("lcb_set_keys_first")) return -1;
    g_keys_first.store(on ? 1 : 0);
    return 0;
}
