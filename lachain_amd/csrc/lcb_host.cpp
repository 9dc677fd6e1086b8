// lachain_amd/csrc/lcb_host.cpp — the core of liblachain_bls.so's host side (include/lachain_bls.h): device
// initialisation and configuration, the scratch gate, the execution contexts, and the exact batch paths on them —
// TPKE and threshold-signature preparation / verification / combination, the coin folds, batch Lagrange, scalar
// multiplication, hashing to G2, the Pippenger MSM and the KDF — with their debug and tuning hooks.
//
// Elsewhere: the mcl single-element surface (lcb_mcl.cpp), the randomized batch check behind the *_batched entry
// points (lcb_batch.cpp; the exact checks and the preparations both use are here), the trustless-DKG commitments
// (lcb_dkg.cpp), Reed-Solomon and the reliable-broadcast Merkle layer (lcb_rbc.cpp), secp256k1 ECDSA / ECIES
// (lcb_ecdsa.cpp, lcb_ecies.cpp), transaction hashing (lcb_txhash.cpp) and the device keystream with the one-call
// TPKE Encrypt / FullDecrypt (lcb_kdf.cpp).  What they share is in lcb_internal.hpp.
// There is deliberately no CPU fallback for the GPU work: without a gfx950 device mclBn_init returns -1 and every
// entry point fails (returns -1 / 0 bytes / leaves outputs zeroed) with lcb_last_error() describing why.
//
// Concurrency model of the batch entry points (the single-element calls' is in lcb_mcl.cpp):
//   * every batch entry point runs in an lcb_ctx — explicit (lcb_ctx_*) or the calling thread's own default
//     context — which owns all device workspaces the call needs (TPKE and TS line sets separately, Lagrange,
//     MSM, staging).  A context's work executes in the order it was enqueued whatever stream it is enqueued on
//     (each call waits on the context's last event and records a new one), and a *_prepared call checks the
//     exact batch shape its prepare recorded, so no two callers can read or overwrite each other's workspace.
//   * the HIP device is bound per calling thread (lcb_set_device applies to every thread that enters).
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <mutex>
#include <atomic>
#include <vector>
#include <string>
#include <algorithm>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include "launch.h"
#include "bls_constants_host.h"
#include "../../include/lachain_bls.h"
#include "host_sha3.hpp"
#include "lcb_ctx.hpp"
#include "lcb_internal.hpp"
#include "fp_host.hpp"

using namespace lcb_int;

namespace {
std::mutex g_mu;               // device initialisation
int g_device = 0;
bool g_ready = false;
thread_local std::string g_err;
thread_local uint64_t g_err_count = 0;   // failures on this thread (lcb_error_count): the void mcl entry points have no
                                         // return code, so a caller detects their failure by this counter changing
thread_local int t_bound_device = -1;
std::atomic<int> g_inject_site{0}, g_inject_count{0};   // lcb_test_inject_failure
} // namespace
int lcb_int::g_orig_cofactor = 0;

void lcb_int::set_err(const char *what, hipError_t e) {
    char buf[256];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    g_err_count++;
}
bool lcb_int::injected(int site) {
    if (g_inject_site.load(std::memory_order_relaxed) != site) return false;
    int c = g_inject_count.load();
    while (c > 0)
        if (g_inject_count.compare_exchange_weak(c, c - 1)) return true;
    return false;
}
bool lcb_int::inject_armed(int site) {
    return g_inject_site.load(std::memory_order_relaxed) == site && g_inject_count.load() > 0;
}

// HIP's current device is per thread: bind every thread that enters the library to the configured device
static bool bind_thread() {
    if (t_bound_device == g_device) return true;
    hipError_t e = hipSetDevice(g_device);
    if (e != hipSuccess) { set_err("hipSetDevice", e); return false; }
    t_bound_device = g_device;
    return true;
}
static bool init_locked() {
    if (g_ready) return bind_thread();
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= g_device) { set_err("no HIP device", e); return false; }
    if (!bind_thread()) return false;
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, g_device)) != hipSuccess) { set_err("hipGetDeviceProperties", e); return false; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { set_err("device is not gfx950"); return false; }
    g_ready = true;
    return true;
}
bool lcb_int::ready() {
    if (g_ready && t_bound_device == g_device) return true;
    std::lock_guard<std::mutex> lk(g_mu);
    return init_locked();
}
int lcb_int::device() { return g_device; }

// opt-in switches read from the environment at call time: the tuning hooks (lcb_set_coop_max, ...) change the kernel
// families a batch runs on and the fault-injection hooks make calls fail; neither belongs in a production process
bool lcb_int::env_on(const char *name) {
    const char *e = getenv(name);
    return e && e[0] == '1';
}
bool lcb_int::tuning_allowed(const char *what) {
    if (env_on("LCB_ALLOW_TUNING")) return true;
    set_err((std::string(what) + ": tuning hooks need LCB_ALLOW_TUNING=1").c_str());
    return false;
}

// ================================================================== init / config
extern "C" int lcb_set_device(int id) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ready) return id == g_device ? 0 : -1;
    g_device = id;
    return 0;
}
extern "C" int lcb_get_device(void) { return g_device; }
extern "C" void lcb_set_original_g2_cofactor(int enable) { g_orig_cofactor = enable != 0; }
int g_line_mode = 0;   // 1: prepare marks every line set un-normalised (test hook for the on-the-fly fallback)
extern "C" int lcb_set_line_mode(int general) {
    if (!tuning_allowed("lcb_set_line_mode")) return -1;
    g_line_mode = general != 0;
    return 0;
}
int lcb_int::prepare_flags() { return g_orig_cofactor | (g_line_mode << 1); }
extern "C" const char *lcb_last_error(void) { return g_err.c_str(); }

// ================================================================== the scratch gate (gate.hpp LCB_LAUNCH_GATED)
// What the runtime does with a dispatch's private segment (ROCr's queue scratch handler; hsa_ext_amd.h:686-703 for the
// two agent limits, measured on the box in profiles/r06/scratch_limits.txt): the per-lane size S is rounded up to 16 B
// (a wave's 1 KB granule) and the FULL-device size  full(S) = S x 64 lanes x CUs x wave slots per CU  is requested for
// the dispatch's hardware queue.  When full(S) <= the agent's async scratch limit (HSA_AMD_AGENT_INFO_SCRATCH_LIMIT_
// CURRENT) the memory stays BOUND to that queue after the dispatch and serves its later dispatches; above it, it is a
// use-once allocation of the dispatch's own size, released when the dispatch retires.  All queues share one pool
// (SCRATCH_LIMIT_MAX).  A use-once request that does not fit waits while another use-once allocation is outstanding;
// a request that finds the pool held by bound reservations of busy queues aborts the process with
// HSA_STATUS_ERROR_OUT_OF_RESOURCES (the round-5 aborts: DESIGN.md §14.1).
// Measured on the box (profiles/r06/scratch_limits.txt): pool 32 GiB, bind limit 24 GiB, 256 CUs x 32 slots — every
// kernel of this library binds (the largest, k_op_gt at 8,148 B per lane, binds 4.27 GB), so the sum of the
// hardware queues' bound reservations is what must stay within the pool.  HIP keeps GPU_MAX_HW_QUEUES queues per stream
// priority and the library uses two priorities (the preparation chains run on high-priority streams), so a process
// holds up to Q = 2 x GPU_MAX_HW_QUEUES queues: 8 at the box's default 4, 16 when a caller raises it to 8 (the round-5
// bench did: 16 queues x up to 2.5 GB bound by the preparation lanes exceed the 32 GiB pool — the aborts).
// The gate therefore bounds the bound reservations: a launch whose full(S) exceeds the per-queue share
// T = (pool - LCB_GATE_RESERVE) / Q runs on one process-wide stream per device, ordered with the caller's stream by
// events, so every other queue binds <= T and the gate's queue at most LCB_GATE_RESERVE (>= every kernel's full(S):
// tests/test_kernel_resources.py), and  Q x T + reserve <= pool.  At Q = 8: T = 3.44 GiB, and only the single-lane
// mcl-surface / debug kernels (> 6.7 KB per lane) are routed; at Q = 16 the pairing kernels above ~3.5 KB are too.
// Launches whose scratch is use-once (full(S) above the bind limit) are left on the caller's stream.
#define LCB_GATE_RESERVE (9ull << 29)                 // 4.5 GiB: the gate queue's bound reservation, >= every kernel's full(S)
namespace {
struct GateDev {
    std::mutex mu, init_mu;
    hipStream_t s = nullptr;
    hipEvent_t in = nullptr, out = nullptr;
    std::atomic<int> ready{0};
    uint64_t slots = 0;           // CUs x wave slots per CU
    uint64_t pool = 0;            // HSA_AMD_AGENT_INFO_SCRATCH_LIMIT_MAX (0: unknown)
    uint64_t bind_limit = 0;      // HSA_AMD_AGENT_INFO_SCRATCH_LIMIT_CURRENT (0: unknown: every full(S) binds)
    uint64_t per_queue = 0;       // T
    int hwq = 8;                  // hardware queues the process may hold (both priorities)
};
GateDev g_gate[64];
std::atomic<long long> g_gate_bytes{-2};            // -2: not read from LCB_SCRATCH_GATE_MB yet; -3: the model's T
std::atomic<unsigned long long> g_gate_routed{0}, g_gate_seen{0};
thread_local int t_gate_dev = -1;                   // device whose gate mutex this thread holds (-1: none)
long long gate_override() {
    long long v = g_gate_bytes.load(std::memory_order_relaxed);
    if (v != -2) return v;
    const char *e = getenv("LCB_SCRATCH_GATE_MB");
    v = e && *e ? atoll(e) * (1ll << 20) : -3;
    long long expect = -2;
    g_gate_bytes.compare_exchange_strong(expect, v);
    return g_gate_bytes.load();
}
struct HsaFind { int want, seen; hsa_agent_t agent; bool found; };
hsa_status_t hsa_find_gpu(hsa_agent_t a, void *d) {
    HsaFind *f = (HsaFind *)d;
    hsa_device_type_t t;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS || t != HSA_DEVICE_TYPE_GPU)
        return HSA_STATUS_SUCCESS;
    if (f->seen++ == f->want) { f->agent = a; f->found = true; return HSA_STATUS_INFO_BREAK; }
    return HSA_STATUS_SUCCESS;
}
// the device's scratch model, read once (HIP device ordinal i = the i-th GPU agent of the runtime)
void gate_model(GateDev &g, int dev) {
    if (g.ready.load(std::memory_order_acquire)) return;
    std::lock_guard<std::mutex> lk(g.init_mu);
    if (g.ready.load()) return;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    uint32_t wpc = 0;
    HsaFind f{dev, 0, {0}, false};
    if (hsa_init() == HSA_STATUS_SUCCESS) {
        hsa_iterate_agents(hsa_find_gpu, &f);
        if (f.found) {
            uint64_t v = 0;
            if (hsa_agent_get_info(f.agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_SCRATCH_LIMIT_MAX, &v) == HSA_STATUS_SUCCESS) g.pool = v;
            v = 0;
            if (hsa_agent_get_info(f.agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_SCRATCH_LIMIT_CURRENT, &v) == HSA_STATUS_SUCCESS) g.bind_limit = v;
            if (hsa_agent_get_info(f.agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_MAX_WAVES_PER_CU, &wpc) != HSA_STATUS_SUCCESS) wpc = 0;
        }
        hsa_shut_down();
    }
    g.slots = (uint64_t)cus * (wpc ? wpc : 32);
    const char *q = getenv("GPU_MAX_HW_QUEUES");
    g.hwq = 2 * (q && atoi(q) > 0 ? atoi(q) : 4);      // queues per priority x the two priorities the library uses
    // unknown pool: assume the measured 32 GiB rather than none
    const uint64_t pool = g.pool ? g.pool : (32ull << 30);
    g.per_queue = pool > LCB_GATE_RESERVE ? (pool - LCB_GATE_RESERVE) / (uint64_t)g.hwq : 0;
    g.ready.store(1, std::memory_order_release);
}
}  // namespace
extern "C" hipStream_t lcb_gate_enter(const void *kern, long long *scratch_cache, size_t lanes, hipStream_t s) {
    long long sc = __atomic_load_n(scratch_cache, __ATOMIC_RELAXED);
    if (sc < 0) {
        hipFuncAttributes a;
        sc = hipFuncGetAttributes(&a, kern) == hipSuccess ? (long long)a.localSizeBytes : 0;
        __atomic_store_n(scratch_cache, sc, __ATOMIC_RELAXED);
    }
    g_gate_seen.fetch_add(1, std::memory_order_relaxed);
    const long long ovr = gate_override();
    if (sc == 0 || ovr == -1 || lanes == 0) return s;
    int dev = -1;
    if (hipStreamGetDevice(s, &dev) != hipSuccess || dev < 0) {          // (the caller's stream decides the device)
        if (hipGetDevice(&dev) != hipSuccess) return s;
    }
    if (dev < 0 || dev >= 64) return s;
    GateDev &g = g_gate[dev];
    gate_model(g, dev);
    const uint64_t per_lane = ((uint64_t)sc + 15) & ~(uint64_t)15;
    const uint64_t full = per_lane * 64 * g.slots;
    const bool binds = g.bind_limit == 0 || full <= g.bind_limit;
    const uint64_t thr = ovr >= 0 ? (uint64_t)ovr : g.per_queue;
    if (ovr != 0 && !(binds && full > thr)) return s;   // (override 0: every launch with scratch is routed)
    g.mu.lock();
    if (!g.s) {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (cur != dev) (void)hipSetDevice(dev);
        if (hipStreamCreateWithFlags(&g.s, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&g.in, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&g.out, hipEventDisableTiming) != hipSuccess)
            g.s = nullptr;
        if (cur >= 0 && cur != dev) (void)hipSetDevice(cur);
        if (!g.s) {                   // (the launch stays on the caller's stream)
            g.mu.unlock();
            return s;
        }
    }
    t_gate_dev = dev;
    g_gate_routed.fetch_add(1, std::memory_order_relaxed);
    (void)hipEventRecord(g.in, s);
    (void)hipStreamWaitEvent(g.s, g.in, 0);
    return g.s;
}
extern "C" void lcb_gate_exit(hipStream_t s, hipStream_t used) {
    if (used == s || t_gate_dev < 0) return;
    GateDev &g = g_gate[t_gate_dev];
    (void)hipEventRecord(g.out, used);
    (void)hipStreamWaitEvent(s, g.out, 0);
    t_gate_dev = -1;
    g.mu.unlock();
}
// the scratch model of the calling thread's device: out[0] pool, [1] bind limit, [2] wave slots, [3] hardware queues,
// [4] the per-queue share T, [5] the gate threshold in force (-1 off)
extern "C" int lcb_scratch_info(uint64_t out[6]) {
    int dev = 0;
    if (!out || hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
    GateDev &g = g_gate[dev];
    gate_model(g, dev);
    const long long ovr = gate_override();
    out[0] = g.pool;
    out[1] = g.bind_limit;
    out[2] = g.slots;
    out[3] = (uint64_t)g.hwq;
    out[4] = g.per_queue;
    out[5] = ovr == -1 ? ~0ull : ovr >= 0 ? (uint64_t)ovr : g.per_queue;
    return 0;
}
// tuning / test hook: the gate's threshold in bytes of reservation (-1: off, 0: every launch with scratch is routed)
extern "C" int lcb_set_scratch_gate(long long bytes) {
    if (!tuning_allowed("lcb_set_scratch_gate")) return -1;
    gate_override();
    g_gate_bytes.store(bytes < -1 ? -3 : bytes);    // < -1: back to the model's per-queue share
    return 0;
}
// test hook: at most this many blocks in the persistent grids (lanetab.hpp workspaces), so a small batch walks several
// items per lane; 0 = as many as are resident
std::atomic<uint32_t> g_persist_cap{0};
extern "C" uint32_t lcb_persist_cap(void) { return g_persist_cap.load(std::memory_order_relaxed); }
extern "C" int lcb_set_persist_blocks(uint32_t max_blocks) {
    if (!tuning_allowed("lcb_set_persist_blocks")) return -1;
    g_persist_cap.store(max_blocks);
    return 0;
}
extern "C" void lcb_scratch_gate_stats(uint64_t *routed, uint64_t *seen) {
    if (routed) *routed = g_gate_routed.load();
    if (seen) *seen = g_gate_seen.load();
}

// line sets of n points a prepare kernel (or the host) stored in their sets: the five-lane kernel (k_lines.hip, ~1.5 ms
// of latency) for the small preparations the single calls and the aggregation queue make, one lane per set (~4 ms of
// latency, but about half the work per set) for large batches
#define LCB_LINES_COOP_MAX 8192
std::atomic<int> g_lines_coop_max{LCB_LINES_COOP_MAX};
void lcb_int::lines_fill(hipStream_t s, u32 *lines, size_t n, const u32 *sets, uint8_t *w_g2) {
    if (!n) return;
    if (n <= (size_t)g_lines_coop_max.load()) lcbk_lineset_coop(s, lines, (u32)n, sets, w_g2);
    else lcbk_lineset_fill(dim3(nblk(n)), s, lines, (u32)n, sets, w_g2);
}
// Un-normalised line sets (only an adversarial W, or the line-mode test hook, makes one): after a preparation the flag
// `which` (0 = the census's ciphertexts, 1 = all) is reduced on the device and copied to pinned memory; the host reads
// it (lines_unnormalised) before it enqueues the checks that use those sets and dispatches the one-lane Miller
// fallback only when it is set.  Any failure reads as "set" (the fallback then runs, as before round 5).
void lcb_int::lines_flag_enqueue(lcb_ctx *c, int which, const u32 *lines, u32 c0, u32 c1, hipStream_t s) {
    c->unn_set[which] = false;
    if (!c->unn_pin && hipHostMalloc((void **)&c->unn_pin, 16, hipHostMallocDefault) != hipSuccess) {
        c->unn_pin = nullptr;
        return;
    }
    for (auto &e : c->unn_ev)
        if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return;
    u32 *d = (u32 *)c->unn.get(16);
    if (!d) return;
    if (hipMemsetAsync(d + which, 0, 4, s) != hipSuccess) return;
    lcbk_lines_unnormalised(s, lines, c0, c1, d + which);
    if (hipMemcpyAsync(c->unn_pin + which, d + which, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return;
    if (hipEventRecord(c->unn_ev[which], s) != hipSuccess) return;
    c->unn_set[which] = true;
}
bool lcb_int::lines_unnormalised(lcb_ctx *c, int which) {
    if (!c->unn_set[which] || hipEventSynchronize(c->unn_ev[which]) != hipSuccess) return true;
    return __atomic_load_n(c->unn_pin + which, __ATOMIC_ACQUIRE) != 0;
}
// a *_prepared call runs on the exact shape (keys, ciphertexts / messages) its context's prepare recorded
bool lcb_int::tpke_shape_ok(lcb_ctx *c, size_t n_keys, size_t n_cts, const char *what) {
    if (!c->t_ready) { set_err((std::string(what) + ": no TPKE batch prepared in this context").c_str()); return false; }
    if (c->t_n_cts != n_cts || c->t_n_keys != n_keys) {
        set_err((std::string(what) + ": batch shape differs from the one prepared in this context").c_str());
        return false;
    }
    return true;
}
bool lcb_int::ts_shape_ok(lcb_ctx *c, size_t n_pks, size_t n_msgs, const char *what) {
    if (!c->s_ready) { set_err((std::string(what) + ": no threshold-signature batch prepared in this context").c_str()); return false; }
    if (c->s_n_msgs != n_msgs || c->s_n_pks != n_pks) {
        set_err((std::string(what) + ": batch shape differs from the one prepared in this context").c_str());
        return false;
    }
    return true;
}

// ================================================================== execution contexts
namespace {

void ctx_free(lcb_ctx *c) {
    if (!c) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->order_valid) (void)hipEventSynchronize(c->order);
    for (DevBuf *b : {&c->t_lines, &c->t_ctok, &c->t_ctg2, &c->t_keys, &c->t_f, &c->s_lines, &c->s_mok, &c->s_keys, &c->s_f})
        b->release();
    for (auto &b : c->lag) b.release();
    c->lws.release();
    for (auto &b : c->sel) b.release();
    for (auto &b : c->msm) b.release();
    for (auto &b : c->stage) b.release();
    c->merkle_ws.release();
    c->pc_lines.release();
    for (auto &b : c->t_coop) b.release();
    c->cc_lines.release();
    c->cc_ok.release();
    for (auto &b : c->rlc) b.release();
    c->unn.release();
    if (c->unn_pin) (void)hipHostFree(c->unn_pin);
    for (auto &e : c->unn_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->rlc_ev_ready) {
        for (auto &e : c->rlc_ev) (void)hipEventDestroy(e);
        for (auto &e : c->rlc_lev_ev) (void)hipEventDestroy(e);
    }
    if (c->fork_ready) {
        for (hipStream_t x : {c->aux, c->hi, c->hi2, c->hi3})
            if (x) {
                (void)hipStreamSynchronize(x);
                (void)hipStreamDestroy(x);
            }
        for (auto &e : c->fork_ev) (void)hipEventDestroy(e);
        for (auto &e : c->prep_ev) (void)hipEventDestroy(e);
    }
    lcb_int::ecdsa_ctx_release(c);
    lcb_int::ecies_ctx_release(c);
    lcb_int::txhash_ctx_release(c);
    lcb_int::rawtx_ctx_release(c);
    lcb_int::trie_ctx_release(c);
    lcb_int::kdf_ctx_release(c);
    if (c->ver_ev_ready) for (auto &e : c->ver_ev) (void)hipEventDestroy(e);
    if (c->msm_ev_ready) for (auto &e : c->msm_ev) (void)hipEventDestroy(e);
    if (c->order) (void)hipEventDestroy(c->order);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}
lcb_ctx *ctx_new() {
    if (!ready()) return nullptr;
    lcb_ctx *c = new lcb_ctx;
    c->device = g_device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->order, hipEventDisableTiming);
    if (e != hipSuccess) { set_err("context creation", e); ctx_free(c); return nullptr; }
    return c;
}
// each thread owns two implicit contexts: one for the *_dev entry points without a context argument, one for the
// synchronous host-pointer entry points (so a host-pointer call never touches a workspace a *_dev caller prepared)
std::mutex &retired_mu() {                           // the list's own lock, leaked like the list
    static std::mutex *m = new std::mutex;
    return *m;
}
std::vector<lcb_ctx *> &retired_ctxs() {
    static std::vector<lcb_ctx *> *v = new std::vector<lcb_ctx *>;
    return *v;
}
struct ThreadCtx {
    lcb_ctx *c = nullptr;
    ~ThreadCtx() {                                   // retired, not freed (see lcb_mcl.cpp OpStage)
        if (!c) return;
        std::lock_guard<std::mutex> lk(retired_mu());
        retired_ctxs().push_back(c);
    }
};
thread_local ThreadCtx t_dev_ctx, t_sync_ctx;
// an implicit context for this thread: a retired one of the current device (its prepared state dropped, its
// buffers, caches keyed by content and event chain kept), else a new one
lcb_ctx *implicit_ctx_new() {
    {
        std::lock_guard<std::mutex> lk(retired_mu());
        auto &v = retired_ctxs();
        for (size_t k = v.size(); k-- > 0;) {
            lcb_ctx *c = v[k];
            if (c->device != g_device) continue;
            v.erase(v.begin() + (long)k);
            std::lock_guard<std::recursive_mutex> cl(c->mu);
            c->t_ready = c->s_ready = false;
            c->t_gen++;
            c->s_gen++;
            return c;
        }
    }
    return ctx_new();
}
} // namespace
lcb_ctx *lcb_int::ctx_resolve(lcb_ctx *c) {
    if (!ready()) return nullptr;
    if (c) {
        if (c->device != g_device) { set_err("context belongs to another device"); return nullptr; }
        return c;
    }
    if (!t_dev_ctx.c) t_dev_ctx.c = implicit_ctx_new();
    return t_dev_ctx.c;
}
lcb_ctx *lcb_int::ctx_sync() {
    if (!ready()) return nullptr;
    if (!t_sync_ctx.c) t_sync_ctx.c = implicit_ctx_new();
    return t_sync_ctx.c;
}
bool lcb_int::launch_ok(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_err(what, e); return false; }
    return true;
}
bool lcb_int::sync_check(lcb_ctx *c, const char *what) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { set_err(what, e); return false; }
    return true;
}
namespace {

// ------------------------------------------------------------------ TPKE
// shares / checks per Miller + final-exponentiation launch pair (bounds the park buffers); lcb_set_verify_chunk (test
// hook) lowers it so small batches run several chunks.  A call reads it once, when it takes its context (lcb_ctx.hpp
// Enq), and uses that value for its buffer sizes and its chunk loops alike.
std::atomic<size_t> g_verify_chunk{(size_t)1 << 21};
#define LCB_VERIFY_CHUNK (c->chunk)
#define LCB_CT_CACHE 2048                       // prepared-ciphertext cache slots per context (52.7 KB of lines each)
#define LCB_KEY_CACHE 4096                      // decompressed verification keys per context (LCB_G1A_ST_BYTES each)

int tpke_prepare(lcb_ctx *c, const uint8_t *d_y, size_t n_keys, const uint8_t *d_u, const uint8_t *d_w,
                 const uint8_t *d_v, const uint32_t *d_voff, size_t n_cts, hipStream_t s) {
    if (n_cts > 0xffffffffu || n_keys > 0xffffffffu) { set_err("tpke prepare: batch too large"); return -1; }
    c->t_ready = false;
    c->unn_set[0] = c->unn_set[1] = false;     // the fallback flags describe the line sets prepared below
    u32 *lines = (u32 *)c->t_lines.get((size_t)n_cts * 2 * LCB_LINESET_BYTES);
    uint8_t *ctok = (uint8_t *)c->t_ctok.get(n_cts);
    void *keys = c->t_keys.get(n_keys * LCB_G1A_ST_BYTES);
    uint8_t *ctg2 = (uint8_t *)c->t_ctg2.get(n_cts);     // from the line sets, for the batch check's sums
    if (!lines || !ctok || !keys || !ctg2) { set_err("device allocation failed"); return -1; }
    if (n_keys) lcbk_g1_decompress(dim3(nblk(n_keys)), s, d_y, (u32)n_keys, keys);
    if (n_cts) {
        lcbk_tpke_ct_prepare(dim3(nblk(n_cts)), s, d_u, d_w, d_v, d_voff, (u32)n_cts, lines, ctok, prepare_flags(),
                             nullptr);
        lines_fill(s, lines, 2 * n_cts, nullptr, ctg2);
    }
    c->unn_census = 1;
    lines_flag_enqueue(c, 1, lines, 0, (u32)n_cts, s);
    if (!launch_ok("tpke prepare launch")) return -1;
    c->t_n_cts = n_cts;
    c->t_n_keys = n_keys;
    c->t_gen++;
    c->t_ready = true;
    return 0;
}
// the exact check of n shares against prepared line sets (lines, ctok: n_cts ciphertexts) and decompressed keys
int tpke_verify_core(lcb_ctx *c, const u32 *lines, const uint8_t *ctok, size_t n_cts, const void *keys, size_t n_keys,
                     uint8_t *d_accept, size_t n, const uint32_t *d_ct, const uint32_t *d_dec, const uint8_t *d_ui,
                     hipStream_t s) {
    if (n > 0xffffffffu) { set_err("tpke verify: batch too large"); return -1; }
    if (n) {
        // chunks of at most LCB_VERIFY_CHUNK shares: bounded park buffer (slots x 576 B per share) whatever n is;
        // the phase events time the first chunk
        const size_t nf = n < LCB_VERIFY_CHUNK ? n : LCB_VERIFY_CHUNK;
        u32 *f = (u32 *)c->t_f.get(nf * 576 * (size_t)lcbk_fe_slots())   /* SoA Fp12 slots: Miller output (+ final-exp parking) */;
        if (!f) { set_err("device allocation failed"); return -1; }
        if (!c->ver_ev_ready) {
            for (auto &e : c->ver_ev) hipEventCreate(&e);
            c->ver_ev_ready = true;
        }
        // small batches (the protocol's one-share-per-call shape, the queue's flushes): nine lanes per check
        // (k_coop.hip) instead of one, below the size where the one-lane kernels fill the GPU
        // (never above one chunk: the cooperative buffers below are sized for n)
        const bool coop = n <= g_coop_max.load() && n <= LCB_VERIFY_CHUNK;
        void *gpts = coop ? c->t_coop[COOP_PTS].get(n * 2 * LCB_G1A_ST_BYTES) : nullptr;
        void *desc = coop ? c->t_coop[COOP_DESC].get(n * 16) : nullptr;
        uint8_t *fl = coop ? (uint8_t *)c->t_coop[COOP_FLAGS].get(2 * n) : nullptr;
        if (coop && (!gpts || !desc || !fl)) { set_err("device allocation failed"); return -1; }
        for (size_t o = 0; o < n; o += LCB_VERIFY_CHUNK) {
            const size_t m = n - o < LCB_VERIFY_CHUNK ? n - o : LCB_VERIFY_CHUNK;
            if (o == 0) hipEventRecord(c->ver_ev[0], s);
            if (coop) {
                lcbk_tpke_exact_points(s, ctok, (u32)n_cts, keys, (u32)n_keys, d_ct + o, d_dec + o,
                                       d_ui + 48 * o, (u32)m, gpts, desc, d_accept + o);
                lcbk_coop_tpke_miller(s, lines, desc, gpts, (u32)m, f, fl, fl + m, 2, 1);
            } else {
                lcbk_tpke_miller(dim3(nblk(m)), s, lines, ctok, (u32)n_cts, keys, (u32)n_keys, d_ct + o,
                                 d_dec + o, d_ui + 48 * o, (u32)m, f, d_accept + o);
            }
            if (o == 0) hipEventRecord(c->ver_ev[1], s);
            if (coop) lcbk_coop_final_exp_check(s, f, (u32)m, d_accept + o);
            else lcbk_final_exp_check(dim3(nblk(m)), s, f, (u32)m, d_accept + o);
            if (o == 0) hipEventRecord(c->ver_ev[2], s);
        }
        c->ver_ran = true;
    }
    return launch_ok("tpke verify launch") ? 0 : -1;
}
int tpke_verify_prepared(lcb_ctx *c, uint8_t *d_accept, size_t n, size_t n_keys, size_t n_cts, const uint32_t *d_ct,
                         const uint32_t *d_dec, const uint8_t *d_ui, hipStream_t s) {
    if (!tpke_shape_ok(c, n_keys, n_cts, "tpke verify")) return -1;
    return tpke_verify_core(c, (const u32 *)c->t_lines.p, (const uint8_t *)c->t_ctok.p, n_cts, c->t_keys.p, n_keys,
                            d_accept, n, d_ct, d_dec, d_ui, s);
}
int tpke_partial_decrypt_prepared(lcb_ctx *c, uint8_t *ui_out, uint8_t *status, const uint8_t *x_raw, size_t x_stride,
                                  const uint8_t *cts_u, size_t n_cts, hipStream_t s) {
    if (!tpke_shape_ok(c, c->t_n_keys, n_cts, "tpke partial decrypt")) return -1;
    for (size_t o = 0; o < n_cts; o += LCB_VERIFY_CHUNK) {
        const size_t m = std::min(LCB_VERIFY_CHUNK, n_cts - o);
        u32 *f = (u32 *)c->t_f.get(m * 576 * (size_t)lcbk_fe_slots());
        if (!f) { set_err("device allocation failed"); return -1; }
        lcbk_tpke_pd_miller(s, (const u32 *)c->t_lines.p, (const uint8_t *)c->t_ctok.p, cts_u, (u32)o, (u32)m, f, status);
        lcbk_final_exp_check(dim3(nblk(m)), s, f, (u32)m, status + o);
        lcbk_tpke_pd_mul(s, cts_u, x_raw, (u32)x_stride, (u32)o, (u32)m, status, ui_out);
    }
    return launch_ok("tpke partial decrypt launch") ? 0 : -1;
}


// ------------------------------------------------------------------ threshold signatures
int ts_prepare(lcb_ctx *c, const uint8_t *d_pks, size_t n_pks, const uint8_t *d_msg, const uint32_t *d_moff,
               size_t n_msgs, hipStream_t s) {
    if (n_msgs > 0xffffffffu || n_pks > 0xffffffffu) { set_err("ts prepare: batch too large"); return -1; }
    c->s_ready = false;
    u32 *lines = (u32 *)c->s_lines.get((size_t)n_msgs * LCB_LINESET_BYTES);
    uint8_t *mok = (uint8_t *)c->s_mok.get(n_msgs);
    void *keys = c->s_keys.get(n_pks * LCB_G1A_ST_BYTES);
    if (!lines || !mok || !keys) { set_err("device allocation failed"); return -1; }
    if (n_pks) lcbk_g1_decompress(dim3(nblk(n_pks)), s, d_pks, (u32)n_pks, keys);
    if (n_msgs) lcbk_ts_msg_prepare(dim3(nblk(n_msgs)), s, d_msg, d_moff, (u32)n_msgs, lines, mok, prepare_flags());
    if (!launch_ok("ts prepare launch")) return -1;
    c->s_n_msgs = n_msgs;
    c->s_n_pks = n_pks;
    c->s_gen++;
    c->s_ready = true;
    return 0;
}
int ts_verify_prepared(lcb_ctx *c, uint8_t *d_accept, size_t n, size_t n_pks, size_t n_msgs, const uint8_t *d_sigs,
                       const uint32_t *d_midx, const uint32_t *d_pidx, hipStream_t s) {
    if (!ts_shape_ok(c, n_pks, n_msgs, "ts verify")) return -1;
    if (n > 0xffffffffu) { set_err("ts verify: batch too large"); return -1; }
    const u32 *lines = (const u32 *)c->s_lines.p;
    const uint8_t *mok = (const uint8_t *)c->s_mok.p;
    if (n) {
        const size_t nf = n < LCB_VERIFY_CHUNK ? n : LCB_VERIFY_CHUNK;
        u32 *f = (u32 *)c->s_f.get(nf * 576 * (size_t)lcbk_fe_slots())   /* SoA Fp12 slots: Miller output (+ final-exp parking) */;
        if (!f) { set_err("device allocation failed"); return -1; }
        for (size_t o = 0; o < n; o += LCB_VERIFY_CHUNK) {
            const size_t m = n - o < LCB_VERIFY_CHUNK ? n - o : LCB_VERIFY_CHUNK;
            lcbk_ts_miller(dim3(nblk(m)), s, lines, mok, (u32)n_msgs, c->s_keys.p, (u32)n_pks, d_sigs + 96 * o,
                           d_midx + o, d_pidx + o, (u32)m, f, d_accept + o);
            lcbk_final_exp_check(dim3(nblk(m)), s, f, (u32)m, d_accept + o);
        }
    }
    return launch_ok("ts verify launch") ? 0 : -1;
}

// ------------------------------------------------------------------ Lagrange / assembly
// device-side Lagrange at 0 for np problems (entries off[j]..off[j+1]); dout = serialized results, dst = status
} // namespace
int lcb_int::lagrange_enqueue(lcb_ctx *c, int g, uint8_t *dout, uint8_t *dst, const uint8_t *dx, const uint8_t *dy,
                              const uint32_t *doff, size_t np, size_t ne, hipStream_t s, const u32 *src, bool pairs) {
    if (np > 0xffffffffu || ne > 0xffffffffu) { set_err("lagrange: batch too large"); return -1; }
    void *lam = c->lag[LAG_LAMBDA].get(LCB_FR_BYTES * (ne ? ne : 1));
    void *pre = c->lag[LAG_PREFIX].get(LCB_FR_BYTES * (ne ? ne : 1));      // the batch inversion's prefix products
    void *parts = c->lag[LAG_PARTS].get((g == 1 ? LCB_G1_JAC_BYTES : LCB_G2_JAC_BYTES) * (ne ? ne : 1));
    uint8_t *pok = (uint8_t *)c->lag[LAG_PARTS_OK].get(ne ? ne : 1);
    if (!lam || !pre || !parts || !pok) { set_err("device allocation failed"); return -1; }
    lcbk_lagrange_coeffs(dim3(nblk(np)), s, dx, doff, (u32)np, lam, pre, dst);
    if (ne) {
        const int which = g == 1 ? 1 : pairs ? 3 : 2;   // pairs: even problem offsets (assembly with even k)
        u32 *ws = (u32 *)c->lag[LAG_LANES_WS].get(lcbk_lanes_ws_bytes(which, (u32)ne));
        if (!ws) { set_err("device allocation failed (Lagrange lanes workspace)"); return -1; }
        if (g == 1) lcbk_g1_mul_lanes(s, dy, lam, (u32)ne, parts, pok, ws);
        else if (pairs)   // two entries per lane, shared doublings
            lcbk_g2_mul2_lanes(s, dy, lam, (u32)ne, parts, pok, src ? c->s_dec.p : nullptr,
                               (u32)std::min<size_t>(c->s_dec_n, 0xffffffffu), src, ws);
        else lcbk_g2_mul_lanes(s, dy, lam, (u32)ne, parts, pok, src ? c->s_dec.p : nullptr,
                               (u32)std::min<size_t>(c->s_dec_n, 0xffffffffu), src, ws);
    }
    if (g == 1) lcbk_g1_sum(dim3(nblk(np)), s, parts, pok, doff, (u32)np, dst, dout);
    else lcbk_g2_sum(dim3(nblk(np)), s, parts, pok, doff, (u32)np, dst, dout);
    return launch_ok("lagrange launch") ? 0 : -1;
}
int lcb_int::assemble_enqueue(lcb_ctx *c, int g, uint8_t *out, uint8_t *status, const uint8_t *accept, const uint8_t *pts,
                              size_t per_group, size_t k, size_t n_groups, hipStream_t s, const uint32_t *order) {
    if (!n_groups) return 0;
    if (k == 0 || k > per_group) { set_err("assemble: need 0 < k <= shares per group"); return -1; }
    size_t pb = g == 1 ? 48 : 96, ne = n_groups * k;
    if (ne > 0xffffffffu || (size_t)n_groups * per_group > 0xffffffffu) { set_err("assemble: batch too large"); return -1; }
    uint8_t *xs = (uint8_t *)c->sel[SEL_XS].get(32 * ne), *ys = (uint8_t *)c->sel[SEL_YS].get(pb * ne);
    u32 *off = (u32 *)c->sel[SEL_OFF].get(4 * (n_groups + 1));
    // G2 (signature shares): each entry's share index, so the lanes can reuse the batched check's decoded shares
    u32 *src = g == 2 && c->s_dec_n ? (u32 *)c->sel[SEL_SRC].get(4 * ne) : nullptr;
    if (!xs || !ys || !off) { set_err("device allocation failed"); return -1; }
    lcbk_select_first_valid(dim3(nblk(n_groups)), s, accept, pts, (u32)pb, (u32)per_group, (u32)k, (u32)n_groups, xs,
                            ys, off, order, src);
    return lagrange_enqueue(c, g, out, status, xs, ys, off, n_groups, ne, s, src, g == 2 && k % 2 == 0);
}
namespace {

// ------------------------------------------------------------------ Pippenger MSM (k_msm.hip)
// window width minimising ceil-windows * (n mixed adds * 11 + 2^(c-1) buckets * 2 Jacobian adds * 16) Fp-mul
// GLV form: 2n points with 128-bit scalars, windows ceil(128 / c); only widths whose top window is nearly full
// (a short top window concentrates 2n records in few buckets, one lane each)
std::atomic<int> g_msm_segs{0};     // lcb_set_msm_segments: bucket-reduction lanes rule (0: by form, see msm_enqueue)
std::atomic<int> g_msm_chunk{64};   // records per lane of k_msm_chunk_acc (0: one lane per bucket, k_msm_bucket_acc)
u32 msm_window(size_t n, bool glv = false) {
    u32 best = 4;
    double best_cost = 1e300;
    if (glv) {
        for (u32 c : {8u, 10u, 13u, 16u}) {
            double w = (128 + c - 1) / c;
            double cost = w * (2.0 * (double)n * 11.0) + (w + 1) * (double)(1u << (c - 1)) * 32.0;
            if (cost < best_cost) { best_cost = cost; best = c; }
        }
        return best;
    }
    for (u32 c = 4; c <= 20; c++) {
        double w = 255 / c + 1;
        double cost = w * ((double)n * 11.0 + (double)(1u << (c - 1)) * 32.0);
        if (cost < best_cost) { best_cost = cost; best = c; }
    }
    return best;
}
// the GLV form halves the serial window combination and the bucket reduction, but at the window widths it can use
// (<= 16) it needs more additions than the plain form's wider windows once n is large
bool msm_use_glv(size_t n) { return n <= ((size_t)1 << 22); }
int msm_enqueue(lcb_ctx *cx, void *out_jac, const void *pts, const uint8_t *scalars, size_t n, int window_bits,
                hipStream_t s, bool glv = false) {
    if (n > (glv ? 0x3fffffffu : 0x7fffffffu)) { set_err("msm: too many points"); return -1; }
    u32 c = window_bits > 0 ? (u32)window_bits : msm_window(n, glv);
    if (c < 2 || c > 24) { set_err("msm: window bits out of range"); return -1; }
    // GLV: nwin windows of the 128-bit halves, plus one key window for the top window's upper digit half
    u32 nwin = glv ? (128 + c - 1) / c : 255 / c + 1, half = 1u << (c - 1);
    u32 nb = (glv ? nwin + 1 : nwin) * half, sentinel = nb;
    size_t np = glv ? 2 * n : n;                 // points the digit records refer to
    size_t m = np * nwin;
    if (m > 0xffffffffu) { set_err("msm: n * windows exceeds 2^32"); return -1; }
    int end_bit = 1;
    while ((1ull << end_bit) <= sentinel) end_bit++;
    u32 L = 1;
    // GLV form (n <= 2^22): the fewest segments up to 65,536 (2^20: 0.87 vs 1.05 ms of reduction); the plain form at
    // 2^24 keeps the most segments of at least 65,536 (6.3 vs 7.7 ms) — profiles/r04/q2
    const int seg_rule = g_msm_segs.load() ? g_msm_segs.load() : (glv ? 65536 : 0);
    if (seg_rule > 0) {                          // the fewest segments (serial lanes) up to seg_rule of them
        while ((size_t)nb / L > (size_t)seg_rule && L * 2 <= half) L *= 2;
    } else {                                     // the most segments of at least 65,536
        while ((size_t)nb / (L * 2) >= 65536 && L * 2 <= half) L *= 2;
    }
    u32 n_seg = nb / L, per_win = half / L, n_l1 = n_seg / (per_win < 256 ? per_win : 256);
    u32 kwin = nb / half;                        // key windows (nwin, or nwin + 1 in the GLV form)
    if (!cx->msm_ev_ready) {
        for (auto &e : cx->msm_ev) hipEventCreate(&e);
        cx->msm_ev_ready = true;
    }
    DevBuf *b = cx->msm;
    u32 *keys = (u32 *)b[MSM_KEYS].get(m * 4), *keys2 = (u32 *)b[MSM_KEYS2].get(m * 4);
    u32 *vals = (u32 *)b[MSM_VALS].get(m * 4), *vals2 = (u32 *)b[MSM_VALS2].get(m * 4);
    u32 *st = (u32 *)b[MSM_START].get((size_t)nb * 4), *en = (u32 *)b[MSM_END].get((size_t)nb * 4);
    void *buckets = b[MSM_BUCKETS].get((size_t)nb * LCB_G1_JAC_BYTES);
    void *segs = b[MSM_SEGS].get((size_t)n_seg * LCB_G1_JAC_BYTES);
    void *l1 = b[MSM_L1].get((size_t)n_l1 * LCB_G1_JAC_BYTES);
    void *wins = b[MSM_WINS].get((size_t)kwin * LCB_G1_JAC_BYTES);
    size_t tb = 0;
    if (n && lcbk_sort_pairs(nullptr, &tb, keys, keys2, vals, vals2, (u32)m, end_bit, s) < 0) { set_err("msm: sort query"); return -1; }
    void *temp = b[MSM_SORT_TMP].get(tb);
    if (!keys || !keys2 || !vals || !vals2 || !st || !en || !buckets || !segs || !l1 || !wins || !temp) {
        set_err("msm: device allocation failed");
        return -1;
    }
    void *phi = glv ? b[MSM_PHI].get(n * 96) : nullptr;
    if (glv && !phi) { set_err("msm: device allocation failed"); return -1; }
    hipEventRecord(cx->msm_ev[0], s);
    if (n && glv) {
        lcbk_msm_phi(dim3(nblk(n)), s, pts, (u32)n, phi);
        lcbk_msm_digits_glv(dim3(nblk(n)), s, scalars, (u32)n, c, nwin, keys, vals);
    } else if (n) {
        lcbk_msm_digits(dim3(nblk(n)), s, scalars, (u32)n, c, nwin, keys, vals);
    }
    hipEventRecord(cx->msm_ev[1], s);
    int alt = n ? lcbk_sort_pairs(temp, &tb, keys, keys2, vals, vals2, (u32)m, end_bit, s) : 0;
    if (alt < 0) { set_err("msm: radix sort"); return -1; }
    if (alt) { keys = keys2; vals = vals2; }
    hipEventRecord(cx->msm_ev[2], s);
    hipMemsetAsync(st, 0, (size_t)nb * 4, s);
    hipMemsetAsync(en, 0, (size_t)nb * 4, s);
    if (m) lcbk_msm_bounds(dim3(nblk(m)), s, keys, (u32)m, sentinel, st, en);
    hipEventRecord(cx->msm_ev[3], s);
    if (g_msm_chunk > 0) {                       // record-balanced accumulation (k_msm_chunk_acc)
        const u32 K = (u32)g_msm_chunk.load();
        const size_t nch = (m + K - 1) / K;
        void *hp = b[MSM_CHUNK_HEAD].get((nch ? nch : 1) * LCB_G1_JAC_BYTES), *tp = b[MSM_CHUNK_TAIL].get((nch ? nch : 1) * LCB_G1_JAC_BYTES);
        if (!hp || !tp) { set_err("msm: device allocation failed"); return -1; }
        if (m) lcbk_msm_chunk_acc(s, pts, phi, (u32)n, keys, vals, (u32)m, K, sentinel, st, en, buckets, hp, tp, L, n_seg);
        lcbk_msm_bucket_fix(s, st, en, K, hp, tp, nb, buckets, L, n_seg);
    } else {
        lcbk_msm_bucket_acc(dim3(nblk(nb)), s, pts, phi, (u32)n, vals, st, en, nb, buckets, L, n_seg);
    }
    hipEventRecord(cx->msm_ev[4], s);
    lcbk_msm_bucket_reduce(dim3(nblk(n_seg)), s, buckets, half, L, n_seg, glv ? nwin : 0xffffffffu, segs);
    hipEventRecord(cx->msm_ev[5], s);
    // per-window sums: LDS tree reductions of up to 256 segment sums per block, ping-ponging segs <-> l1
    void *cur = segs, *nxt = l1;
    for (u32 cnt = per_win, total = n_seg; cnt > 1;) {
        u32 g = cnt < 256 ? cnt : 256;
        void *dst = (cnt == g) ? wins : nxt;
        lcbk_g1_jac_reduce_block(s, cur, total, g, dst);
        cnt /= g;
        total /= g;
        cur = dst;
        nxt = (dst == l1) ? segs : l1;
    }
    if (per_win == 1) hipMemcpyAsync(wins, segs, (size_t)kwin * LCB_G1_JAC_BYTES, hipMemcpyDeviceToDevice, s);
    lcbk_msm_horner(s, wins, nwin, c, glv ? 1u : 0u, out_jac);
    hipEventRecord(cx->msm_ev[6], s);
    cx->msm_ran = true;
    return launch_ok("msm launch") ? 0 : -1;
}

} // namespace
size_t lcb_verify_chunk_now() { return g_verify_chunk.load(std::memory_order_relaxed); }

extern "C" lcb_ctx *lcb_ctx_create(void) { return ctx_new(); }
extern "C" void lcb_ctx_destroy(lcb_ctx *ctx) {
    if (!ctx) return;
    { std::lock_guard<std::recursive_mutex> lk(ctx->mu); }
    ctx_free(ctx);
}
extern "C" int lcb_ctx_synchronize(lcb_ctx *ctx) {
    CTX_OR(c, ctx, -1)
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!c->order_valid) return 0;
    hipError_t e = hipEventSynchronize(c->order);
    if (e != hipSuccess) { set_err("context synchronize", e); return -1; }
    return 0;
}

// ================================================================== batch: TPKE
extern "C" int lcb_ctx_tpke_prepare_dev(lcb_ctx *ctx, const uint8_t *y_keys, size_t n_keys, const uint8_t *cts_u,
                                        const uint8_t *cts_w, const uint8_t *v_data, const uint32_t *v_off,
                                        size_t n_cts, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return tpke_prepare(c, y_keys, n_keys, cts_u, cts_w, v_data, v_off, n_cts, q.s);
}
extern "C" int lcb_ctx_tpke_verify_prepared_dev(lcb_ctx *ctx, uint8_t *accept, size_t n, size_t n_keys, size_t n_cts,
                                                const uint32_t *ct_idx, const uint32_t *dec_idx, const uint8_t *ui,
                                                void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return tpke_verify_prepared(c, accept, n, n_keys, n_cts, ct_idx, dec_idx, ui, q.s);
}
extern "C" int lcb_ctx_tpke_partial_decrypt_prepared_dev(lcb_ctx *ctx, uint8_t *ui_out, uint8_t *status,
                                                         const uint8_t *x_raw, size_t x_stride, const uint8_t *cts_u,
                                                         size_t n_cts, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return tpke_partial_decrypt_prepared(c, ui_out, status, x_raw, x_stride, cts_u, n_cts, q.s);
}
extern "C" int lcb_ctx_tpke_combine_dev(lcb_ctx *ctx, uint8_t *u_out, uint8_t *status, const uint8_t *accept,
                                        const uint8_t *shares, size_t per_ct, size_t k, size_t n_cts, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return assemble_enqueue(c, 1, u_out, status, accept, shares, per_ct, k, n_cts, q.s);
}
extern "C" int lcb_ctx_tpke_combine_ordered_dev(lcb_ctx *ctx, uint8_t *u_out, uint8_t *status, const uint8_t *accept,
                                                const uint8_t *shares, const uint32_t *order, size_t per_ct, size_t k,
                                                size_t n_cts, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return assemble_enqueue(c, 1, u_out, status, accept, shares, per_ct, k, n_cts, q.s, order);
}
extern "C" int lcb_tpke_combine_ordered_dev(uint8_t *u_out, uint8_t *status, const uint8_t *accept,
                                           const uint8_t *shares, const uint32_t *order, size_t per_ct, size_t k,
                                           size_t n_cts, void *stream) {
    return lcb_ctx_tpke_combine_ordered_dev(nullptr, u_out, status, accept, shares, order, per_ct, k, n_cts, stream);
}
extern "C" int lcb_ctx_tpke_verify_phase_ms(lcb_ctx *ctx, float ms[2]) {
    CTX_OR(c, ctx, -1)
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!c->ver_ran) { set_err("tpke verify: no split verify has run in this context"); return -1; }
    if (hipEventSynchronize(c->ver_ev[2]) != hipSuccess) { set_err("tpke verify: event sync"); return -1; }
    for (int i = 0; i < 2; i++)
        if (hipEventElapsedTime(&ms[i], c->ver_ev[i], c->ver_ev[i + 1]) != hipSuccess) ms[i] = -1.0f;
    return 0;
}
extern "C" int lcb_set_verify_chunk(size_t checks) {
    if (!tuning_allowed("lcb_set_verify_chunk")) return -1;
    if (checks == 0 || checks > ((size_t)1 << 21)) { set_err("lcb_set_verify_chunk: 1 .. 2^21"); return -1; }
    g_verify_chunk.store(checks);
    return 0;
}
extern "C" int lcb_set_wave_priority(int on) {
    if (!tuning_allowed("lcb_set_wave_priority")) return -1;
    if (!ready()) return -1;
    if (lcbk_set_wave_prio(on != 0)) { set_err("lcb_set_wave_priority: device configuration failed"); return -1; }
    return 0;
}
extern "C" int lcb_set_msm_segments(int max_segments) {
    if (!tuning_allowed("lcb_set_msm_segments")) return -1;
    g_msm_segs.store(max_segments > 0 ? max_segments : 0);
    return 0;
}
extern "C" int lcb_set_lines_coop_max(int max_sets) {
    if (!tuning_allowed("lcb_set_lines_coop_max")) return -1;
    g_lines_coop_max.store(max_sets < 0 ? LCB_LINES_COOP_MAX : max_sets);
    return 0;
}
extern "C" int lcb_set_msm_chunk(int records_per_lane) {
    if (!tuning_allowed("lcb_set_msm_chunk")) return -1;
    if (records_per_lane < 0 || records_per_lane > 65536) { set_err("lcb_set_msm_chunk: 0..65536"); return -1; }
    g_msm_chunk.store(records_per_lane);
    return 0;
}
extern "C" int lcb_test_inject_failure(int site, int count) {
    if (!env_on("LCB_ALLOW_TEST_HOOKS")) { set_err("lcb_test_inject_failure: needs LCB_ALLOW_TEST_HOOKS=1"); return -1; }
    g_inject_count.store(0);
    g_inject_site.store(site);
    g_inject_count.store(count);
    return 0;
}
extern "C" uint64_t lcb_error_count(void) { return g_err_count; }
// test hook: the line sets of n G2 wire points (an undecodable encoding -> the point at infinity) on the five-lane
// (coop = 1) or the one-lane kernel, force[k] = the set's force-general flag; out: n sets of LCB_LINESET_BYTES,
// w_g2[k] = the G2 flag of set 2k + 1 (k_lineset_fill's contract)
extern "C" int lcb_test_linesets(int coop, const uint8_t *g2_wire, const uint8_t *force, size_t n, uint32_t *out,
                                 uint8_t *w_g2) {
    if (!env_on("LCB_ALLOW_TEST_HOOKS")) { set_err("lcb_test_linesets: needs LCB_ALLOW_TEST_HOOKS=1"); return -1; }
    if (!n || n > 4096) { set_err("lcb_test_linesets: 1..4096 points"); return -1; }
    SYNC_CTX_OR(c, -1)
    HostCall h(c, "lcb_test_linesets");
    hipStream_t s = h.s;
    const size_t W = LCB_LINESET_BYTES / 4;
    u32 *lines = h.out<u32>(n * W);
    uint8_t *dg = h.out<uint8_t>(n / 2 + 1);
    if (!h.ok()) return -1;
    std::vector<u32> host(n * W, 0u);
    for (size_t k = 0; k < n; k++) {
        fph::g2a a;
        const bool ok = fph::g2_decompress(a, g2_wire + 96 * k, g_g2_sign_b.load() != 0);
        u32 *pt = &host[k * W + LCB_LS_POINT_WORD];
        if (ok && !a.inf) {
            memcpy(pt, &a.x, 96);
            memcpy(pt + 24, &a.y, 96);
        }
        pt[49] = (ok && !a.inf) ? 0u : 1u;
        pt[50] = force[k] ? 1u : 0u;
    }
    if (hipMemcpyAsync(lines, host.data(), n * LCB_LINESET_BYTES, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(dg, 0, n / 2 + 1, s) != hipSuccess) { set_err("lcb_test_linesets: upload"); return -1; }
    if (coop == 2) lcbk_lineset_coop_2w(s, lines, (u32)n, nullptr, dg);     // the fused census's instance (k_prep.hip)
    else if (coop) lcbk_lineset_coop(s, lines, (u32)n, nullptr, dg);
    else lcbk_lineset_fill(dim3(nblk(n)), s, lines, (u32)n, nullptr, dg);
    h.back(out, lines, n * LCB_LINESET_BYTES);
    h.back(w_g2, dg, n / 2);
    return h.finish();
}
// one cooperative Fp12 operation (k_coop_debug) on n values a (and b) vs the one-lane field.hpp routine: AoS in / out
extern "C" int lcb_debug_coop_op(int op, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out, uint32_t *ref) {
    SYNC_CTX_OR(c, -1)
    if (!n || n > 65536) { set_err("debug coop op: 1..65536 values"); return -1; }
    const size_t W = (size_t)144 * n;
    std::vector<u32> sa(W * 6, 0), sb(W), so(W), sr(W);
    for (size_t i = 0; i < n; i++)
        for (int w = 0; w < 144; w++) {
            sa[((size_t)(w >> 2) * n + i) * 4 + (w & 3)] = a[144 * i + w];
            sb[((size_t)(w >> 2) * n + i) * 4 + (w & 3)] = b[144 * i + w];
        }
    HostCall h(c, "debug coop op");
    u32 *da = h.work(sa.data(), W * 6);
    const u32 *db = h.in(sb.data(), W);
    u32 *dout = h.out<u32>(W), *dref = h.out<u32>(W);
    if (!h.ok()) return -1;
    lcbk_coop_debug(h.s, op, da, db, (u32)n, dout, dref);
    h.back(so.data(), dout, W * 4);
    h.back(sr.data(), dref, W * 4);
    if (h.finish()) return -1;
    for (size_t i = 0; i < n; i++)
        for (int w = 0; w < 144; w++) {
            out[144 * i + w] = so[((size_t)(w >> 2) * n + i) * 4 + (w & 3)];
            ref[144 * i + w] = sr[((size_t)(w >> 2) * n + i) * 4 + (w & 3)];
        }
    return 0;
}
// the final exponentiation of n Fp12 values (144 words each, Montgomery form, AoS) by the one-lane kernel (coop = 0) or
// the nine-lane kernel (coop = 1): tests compare the two bit for bit
extern "C" int lcb_debug_final_exp(const uint32_t *in, size_t n, uint32_t *out, int coop) {
    SYNC_CTX_OR(c, -1)
    if (!n || n > 65536) { set_err("debug final exp: 1..65536 values"); return -1; }
    std::vector<u32> soa((size_t)144 * n * lcbk_fe_slots(), 0);
    for (size_t i = 0; i < n; i++)
        for (int w = 0; w < 144; w++) soa[((size_t)(w >> 2) * n + i) * 4 + (w & 3)] = in[144 * i + w];
    HostCall h(c, "debug final exp");
    u32 *d = h.work(soa.data(), soa.size());
    uint8_t *acc = h.out<uint8_t>(n);
    if (!h.ok()) return -1;
    hipMemsetAsync(acc, 1, n, h.s);
    if (coop) lcbk_coop_final_exp_check(h.s, d, (u32)n, acc);
    else lcbk_final_exp_check(dim3(nblk(n)), h.s, d, (u32)n, acc);
    h.back(soa.data(), d, (size_t)144 * n * 4);
    if (h.finish()) return -1;
    for (size_t i = 0; i < n; i++)
        for (int w = 0; w < 144; w++) out[144 * i + w] = soa[((size_t)(w >> 2) * n + i) * 4 + (w & 3)];
    return 0;
}
// one assembly tower routine (asm_tower.hpp through fe_asm.hpp's wrappers, k_asm_tower_debug) on n operands, AoS in /
// out as above.  op & 255: 0 a b, 1 conj(a) b (lcb_r_fp12_mul_n), 2 one Granger-Scott squaring, 3 op >> 8 (1..255)
// squarings in one call (lcb_r_cyc_sqr_n), 4 a^z (lcb_r_pow_z); b is read by ops 0 and 1 only
extern "C" int lcb_debug_asm_tower(int op, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out) {
    SYNC_CTX_OR(c, -1)
    const int what = op & 255, count = op >> 8;
    if (!n || n > 65536) { set_err("debug asm tower: 1..65536 values"); return -1; }
    if (op < 0 || what > 4 || (what == 3 ? count < 1 || count > 255 : count != 0)) {
        set_err("debug asm tower: op 0..4, a run length of 1..255 above bit 8 for op 3 only");
        return -1;
    }
    if (what < 2 && !b) { set_err("debug asm tower: the product needs b"); return -1; }
    const size_t W = (size_t)144 * n;
    std::vector<u32> soa(W * 4, 0);
    for (size_t i = 0; i < n; i++)
        for (int w = 0; w < 144; w++) {
            soa[((size_t)(w >> 2) * n + i) * 4 + (w & 3)] = a[144 * i + w];
            if (what < 2) soa[W + ((size_t)(w >> 2) * n + i) * 4 + (w & 3)] = b[144 * i + w];
        }
    HostCall h(c, "debug asm tower");
    u32 *d = h.work(soa.data(), soa.size());
    if (!h.ok()) return -1;
    lcbk_asm_tower_debug(dim3(nblk(n)), h.s, what, d, (u32)n, (u32)(count ? count : 1));
    h.back(soa.data(), d + 2 * W, W * 4);
    if (h.finish()) return -1;
    for (size_t i = 0; i < n; i++)
        for (int w = 0; w < 144; w++) out[144 * i + w] = soa[((size_t)(w >> 2) * n + i) * 4 + (w & 3)];
    return 0;
}
// the exact per-share check up to its Miller loop: lcb_tpke_verify_shares's uploads and prepare, then k_tpke_miller (the
// one-lane kernel, whatever lcb_set_coop_max says) and no final exponentiation.  f_out: each share's parked Miller value
// (slot 0, 144 words, AoS); ok_out: its validity flag (index range, decompression, key, ciphertext)
extern "C" int lcb_debug_tpke_miller(uint32_t *f_out, uint8_t *ok_out, size_t n, const uint8_t *y_keys, size_t n_keys,
                                     const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data,
                                     const uint32_t *v_off, size_t n_cts, const uint32_t *ct_idx,
                                     const uint32_t *dec_idx, const uint8_t *ui) {
    SYNC_CTX_OR(c, -1)
    if (!n || n > 65536 || !n_cts || !n_keys) { set_err("debug tpke miller: 1..65536 shares, some keys and ciphertexts"); return -1; }
    for (size_t i = 0; i < n; i++)
        if (ct_idx[i] >= n_cts || dec_idx[i] >= n_keys) { set_err("debug tpke miller: index out of range"); return -1; }
    HostCall h(c, "debug tpke miller");
    hipStream_t s = h.s;
    const uint8_t *dy = h.in(y_keys, 48 * n_keys);
    const uint8_t *du = h.in(cts_u, 48 * n_cts);
    const uint8_t *dw = h.in(cts_w, 96 * n_cts);
    const uint8_t *dv = h.in(v_data, (size_t)v_off[n_cts]);
    const uint32_t *dvo = h.in(v_off, n_cts + 1);
    const uint32_t *dct = h.in(ct_idx, n);
    const uint32_t *ddec = h.in(dec_idx, n);
    const uint8_t *dui = h.in(ui, 48 * n);
    uint8_t *dacc = h.out<uint8_t>(n);
    u32 *f = h.out<u32>(n * 144 * (size_t)lcbk_fe_slots());
    if (!h.ok()) return -1;
    if (tpke_prepare(c, dy, n_keys, du, dw, dv, dvo, n_cts, s)) return -1;
    lcbk_tpke_miller(dim3(nblk(n)), s, (const u32 *)c->t_lines.p, (const uint8_t *)c->t_ctok.p, (u32)n_cts, c->t_keys.p,
                     (u32)n_keys, dct, ddec, dui, (u32)n, f, dacc);
    std::vector<u32> soa((size_t)144 * n);
    h.back(soa.data(), f, soa.size() * 4);
    h.back(ok_out, dacc, n);
    if (h.finish()) return -1;
    for (size_t i = 0; i < n; i++)
        for (int w = 0; w < 144; w++) f_out[144 * i + w] = soa[((size_t)(w >> 2) * n + i) * 4 + (w & 3)];
    return 0;
}

extern "C" int lcb_tpke_prepare_dev(const uint8_t *y_keys, size_t n_keys, const uint8_t *cts_u, const uint8_t *cts_w,
                                    const uint8_t *v_data, const uint32_t *v_off, size_t n_cts, void *stream) {
    return lcb_ctx_tpke_prepare_dev(nullptr, y_keys, n_keys, cts_u, cts_w, v_data, v_off, n_cts, stream);
}
extern "C" int lcb_tpke_verify_prepared_dev(uint8_t *accept, size_t n, size_t n_keys, size_t n_cts, const uint32_t *ct_idx,
                                            const uint32_t *dec_idx, const uint8_t *ui, void *stream) {
    return lcb_ctx_tpke_verify_prepared_dev(nullptr, accept, n, n_keys, n_cts, ct_idx, dec_idx, ui, stream);
}
extern "C" int lcb_tpke_partial_decrypt_prepared_dev(uint8_t *ui_out, uint8_t *status, const uint8_t *x_raw,
                                                     size_t x_stride, const uint8_t *cts_u, size_t n_cts, void *stream) {
    return lcb_ctx_tpke_partial_decrypt_prepared_dev(nullptr, ui_out, status, x_raw, x_stride, cts_u, n_cts, stream);
}
extern "C" int lcb_tpke_combine_dev(uint8_t *u_out, uint8_t *status, const uint8_t *accept, const uint8_t *shares,
                                    size_t per_ct, size_t k, size_t n_cts, void *stream) {
    return lcb_ctx_tpke_combine_dev(nullptr, u_out, status, accept, shares, per_ct, k, n_cts, stream);
}
extern "C" int lcb_tpke_verify_phase_ms(float ms[2]) { return lcb_ctx_tpke_verify_phase_ms(nullptr, ms); }
extern "C" int lcb_tpke_verify_shares_dev(uint8_t *accept, size_t n, const uint8_t *y_keys, size_t n_keys,
                                          const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data,
                                          const uint32_t *v_off, size_t n_cts, const uint32_t *ct_idx,
                                          const uint32_t *dec_idx, const uint8_t *ui, void *stream) {
    CTX_OR(c, nullptr, -1)
    Enq q(c, (hipStream_t)stream);
    if (tpke_prepare(c, y_keys, n_keys, cts_u, cts_w, v_data, v_off, n_cts, q.s)) return -1;
    return tpke_verify_prepared(c, accept, n, n_keys, n_cts, ct_idx, dec_idx, ui, q.s);
}
static int tpke_verify_shares_host(uint8_t *accept, size_t n, const uint8_t *y_keys, size_t n_keys,
                                   const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data,
                                   const uint32_t *v_off, size_t n_cts, const uint32_t *ct_idx,
                                   const uint32_t *dec_idx, const uint8_t *ui, bool batched) {
    SYNC_CTX_OR(c, -1)
    for (size_t i = 0; i < n; i++) {
        if (ct_idx[i] >= n_cts) { set_err("ct_idx out of range"); return -1; }
        if (dec_idx[i] >= n_keys) { set_err("dec_idx out of range"); return -1; }
    }
    HostCall h(c, "tpke verify");
    hipStream_t s = h.s;
    size_t vbytes = n_cts ? v_off[n_cts] : 0;
    const uint8_t *dy = h.in(y_keys, 48 * n_keys);
    const uint8_t *du = h.in(cts_u, 48 * n_cts);
    const uint8_t *dw = h.in(cts_w, 96 * n_cts);
    const uint8_t *dv = h.in(v_data, vbytes);
    const uint32_t *dvo = h.in(v_off, n_cts + 1);
    const uint32_t *dct = h.in(ct_idx, n);
    const uint32_t *ddec = h.in(dec_idx, n);
    const uint8_t *dui = h.in(ui, 48 * n);
    uint8_t *dacc = h.out<uint8_t>(n);
    if (!h.ok()) return -1;
    if (batched) {
        if (tpke_verify_shares_rlc_fused(c, dacc, n, dy, n_keys, du, dw, dv, dvo, n_cts, dct, ddec, dui, s)) return -1;
    } else {
        if (tpke_prepare(c, dy, n_keys, du, dw, dv, dvo, n_cts, s)) return -1;
        if (tpke_verify_prepared(c, dacc, n, n_keys, n_cts, dct, ddec, dui, s)) return -1;
    }
    h.back(accept, dacc, n);
    return h.finish();
}
// lcb_tpke_verify_shares with a per-context cache of prepared ciphertexts (the line sets of H and W and the
// validity, keyed by the ciphertext's bytes, least recently used slot replaced): the protocol verifies the N shares of
// a ciphertext in separate calls (HoneyBadger.cs:211-212), so each ciphertext is hashed to G2 and its lines computed
// once, not once per call.  Same decisions as lcb_tpke_verify_shares (a cache entry is the prepare output for the
// same bytes under the same prepare flags).
extern "C" int lcb_tpke_verify_shares_cached(uint8_t *accept, size_t n, const uint8_t *y_keys, size_t n_keys,
                                             const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data,
                                             const uint32_t *v_off, size_t n_cts, const uint32_t *ct_idx,
                                             const uint32_t *dec_idx, const uint8_t *ui) {
    SYNC_CTX_OR(c, -1)
    // a batch this wide gains nothing from the caches (and more keys than the key cache holds cannot use it): the
    // uncached call gives the same decisions
    if (n_cts > LCB_CT_CACHE / 2 || n_keys > LCB_KEY_CACHE)
        return tpke_verify_shares_host(accept, n, y_keys, n_keys, cts_u, cts_w, v_data, v_off, n_cts, ct_idx, dec_idx,
                                       ui, false);
    for (size_t i = 0; i < n; i++) {
        if (ct_idx[i] >= n_cts) { set_err("ct_idx out of range"); return -1; }
        if (dec_idx[i] >= n_keys) { set_err("dec_idx out of range"); return -1; }
    }
    HostCall h(c, "tpke verify (cached)");
    hipStream_t s = h.s;
    const int flags = prepare_flags();
    if (c->cc_used.empty() || c->cc_flags != flags) {           // first use, or prepare flags changed: empty cache
        c->cc_map.clear();
        c->cc_keys.assign(LCB_CT_CACHE, std::string());
        c->cc_used.assign(LCB_CT_CACHE, 0);
        c->cc_flags = flags;
    }
    u32 *lines = (u32 *)c->cc_lines.get((size_t)LCB_CT_CACHE * 2 * LCB_LINESET_BYTES);
    uint8_t *ctok = (uint8_t *)c->cc_ok.get(LCB_CT_CACHE);
    void *keys = c->kc_pts.get((size_t)LCB_KEY_CACHE * LCB_G1A_ST_BYTES);
    if (!lines || !ctok || !keys) { set_err("device allocation failed"); return -1; }
    const uint64_t tick = ++c->cc_tick;
    // the maps below name slots before their line sets / points exist: any failure from here on empties both caches
    // (the next call starts from first use), so no later call can take a slot this call left unfilled
    auto cache_fail = [c]() {
        c->cc_used.clear();
        c->kc_map.clear();
        c->kc_n = 0;
        return -1;
    };
    // verification keys -> key-cache slots; the misses are decompressed into consecutive slots [kc_n, kc_n + misses)
    std::vector<u32> kslot(n_keys);
    u32 kfirst = c->kc_n;
    for (int pass = 0; pass < 2; pass++) {
        kfirst = c->kc_n;
        u32 next = kfirst;
        bool full = false;
        for (size_t k = 0; k < n_keys && !full; k++) {
            std::string key((const char *)y_keys + 48 * k, 48);
            auto it = c->kc_map.find(key);
            if (it != c->kc_map.end()) { kslot[k] = it->second; continue; }
            if (next == LCB_KEY_CACHE) { full = true; break; }
            kslot[k] = next;
            c->kc_map.emplace(std::move(key), next++);
        }
        if (!full) { c->kc_n = next; break; }
        c->kc_map.clear();                               // this call's keys do not fit beside the old ones: start afresh
        c->kc_n = 0;
    }
    std::vector<uint8_t> kmiss;
    for (size_t k = 0; k < n_keys; k++)
        if (kslot[k] >= kfirst) {                        // first sight, in slot order (a repeated key maps to one slot)
            if (kmiss.size() / 48 == kslot[k] - kfirst) kmiss.insert(kmiss.end(), y_keys + 48 * k, y_keys + 48 * k + 48);
        }
    std::vector<u32> slot_of(n_cts), miss;
    for (size_t k = 0; k < n_cts; k++) {
        const u32 v0 = v_off[k], v1 = v_off[k + 1];
        std::string key((const char *)cts_u + 48 * k, 48);
        key.append((const char *)cts_w + 96 * k, 96);
        key.append((const char *)v_data + v0, v1 - v0);
        auto it = c->cc_map.find(key);
        if (it != c->cc_map.end()) {
            slot_of[k] = it->second;
            c->cc_used[it->second] = tick;
            continue;
        }
        u32 victim = 0;                  // least recently used slot not taken by this batch
        for (u32 j = 1; j < LCB_CT_CACHE; j++)
            if (c->cc_used[j] < c->cc_used[victim]) victim = j;
        if (!c->cc_keys[victim].empty()) c->cc_map.erase(c->cc_keys[victim]);
        c->cc_keys[victim] = key;
        c->cc_map.emplace(std::move(key), victim);
        c->cc_used[victim] = tick;
        slot_of[k] = victim;
        miss.push_back((u32)k);
    }
    // prepare the misses straight into their slots
    if (!kmiss.empty()) {
        const size_t km = kmiss.size() / 48;
        const uint8_t *dy = h.in(kmiss.data(), kmiss.size());
        if (!h.ok()) return cache_fail();
        lcbk_g1_decompress(dim3(nblk(km)), s, dy, (u32)km, (uint8_t *)keys + (size_t)kfirst * LCB_G1A_ST_BYTES);
    }
    if (!miss.empty()) {
        const size_t m = miss.size();
        std::vector<uint8_t> mu(48 * m), mw(96 * m), mv;
        std::vector<u32> mvo(1, 0), mslot(m), msets(2 * m);
        for (size_t j = 0; j < m; j++) {
            const u32 k = miss[j];
            memcpy(&mu[48 * j], cts_u + 48 * (size_t)k, 48);
            memcpy(&mw[96 * j], cts_w + 96 * (size_t)k, 96);
            mv.insert(mv.end(), v_data + v_off[k], v_data + v_off[k + 1]);
            mvo.push_back((u32)mv.size());
            mslot[j] = slot_of[k];
            msets[2 * j] = 2 * slot_of[k];
            msets[2 * j + 1] = 2 * slot_of[k] + 1;
        }
        if (mv.empty()) mv.push_back(0);
        const uint8_t *du = h.in(mu.data(), mu.size());
        const uint8_t *dw = h.in(mw.data(), mw.size());
        const uint8_t *dv = h.in(mv.data(), mv.size());
        const uint32_t *dvo = h.in(mvo.data(), mvo.size());
        const uint32_t *dsl = h.in(mslot.data(), m);
        const uint32_t *dse = h.in(msets.data(), 2 * m);
        if (h.ok() && injected(INJ_CT_CACHE_ALLOC)) h.fail();
        if (!h.ok()) return cache_fail();
        lcbk_tpke_ct_prepare(dim3(nblk(m)), s, du, dw, dv, dvo, (u32)m, lines, ctok, flags, dsl);
        lines_fill(s, lines, 2 * m, dse, nullptr);
    }
    std::vector<u32> cslot(n);
    for (size_t i = 0; i < n; i++) cslot[i] = slot_of[ct_idx[i]];
    const uint32_t *dct = h.in(cslot.data(), n);
    std::vector<u32> kdec(n);
    for (size_t i = 0; i < n; i++) kdec[i] = kslot[dec_idx[i]];
    const uint32_t *ddec = h.in(kdec.data(), n);
    const uint8_t *dui = h.in(ui, 48 * n);
    uint8_t *dacc = h.out<uint8_t>(n);
    if (!h.ok()) return cache_fail();
    if (tpke_verify_core(c, lines, ctok, LCB_CT_CACHE, keys, c->kc_n, dacc, n, dct, ddec, dui, s)) return cache_fail();
    h.back(accept, dacc, n);
    if (h.finish()) return cache_fail();
    return 0;
}
extern "C" int lcb_tpke_verify_shares(uint8_t *accept, size_t n, const uint8_t *y_keys, size_t n_keys,
                                      const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data,
                                      const uint32_t *v_off, size_t n_cts, const uint32_t *ct_idx,
                                      const uint32_t *dec_idx, const uint8_t *ui) {
    return tpke_verify_shares_host(accept, n, y_keys, n_keys, cts_u, cts_w, v_data, v_off, n_cts, ct_idx, dec_idx, ui,
                                   false);
}
extern "C" int lcb_tpke_verify_shares_batched(uint8_t *accept, size_t n, const uint8_t *y_keys, size_t n_keys,
                                              const uint8_t *cts_u, const uint8_t *cts_w, const uint8_t *v_data,
                                              const uint32_t *v_off, size_t n_cts, const uint32_t *ct_idx,
                                              const uint32_t *dec_idx, const uint8_t *ui) {
    return tpke_verify_shares_host(accept, n, y_keys, n_keys, cts_u, cts_w, v_data, v_off, n_cts, ct_idx, dec_idx, ui,
                                   true);
}

extern "C" int lcb_tpke_partial_decrypt(uint8_t *ui_out, uint8_t *status, const uint8_t x[32], const uint8_t *cts_u,
                                        const uint8_t *cts_w, const uint8_t *v_data, const uint32_t *v_off,
                                        size_t n_cts) {
    SYNC_CTX_OR(c, -1)
    if (!n_cts) return 0;
    HostCall h(c, "tpke partial decrypt");
    hipStream_t s = h.s;
    size_t vbytes = v_off[n_cts];
    const uint8_t *du = h.in(cts_u, 48 * n_cts);
    const uint8_t *dw = h.in(cts_w, 96 * n_cts);
    const uint8_t *dv = h.in(v_data, vbytes);
    const uint32_t *dvo = h.in(v_off, n_cts + 1);
    const uint8_t *dx = h.in(x, 32);
    uint8_t *dui = h.out<uint8_t>(48 * n_cts);
    uint8_t *dst = h.out<uint8_t>(n_cts);
    if (!h.ok()) return -1;
    if (tpke_prepare(c, nullptr, 0, du, dw, dv, dvo, n_cts, s)) return -1;
    if (tpke_partial_decrypt_prepared(c, dui, dst, dx, 0, du, n_cts, s)) return -1;
    h.back(ui_out, dui, 48 * n_cts);
    h.back(status, dst, n_cts);
    return h.finish();
}

extern "C" int lcb_tpke_encrypt_phase1(uint8_t *u_out, uint8_t *t_out, const uint8_t y[48], const uint8_t *r, size_t n) {
    SYNC_CTX_OR(c, -1)
    if (!n) return 0;
    HostCall h(c, "tpke encrypt1");
    const uint8_t *dy = h.in(y, 48);
    const uint8_t *dr = h.in(r, 32 * n);
    uint8_t *du = h.out<uint8_t>(48 * n), *dt = h.out<uint8_t>(48 * n), *dok = h.out<uint8_t>(n);
    u32 *ws = h.lws(lcbk_scalar_ws_bytes(3, (u32)n));
    if (!h.ok()) return -1;
    lcbk_tpke_encrypt1(h.s, dy, dr, (u32)n, du, dt, dok, ws);
    std::vector<uint8_t> ok(n);
    h.back(u_out, du, 48 * n);
    h.back(t_out, dt, 48 * n);
    h.back(ok.data(), dok, n);
    if (h.finish()) return -1;
    for (size_t i = 0; i < n; i++) if (!ok[i]) { set_err("invalid public key or scalar"); return -1; }
    return 0;
}
extern "C" int lcb_tpke_encrypt_phase2(uint8_t *w_out, const uint8_t *u, const uint8_t *r, const uint8_t *v_data,
                                       const uint32_t *v_off, size_t n) {
    SYNC_CTX_OR(c, -1)
    if (!n) return 0;
    HostCall h(c, "tpke encrypt2");
    const uint8_t *du = h.in(u, 48 * n);
    const uint8_t *dr = h.in(r, 32 * n);
    const uint8_t *dv = h.in(v_data, v_off[n]);
    const uint32_t *dvo = h.in(v_off, n + 1);
    uint8_t *dw = h.out<uint8_t>(96 * n), *dok = h.out<uint8_t>(n);
    if (!h.ok()) return -1;
    lcbk_tpke_encrypt2(dim3(nblk(n)), h.s, du, dr, dv, dvo, (u32)n, dw, dok, g_orig_cofactor);
    std::vector<uint8_t> ok(n);
    h.back(w_out, dw, 96 * n);
    h.back(ok.data(), dok, n);
    if (h.finish()) return -1;
    for (size_t i = 0; i < n; i++) if (!ok[i]) { set_err("hash-to-G2 failed"); return -1; }
    return 0;
}

// ================================================================== batch: threshold signatures
extern "C" int lcb_ctx_ts_prepare_dev(lcb_ctx *ctx, const uint8_t *pks, size_t n_pks, const uint8_t *msg_data,
                                      const uint32_t *msg_off, size_t n_msgs, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return ts_prepare(c, pks, n_pks, msg_data, msg_off, n_msgs, q.s);
}
extern "C" int lcb_ctx_ts_verify_prepared_dev(lcb_ctx *ctx, uint8_t *accept, size_t n, size_t n_pks, size_t n_msgs,
                                              const uint8_t *sigs, const uint32_t *msg_idx, const uint32_t *pk_idx,
                                              void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return ts_verify_prepared(c, accept, n, n_pks, n_msgs, sigs, msg_idx, pk_idx, q.s);
}
extern "C" int lcb_ctx_ts_assemble_dev(lcb_ctx *ctx, uint8_t *sig_out, uint8_t *status, const uint8_t *accept,
                                       const uint8_t *sigs, size_t per_round, size_t k, size_t n_rounds, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return assemble_enqueue(c, 2, sig_out, status, accept, sigs, per_round, k, n_rounds, q.s);
}
extern "C" int lcb_ctx_ts_assemble_ordered_dev(lcb_ctx *ctx, uint8_t *sig_out, uint8_t *status, const uint8_t *accept,
                                               const uint8_t *sigs, const uint32_t *order, size_t per_round, size_t k,
                                               size_t n_rounds, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return assemble_enqueue(c, 2, sig_out, status, accept, sigs, per_round, k, n_rounds, q.s, order);
}
extern "C" int lcb_ts_assemble_ordered_dev(uint8_t *sig_out, uint8_t *status, const uint8_t *accept, const uint8_t *sigs,
                                          const uint32_t *order, size_t per_round, size_t k, size_t n_rounds,
                                          void *stream) {
    return lcb_ctx_ts_assemble_ordered_dev(nullptr, sig_out, status, accept, sigs, order, per_round, k, n_rounds, stream);
}
extern "C" int lcb_ts_prepare_dev(const uint8_t *pks, size_t n_pks, const uint8_t *msg_data, const uint32_t *msg_off,
                                  size_t n_msgs, void *stream) {
    return lcb_ctx_ts_prepare_dev(nullptr, pks, n_pks, msg_data, msg_off, n_msgs, stream);
}
extern "C" int lcb_ts_verify_prepared_dev(uint8_t *accept, size_t n, size_t n_pks, size_t n_msgs, const uint8_t *sigs,
                                          const uint32_t *msg_idx, const uint32_t *pk_idx, void *stream) {
    return lcb_ctx_ts_verify_prepared_dev(nullptr, accept, n, n_pks, n_msgs, sigs, msg_idx, pk_idx, stream);
}
extern "C" int lcb_ts_assemble_dev(uint8_t *sig_out, uint8_t *status, const uint8_t *accept, const uint8_t *sigs,
                                   size_t per_round, size_t k, size_t n_rounds, void *stream) {
    return lcb_ctx_ts_assemble_dev(nullptr, sig_out, status, accept, sigs, per_round, k, n_rounds, stream);
}
extern "C" int lcb_ts_verify_shares_dev(uint8_t *accept, size_t n, const uint8_t *pks, size_t n_pks, const uint8_t *sigs,
                                        const uint8_t *msg_data, const uint32_t *msg_off, size_t n_msgs,
                                        const uint32_t *msg_idx, const uint32_t *pk_idx, void *stream) {
    CTX_OR(c, nullptr, -1)
    Enq q(c, (hipStream_t)stream);
    if (ts_prepare(c, pks, n_pks, msg_data, msg_off, n_msgs, q.s)) return -1;
    return ts_verify_prepared(c, accept, n, n_pks, n_msgs, sigs, msg_idx, pk_idx, q.s);
}
static int ts_verify_shares_host(uint8_t *accept, size_t n, const uint8_t *pks, size_t n_pks, const uint8_t *sigs,
                                 const uint8_t *msg_data, const uint32_t *msg_off, size_t n_msgs,
                                 const uint32_t *msg_idx, const uint32_t *pk_idx, bool batched) {
    SYNC_CTX_OR(c, -1)
    for (size_t i = 0; i < n; i++) {
        if (msg_idx[i] >= n_msgs) { set_err("msg_idx out of range"); return -1; }
        if (pk_idx[i] >= n_pks) { set_err("pk_idx out of range"); return -1; }
    }
    HostCall h(c, "ts verify");
    hipStream_t s = h.s;
    size_t mbytes = n_msgs ? msg_off[n_msgs] : 0;
    const uint8_t *dpk = h.in(pks, 48 * n_pks);
    const uint8_t *dsig = h.in(sigs, 96 * n);
    const uint8_t *dm = h.in(msg_data, mbytes);
    const uint32_t *dmo = h.in(msg_off, n_msgs + 1);
    const uint32_t *dmi = h.in(msg_idx, n);
    const uint32_t *dpi = h.in(pk_idx, n);
    uint8_t *dacc = h.out<uint8_t>(n);
    if (!h.ok()) return -1;
    if (batched) {
        if (ts_verify_shares_rlc_fused(c, dacc, n, dpk, n_pks, dsig, dm, dmo, n_msgs, dmi, dpi, s)) return -1;
    } else {
        if (ts_prepare(c, dpk, n_pks, dm, dmo, n_msgs, s)) return -1;
        if (ts_verify_prepared(c, dacc, n, n_pks, n_msgs, dsig, dmi, dpi, s)) return -1;
    }
    h.back(accept, dacc, n);
    return h.finish();
}
extern "C" int lcb_ts_verify_shares(uint8_t *accept, size_t n, const uint8_t *pks, size_t n_pks, const uint8_t *sigs,
                                    const uint8_t *msg_data, const uint32_t *msg_off, size_t n_msgs,
                                    const uint32_t *msg_idx, const uint32_t *pk_idx) {
    return ts_verify_shares_host(accept, n, pks, n_pks, sigs, msg_data, msg_off, n_msgs, msg_idx, pk_idx, false);
}
extern "C" int lcb_ts_verify_shares_batched(uint8_t *accept, size_t n, const uint8_t *pks, size_t n_pks,
                                            const uint8_t *sigs, const uint8_t *msg_data, const uint32_t *msg_off,
                                            size_t n_msgs, const uint32_t *msg_idx, const uint32_t *pk_idx) {
    return ts_verify_shares_host(accept, n, pks, n_pks, sigs, msg_data, msg_off, n_msgs, msg_idx, pk_idx, true);
}
extern "C" int lcb_ts_sign(uint8_t *sigs_out, const uint8_t *sks, const uint8_t *msg_data, const uint32_t *msg_off,
                           const uint32_t *msg_idx, size_t n) {
    SYNC_CTX_OR(c, -1)
    if (!n) return 0;
    u32 nm = 0;
    for (size_t i = 0; i < n; i++) nm = msg_idx[i] + 1 > nm ? msg_idx[i] + 1 : nm;
    HostCall h(c, "ts sign");
    const uint8_t *dsk = h.in(sks, 32 * n);
    const uint8_t *dm = h.in(msg_data, msg_off[nm]);
    const uint32_t *dmo = h.in(msg_off, nm + 1);
    const uint32_t *dmi = h.in(msg_idx, n);
    uint8_t *dsig = h.out<uint8_t>(96 * n), *dok = h.out<uint8_t>(n);
    if (!h.ok()) return -1;
    lcbk_ts_sign(dim3(nblk(n)), h.s, dsk, dm, dmo, dmi, (u32)n, dsig, dok, g_orig_cofactor);
    std::vector<uint8_t> ok(n);
    h.back(sigs_out, dsig, 96 * n);
    h.back(ok.data(), dok, n);
    if (h.finish()) return -1;
    for (size_t i = 0; i < n; i++) if (!ok[i]) { set_err("invalid key share"); return -1; }
    return 0;
}

// ================================================================== coin consumers (CoinResult.Parity, block nonce)
extern "C" int lcb_coin_parity(const uint8_t *sig_bytes, size_t len) {
    uint32_t acc = 0;
    for (size_t i = 0; i < len; i++) acc ^= sig_bytes[i];
    return __builtin_popcount(acc) & 1;
}
extern "C" uint64_t lcb_coin_nonce(const uint8_t *sig_bytes, size_t len) {
    uint8_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < len; i++) r[i % 8] ^= sig_bytes[i];
    uint64_t v = 0;
    for (int j = 7; j >= 0; j--) v = (v << 8) | r[j];
    return v;
}
extern "C" int lcb_coin_fold_dev(uint8_t *parity, uint64_t *nonce, const uint8_t *sigs, size_t n, void *stream) {
    if (!ready()) return -1;
    if (n > 0xffffffffu) { set_err("coin fold: batch too large"); return -1; }
    if (n) lcbk_coin_fold(dim3(nblk(n)), (hipStream_t)stream, sigs, (u32)n, parity, nonce);
    return launch_ok("coin fold launch") ? 0 : -1;
}

// ================================================================== batch: Lagrange, scalar mul, hash, MSM
static int lagrange_batch(int g, uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys, const uint32_t *off,
                          size_t np) {
    SYNC_CTX_OR(c, -1)
    if (!np) return 0;
    HostCall h(c, "lagrange");
    size_t ne = off[np];
    size_t pb = g == 1 ? 48 : 96;
    const uint8_t *dx = h.in(xs, 32 * ne);
    const uint8_t *dy = h.in(ys, pb * ne);
    const uint32_t *doff = h.in(off, np + 1);
    uint8_t *dst = h.out<uint8_t>(np), *dout = h.out<uint8_t>(pb * np);
    if (!h.ok()) return -1;
    if (lagrange_enqueue(c, g, dout, dst, dx, dy, doff, np, ne, h.s)) return -1;
    h.back(out, dout, pb * np);
    h.back(status, dst, np);
    return h.finish();
}
extern "C" int lcb_ctx_g1_lagrange_dev(lcb_ctx *ctx, uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys,
                                       const uint32_t *off, size_t n_problems, size_t n_entries, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return n_problems ? lagrange_enqueue(c, 1, out, status, xs, ys, off, n_problems, n_entries, q.s) : 0;
}
extern "C" int lcb_ctx_g2_lagrange_dev(lcb_ctx *ctx, uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys,
                                       const uint32_t *off, size_t n_problems, size_t n_entries, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return n_problems ? lagrange_enqueue(c, 2, out, status, xs, ys, off, n_problems, n_entries, q.s) : 0;
}
extern "C" int lcb_g1_lagrange_dev(uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys,
                                   const uint32_t *off, size_t n_problems, size_t n_entries, void *stream) {
    return lcb_ctx_g1_lagrange_dev(nullptr, out, status, xs, ys, off, n_problems, n_entries, stream);
}
extern "C" int lcb_g2_lagrange_dev(uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys,
                                   const uint32_t *off, size_t n_problems, size_t n_entries, void *stream) {
    return lcb_ctx_g2_lagrange_dev(nullptr, out, status, xs, ys, off, n_problems, n_entries, stream);
}
extern "C" int lcb_g1_lagrange_batch(uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys,
                                     const uint32_t *off, size_t n) { return lagrange_batch(1, out, status, xs, ys, off, n); }
extern "C" int lcb_g2_lagrange_batch(uint8_t *out, uint8_t *status, const uint8_t *xs, const uint8_t *ys,
                                     const uint32_t *off, size_t n) { return lagrange_batch(2, out, status, xs, ys, off, n); }

static int mul_batch(int g, uint8_t *out, const uint8_t *points, int use_gen, const uint8_t *scalars, size_t n) {
    SYNC_CTX_OR(c, -1)
    if (!n) return 0;
    if (n > 0xffffffffu) { set_err("mul batch: too large"); return -1; }
    HostCall h(c, "mul batch");
    size_t pb = g == 1 ? 48 : 96;
    hipStream_t s = h.s;
    const uint8_t *dp = use_gen ? h.out<uint8_t>(16) : h.in(points, pb * n);
    const uint8_t *dsc = h.in(scalars, 32 * n);
    uint8_t *dout = h.out<uint8_t>(pb * n), *dok = h.out<uint8_t>(n);
    u32 *ws = h.lws(lcbk_scalar_ws_bytes(g, (u32)n));
    if (!h.ok()) return -1;
    if (g == 1) lcbk_g1_mul(s, dp, use_gen, dsc, (u32)n, dout, dok, ws);
    else lcbk_g2_mul(s, dp, use_gen, dsc, (u32)n, dout, dok, ws);
    std::vector<uint8_t> ok(n);
    h.back(out, dout, pb * n);
    h.back(ok.data(), dok, n);
    if (h.finish()) return -1;
    for (size_t i = 0; i < n; i++) if (!ok[i]) { set_err("invalid point or scalar"); return -1; }
    return 0;
}
extern "C" int lcb_g1_mul_batch(uint8_t *out, const uint8_t *points, int gen, const uint8_t *scalars, size_t n) {
    return mul_batch(1, out, points, gen, scalars, n);
}
extern "C" int lcb_g2_mul_batch(uint8_t *out, const uint8_t *points, int gen, const uint8_t *scalars, size_t n) {
    return mul_batch(2, out, points, gen, scalars, n);
}
extern "C" int lcb_g2_hash_batch(uint8_t *out, const uint8_t *msg_data, const uint32_t *msg_off, size_t n) {
    SYNC_CTX_OR(c, -1)
    if (!n) return 0;
    HostCall h(c, "hash batch");
    const uint8_t *dm = h.in(msg_data, msg_off[n]);
    const uint32_t *dmo = h.in(msg_off, n + 1);
    uint8_t *dout = h.out<uint8_t>(96 * n), *dok = h.out<uint8_t>(n);
    if (!h.ok()) return -1;
    lcbk_g2_hash(dim3(nblk(n)), h.s, dm, dmo, (u32)n, dout, dok, g_orig_cofactor);
    std::vector<uint8_t> ok(n);
    h.back(out, dout, 96 * n);
    h.back(ok.data(), dok, n);
    if (h.finish()) return -1;
    for (size_t i = 0; i < n; i++) if (!ok[i]) { set_err("hash-to-G2 failed"); return -1; }
    return 0;
}

extern "C" int lcb_g1_msm_window(size_t n) { return (int)msm_window(n); }
extern "C" int lcb_g1_msm_glv_window(size_t n) { return msm_use_glv(n) ? (int)msm_window(n, true) : -(int)msm_window(n); }
// GLV form: every point must have order r (generated as a G or checked); see include/lachain_bls.h
extern "C" int lcb_ctx_g1_msm_glv_dev(lcb_ctx *ctx, void *out_jac, const void *points_aff, const uint8_t *scalars,
                                      size_t n, int window_bits, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    bool glv = window_bits > 0 || msm_use_glv(n);   // an explicit width selects the GLV form
    return msm_enqueue(c, out_jac, points_aff, scalars, n, window_bits, q.s, glv);
}
extern "C" int lcb_g1_msm_glv_dev(void *out_jac, const void *points_aff, const uint8_t *scalars, size_t n,
                                  int window_bits, void *stream) {
    return lcb_ctx_g1_msm_glv_dev(nullptr, out_jac, points_aff, scalars, n, window_bits, stream);
}
extern "C" int lcb_ctx_g1_msm_dev(lcb_ctx *ctx, void *out_jac, const void *points_aff, const uint8_t *scalars, size_t n,
                                  int window_bits, void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    return msm_enqueue(c, out_jac, points_aff, scalars, n, window_bits, q.s);
}
extern "C" int lcb_g1_msm_dev(void *out_jac, const void *points_aff, const uint8_t *scalars, size_t n, int window_bits,
                              void *stream) {
    return lcb_ctx_g1_msm_dev(nullptr, out_jac, points_aff, scalars, n, window_bits, stream);
}
extern "C" int lcb_ctx_g1_msm_phase_ms(lcb_ctx *ctx, float *ms, int n_phases) {
    CTX_OR(c, ctx, -1)
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!c->msm_ran) { set_err("msm: no MSM has run in this context"); return -1; }
    if (hipEventSynchronize(c->msm_ev[6]) != hipSuccess) { set_err("msm: event sync"); return -1; }
    for (int i = 0; i < n_phases && i < 6; i++)
        if (hipEventElapsedTime(&ms[i], c->msm_ev[i], c->msm_ev[i + 1]) != hipSuccess) ms[i] = -1.0f;
    return 0;
}
extern "C" int lcb_g1_msm_phase_ms(float *ms, int n_phases) { return lcb_ctx_g1_msm_phase_ms(nullptr, ms, n_phases); }
extern "C" int lcb_g1_to_affine_dev(void *out_aff, uint8_t *ok, const uint8_t *points, size_t n, void *stream) {
    if (!ready()) return -1;
    if (n > 0xffffffffu) { set_err("to_affine: batch too large"); return -1; }
    if (n) lcbk_g1_to_affine(dim3(nblk(n)), (hipStream_t)stream, points, (u32)n, out_aff, ok);
    return launch_ok("to_affine launch") ? 0 : -1;
}
extern "C" int lcb_ctx_g1_jac_sum_dev(lcb_ctx *ctx, uint8_t *out48, void *out_jac, const void *parts, size_t k,
                                      void *stream) {
    CTX_OR(c, ctx, -1)
    Enq q(c, (hipStream_t)stream);
    if (k == 1 && !out_jac && out48) {          // one partial (a single rank): serialise it as it is
        lcbk_g1_jac_compress(dim3(1), q.s, parts, 1, out48);
        return launch_ok("jac sum launch") ? 0 : -1;
    }
    void *acc = out_jac ? out_jac : c->msm[MSM_JAC_SUM].get(LCB_G1_JAC_BYTES);
    if (!acc) { set_err("device allocation failed"); return -1; }
    lcbk_g1_jac_reduce_groups(dim3(1), q.s, parts, (u32)k, k ? (u32)k : 1u, acc);
    if (out48) lcbk_g1_jac_compress(dim3(1), q.s, acc, 1, out48);
    return launch_ok("jac sum launch") ? 0 : -1;
}
extern "C" int lcb_g1_jac_sum_dev(uint8_t *out48, void *out_jac, const void *parts, size_t k, void *stream) {
    return lcb_ctx_g1_jac_sum_dev(nullptr, out48, out_jac, parts, k, stream);
}
// canonical Fr bytes (32-byte LE < r)
static bool fr_bytes_lt_r(const uint8_t *b) {
    for (int j = 7; j >= 0; j--) {
        uint32_t w = (uint32_t)b[4 * j] | (uint32_t)b[4 * j + 1] << 8 | (uint32_t)b[4 * j + 2] << 16 | (uint32_t)b[4 * j + 3] << 24;
        if (w != LCB_R_HOST[j]) return w < LCB_R_HOST[j];
    }
    return false;
}
extern "C" int lcb_g1_msm(uint8_t out[48], const uint8_t *points, const uint8_t *scalars, size_t n) {
    SYNC_CTX_OR(c, -1)
    if (n == 0) { memset(out, 0, 48); return 0; }
    for (size_t i = 0; i < n; i++) {   // mclBnFr values are canonical (< r); reject what mcl would not hold
        const uint8_t *sc = scalars + 32 * i;
        if (!fr_bytes_lt_r(sc)) { set_err("invalid point or scalar"); return -1; }
    }
    HostCall h(c, "msm");
    hipStream_t s = h.s;
    const uint8_t *dp = h.in(points, 48 * n);
    const uint8_t *dsc = h.in(scalars, 32 * n);
    void *aff = h.out<uint8_t>(96 * n);
    uint8_t *dok = h.out<uint8_t>(n), *dout = h.out<uint8_t>(48);
    void *jac = h.out<uint8_t>(LCB_G1_JAC_BYTES);
    if (!h.ok()) return -1;
    lcbk_g1_to_affine(dim3(nblk(n)), s, dp, (u32)n, aff, dok);
    if (msm_enqueue(c, jac, aff, dsc, n, 0, s)) return -1;
    lcbk_g1_jac_compress(dim3(1), s, jac, 1, dout);
    std::vector<uint8_t> ok(n);
    h.back(out, dout, 48);
    h.back(ok.data(), dok, n);
    if (h.finish()) return -1;
    for (size_t i = 0; i < n; i++) if (!ok[i]) { set_err("invalid point or scalar"); return -1; }
    return 0;
}

// ================================================================== KDF (host byte work)
extern "C" void lcb_xor_with_hash(uint8_t *out, const uint8_t g1b[48], const uint8_t *data, size_t len) {
    lcb_host::xor_with_hash(out, g1b, data, len);
}
