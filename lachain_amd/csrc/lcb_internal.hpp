// lachain_amd/csrc/lcb_internal.hpp — the few host internals the host files share: what lcb_host.cpp gives every
// feature file (error slot, device, context resolution, launch / synchronisation checks, fault injection),
// what the batch-check driver (lcb_batch.cpp) and the mcl surface (lcb_mcl.cpp) need from the exact paths in
// lcb_host.cpp, and the driver calls lcb_host.cpp's host-pointer entry points make.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include "lcb_ctx.hpp"

namespace lcb_int {
// ---- lcb_host.cpp, for every host file
void set_err(const char *what, hipError_t e = hipSuccess);   // the calling thread's lcb_last_error / lcb_error_count
bool ready();                         // the library is usable from this thread (device opened once, bound per thread)
int device();
lcb_ctx *ctx_resolve(lcb_ctx *c);     // explicit context, or the calling thread's default *_dev context
lcb_ctx *ctx_sync();                  // the calling thread's context for host-pointer entry points
bool launch_ok(const char *what);     // hipGetLastError after launches
bool sync_check(lcb_ctx *c, const char *what);   // the same, then the context's stream synchronised
#define CTX_OR(var, ctxarg, ret)                 \
    lcb_ctx *var = ctx_resolve(ctxarg);          \
    if (!var) return ret;
#define SYNC_CTX_OR(var, ret)                    \
    lcb_ctx *var = ctx_sync();                   \
    if (!var) return ret;
inline uint32_t nblk(size_t n) { return (uint32_t)((n + 255) / 256); }   // blocks of 256 lanes
// fault injection (lcb_test_inject_failure, LCB_ALLOW_TEST_HOOKS=1): the next `count` passes through site `site` fail
enum { INJ_STAGE_HOST_ALLOC = 1, INJ_CT_CACHE_ALLOC = 2, INJ_PAIRING_ALLOC = 3, INJ_STAGE_OP = 4 };
bool injected(int site);              // consumes one pending failure at `site`
bool inject_armed(int site);          // a pending failure at `site` (not consumed)
extern int g_orig_cofactor;           // lcb_set_original_g2_cofactor: the hashing kernels' cofactor flag

// ---- the feature files, for lcb_host.cpp's context release
void ecdsa_ctx_release(lcb_ctx *c);   // lcb_ecdsa.cpp: the context's cached key set
void ecies_ctx_release(lcb_ctx *c);   // lcb_ecies.cpp: the envelope workspaces and events
void txhash_ctx_release(lcb_ctx *c);  // lcb_txhash.cpp: the transaction workspaces and events
void rawtx_ctx_release(lcb_ctx *c);   // lcb_rawtx.cpp: the raw-transaction ingress's workspaces and events
void trie_ctx_release(lcb_ctx *c);    // lcb_trie.cpp: the state-trie workspaces
void kdf_ctx_release(lcb_ctx *c);     // lcb_kdf.cpp: the keystream compositions' workspaces and events

// ---- lcb_host.cpp, for lcb_batch.cpp
bool env_on(const char *name);              // an opt-in switch of the environment, read at call time
bool tuning_allowed(const char *what);      // LCB_ALLOW_TUNING=1, else the error names `what`
int prepare_flags();                        // the prepare kernels' flag word: original cofactor | line mode << 1
void lines_fill(hipStream_t s, uint32_t *lines, size_t n, const uint32_t *sets, uint8_t *w_g2);
void lines_flag_enqueue(lcb_ctx *c, int which, const uint32_t *lines, uint32_t c0, uint32_t c1, hipStream_t s);
bool lines_unnormalised(lcb_ctx *c, int which);
bool tpke_shape_ok(lcb_ctx *c, size_t n_keys, size_t n_cts, const char *what);
bool ts_shape_ok(lcb_ctx *c, size_t n_pks, size_t n_msgs, const char *what);

// ---- lcb_host.cpp, for lcb_mcl.cpp: device-side Lagrange at 0 (mclBn_G1 / G2LagrangeInterpolation's batch path)
int lagrange_enqueue(lcb_ctx *c, int g, uint8_t *dout, uint8_t *dst, const uint8_t *dx, const uint8_t *dy,
                     const uint32_t *doff, size_t np, size_t ne, hipStream_t s, const uint32_t *src = nullptr,
                     bool pairs = false);

// ---- lcb_host.cpp, for lcb_kdf.cpp: the first k accepted shares of every group (index order, or `order`), combined at 0
int assemble_enqueue(lcb_ctx *c, int g, uint8_t *out, uint8_t *status, const uint8_t *accept, const uint8_t *pts,
                     size_t per_group, size_t k, size_t n_groups, hipStream_t s, const uint32_t *order = nullptr);

// ---- lcb_batch.cpp, for lcb_host.cpp
extern std::atomic<uint32_t> g_coop_max;    // lcb_set_coop_max: the exact TPKE check (tpke_verify_core) reads it too
int tpke_verify_shares_rlc_fused(lcb_ctx *c, uint8_t *d_accept, size_t n, const uint8_t *d_y, size_t n_keys,
                                 const uint8_t *d_u, const uint8_t *d_w, const uint8_t *d_v, const uint32_t *d_voff,
                                 size_t n_cts, const uint32_t *d_ct, const uint32_t *d_dec, const uint8_t *d_ui,
                                 hipStream_t s);
int ts_verify_shares_rlc_fused(lcb_ctx *c, uint8_t *d_accept, size_t n, const uint8_t *d_pks, size_t n_pks,
                               const uint8_t *d_sigs, const uint8_t *d_msg, const uint32_t *d_moff, size_t n_msgs,
                               const uint32_t *d_midx, const uint32_t *d_pidx, hipStream_t s);
}  // namespace lcb_int

// ---- lcb_mcl.cpp, for lcb_host.cpp (at global scope, as it always was: the library's unmangled exports stay the same)
extern std::atomic<int> g_g2_sign_b;        // lcb_set_g2_sign_from_b: lcb_test_linesets decodes its points with it too

#include "host_call.hpp"                    // HostCall: the scope and staging slots of a host-pointer entry point
