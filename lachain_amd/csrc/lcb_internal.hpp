// lachain_amd/csrc/lcb_internal.hpp — the few host internals the host files share: what lcb_host.cpp gives the
// feature files (error slot, context resolution, launch / synchronisation checks), what the batch-check driver
// (lcb_batch.cpp) needs from the exact paths in lcb_host.cpp, and the driver calls lcb_host.cpp's host-pointer entry
// points make.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include "lcb_ctx.hpp"

namespace lcb_int {
void set_error(const char *what, hipError_t e = hipSuccess);
lcb_ctx *ctx_resolve(lcb_ctx *c);     // explicit context, or the calling thread's default *_dev context
lcb_ctx *ctx_sync();                  // the calling thread's context for host-pointer entry points
bool launch_ok(const char *what);     // hipGetLastError after launches
bool sync_ok(lcb_ctx *c, const char *what);
int device();
void ecdsa_ctx_release(lcb_ctx *c);   // lcb_ecdsa.cpp: the context's cached key set
void ecies_ctx_release(lcb_ctx *c);   // lcb_ecies.cpp: the envelope workspaces and events
void txhash_ctx_release(lcb_ctx *c);  // lcb_txhash.cpp: the transaction workspaces and events

// ---- lcb_host.cpp, for lcb_batch.cpp
inline uint32_t nblk(size_t n) { return (uint32_t)((n + 255) / 256); }   // blocks of 256 lanes
bool env_on(const char *name);              // an opt-in switch of the environment, read at call time
bool tuning_allowed(const char *what);      // LCB_ALLOW_TUNING=1, else the error names `what`
int prepare_flags();                        // the prepare kernels' flag word: original cofactor | line mode << 1
void lines_fill(hipStream_t s, uint32_t *lines, size_t n, const uint32_t *sets, uint8_t *w_g2);
void lines_flag_enqueue(lcb_ctx *c, int which, const uint32_t *lines, uint32_t c0, uint32_t c1, hipStream_t s);
bool lines_unnormalised(lcb_ctx *c, int which);
bool tpke_shape_ok(lcb_ctx *c, size_t n_keys, size_t n_cts, const char *what);
bool ts_shape_ok(lcb_ctx *c, size_t n_pks, size_t n_msgs, const char *what);

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
