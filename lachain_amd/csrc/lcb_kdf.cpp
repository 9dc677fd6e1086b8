// lachain_amd/csrc/lcb_kdf.cpp — host side of the device keystream (include/lachain_bls.h "TPKE keystream"; SURVEY.md §8
// row a7): Utils.XorWithHash for a batch, and the two TPKE operations it used to cut in half, each in one call.
//
// Reference calls: Utils.XorWithHash (TPKE/Utils.cs:12-19), PublicKey.Encrypt (TPKE/PublicKey.cs:25-37: U = rG,
// V = data ^ KDF(rY), W = r H(U || V)), PublicKey.FullDecrypt (TPKE/PublicKey.cs:55-86: u = sum lambda_i U_i,
// plaintext = V ^ KDF(u)).  Each composition is the existing kernels with k_kdf_xor (k_kdf.hip) between or behind them
// on one stream; what passes from stage to stage (T, u, the evaluation points) stays on the device in the context's
// named buffers (lcb_ctx::kdf).  T and u open the ciphertext: their buffers are cleared on the stream once the
// keystream has read them, and a host form clears its staged copy of r.  No constant-time claim is made.  No CPU
// fallback: the single-item lcb_xor_with_hash stays the host keystream it was.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>

#include "launch.h"
#include "lcb_internal.hpp"
#include "../../include/lachain_bls.h"

using namespace lcb_int;

namespace {

const size_t MAX_ITEMS = 0x7fffffffu;

bool events_ready(lcb_ctx *c) {
    if (c->kdf_ev_ready) return true;
    for (auto &e : c->kdf_ev)
        if (hipEventCreate(&e) != hipSuccess) { set_err("event creation"); return false; }
    c->kdf_ev_ready = true;
    return true;
}
void wipe(DevBuf &b, size_t bytes, hipStream_t s) {
    if (b.p && bytes) (void)hipMemsetAsync(b.p, 0, bytes < b.cap ? bytes : b.cap, s);
}
// rebase() for the TPKE family's 32-bit offsets
bool rebase32(std::vector<uint32_t> &rel, const uint32_t *off, size_t n, const char *err) {
    rel.assign(n + 1, 0);
    for (size_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) { set_err(err); return false; }
    for (size_t i = 1; i <= n; i++) rel[i] = off[i] - off[0];
    return true;
}

// the keystream kernel between the context's two events: seed_off, or 48-byte seeds back to back
int kdf_enqueue(lcb_ctx *c, hipStream_t s, uint8_t *out, const uint8_t *seeds, const uint32_t *seed_off, const uint8_t *data,
                const uint32_t *data_off, const uint8_t *ok, size_t n) {
    if (!events_ready(c)) return -1;
    (void)hipEventRecord(c->kdf_ev[0], s);
    if (seed_off) lcbk_kdf_xor(s, out, seeds, seed_off, data, data_off, ok, (u32)n);
    else lcbk_kdf_xor_strided(s, out, seeds, 48, data, data_off, ok, (u32)n);
    (void)hipEventRecord(c->kdf_ev[1], s);
    c->kdf_ran = true;
    return launch_ok("xor with hash launch") ? 0 : -1;
}

// Encrypt on device pointers: phase 1, the keystream with T as seeds, phase 2.  ok1: key and scalar validity (an item
// with ok1 = 0 gets a zero V), ok2: H(U || V) exists.
int encrypt_enqueue(lcb_ctx *c, hipStream_t s, uint8_t *u_out, uint8_t *v_out, uint8_t *w_out, uint8_t *ok1, uint8_t *ok2,
                    const uint8_t *y, const uint8_t *r, const uint8_t *data, const uint32_t *data_off, size_t n) {
    uint8_t *t = (uint8_t *)c->kdf[KDF_T].get(48 * n);
    u32 *ws = (u32 *)c->lws.get(lcbk_scalar_ws_bytes(3, (u32)n));
    if (!t || !ws) { set_err("device allocation failed"); return -1; }
    lcbk_tpke_encrypt1(s, y, r, (u32)n, u_out, t, ok1, ws);
    const int rc = kdf_enqueue(c, s, v_out, t, nullptr, data, data_off, ok1, n);
    wipe(c->kdf[KDF_T], 48 * n, s);
    if (rc) return -1;
    lcbk_tpke_encrypt2(dim3(nblk(n)), s, u_out, r, v_out, data_off, (u32)n, w_out, ok2, g_orig_cofactor);
    return launch_ok("tpke encrypt launch") ? 0 : -1;
}

// FullDecrypt literally on device pointers: problem j combines all its entries at x = ids + 1, then opens V_j
int literal_enqueue(lcb_ctx *c, hipStream_t s, uint8_t *pt_out, uint8_t *status, const int32_t *ids, const uint8_t *uis,
                    const uint32_t *off, const uint8_t *v_data, const uint32_t *v_off, size_t n, size_t ne) {
    uint8_t *xs = (uint8_t *)c->kdf[KDF_XS].get(32 * ne), *u = (uint8_t *)c->kdf[KDF_U].get(48 * n);
    if (!xs || !u) { set_err("device allocation failed"); return -1; }
    lcbk_tpke_ids_to_x(s, ids, (u32)ne, xs);
    if (lagrange_enqueue(c, 1, u, status, xs, uis, off, n, ne, s)) return -1;
    const int rc = kdf_enqueue(c, s, pt_out, u, nullptr, v_data, v_off, status, n);
    wipe(c->kdf[KDF_U], 48 * n, s);
    return rc;
}

}  // namespace

namespace lcb_int {
void kdf_ctx_release(lcb_ctx *c) {
    if (c->kdf_ev_ready) for (auto &e : c->kdf_ev) (void)hipEventDestroy(e);
    c->kdf_ev_ready = false;
    for (auto &b : c->kdf) b.release();
}
}  // namespace lcb_int

// ------------------------------------------------------------------ Utils.XorWithHash
extern "C" int lcb_ctx_xor_with_hash_dev(lcb_ctx *ctx, uint8_t *out, const uint8_t *seeds, const uint32_t *seed_off,
                                         const uint8_t *data, const uint32_t *data_off, size_t n, void *stream) {
    CTX_OR(c, ctx, -1)
    if (n > MAX_ITEMS) { set_err("xor with hash: batch too large"); return -1; }
    if (n && !seed_off) { set_err("xor with hash: seed offsets are required"); return -1; }
    Enq q(c, (hipStream_t)stream);
    if (!n) return 0;
    return kdf_enqueue(c, q.s, out, seeds, seed_off, data, data_off, nullptr, n);
}
extern "C" int lcb_xor_with_hash_dev(uint8_t *out, const uint8_t *seeds, const uint32_t *seed_off, const uint8_t *data,
                                     const uint32_t *data_off, size_t n, void *stream) {
    return lcb_ctx_xor_with_hash_dev(nullptr, out, seeds, seed_off, data, data_off, n, stream);
}
extern "C" int lcb_xor_with_hash_batch(uint8_t *out, const uint8_t *seeds, const uint32_t *seed_off, const uint8_t *data,
                                       const uint32_t *data_off, size_t n) {
    SYNC_CTX_OR(c, -1)
    if (!n) return 0;
    if (n > MAX_ITEMS) { set_err("xor with hash: batch too large"); return -1; }
    std::vector<uint32_t> soff, doff;
    if (!rebase32(soff, seed_off, n, "xor with hash: seed offsets must not decrease") ||
        !rebase32(doff, data_off, n, "xor with hash: data offsets must not decrease"))
        return -1;
    HostCall h(c, "xor with hash");
    const uint8_t *dseed = h.in(seeds + seed_off[0], soff[n]);
    const uint32_t *dsoff = h.in(soff.data(), n + 1);
    const uint8_t *dd = h.in(data + data_off[0], doff[n]);
    const uint32_t *ddoff = h.in(doff.data(), n + 1);
    uint8_t *dout = h.out<uint8_t>(doff[n]);
    if (!h.ok()) return -1;
    if (lcb_ctx_xor_with_hash_dev(c, dout, dseed, dsoff, dd, ddoff, n, h.s)) return -1;
    h.back(out + data_off[0], dout, doff[n]);
    return h.finish();
}
// kernel milliseconds of k_kdf_xor in the context's last keystream call (any of the entry points of this file)
extern "C" int lcb_ctx_kdf_phase_ms(lcb_ctx *ctx, float ms[1]) {
    CTX_OR(c, ctx, -1)
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!c->kdf_ran) { set_err("no keystream call has run in this context"); return -1; }
    hipError_t e = hipEventSynchronize(c->kdf_ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms[0], c->kdf_ev[0], c->kdf_ev[1]);
    if (e != hipSuccess) { set_err("kdf phase timing", e); return -1; }
    return 0;
}
// the same for the calling thread's host-pointer forms (they run in the thread's own synchronous context)
extern "C" int lcb_kdf_phase_ms(float ms[1]) {
    SYNC_CTX_OR(c, -1)
    return lcb_ctx_kdf_phase_ms(c, ms);
}

// ------------------------------------------------------------------ PublicKey.Encrypt
extern "C" int lcb_ctx_tpke_encrypt_dev(lcb_ctx *ctx, uint8_t *u_out, uint8_t *v_out, uint8_t *w_out, uint8_t *ok,
                                        const uint8_t *y, const uint8_t *r, const uint8_t *data, const uint32_t *data_off,
                                        size_t n, void *stream) {
    CTX_OR(c, ctx, -1)
    if (n > MAX_ITEMS) { set_err("tpke encrypt: batch too large"); return -1; }
    Enq q(c, (hipStream_t)stream);
    if (!n) return 0;
    uint8_t *ok1 = ok ? ok : (uint8_t *)c->kdf[KDF_OK1].get(n), *ok2 = (uint8_t *)c->kdf[KDF_OK2].get(n);
    if (!ok1 || !ok2) { set_err("device allocation failed"); return -1; }
    if (encrypt_enqueue(c, q.s, u_out, v_out, w_out, ok1, ok2, y, r, data, data_off, n)) return -1;
    if (ok) lcbk_ct_ok_merge(q.s, ok, ok2, 0, (u32)n);
    return launch_ok("tpke encrypt launch") ? 0 : -1;
}
extern "C" int lcb_tpke_encrypt_dev(uint8_t *u_out, uint8_t *v_out, uint8_t *w_out, uint8_t *ok, const uint8_t *y,
                                    const uint8_t *r, const uint8_t *data, const uint32_t *data_off, size_t n, void *stream) {
    return lcb_ctx_tpke_encrypt_dev(nullptr, u_out, v_out, w_out, ok, y, r, data, data_off, n, stream);
}
extern "C" int lcb_tpke_encrypt_batch(uint8_t *u_out, uint8_t *v_out, uint8_t *w_out, const uint8_t y[48], const uint8_t *r,
                                      const uint8_t *data, const uint32_t *data_off, size_t n) {
    SYNC_CTX_OR(c, -1)
    if (!n) return 0;
    if (n > MAX_ITEMS) { set_err("tpke encrypt: batch too large"); return -1; }
    std::vector<uint32_t> doff;
    if (!rebase32(doff, data_off, n, "tpke encrypt: data offsets must not decrease")) return -1;
    HostCall h(c, "tpke encrypt");
    const uint8_t *dy = h.in(y, 48);
    const uint8_t *dr = h.in(r, 32 * n);
    const uint8_t *dd = h.in(data + data_off[0], doff[n]);
    const uint32_t *ddoff = h.in(doff.data(), n + 1);
    uint8_t *du = h.out<uint8_t>(48 * n), *dv = h.out<uint8_t>(doff[n]), *dw = h.out<uint8_t>(96 * n);
    uint8_t *dok1 = h.out<uint8_t>(n), *dok2 = h.out<uint8_t>(n);
    const int rc = h.ok() ? encrypt_enqueue(c, h.s, du, dv, dw, dok1, dok2, dy, dr, dd, ddoff, n) : -1;
    h.wipe(dr, 32 * n);
    if (rc) return -1;
    std::vector<uint8_t> ok1(n), ok2(n);
    h.back(u_out, du, 48 * n);
    h.back(v_out + data_off[0], dv, doff[n]);
    h.back(w_out, dw, 96 * n);
    h.back(ok1.data(), dok1, n);
    h.back(ok2.data(), dok2, n);
    if (h.finish()) return -1;
    for (size_t i = 0; i < n; i++) if (!ok1[i]) { set_err("invalid public key or scalar"); return -1; }
    for (size_t i = 0; i < n; i++) if (!ok2[i]) { set_err("hash-to-G2 failed"); return -1; }
    return 0;
}

// ------------------------------------------------------------------ PublicKey.FullDecrypt
extern "C" int lcb_ctx_tpke_full_decrypt_dev(lcb_ctx *ctx, uint8_t *pt_out, uint8_t *status, const uint8_t *accept,
                                             const uint8_t *shares, const uint32_t *order, size_t per_ct, size_t k,
                                             const uint8_t *v_data, const uint32_t *v_off, size_t n_cts, void *stream) {
    CTX_OR(c, ctx, -1)
    if (n_cts > MAX_ITEMS) { set_err("tpke full decrypt: batch too large"); return -1; }
    Enq q(c, (hipStream_t)stream);
    if (!n_cts) return 0;
    uint8_t *u = (uint8_t *)c->kdf[KDF_U].get(48 * n_cts);
    if (!u) { set_err("device allocation failed"); return -1; }
    if (assemble_enqueue(c, 1, u, status, accept, shares, per_ct, k, n_cts, q.s, order)) return -1;
    const int rc = kdf_enqueue(c, q.s, pt_out, u, nullptr, v_data, v_off, status, n_cts);
    wipe(c->kdf[KDF_U], 48 * n_cts, q.s);
    return rc;
}
extern "C" int lcb_tpke_full_decrypt_dev(uint8_t *pt_out, uint8_t *status, const uint8_t *accept, const uint8_t *shares,
                                         const uint32_t *order, size_t per_ct, size_t k, const uint8_t *v_data,
                                         const uint32_t *v_off, size_t n_cts, void *stream) {
    return lcb_ctx_tpke_full_decrypt_dev(nullptr, pt_out, status, accept, shares, order, per_ct, k, v_data, v_off, n_cts,
                                         stream);
}
extern "C" int lcb_tpke_full_decrypt_batch(uint8_t *pt_out, uint8_t *status, const int32_t *ids, const uint8_t *uis,
                                           const uint32_t *off, const uint8_t *v_data, const uint32_t *v_off, size_t n_cts) {
    SYNC_CTX_OR(c, -1)
    if (!n_cts) return 0;
    if (n_cts > MAX_ITEMS) { set_err("tpke full decrypt: batch too large"); return -1; }
    std::vector<uint32_t> eoff, voff;
    if (!rebase32(eoff, off, n_cts, "tpke full decrypt: entry offsets must not decrease") ||
        !rebase32(voff, v_off, n_cts, "tpke full decrypt: data offsets must not decrease"))
        return -1;
    const size_t ne = eoff[n_cts];
    HostCall h(c, "tpke full decrypt");
    const int32_t *dids = h.in(ids + off[0], ne);
    const uint8_t *duis = h.in(uis + 48 * (size_t)off[0], 48 * ne);
    const uint32_t *deoff = h.in(eoff.data(), n_cts + 1);
    const uint8_t *dv = h.in(v_data + v_off[0], voff[n_cts]);
    const uint32_t *dvoff = h.in(voff.data(), n_cts + 1);
    uint8_t *dpt = h.out<uint8_t>(voff[n_cts]), *dst = h.out<uint8_t>(n_cts);
    if (!h.ok()) return -1;
    if (literal_enqueue(c, h.s, dpt, dst, dids, duis, deoff, dv, dvoff, n_cts, ne)) return -1;
    h.back(pt_out + v_off[0], dpt, voff[n_cts]);
    h.back(status, dst, n_cts);
    return h.finish();
}
