// lachain_amd/csrc/lcb_ecies.cpp — host side of the batched secp256k1 ECIES envelope (include/lachain_bls.h "secp256k1
// ECIES").
//
// Reference: every secret of the trustless DKG travels in DefaultCrypto.Secp256K1Encrypt and is opened by
// Secp256K1Decrypt (DefaultCrypto.cs:301-336; TrustlessKeygen.cs:63-76,90-135): Secp256K1.Ecdh (libsecp256k1's
// secp256k1_ecdh, default hash) gives the AES-256-GCM key, AesGcmEncrypt / AesGcmDecrypt (DefaultCrypto.cs:267-299) do
// the rest.  Kernels: k_ecies.hip; the ephemeral public key d G comes from the generator's comb table through
// lcb_ctx_ecdsa_pubkey_dev (k_secp.hip).  No CPU fallback.
//
// Secrets: the job records (the scalar's digits), the Jacobian results and the session keys live in the context's
// workspaces and are cleared on the stream before a call returns; so are the host-pointer forms' staging copies of
// private, ephemeral and session keys.  In the fused envelope calls the session keys never leave device memory.
#include <hip/hip_runtime.h>
#include <string.h>
#include <mutex>
#include <vector>

#include "launch.h"
#include "lcb_internal.hpp"
#include "../../include/lachain_bls.h"

using namespace lcb_int;

namespace {

enum { W_JOBS, W_PTS, W_KEYS, W_EOK, W_EPH, W_POK, W_OFF, S_PUB, S_SCALAR, S_IDX, S_OUT, S_NONCE, S_DATA, S_KEYS };

bool size_ok(const char *what, size_t n) {
    if (n > 0xffffffffu / 2) { set_err(what); return false; }
    return true;
}
bool events_ready(lcb_ctx *c) {
    if (c->ecies_ev_ready) return true;
    for (auto &e : c->ecies_ev)
        if (hipEventCreate(&e) != hipSuccess) { set_err("event creation"); return false; }
    c->ecies_ev_ready = true;
    return true;
}
void mark(lcb_ctx *c, hipStream_t s, int from) {       // events from .. 4 at this point of the stream
    for (int k = from; k < 5; k++) (void)hipEventRecord(c->ecies_ev[k], s);
    c->ecies_ran = true;
}
void wipe(DevBuf &b, size_t bytes, hipStream_t s) {
    if (b.p && bytes) (void)hipMemsetAsync(b.p, 0, bytes < b.cap ? bytes : b.cap, s);
}

// the three ECDH kernels on device pointers: events 0..3, job and point records cleared afterwards.  off / min_len:
// the keys are the first 33 bytes of variable-length items (the envelopes).
int ecdh_core(lcb_ctx *c, hipStream_t s, uint8_t *key32, uint8_t *ok, const uint8_t *pub, const uint64_t *off,
              u32 min_len, const uint8_t *scalars32, const u32 *idx, size_t n_scalars, size_t n) {
    size_t jb = lcbk_ecdh_job_bytes() * n, pb = lcbk_ecdh_point_bytes() * n;
    void *jobs = c->ecies[W_JOBS].get(jb), *pts = c->ecies[W_PTS].get(pb);
    if (!jobs || !pts) { set_err("device allocation failed"); return -1; }
    (void)hipEventRecord(c->ecies_ev[0], s);
    lcbk_ecdh_scalars(s, pub, off, min_len, scalars32, idx, (u32)(n_scalars > 0xffffffffu ? 0xffffffffu : n_scalars),
                      (u32)n, jobs);
    (void)hipEventRecord(c->ecies_ev[1], s);
    lcbk_ecdh_mul(s, jobs, (u32)n, pts);
    (void)hipEventRecord(c->ecies_ev[2], s);
    lcbk_ecdh_finish(s, pts, (u32)n, key32, ok);
    (void)hipEventRecord(c->ecies_ev[3], s);
    wipe(c->ecies[W_JOBS], jb, s);
    wipe(c->ecies[W_PTS], pb, s);
    return 0;
}

int ecdh_dev(lcb_ctx *c, hipStream_t s, uint8_t *key32, uint8_t *ok, const uint8_t *pub33, const uint8_t *scalars32,
             const u32 *idx, size_t n_scalars, size_t n) {
    if (!n) return 0;
    if (!key32 || !ok || !pub33 || !scalars32) { set_err("secp ecdh: null pointer"); return -1; }
    if (!size_ok("secp ecdh: batch too large", n) || !events_ready(c)) return -1;
    if (ecdh_core(c, s, key32, ok, pub33, nullptr, 0, scalars32, idx, idx ? n_scalars : n, n)) return -1;
    mark(c, s, 4);
    return launch_ok("secp ecdh launch") ? 0 : -1;
}
int gcm_encrypt_dev(lcb_ctx *c, hipStream_t s, uint8_t *out, const uint8_t *keys32, const uint8_t *nonces16,
                    const uint8_t *pt, const uint64_t *pt_off, size_t n) {
    if (!n) return 0;
    if (!out || !keys32 || !nonces16 || !pt || !pt_off) { set_err("aes-256-gcm encrypt: null pointer"); return -1; }
    if (!size_ok("aes-256-gcm encrypt: batch too large", n) || !events_ready(c)) return -1;
    mark(c, s, 0);
    lcbk_gcm_encrypt(s, keys32, nonces16, pt, pt_off, (u32)n, out, nullptr, nullptr);
    (void)hipEventRecord(c->ecies_ev[4], s);
    return launch_ok("aes-256-gcm encrypt launch") ? 0 : -1;
}
int gcm_decrypt_dev(lcb_ctx *c, hipStream_t s, uint8_t *pt_out, uint8_t *ok, const uint8_t *keys32, const uint8_t *ct,
                    const uint64_t *ct_off, size_t n) {
    if (!n) return 0;
    if (!pt_out || !ok || !keys32 || !ct || !ct_off) { set_err("aes-256-gcm decrypt: null pointer"); return -1; }
    if (!size_ok("aes-256-gcm decrypt: batch too large", n) || !events_ready(c)) return -1;
    uint64_t *oo = (uint64_t *)c->ecies[W_OFF].get(8 * (n + 1));
    if (!oo) { set_err("device allocation failed"); return -1; }
    mark(c, s, 0);
    lcbk_gcm_offsets(s, ct_off, (u32)n, 32, oo);
    lcbk_gcm_decrypt(s, keys32, ct, ct_off, oo, (u32)n, 0, pt_out, ok, nullptr);
    (void)hipEventRecord(c->ecies_ev[4], s);
    return launch_ok("aes-256-gcm decrypt launch") ? 0 : -1;
}
int envelope_encrypt_dev(lcb_ctx *c, hipStream_t s, uint8_t *out, uint8_t *ok, const uint8_t *recipient_pub33,
                         const uint8_t *eph_priv32, const uint8_t *nonces16, const uint8_t *pt, const uint64_t *pt_off,
                         size_t n) {
    if (!n) return 0;
    if (!out || !ok || !recipient_pub33 || !eph_priv32 || !nonces16 || !pt || !pt_off) {
        set_err("secp256k1 encrypt: null pointer");
        return -1;
    }
    if (!size_ok("secp256k1 encrypt: batch too large", n) || !events_ready(c)) return -1;
    uint8_t *keys = (uint8_t *)c->ecies[W_KEYS].get(32 * n), *eok = (uint8_t *)c->ecies[W_EOK].get(n);
    uint8_t *eph = (uint8_t *)c->ecies[W_EPH].get(33 * n), *pok = (uint8_t *)c->ecies[W_POK].get(n);
    if (!keys || !eok || !eph || !pok) { set_err("device allocation failed"); return -1; }
    if (ecdh_core(c, s, keys, eok, recipient_pub33, nullptr, 0, eph_priv32, nullptr, n, n)) return -1;
    // the ephemeral public keys d G from the generator's comb table (timed with the GCM phase)
    if (lcb_ctx_ecdsa_pubkey_dev(c, eph, pok, eph_priv32, n, s)) { wipe(c->ecies[W_KEYS], 32 * n, s); return -1; }
    lcbk_gcm_encrypt(s, keys, nonces16, pt, pt_off, (u32)n, out, eph, eok);
    (void)hipMemcpyAsync(ok, eok, n, hipMemcpyDeviceToDevice, s);
    (void)hipEventRecord(c->ecies_ev[4], s);
    c->ecies_ran = true;
    wipe(c->ecies[W_KEYS], 32 * n, s);
    return launch_ok("secp256k1 encrypt launch") ? 0 : -1;
}
int envelope_decrypt_dev(lcb_ctx *c, hipStream_t s, uint8_t *pt_out, uint8_t *ok, const uint8_t *privs32,
                         const u32 *priv_idx, size_t n_privs, const uint8_t *ct, const uint64_t *ct_off, size_t n) {
    if (!n) return 0;
    if (!pt_out || !ok || !privs32 || !ct || !ct_off) { set_err("secp256k1 decrypt: null pointer"); return -1; }
    if (!size_ok("secp256k1 decrypt: batch too large", n) || !events_ready(c)) return -1;
    uint8_t *keys = (uint8_t *)c->ecies[W_KEYS].get(32 * n), *eok = (uint8_t *)c->ecies[W_EOK].get(n);
    uint64_t *oo = (uint64_t *)c->ecies[W_OFF].get(8 * (n + 1));
    if (!keys || !eok || !oo) { set_err("device allocation failed"); return -1; }
    if (ecdh_core(c, s, keys, eok, ct, ct_off, 65, privs32, priv_idx, priv_idx ? n_privs : n, n)) return -1;
    lcbk_gcm_offsets(s, ct_off, (u32)n, 65, oo);
    lcbk_gcm_decrypt(s, keys, ct, ct_off, oo, (u32)n, 33, pt_out, ok, eok);
    (void)hipEventRecord(c->ecies_ev[4], s);
    c->ecies_ran = true;
    wipe(c->ecies[W_KEYS], 32 * n, s);
    return launch_ok("secp256k1 decrypt launch") ? 0 : -1;
}

// offsets of a host-pointer call: non-decreasing, rebased to off[0]; the summed plaintext lengths of a decryption
bool host_offsets(const char *what, std::vector<uint64_t> &rel, const uint64_t *off, size_t n) {
    rel.resize(n + 1);
    for (size_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) { set_err(what); return false; }
    for (size_t i = 0; i <= n; i++) rel[i] = off[i] - off[0];
    return true;
}
size_t plain_total(const std::vector<uint64_t> &rel, size_t overhead) {
    size_t t = 0;
    for (size_t i = 0; i + 1 < rel.size(); i++) {
        uint64_t len = rel[i + 1] - rel[i];
        if (len >= overhead) t += (size_t)(len - overhead);
    }
    return t;
}
void *stage(lcb_ctx *c, int slot, const void *src, size_t bytes, hipStream_t s) {
    void *d = c->ecies[slot].get(bytes);
    if (d && bytes) (void)hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, s);
    return d;
}

}  // namespace

namespace lcb_int {
void ecies_ctx_release(lcb_ctx *c) {
    if (c->ecies_ev_ready) for (auto &e : c->ecies_ev) (void)hipEventDestroy(e);
    c->ecies_ev_ready = false;
    for (auto &b : c->ecies) b.release();
}
}  // namespace lcb_int

// ------------------------------------------------------------------ device-pointer forms
extern "C" int lcb_ctx_secp_ecdh_dev(lcb_ctx *ctx, uint8_t *key32_out, uint8_t *ok, const uint8_t *pub33,
                                     const uint8_t *scalars32, const uint32_t *scalar_idx, size_t n_scalars, size_t n,
                                     void *stream) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    Enq q(c, (hipStream_t)stream);
    return ecdh_dev(c, q.s, key32_out, ok, pub33, scalars32, scalar_idx, n_scalars, n);
}
extern "C" int lcb_ctx_aes256_gcm_encrypt_dev(lcb_ctx *ctx, uint8_t *out, const uint8_t *keys32, const uint8_t *nonces16,
                                              const uint8_t *pt, const uint64_t *pt_off, size_t n, void *stream) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    Enq q(c, (hipStream_t)stream);
    return gcm_encrypt_dev(c, q.s, out, keys32, nonces16, pt, pt_off, n);
}
extern "C" int lcb_ctx_aes256_gcm_decrypt_dev(lcb_ctx *ctx, uint8_t *pt_out, uint8_t *ok, const uint8_t *keys32,
                                              const uint8_t *ct, const uint64_t *ct_off, size_t n, void *stream) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    Enq q(c, (hipStream_t)stream);
    return gcm_decrypt_dev(c, q.s, pt_out, ok, keys32, ct, ct_off, n);
}
extern "C" int lcb_ctx_secp256k1_encrypt_dev(lcb_ctx *ctx, uint8_t *out, uint8_t *ok, const uint8_t *recipient_pub33,
                                             const uint8_t *eph_priv32, const uint8_t *nonces16, const uint8_t *pt,
                                             const uint64_t *pt_off, size_t n, void *stream) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    Enq q(c, (hipStream_t)stream);
    return envelope_encrypt_dev(c, q.s, out, ok, recipient_pub33, eph_priv32, nonces16, pt, pt_off, n);
}
extern "C" int lcb_ctx_secp256k1_decrypt_dev(lcb_ctx *ctx, uint8_t *pt_out, uint8_t *ok, const uint8_t *privs32,
                                             const uint32_t *priv_idx, size_t n_privs, const uint8_t *ct,
                                             const uint64_t *ct_off, size_t n, void *stream) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    Enq q(c, (hipStream_t)stream);
    return envelope_decrypt_dev(c, q.s, pt_out, ok, privs32, priv_idx, n_privs, ct, ct_off, n);
}
extern "C" int lcb_secp_ecdh_dev(uint8_t *key32_out, uint8_t *ok, const uint8_t *pub33, const uint8_t *scalars32,
                                 const uint32_t *scalar_idx, size_t n_scalars, size_t n, void *stream) {
    return lcb_ctx_secp_ecdh_dev(nullptr, key32_out, ok, pub33, scalars32, scalar_idx, n_scalars, n, stream);
}
extern "C" int lcb_aes256_gcm_encrypt_dev(uint8_t *out, const uint8_t *keys32, const uint8_t *nonces16,
                                          const uint8_t *pt, const uint64_t *pt_off, size_t n, void *stream) {
    return lcb_ctx_aes256_gcm_encrypt_dev(nullptr, out, keys32, nonces16, pt, pt_off, n, stream);
}
extern "C" int lcb_aes256_gcm_decrypt_dev(uint8_t *pt_out, uint8_t *ok, const uint8_t *keys32, const uint8_t *ct,
                                          const uint64_t *ct_off, size_t n, void *stream) {
    return lcb_ctx_aes256_gcm_decrypt_dev(nullptr, pt_out, ok, keys32, ct, ct_off, n, stream);
}
extern "C" int lcb_secp256k1_encrypt_dev(uint8_t *out, uint8_t *ok, const uint8_t *recipient_pub33,
                                         const uint8_t *eph_priv32, const uint8_t *nonces16, const uint8_t *pt,
                                         const uint64_t *pt_off, size_t n, void *stream) {
    return lcb_ctx_secp256k1_encrypt_dev(nullptr, out, ok, recipient_pub33, eph_priv32, nonces16, pt, pt_off, n, stream);
}
extern "C" int lcb_secp256k1_decrypt_dev(uint8_t *pt_out, uint8_t *ok, const uint8_t *privs32, const uint32_t *priv_idx,
                                         size_t n_privs, const uint8_t *ct, const uint64_t *ct_off, size_t n,
                                         void *stream) {
    return lcb_ctx_secp256k1_decrypt_dev(nullptr, pt_out, ok, privs32, priv_idx, n_privs, ct, ct_off, n, stream);
}
// kernel milliseconds of the context's last ECIES call: scalars, multiplication, finish, GCM (0 for a phase not run)
extern "C" int lcb_ctx_ecies_phase_ms(lcb_ctx *ctx, float ms[4]) {
    lcb_ctx *c = ctx_resolve(ctx);
    if (!c) return -1;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!c->ecies_ran) { set_err("no ECIES call has run in this context"); return -1; }
    for (int k = 0; k < 4; k++) {
        hipError_t e = hipEventSynchronize(c->ecies_ev[k + 1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[k], c->ecies_ev[k], c->ecies_ev[k + 1]);
        if (e != hipSuccess) { set_err("ecies phase timing", e); return -1; }
    }
    return 0;
}
extern "C" int lcb_ecies_phase_ms(float ms[4]) { return lcb_ctx_ecies_phase_ms(nullptr, ms); }

// ------------------------------------------------------------------ host-pointer forms
extern "C" int lcb_secp_ecdh_batch(uint8_t *key32_out, uint8_t *ok, const uint8_t *pub33, const uint8_t *scalars32,
                                   const uint32_t *scalar_idx, size_t n_scalars, size_t n) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!n) return 0;
    if (!key32_out || !ok || !pub33 || !scalars32) { set_err("secp ecdh: null pointer"); return -1; }
    if (!size_ok("secp ecdh: batch too large", n)) return -1;
    Enq q(c, c->stream);
    hipStream_t s = c->stream;
    size_t ns = scalar_idx ? n_scalars : n;
    uint8_t *dpub = (uint8_t *)stage(c, S_PUB, pub33, 33 * n, s), *dsc = (uint8_t *)stage(c, S_SCALAR, scalars32, 32 * ns, s);
    u32 *didx = scalar_idx ? (u32 *)stage(c, S_IDX, scalar_idx, 4 * n, s) : nullptr;
    uint8_t *dout = (uint8_t *)c->ecies[S_OUT].get(33 * n);
    int rc = -1;
    if (!dpub || !dsc || (scalar_idx && !didx) || !dout) set_err("device allocation failed");
    else rc = ecdh_dev(c, s, dout, dout + 32 * n, dpub, dsc, didx, ns, n);
    if (!rc) {
        hipMemcpyAsync(key32_out, dout, 32 * n, hipMemcpyDeviceToHost, s);
        hipMemcpyAsync(ok, dout + 32 * n, n, hipMemcpyDeviceToHost, s);
    }
    wipe(c->ecies[S_SCALAR], 32 * ns, s);
    wipe(c->ecies[S_OUT], 33 * n, s);
    return sync_check(c, "secp ecdh") && !rc ? 0 : -1;
}
extern "C" int lcb_aes256_gcm_encrypt_batch(uint8_t *out, const uint8_t *keys32, const uint8_t *nonces16,
                                            const uint8_t *pt, const uint64_t *pt_off, size_t n) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!n) return 0;
    if (!out || !keys32 || !nonces16 || !pt || !pt_off) { set_err("aes-256-gcm encrypt: null pointer"); return -1; }
    if (!size_ok("aes-256-gcm encrypt: batch too large", n)) return -1;
    std::vector<uint64_t> rel;
    if (!host_offsets("aes-256-gcm encrypt: offsets must not decrease", rel, pt_off, n)) return -1;
    Enq q(c, c->stream);
    hipStream_t s = c->stream;
    size_t bytes = (size_t)rel[n], ob = bytes + 32 * n;
    uint8_t *dk = (uint8_t *)stage(c, S_KEYS, keys32, 32 * n, s), *dn = (uint8_t *)stage(c, S_NONCE, nonces16, 16 * n, s);
    uint8_t *dd = (uint8_t *)stage(c, S_DATA, pt + pt_off[0], bytes, s);
    uint64_t *doff = (uint64_t *)stage(c, S_IDX, rel.data(), 8 * (n + 1), s);
    uint8_t *dout = (uint8_t *)c->ecies[S_OUT].get(ob);
    int rc = -1;
    if (!dk || !dn || !dd || !doff || !dout) set_err("device allocation failed");
    else rc = gcm_encrypt_dev(c, s, dout, dk, dn, dd, doff, n);
    if (!rc) hipMemcpyAsync(out, dout, ob, hipMemcpyDeviceToHost, s);
    wipe(c->ecies[S_KEYS], 32 * n, s);
    return sync_check(c, "aes-256-gcm encrypt") && !rc ? 0 : -1;
}
extern "C" int lcb_aes256_gcm_decrypt_batch(uint8_t *pt_out, uint8_t *ok, const uint8_t *keys32, const uint8_t *ct,
                                            const uint64_t *ct_off, size_t n) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!n) return 0;
    if (!pt_out || !ok || !keys32 || !ct || !ct_off) { set_err("aes-256-gcm decrypt: null pointer"); return -1; }
    if (!size_ok("aes-256-gcm decrypt: batch too large", n)) return -1;
    std::vector<uint64_t> rel;
    if (!host_offsets("aes-256-gcm decrypt: offsets must not decrease", rel, ct_off, n)) return -1;
    Enq q(c, c->stream);
    hipStream_t s = c->stream;
    size_t bytes = (size_t)rel[n], pb = plain_total(rel, 32);
    uint8_t *dk = (uint8_t *)stage(c, S_KEYS, keys32, 32 * n, s), *dd = (uint8_t *)stage(c, S_DATA, ct + ct_off[0], bytes, s);
    uint64_t *doff = (uint64_t *)stage(c, S_IDX, rel.data(), 8 * (n + 1), s);
    uint8_t *dout = (uint8_t *)c->ecies[S_OUT].get(pb + n);
    int rc = -1;
    if (!dk || !dd || !doff || !dout) set_err("device allocation failed");
    else rc = gcm_decrypt_dev(c, s, dout, dout + pb, dk, dd, doff, n);
    if (!rc) {
        if (pb) hipMemcpyAsync(pt_out, dout, pb, hipMemcpyDeviceToHost, s);
        hipMemcpyAsync(ok, dout + pb, n, hipMemcpyDeviceToHost, s);
    }
    wipe(c->ecies[S_KEYS], 32 * n, s);
    return sync_check(c, "aes-256-gcm decrypt") && !rc ? 0 : -1;
}
extern "C" int lcb_secp256k1_encrypt_batch(uint8_t *out, uint8_t *ok, const uint8_t *recipient_pub33,
                                           const uint8_t *eph_priv32, const uint8_t *nonces16, const uint8_t *pt,
                                           const uint64_t *pt_off, size_t n) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!n) return 0;
    if (!out || !ok || !recipient_pub33 || !eph_priv32 || !nonces16 || !pt || !pt_off) {
        set_err("secp256k1 encrypt: null pointer");
        return -1;
    }
    if (!size_ok("secp256k1 encrypt: batch too large", n)) return -1;
    std::vector<uint64_t> rel;
    if (!host_offsets("secp256k1 encrypt: offsets must not decrease", rel, pt_off, n)) return -1;
    Enq q(c, c->stream);
    hipStream_t s = c->stream;
    size_t bytes = (size_t)rel[n], ob = bytes + 65 * n;
    uint8_t *dpub = (uint8_t *)stage(c, S_PUB, recipient_pub33, 33 * n, s);
    uint8_t *dsc = (uint8_t *)stage(c, S_SCALAR, eph_priv32, 32 * n, s), *dn = (uint8_t *)stage(c, S_NONCE, nonces16, 16 * n, s);
    uint8_t *dd = (uint8_t *)stage(c, S_DATA, pt + pt_off[0], bytes, s);
    uint64_t *doff = (uint64_t *)stage(c, S_IDX, rel.data(), 8 * (n + 1), s);
    uint8_t *dout = (uint8_t *)c->ecies[S_OUT].get(ob + n);
    int rc = -1;
    if (!dpub || !dsc || !dn || !dd || !doff || !dout) set_err("device allocation failed");
    else rc = envelope_encrypt_dev(c, s, dout, dout + ob, dpub, dsc, dn, dd, doff, n);
    if (!rc) {
        hipMemcpyAsync(out, dout, ob, hipMemcpyDeviceToHost, s);
        hipMemcpyAsync(ok, dout + ob, n, hipMemcpyDeviceToHost, s);
    }
    wipe(c->ecies[S_SCALAR], 32 * n, s);
    return sync_check(c, "secp256k1 encrypt") && !rc ? 0 : -1;
}
extern "C" int lcb_secp256k1_decrypt_batch(uint8_t *pt_out, uint8_t *ok, const uint8_t *privs32, const uint32_t *priv_idx,
                                           size_t n_privs, const uint8_t *ct, const uint64_t *ct_off, size_t n) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!n) return 0;
    if (!pt_out || !ok || !privs32 || !ct || !ct_off) { set_err("secp256k1 decrypt: null pointer"); return -1; }
    if (!size_ok("secp256k1 decrypt: batch too large", n)) return -1;
    std::vector<uint64_t> rel;
    if (!host_offsets("secp256k1 decrypt: offsets must not decrease", rel, ct_off, n)) return -1;
    Enq q(c, c->stream);
    hipStream_t s = c->stream;
    size_t bytes = (size_t)rel[n], pb = plain_total(rel, 65), np = priv_idx ? n_privs : n;
    uint8_t *dsc = (uint8_t *)stage(c, S_SCALAR, privs32, 32 * np, s), *dd = (uint8_t *)stage(c, S_DATA, ct + ct_off[0], bytes, s);
    u32 *didx = priv_idx ? (u32 *)stage(c, S_PUB, priv_idx, 4 * n, s) : nullptr;
    uint64_t *doff = (uint64_t *)stage(c, S_IDX, rel.data(), 8 * (n + 1), s);
    uint8_t *dout = (uint8_t *)c->ecies[S_OUT].get(pb + n);
    int rc = -1;
    if (!dsc || !dd || (priv_idx && !didx) || !doff || !dout) set_err("device allocation failed");
    else rc = envelope_decrypt_dev(c, s, dout, dout + pb, dsc, didx, np, dd, doff, n);
    if (!rc) {
        if (pb) hipMemcpyAsync(pt_out, dout, pb, hipMemcpyDeviceToHost, s);
        hipMemcpyAsync(ok, dout + pb, n, hipMemcpyDeviceToHost, s);
    }
    wipe(c->ecies[S_SCALAR], 32 * np, s);
    return sync_check(c, "secp256k1 decrypt") && !rc ? 0 : -1;
}
