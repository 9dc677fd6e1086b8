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
    void *jobs = c->ecies[ECIES_JOBS].get(jb), *pts = c->ecies[ECIES_PTS].get(pb);
    if (!jobs || !pts) { set_err("device allocation failed"); return -1; }
    (void)hipEventRecord(c->ecies_ev[0], s);
    lcbk_ecdh_scalars(s, pub, off, min_len, scalars32, idx, (u32)(n_scalars > 0xffffffffu ? 0xffffffffu : n_scalars),
                      (u32)n, jobs);
    (void)hipEventRecord(c->ecies_ev[1], s);
    lcbk_ecdh_mul(s, jobs, (u32)n, pts);
    (void)hipEventRecord(c->ecies_ev[2], s);
    lcbk_ecdh_finish(s, pts, (u32)n, key32, ok);
    (void)hipEventRecord(c->ecies_ev[3], s);
    wipe(c->ecies[ECIES_JOBS], jb, s);
    wipe(c->ecies[ECIES_PTS], pb, s);
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
    uint64_t *oo = (uint64_t *)c->ecies[ECIES_OFF].get(8 * (n + 1));
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
    uint8_t *keys = (uint8_t *)c->ecies[ECIES_KEYS].get(32 * n), *eok = (uint8_t *)c->ecies[ECIES_EOK].get(n);
    uint8_t *eph = (uint8_t *)c->ecies[ECIES_EPH].get(33 * n), *pok = (uint8_t *)c->ecies[ECIES_POK].get(n);
    if (!keys || !eok || !eph || !pok) { set_err("device allocation failed"); return -1; }
    if (ecdh_core(c, s, keys, eok, recipient_pub33, nullptr, 0, eph_priv32, nullptr, n, n)) return -1;
    // the ephemeral public keys d G from the generator's comb table (timed with the GCM phase)
    if (lcb_ctx_ecdsa_pubkey_dev(c, eph, pok, eph_priv32, n, s)) { wipe(c->ecies[ECIES_KEYS], 32 * n, s); return -1; }
    lcbk_gcm_encrypt(s, keys, nonces16, pt, pt_off, (u32)n, out, eph, eok);
    (void)hipMemcpyAsync(ok, eok, n, hipMemcpyDeviceToDevice, s);
    (void)hipEventRecord(c->ecies_ev[4], s);
    c->ecies_ran = true;
    wipe(c->ecies[ECIES_KEYS], 32 * n, s);
    return launch_ok("secp256k1 encrypt launch") ? 0 : -1;
}
int envelope_decrypt_dev(lcb_ctx *c, hipStream_t s, uint8_t *pt_out, uint8_t *ok, const uint8_t *privs32,
                         const u32 *priv_idx, size_t n_privs, const uint8_t *ct, const uint64_t *ct_off, size_t n) {
    if (!n) return 0;
    if (!pt_out || !ok || !privs32 || !ct || !ct_off) { set_err("secp256k1 decrypt: null pointer"); return -1; }
    if (!size_ok("secp256k1 decrypt: batch too large", n) || !events_ready(c)) return -1;
    uint8_t *keys = (uint8_t *)c->ecies[ECIES_KEYS].get(32 * n), *eok = (uint8_t *)c->ecies[ECIES_EOK].get(n);
    uint64_t *oo = (uint64_t *)c->ecies[ECIES_OFF].get(8 * (n + 1));
    if (!keys || !eok || !oo) { set_err("device allocation failed"); return -1; }
    if (ecdh_core(c, s, keys, eok, ct, ct_off, 65, privs32, priv_idx, priv_idx ? n_privs : n, n)) return -1;
    lcbk_gcm_offsets(s, ct_off, (u32)n, 65, oo);
    lcbk_gcm_decrypt(s, keys, ct, ct_off, oo, (u32)n, 33, pt_out, ok, eok);
    (void)hipEventRecord(c->ecies_ev[4], s);
    c->ecies_ran = true;
    wipe(c->ecies[ECIES_KEYS], 32 * n, s);
    return launch_ok("secp256k1 decrypt launch") ? 0 : -1;
}

// the summed plaintext lengths of a decryption, from its rebased offsets
size_t plain_total(const std::vector<uint64_t> &rel, size_t overhead) {
    size_t t = 0;
    for (size_t i = 0; i + 1 < rel.size(); i++) {
        uint64_t len = rel[i + 1] - rel[i];
        if (len >= overhead) t += (size_t)(len - overhead);
    }
    return t;
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
    HostCall h(c, "secp ecdh");
    size_t ns = scalar_idx ? n_scalars : n;
    const uint8_t *dpub = h.in(pub33, 33 * n), *dsc = h.in(scalars32, 32 * ns);
    const u32 *didx = scalar_idx ? h.in(scalar_idx, n) : nullptr;
    uint8_t *dout = h.out<uint8_t>(33 * n);
    int rc = h.ok() ? ecdh_dev(c, h.s, dout, dout + 32 * n, dpub, dsc, didx, ns, n) : -1;
    if (!rc) {
        h.back(key32_out, dout, 32 * n);
        h.back(ok, dout + 32 * n, n);
    }
    h.wipe(dsc, 32 * ns);
    h.wipe(dout, 33 * n);
    return h.finish() || rc ? -1 : 0;
}
extern "C" int lcb_aes256_gcm_encrypt_batch(uint8_t *out, const uint8_t *keys32, const uint8_t *nonces16,
                                            const uint8_t *pt, const uint64_t *pt_off, size_t n) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!n) return 0;
    if (!out || !keys32 || !nonces16 || !pt || !pt_off) { set_err("aes-256-gcm encrypt: null pointer"); return -1; }
    if (!size_ok("aes-256-gcm encrypt: batch too large", n)) return -1;
    std::vector<uint64_t> rel;
    if (!rebase(rel, pt_off, n, "aes-256-gcm encrypt: offsets must not decrease")) return -1;
    HostCall h(c, "aes-256-gcm encrypt");
    size_t bytes = (size_t)rel[n], ob = bytes + 32 * n;
    const uint8_t *dk = h.in(keys32, 32 * n), *dn = h.in(nonces16, 16 * n), *dd = h.in(pt + pt_off[0], bytes);
    const uint64_t *doff = h.in(rel.data(), n + 1);
    uint8_t *dout = h.out<uint8_t>(ob);
    int rc = h.ok() ? gcm_encrypt_dev(c, h.s, dout, dk, dn, dd, doff, n) : -1;
    if (!rc) h.back(out, dout, ob);
    h.wipe(dk, 32 * n);
    return h.finish() || rc ? -1 : 0;
}
extern "C" int lcb_aes256_gcm_decrypt_batch(uint8_t *pt_out, uint8_t *ok, const uint8_t *keys32, const uint8_t *ct,
                                            const uint64_t *ct_off, size_t n) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!n) return 0;
    if (!pt_out || !ok || !keys32 || !ct || !ct_off) { set_err("aes-256-gcm decrypt: null pointer"); return -1; }
    if (!size_ok("aes-256-gcm decrypt: batch too large", n)) return -1;
    std::vector<uint64_t> rel;
    if (!rebase(rel, ct_off, n, "aes-256-gcm decrypt: offsets must not decrease")) return -1;
    HostCall h(c, "aes-256-gcm decrypt");
    size_t bytes = (size_t)rel[n], pb = plain_total(rel, 32);
    const uint8_t *dk = h.in(keys32, 32 * n), *dd = h.in(ct + ct_off[0], bytes);
    const uint64_t *doff = h.in(rel.data(), n + 1);
    uint8_t *dout = h.out<uint8_t>(pb + n);
    int rc = h.ok() ? gcm_decrypt_dev(c, h.s, dout, dout + pb, dk, dd, doff, n) : -1;
    if (!rc) {
        h.back(pt_out, dout, pb);
        h.back(ok, dout + pb, n);
    }
    h.wipe(dk, 32 * n);
    return h.finish() || rc ? -1 : 0;
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
    if (!rebase(rel, pt_off, n, "secp256k1 encrypt: offsets must not decrease")) return -1;
    HostCall h(c, "secp256k1 encrypt");
    size_t bytes = (size_t)rel[n], ob = bytes + 65 * n;
    const uint8_t *dpub = h.in(recipient_pub33, 33 * n), *dsc = h.in(eph_priv32, 32 * n), *dn = h.in(nonces16, 16 * n);
    const uint8_t *dd = h.in(pt + pt_off[0], bytes);
    const uint64_t *doff = h.in(rel.data(), n + 1);
    uint8_t *dout = h.out<uint8_t>(ob + n);
    int rc = h.ok() ? envelope_encrypt_dev(c, h.s, dout, dout + ob, dpub, dsc, dn, dd, doff, n) : -1;
    if (!rc) {
        h.back(out, dout, ob);
        h.back(ok, dout + ob, n);
    }
    h.wipe(dsc, 32 * n);
    return h.finish() || rc ? -1 : 0;
}
extern "C" int lcb_secp256k1_decrypt_batch(uint8_t *pt_out, uint8_t *ok, const uint8_t *privs32, const uint32_t *priv_idx,
                                           size_t n_privs, const uint8_t *ct, const uint64_t *ct_off, size_t n) {
    lcb_ctx *c = ctx_sync();
    if (!c) return -1;
    if (!n) return 0;
    if (!pt_out || !ok || !privs32 || !ct || !ct_off) { set_err("secp256k1 decrypt: null pointer"); return -1; }
    if (!size_ok("secp256k1 decrypt: batch too large", n)) return -1;
    std::vector<uint64_t> rel;
    if (!rebase(rel, ct_off, n, "secp256k1 decrypt: offsets must not decrease")) return -1;
    HostCall h(c, "secp256k1 decrypt");
    size_t bytes = (size_t)rel[n], pb = plain_total(rel, 65), np = priv_idx ? n_privs : n;
    const uint8_t *dsc = h.in(privs32, 32 * np), *dd = h.in(ct + ct_off[0], bytes);
    const u32 *didx = priv_idx ? h.in(priv_idx, n) : nullptr;
    const uint64_t *doff = h.in(rel.data(), n + 1);
    uint8_t *dout = h.out<uint8_t>(pb + n);
    int rc = h.ok() ? envelope_decrypt_dev(c, h.s, dout, dout + pb, dsc, didx, np, dd, doff, n) : -1;
    if (!rc) {
        h.back(pt_out, dout, pb);
        h.back(ok, dout + pb, n);
    }
    h.wipe(dsc, 32 * np);
    return h.finish() || rc ? -1 : 0;
}
