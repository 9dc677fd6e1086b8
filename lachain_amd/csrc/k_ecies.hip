// lachain_amd/csrc/k_ecies.hip — gfx950 kernels for the secp256k1 ECIES envelope of the trustless DKG
// (TrustlessKeygen.cs:63-76,90-135 -> DefaultCrypto.Secp256K1Encrypt / Secp256K1Decrypt, DefaultCrypto.cs:264-336) and
// its two halves on their own: batched ECDH (Secp256K1.Ecdh: libsecp256k1's secp256k1_ecdh with the default hash) and
// batched AES-256-GCM with 16-byte nonces (AesGcmEncrypt / AesGcmDecrypt, DefaultCrypto.cs:267-299).  The per-lane code
// and the statement on constant time (none is claimed) are in ecies_lane.hpp.  Kernels:
//   k_ecdh_scalars   key parsing, scalar range check, lambda-split and digit recoding -> job records (one item per lane)
//   k_ecdh_mul       P from x and the prefix's parity, d P -> Jacobian point (one item per lane, 768 B table in scratch)
//   k_ecdh_finish    to affine (one field inversion per 16 items), key = SHA-256(compressed d P)
//   k_gcm_offsets    where each decrypted item goes: prefix sums of the plaintext lengths (one block)
//   k_gcm_encrypt    one envelope per lane; the block fills the 1 KB T-table in LDS first
//   k_gcm_decrypt    one envelope per lane: tag check over the received C, then the plaintext or zero bytes
#include "ecies_lane.hpp"
#ifndef SECP_HOST_EMULATION
#include "gate.hpp"
#endif

// item i: key at pub + 33 i, or (off given) the first 33 bytes of item [off[i], off[i + 1]) of pub when the item has
// at least min_len bytes; scalar scalars32[idx ? idx[i] : i] (an index >= n_scalars fails the item)
extern "C" __global__ void __launch_bounds__(SECP_BLOCK) k_ecdh_scalars(const uint8_t *pub, const u64 *off, u32 min_len,
                                                                       const uint8_t *scalars32, const u32 *idx,
                                                                       u32 n_scalars, u32 n, ecdh_job *jobs) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *p = pub + 33 * (size_t)i;
    if (off) p = off[i + 1] - off[i] >= min_len ? pub + off[i] : nullptr;
    u32 si = idx ? idx[i] : i;
    const uint8_t *d = si < n_scalars ? scalars32 + 32 * (size_t)si : nullptr;
    ecdh_job j;
    ecdh_make_job(j, p, d);
    jobs[i] = j;
}
extern "C" __global__ void __launch_bounds__(SECP_BLOCK) k_ecdh_mul(const ecdh_job *jobs, u32 n, ecdh_point *out) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ecdh_mul_lane(out + i, jobs + i);
}
extern "C" __global__ void __launch_bounds__(SECP_BLOCK) k_ecdh_finish(const ecdh_point *pts, u32 n, uint8_t *key32,
                                                                      uint8_t *ok_out) {
    const size_t T = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    ecdh_finish_lane(pts, n, tid, T, key32, ok_out);
}

// out_off[i] = sum over j < i of max(len_j - overhead, 0), i = 0..n: item i's plaintext position.  One block; each
// thread sums a contiguous run of items, the runs' totals are scanned in LDS.
SDI u64 gcm_plain_len(const u64 *off, u32 i, u32 overhead) {
    u64 len = off[i + 1] - off[i];
    return len >= overhead ? len - overhead : 0;
}
extern "C" __global__ void __launch_bounds__(SECP_BLOCK) k_gcm_offsets(const u64 *off, u32 n, u32 overhead, u64 *out_off) {
#ifndef SECP_HOST_EMULATION
    __shared__ u64 part[SECP_BLOCK];
    const u32 t = threadIdx.x, per = (n + SECP_BLOCK - 1) / SECP_BLOCK;
    const u32 lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    u64 sum = 0;
    for (u32 i = lo; i < hi; i++) sum += gcm_plain_len(off, i, overhead);
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        u64 run = 0;
        for (u32 k = 0; k < SECP_BLOCK; k++) { u64 v = part[k]; part[k] = run; run += v; }
        out_off[n] = run;
    }
    __syncthreads();
    u64 run = part[t];
    for (u32 i = lo; i < hi; i++) { out_off[i] = run; run += gcm_plain_len(off, i, overhead); }
#else
    u64 run = 0;
    for (u32 i = 0; i < n; i++) { out_off[i] = run; run += gcm_plain_len(off, i, overhead); }
    out_off[n] = run;
#endif
}

#ifndef SECP_HOST_EMULATION
// the block's T-table: every thread takes part and reaches the one barrier before any lane returns
#define GCM_TABLE(te)                                                                      \
    __shared__ u32 te[256];                                                                \
    for (u32 t = threadIdx.x; t < 256; t += blockDim.x) te[t] = aes_te0_entry(t);          \
    __syncthreads()
#else
static u32 emu_te[256];
#define GCM_TABLE(te) const u32 *te = emu_te
#endif

// out item i at out + (pt_off[i] - pt_off[0]) + (32 + hdr) i, hdr = 33 when hdr33 is given (the envelope's ephemeral
// key, hdr33 + 33 i); ok_in may be null
extern "C" __global__ void __launch_bounds__(SECP_BLOCK) k_gcm_encrypt(const uint8_t *keys32, const uint8_t *nonces16,
                                                                      const uint8_t *pt, const u64 *pt_off, u32 n,
                                                                      uint8_t *out, const uint8_t *hdr33,
                                                                      const uint8_t *ok_in) {
    GCM_TABLE(te);
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 len = pt_off[i + 1] - pt_off[i];
    uint8_t *o = out + (pt_off[i] - pt_off[0]) + (size_t)(hdr33 ? 65 : 32) * i;
    gcm_encrypt_lane(te, o, hdr33 ? hdr33 + 33 * (size_t)i : nullptr, keys32 + 32 * (size_t)i, nonces16 + 16 * (size_t)i,
                     pt + pt_off[i], len, ok_in ? ok_in[i] != 0 : true);
}
// item i = ct[ct_off[i], ct_off[i + 1]) with hdr bytes (0 or 33) before the nonce; plaintext at pt_out + out_off[i]
extern "C" __global__ void __launch_bounds__(SECP_BLOCK) k_gcm_decrypt(const uint8_t *keys32, const uint8_t *ct,
                                                                      const u64 *ct_off, const u64 *out_off, u32 n,
                                                                      u32 hdr, uint8_t *pt_out, uint8_t *ok_out,
                                                                      const uint8_t *ok_in) {
    GCM_TABLE(te);
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool ok = gcm_decrypt_lane(te, pt_out + out_off[i], ct + ct_off[i], ct_off[i + 1] - ct_off[i], hdr,
                               keys32 + 32 * (size_t)i, ok_in ? ok_in[i] != 0 : true);
    ok_out[i] = ok;
}

#ifndef SECP_HOST_EMULATION
// ---------------------------------------------------------------- host launch wrappers
static unsigned ecies_blocks_for(size_t n) { return (unsigned)((n + SECP_BLOCK - 1) / SECP_BLOCK); }
extern "C" size_t lcbk_ecdh_job_bytes(void) { return sizeof(ecdh_job); }
extern "C" size_t lcbk_ecdh_point_bytes(void) { return sizeof(ecdh_point); }
extern "C" void lcbk_ecdh_scalars(hipStream_t s, const uint8_t *pub, const uint64_t *off, u32 min_len,
                                  const uint8_t *scalars32, const u32 *idx, u32 n_scalars, u32 n, void *jobs) {
    if (!n) return;
    LCB_LAUNCH_GATED(k_ecdh_scalars, dim3(ecies_blocks_for(n)), dim3(SECP_BLOCK), 0, s, pub, (const u64 *)off, min_len,
                     scalars32, idx, n_scalars, n, (ecdh_job *)jobs);
}
extern "C" void lcbk_ecdh_mul(hipStream_t s, const void *jobs, u32 n, void *pts) {
    if (!n) return;
    LCB_LAUNCH_GATED(k_ecdh_mul, dim3(ecies_blocks_for(n)), dim3(SECP_BLOCK), 0, s, (const ecdh_job *)jobs, n,
                     (ecdh_point *)pts);
}
extern "C" void lcbk_ecdh_finish(hipStream_t s, const void *pts, u32 n, uint8_t *key32, uint8_t *ok) {
    if (!n) return;
    size_t threads = (n + SECP_BATCH - 1) / SECP_BATCH;
    LCB_LAUNCH_GATED(k_ecdh_finish, dim3(ecies_blocks_for(threads)), dim3(SECP_BLOCK), 0, s, (const ecdh_point *)pts, n,
                     key32, ok);
}
extern "C" void lcbk_gcm_offsets(hipStream_t s, const uint64_t *off, u32 n, u32 overhead, uint64_t *out_off) {
    LCB_LAUNCH_GATED(k_gcm_offsets, dim3(1), dim3(SECP_BLOCK), 0, s, (const u64 *)off, n, overhead, (u64 *)out_off);
}
extern "C" void lcbk_gcm_encrypt(hipStream_t s, const uint8_t *keys32, const uint8_t *nonces16, const uint8_t *pt,
                                 const uint64_t *pt_off, u32 n, uint8_t *out, const uint8_t *hdr33, const uint8_t *ok_in) {
    if (!n) return;
    LCB_LAUNCH_GATED(k_gcm_encrypt, dim3(ecies_blocks_for(n)), dim3(SECP_BLOCK), 0, s, keys32, nonces16, pt,
                     (const u64 *)pt_off, n, out, hdr33, ok_in);
}
extern "C" void lcbk_gcm_decrypt(hipStream_t s, const uint8_t *keys32, const uint8_t *ct, const uint64_t *ct_off,
                                 const uint64_t *out_off, u32 n, u32 hdr, uint8_t *pt_out, uint8_t *ok_out,
                                 const uint8_t *ok_in) {
    if (!n) return;
    LCB_LAUNCH_GATED(k_gcm_decrypt, dim3(ecies_blocks_for(n)), dim3(SECP_BLOCK), 0, s, keys32, ct, (const u64 *)ct_off,
                     (const u64 *)out_off, n, hdr, pt_out, ok_out, ok_in);
}
#endif  // SECP_HOST_EMULATION
