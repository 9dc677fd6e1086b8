// lachain_amd/csrc/ecies_lane.hpp — the per-lane pieces of the secp256k1 ECIES envelope the trustless DKG wraps every
// secret in: DefaultCrypto.Secp256K1Encrypt / Secp256K1Decrypt (DefaultCrypto.cs:264-336) = libsecp256k1's ECDH with its
// default hash, then BouncyCastle's GcmBlockCipher(AesEngine) with a 32-byte key, a 16-byte nonce, no associated data
// and a 16-byte tag (DefaultCrypto.cs:267-299).  Shared by k_ecies.hip (gfx950) and tools/emul/ecies_emul.cpp, which
// compiles this file for the host under SECP_HOST_EMULATION.
//
// NO CONSTANT-TIME CLAIM.  The library makes no constant-time claim on the GPU: the ladder's table lookups and the
// zero digits it skips depend on the scalar, and the AES table lookups depend on the key.  That is the standing of
// lcb_ecdsa_sign_hashed_batch, lcb_ts_sign and lcb_tpke_partial_decrypt, which already take private keys.
//
// ECDH: d P with d = k1 + k2 lambda (glv_split), both halves as signed 4-bit digits, one Jacobian table 1P .. 8P per
// lane (768 B of scratch) serving P and phi(P): 132 doublings and at most 66 complete additions from the top window
// down — the loop of k_secp_recover without its u1 G tail.  The ladder is kept local to this unit so that k_secp.hip and
// k_secp_recover.hip compile exactly as before.
// AES-256-GCM: one 256-entry T-table (1 KB, Te0; the other three are its rotations and the S-box is its second byte),
// the 60 round-key words in registers (every index is a compile-time constant), GHASH as the plain 128-step
// shift-and-xor product of NIST SP 800-38D algorithm 1.
#pragma once
#include "secp_comb.hpp"

#define ECDH_WIN 33                  // signed 4-bit digits of a magnitude < 2^129
#define ECDH_TAB 8                   // multiples 1..8 of P per lane

struct ecdh_job {                    // 108 B, written by k_ecdh_scalars, read by k_ecdh_mul
    int8_t e1[36], e2[36];           // signed 4-bit digits of k1 and k2, windows 0..32
    u32 x[8];                        // x(P), below p
    u32 flags;                       // bit 0: parsing and range checks passed; bit 1: y(P) is odd
};
static_assert(sizeof(ecdh_job) == 108, "job record");
struct ecdh_point {                  // 100 B, written by k_ecdh_mul, read by k_ecdh_finish
    fe x, y, z;
    u32 ok;                          // 0: no shared point (failed check, x not on the curve)
};
static_assert(sizeof(ecdh_point) == 100, "point record");

// ------------------------------------------------------------------------------------------------ ECDH
// signed 4-bit digits in [-7, 8] of a magnitude below 2^129 (33 windows), negated for a negative half
SDI void ecdh_recode4(int8_t *d, const u32 *m, bool neg) {
    u32 carry = 0;
#pragma unroll
    for (int w = 0; w < ECDH_WIN; w++) {
        u32 v = ((m[w >> 3] >> (4 * (w & 7))) & 0xfu) + carry;
        carry = v > 8u;
        int dv = carry ? (int)v - 16 : (int)v;
        d[w] = (int8_t)(neg ? -dv : dv);
    }
#pragma unroll
    for (int w = ECDH_WIN; w < 36; w++) d[w] = 0;
}
// secp256k1_ec_pubkey_parse on a 33-byte slot (prefix 2 or 3, x < p; the curve check needs the square root and is the
// multiplication kernel's) and secp256k1_ecdh's scalar check (1 <= d < n).  pub / d are null for an item that has none.
SDI void ecdh_make_job(ecdh_job &j, const uint8_t *pub33, const uint8_t *d32) {
    u32 d[8], m1[8], m2[8];
    bool ok = pub33 != nullptr && d32 != nullptr;
#pragma unroll
    for (int l = 0; l < 8; l++) { d[l] = 0; j.x[l] = 0; }
    u32 pfx = 0;
    if (ok) {
        pfx = pub33[0];
        u256_from_be(j.x, pub33 + 1);
        u256_from_be(d, d32);
    }
    ok = ok && (pfx == 2u || pfx == 3u);
    ok = ok && u256_lt(j.x, SECP_P);
    ok = ok && !u256_is_zero(d) && u256_lt(d, SECP_N);
    if (!ok) {
#pragma unroll
        for (int l = 0; l < 8; l++) d[l] = 0;
    }
    bool n1, n2;
    glv_split(m1, n1, m2, n2, d);
    ecdh_recode4(j.e1, m1, n1);
    ecdh_recode4(j.e2, m2, n2);
    j.flags = (ok ? 1u : 0u) | ((pfx & 1u) ? 2u : 0u);
}
// d P as a Jacobian point
SDI void ecdh_mul_lane(ecdh_point *op, const ecdh_job *jp) {
    const u32 flags = jp->flags;
    if (!(flags & 1u)) { op->ok = 0; return; }
    // P = (x, y) with y^2 = x^3 + 7 and the parity of the prefix (secp256k1_ge_set_xo_var)
    fe x, y;
#pragma unroll
    for (int l = 0; l < 8; l++) x.v[l] = jp->x[l];
    {
        fe x3, t;
        fe_sqr(t, x); fe_mul(x3, t, x); fe_add(x3, x3, fe_small(7));
        fe_sqrt(y, x3);
        fe_sqr(t, y);
        if (!fe_eq(t, x3)) { op->ok = 0; return; }
        y = fe_canon(y);
        if ((y.v[0] & 1) != ((flags >> 1) & 1)) fe_neg(y, y);
    }
    // T[m - 1] = m P for m = 1..8; none is infinity (P has the odd prime order n)
    fe T[3 * ECDH_TAB];
    {
        secp_jac P, Q;
        jac_set_aff(P, x, y);
        T[0] = P.x; T[1] = P.y; T[2] = P.z;
        jac_dbl(Q, P);
        T[3] = Q.x; T[4] = Q.y; T[5] = Q.z;
#pragma unroll 1
        for (int m = 2; m < ECDH_TAB; m++) {
            jac_add_aff(Q, Q, x, y);
            T[3 * m] = Q.x; T[3 * m + 1] = Q.y; T[3 * m + 2] = Q.z;
        }
    }
    secp_jac acc;
    acc.inf = true;
    acc.x = acc.y = acc.z = fe_zero();
    const fe beta = fe_from(SECP_BETA);
    // k1 P + k2 phi(P): from the top window down, four doublings, then the two halves' digits (one addition site; h is
    // uniform across the wave).  The additions keep every exceptional case (jac_add).
#pragma unroll 1
    for (int w = ECDH_WIN - 1; w >= 0; w--) {
#pragma unroll 1
        for (int k = 0; k < 4; k++) jac_dbl(acc, acc);
#pragma unroll 1
        for (int h = 0; h < 2; h++) {
            int d = h ? jp->e2[w] : jp->e1[w];
            if (d == 0) continue;
            int m = (d < 0 ? -d : d) - 1;
            secp_jac q;
            q.x = T[3 * m]; q.y = T[3 * m + 1]; q.z = T[3 * m + 2];
            q.inf = false;
            if (h) fe_mul(q.x, q.x, beta);
            if (d < 0) fe_neg(q.y, q.y);
            jac_add(acc, acc, q);
        }
    }
    if (acc.inf) { op->ok = 0; return; }
    op->x = acc.x; op->y = acc.y; op->z = acc.z;
    op->ok = 1;
}

// ------------------------------------------------------------------------------------------------ SHA-256
__constant__ static const u32 SHA256_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
SDI u32 ror32(u32 v, int s) { return (v >> s) | (v << (32 - s)); }
SDI void sha256_init(u32 *h) {
    h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}
// one compression: h += compress(h, block), block as 16 big-endian words (overwritten by the message schedule)
SDI void sha256_compress(u32 *h, u32 *w) {
    u32 a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int t = 0; t < 64; t++) {
        if (t >= 16) {
            u32 w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
            u32 s0 = ror32(w15, 7) ^ ror32(w15, 18) ^ (w15 >> 3);
            u32 s1 = ror32(w2, 17) ^ ror32(w2, 19) ^ (w2 >> 10);
            w[t & 15] += s0 + w[(t + 9) & 15] + s1;
        }
        u32 t1 = hh + (ror32(e, 6) ^ ror32(e, 11) ^ ror32(e, 25)) + ((e & f) ^ (~e & g)) + SHA256_K[t] + w[t & 15];
        u32 t2 = (ror32(a, 2) ^ ror32(a, 13) ^ ror32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
// libsecp256k1's default ECDH hash: SHA-256(byte(0x02 | (y & 1)) || x), 33 bytes padded into one block
SDI void ecdh_hash(uint8_t *key32, const fe &x, u32 y_odd) {
    u32 w[16], h[8];
    w[0] = ((2u | (y_odd & 1u)) << 24) | (x.v[7] >> 8);
#pragma unroll
    for (int k = 1; k < 8; k++) w[k] = (x.v[8 - k] << 24) | (x.v[7 - k] >> 8);
    w[8] = (x.v[0] << 24) | 0x00800000u;
#pragma unroll
    for (int k = 9; k < 15; k++) w[k] = 0;
    w[15] = 33 * 8;
    sha256_init(h);
    sha256_compress(h, w);
#pragma unroll
    for (int k = 0; k < 32; k++) key32[k] = (uint8_t)(h[k / 4] >> (8 * (3 - k % 4)));
}
// SECP_BATCH items per thread: Jacobian -> affine with one field inversion (Montgomery's trick), then the hash.
// A failed item gets ok = 0 and a zero key.
SDI void ecdh_finish_lane(const ecdh_point *pts, u32 n, size_t tid, size_t T, uint8_t *key32, uint8_t *ok_out) {
    fe pre[SECP_BATCH];
#pragma unroll 1
    for (int k = 0; k < SECP_BATCH; k++) {
        size_t i = tid + k * T;
        fe z = fe_small(1);
        if (i < n && pts[i].ok) z = pts[i].z;
        if (k == 0) pre[k] = z; else fe_mul(pre[k], pre[k - 1], z);
    }
    fe inv;
    fe_inv(inv, pre[SECP_BATCH - 1]);
#pragma unroll 1
    for (int k = SECP_BATCH - 1; k >= 0; k--) {
        size_t i = tid + k * T;
        bool ok = i < n && pts[i].ok;
        fe z = fe_small(1);
        if (ok) z = pts[i].z;
        fe zi;
        if (k > 0) fe_mul(zi, inv, pre[k - 1]); else zi = inv;
        fe_mul(inv, inv, z);
        if (i >= n) continue;
        uint8_t *o = key32 + 32 * i;
        if (ok) {
            fe zi2, x, y;
            fe_sqr(zi2, zi);
            fe_mul(x, pts[i].x, zi2);
            fe_mul(zi2, zi2, zi);
            fe_mul(y, pts[i].y, zi2);
            x = fe_canon(x);
            y = fe_canon(y);
            ecdh_hash(o, x, y.v[0] & 1);
        } else {
#pragma unroll
            for (int b = 0; b < 32; b++) o[b] = 0;
        }
        ok_out[i] = ok;
    }
}

// ------------------------------------------------------------------------------------------------ AES-256
// GF(2^8) mod x^8 + x^4 + x^3 + x + 1, for the table only
SDI u32 gf8_mul(u32 a, u32 b) {
    u32 r = 0;
    for (int k = 0; k < 8; k++) {
        if (b & 1u) r ^= a;
        a = (a << 1) ^ ((a & 0x80u) ? 0x11bu : 0u);
        b >>= 1;
    }
    return r & 0xffu;
}
// Te0[x] = (2 S[x], S[x], S[x], 3 S[x]) with S[x] = affine(x^-1) (FIPS 197 §5.1.1); the block fills its table with this
SDI u32 aes_te0_entry(u32 x) {
    u32 inv = 1, p = x;
    for (int k = 0; k < 7; k++) { p = gf8_mul(p, p); inv = gf8_mul(inv, p); }      // x^254 (0 for x = 0)
    u32 s = inv;
    for (int k = 1; k < 5; k++) s ^= ((inv << k) | (inv >> (8 - k))) & 0xffu;
    s ^= 0x63u;
    u32 s2 = gf8_mul(s, 2);
    return (s2 << 24) | (s << 16) | (s << 8) | (s2 ^ s);
}
#define AES_S(te, b) (((te)[(b) & 0xffu] >> 8) & 0xffu)
SDI u32 aes_sub_word(const u32 *te, u32 w) {
    return (AES_S(te, w >> 24) << 24) | (AES_S(te, w >> 16) << 16) | (AES_S(te, w >> 8) << 8) | AES_S(te, w);
}
struct aes256 { u32 rk[60]; };
SDI void aes256_expand(aes256 &k, const u32 *te, const uint8_t *key32) {
#pragma unroll
    for (int i = 0; i < 8; i++)
        k.rk[i] = ((u32)key32[4 * i] << 24) | ((u32)key32[4 * i + 1] << 16) | ((u32)key32[4 * i + 2] << 8) | key32[4 * i + 3];
    u32 rcon = 1;
#pragma unroll
    for (int i = 8; i < 60; i++) {
        u32 t = k.rk[i - 1];
        if (i % 8 == 0) { t = aes_sub_word(te, (t << 8) | (t >> 24)) ^ (rcon << 24); rcon <<= 1; }
        else if (i % 8 == 4) t = aes_sub_word(te, t);
        k.rk[i] = k.rk[i - 8] ^ t;
    }
}
SDI u32 aes_col(const u32 *te, u32 a, u32 b, u32 c, u32 d) {
    return te[a >> 24] ^ ror32(te[(b >> 16) & 0xffu], 8) ^ ror32(te[(c >> 8) & 0xffu], 16) ^ ror32(te[d & 0xffu], 24);
}
SDI void aes256_encrypt(u32 *out, const aes256 &k, const u32 *te, const u32 *in) {
    u32 s0 = in[0] ^ k.rk[0], s1 = in[1] ^ k.rk[1], s2 = in[2] ^ k.rk[2], s3 = in[3] ^ k.rk[3];
#pragma unroll
    for (int r = 1; r < 14; r++) {
        u32 t0 = aes_col(te, s0, s1, s2, s3) ^ k.rk[4 * r];
        u32 t1 = aes_col(te, s1, s2, s3, s0) ^ k.rk[4 * r + 1];
        u32 t2 = aes_col(te, s2, s3, s0, s1) ^ k.rk[4 * r + 2];
        u32 t3 = aes_col(te, s3, s0, s1, s2) ^ k.rk[4 * r + 3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    out[0] = ((AES_S(te, s0 >> 24) << 24) | (AES_S(te, s1 >> 16) << 16) | (AES_S(te, s2 >> 8) << 8) | AES_S(te, s3)) ^ k.rk[56];
    out[1] = ((AES_S(te, s1 >> 24) << 24) | (AES_S(te, s2 >> 16) << 16) | (AES_S(te, s3 >> 8) << 8) | AES_S(te, s0)) ^ k.rk[57];
    out[2] = ((AES_S(te, s2 >> 24) << 24) | (AES_S(te, s3 >> 16) << 16) | (AES_S(te, s0 >> 8) << 8) | AES_S(te, s1)) ^ k.rk[58];
    out[3] = ((AES_S(te, s3 >> 24) << 24) | (AES_S(te, s0 >> 16) << 16) | (AES_S(te, s1 >> 8) << 8) | AES_S(te, s2)) ^ k.rk[59];
}

// ------------------------------------------------------------------------------------------------ GCM
// y = y * h in GF(2^128) (SP 800-38D algorithm 1; word 0 holds the first four bytes)
SDI void ghash_mul(u32 *y, const u32 *h) {
    u32 z0 = 0, z1 = 0, z2 = 0, z3 = 0, v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3];
#pragma unroll
    for (int w = 0; w < 4; w++) {
        u32 yw = y[w];
#pragma unroll 1
        for (int b = 0; b < 32; b++) {
            u32 m = 0u - (yw >> 31);
            yw <<= 1;
            z0 ^= v0 & m; z1 ^= v1 & m; z2 ^= v2 & m; z3 ^= v3 & m;
            u32 r = (0u - (v3 & 1u)) & 0xe1000000u;
            v3 = (v3 >> 1) | (v2 << 31);
            v2 = (v2 >> 1) | (v1 << 31);
            v1 = (v1 >> 1) | (v0 << 31);
            v0 = (v0 >> 1) ^ r;
        }
    }
    y[0] = z0; y[1] = z1; y[2] = z2; y[3] = z3;
}
// up to 16 bytes of an item as big-endian words, zero-padded; no byte at or past p + rem is read
SDI void gcm_load_block(u32 *b, const uint8_t *p, u64 rem) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
        u32 v = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) v = (v << 8) | ((u64)(4 * w + k) < rem ? (u32)p[4 * w + k] : 0u);
        b[w] = v;
    }
}
SDI void gcm_store_block(uint8_t *p, const u32 *b, u64 rem) {
#pragma unroll
    for (int k = 0; k < 16; k++)
        if ((u64)k < rem) p[k] = (uint8_t)(b[k / 4] >> (8 * (3 - k % 4)));
}
struct gcm_lane {
    aes256 k;
    u32 h[4], j0[4];
};
// H = E_K(0); the nonce is 16 bytes, not 12, so J0 = GHASH_H(nonce || 0^64 || [128]_64) (SP 800-38D §7.1 step 2)
SDI void gcm_init(gcm_lane &g, const u32 *te, const uint8_t *key32, const uint8_t *nonce16) {
    aes256_expand(g.k, te, key32);
    u32 zero[4] = {0, 0, 0, 0};
    aes256_encrypt(g.h, g.k, te, zero);
    gcm_load_block(g.j0, nonce16, 16);
    ghash_mul(g.j0, g.h);
    g.j0[3] ^= 128u;
    ghash_mul(g.j0, g.h);
}
// out = in xor the key stream E_K(inc32^k(J0)), k = 1, 2, ..
SDI void gcm_ctr(const gcm_lane &g, const u32 *te, const uint8_t *in, uint8_t *out, u64 len) {
    u32 ctr[4] = {g.j0[0], g.j0[1], g.j0[2], g.j0[3]};
#pragma unroll 1
    for (u64 o = 0; o < len; o += 16) {
        u32 ks[4], b[4];
        ctr[3]++;
        aes256_encrypt(ks, g.k, te, ctr);
        gcm_load_block(b, in + o, len - o);
#pragma unroll
        for (int w = 0; w < 4; w++) b[w] ^= ks[w];
        gcm_store_block(out + o, b, len - o);
    }
}
// tag = E_K(J0) xor GHASH_H(C zero-padded || [0]_64 || [8 len]_64)
SDI void gcm_tag(u32 *tag, const gcm_lane &g, const u32 *te, const uint8_t *c, u64 len) {
    u32 y[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (u64 o = 0; o < len; o += 16) {
        u32 b[4];
        gcm_load_block(b, c + o, len - o);
#pragma unroll
        for (int w = 0; w < 4; w++) y[w] ^= b[w];
        ghash_mul(y, g.h);
    }
    y[2] ^= (u32)((8 * len) >> 32);
    y[3] ^= (u32)(8 * len);
    ghash_mul(y, g.h);
    aes256_encrypt(tag, g.k, te, g.j0);
#pragma unroll
    for (int w = 0; w < 4; w++) tag[w] ^= y[w];
}
// AesGcmEncrypt (DefaultCrypto.cs:267-281): o = [hdr33 ||] nonce || C || tag; a failed item (ok = false: its session key
// does not exist) gets zero bytes
SDI void gcm_encrypt_lane(const u32 *te, uint8_t *o, const uint8_t *hdr33, const uint8_t *key32, const uint8_t *nonce16,
                          const uint8_t *pt, u64 len, bool ok) {
    const u32 hdr = hdr33 ? 33u : 0u;
    if (!ok) {
#pragma unroll 1
        for (u64 b = 0; b < hdr + 32 + len; b++) o[b] = 0;
        return;
    }
#pragma unroll 1
    for (u32 b = 0; b < hdr; b++) o[b] = hdr33[b];
#pragma unroll 1
    for (u32 b = 0; b < 16; b++) o[hdr + b] = nonce16[b];
    gcm_lane g;
    gcm_init(g, te, key32, nonce16);
    uint8_t *c = o + hdr + 16;
    gcm_ctr(g, te, pt, c, len);
    u32 tag[4];
    gcm_tag(tag, g, te, c, len);
    gcm_store_block(c + len, tag, 16);
}
// AesGcmDecrypt (DefaultCrypto.cs:283-299) of item = [33-byte header ||] nonce || C || tag: the tag is recomputed over
// the received C and all 16 bytes compared (BouncyCastle's InvalidCipherTextException otherwise); a rejected item's
// plaintext slot (plen bytes) is zero.  ok: the item has its session key.
SDI bool gcm_decrypt_lane(const u32 *te, uint8_t *pt, const uint8_t *item, u64 len, u32 hdr, const uint8_t *key32,
                          bool ok) {
    ok = ok && len >= hdr + 32;
    const u64 plen = len >= hdr + 32 ? len - hdr - 32 : 0;
    if (ok) {
        gcm_lane g;
        const uint8_t *c = item + hdr + 16;
        gcm_init(g, te, key32, item + hdr);
        u32 tag[4], got[4];
        gcm_tag(tag, g, te, c, plen);
        gcm_load_block(got, c + plen, 16);
        u32 diff = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) diff |= tag[w] ^ got[w];
        ok = diff == 0;
        if (ok) gcm_ctr(g, te, c, pt, plen);
    }
    if (!ok) {
#pragma unroll 1
        for (u64 b = 0; b < plen; b++) pt[b] = 0;
    }
    return ok;
}
