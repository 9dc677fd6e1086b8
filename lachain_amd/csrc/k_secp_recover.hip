// lachain_amd/csrc/k_secp_recover.hip — gfx950 kernels for batched secp256k1 public-key recovery (transaction
// authentication) and Keccak-256 over variable-length messages.
//
// Reference: TransactionVerifier.VerifyTransactions hands a block's receipts to one worker that recovers each sender
//   receipt.RecoverPublicKey -> DefaultCrypto.RecoverSignatureHashed -> ComputeAddress -> compare with Transaction.From
// (TransactionVerifier.cs:72-91,124-130; CryptoUtils.cs:53-58; DefaultCrypto.cs:146-168,197-200 over libsecp256k1's
// secp256k1_ecdsa_recover); the VM's ecrecover handlers call the same and SpecialRecoverSignatureHashed
// (ExternalHandler.cs:1197,1225,1242; DefaultCrypto.cs:170-195).
//
// Q = r^-1 (s R - z G) = u1 G + u2 R with u1 = -z / r, u2 = s / r.  R differs per signature, so u2 R is a
// variable-base multiplication: u2 = k1 + k2 lambda with |k1|, |k2| < 2^128 (secp.hpp), signed 4-bit digits of both
// halves, one per-lane table 1R .. 8R (Jacobian, 768 B of scratch) serving R and phi(R) = (beta X, Y, Z): 132
// doublings and 66 general additions.  Every lane adds at the same 66 places (fixed windows), so a wave does not
// diverge the way a sparse signed form (wNAF) would.  u1 G comes from the generator's comb table (33 mixed additions).
// One signature per lane, no LDS, no barriers.  Kernels:
//   k_secp_rec_scalars  parsing / recId / range checks, r^-1 (one inversion per 16 signatures), u1, u2 -> job records
//   k_secp_recover      R from x and the parity bit, u2 R + u1 G -> Jacobian Q
//   k_secp_rec_finish   Q to affine (one field inversion per 16 points), compressed key, address, optional From check
//   k_keccak256         Keccak-256 (original 0x01 padding) of variable-length messages, one lane per message
#include "secp_comb.hpp"
#ifndef SECP_HOST_EMULATION
#include "gate.hpp"
#endif

#define SECP_RWIN 33                 // signed 4-bit digits of a magnitude < 2^129: 32 nibbles + bit 128 and the carry
#define SECP_RTAB 8                  // multiples 1..8 of R per lane

struct secp_rjob {                   // 144 B, written by k_secp_rec_scalars, read by k_secp_recover
    int8_t d1[36];                   // comb digits of u1 (generator), windows 0..32
    int8_t e1[36], e2[36];           // signed 4-bit digits of k1 and k2, windows 0..32
    u32 x[8];                        // x(R): r, or r + n for recId & 2 (below p)
    u32 flags;                       // bit 0: all checks passed; bit 1: y(R) is odd
};
static_assert(sizeof(secp_rjob) == 144, "job record");
struct secp_rpoint {                 // 100 B, written by k_secp_recover, read by k_secp_rec_finish
    fe x, y, z;
    u32 ok;                          // 0: no key (failed check, x not on the curve, Q at infinity)
};
static_assert(sizeof(secp_rpoint) == 100, "point record");

// ------------------------------------------------------------------------------------------------ scalars
struct rsig_in {
    u32 r[8], s[8], z[8];
    int rec;
    bool ok;
};
// the checks of RecoverSignatureHashed / SpecialRecoverSignatureHashed and secp256k1_ecdsa_recoverable_signature_
// parse_compact before the curve arithmetic (no low-s rule here, unlike verification); z = hash mod n
SDI void load_rsig(rsig_in &q, size_t i, const uint8_t *hashes, const uint8_t *sigs, u32 sig_len, u32 want_len,
                   int chain_id, int special) {
    const uint8_t *sg = sigs + i * sig_len;
    u256_from_be(q.r, sg);
    u256_from_be(q.s, sg + 32);
    u256_from_be(q.z, hashes + 32 * i);
    sc_reduce_once(q.z);
    int rec = -1;
    if (sig_len == want_len) {
        if (special) rec = sg[64] == 27 ? 0 : (sg[64] == 28 ? 1 : -1);      // DefaultCrypto.cs:180-185
        else rec = secp_rec_id(sg, sig_len, chain_id);
    }
    bool ok = rec >= 0;
    ok = ok && u256_lt(q.r, SECP_N) && u256_lt(q.s, SECP_N);          // compact parse: overflow
    ok = ok && !u256_is_zero(q.r) && !u256_is_zero(q.s);              // secp256k1_ecdsa_sig_recover
    if (rec >= 2) ok = ok && u256_lt(q.r, SECP_PMN);                  // r + n must be a field element
    q.rec = rec < 0 ? 0 : rec;
    q.ok = ok;
}
// signed 4-bit digits in [-7, 8] of a magnitude below 2^129 (33 windows), negated for a negative half
SDI void recode4(int8_t *d, const u32 *m, bool neg) {
    u32 carry = 0;
#pragma unroll
    for (int w = 0; w < SECP_RWIN; w++) {
        u32 v = ((m[w >> 3] >> (4 * (w & 7))) & 0xfu) + carry;
        carry = v > 8u;
        int dv = carry ? (int)v - 16 : (int)v;
        d[w] = (int8_t)(neg ? -dv : dv);
    }
#pragma unroll
    for (int w = SECP_RWIN; w < 36; w++) d[w] = 0;
}
extern "C" __global__ void __launch_bounds__(SECP_BLOCK) k_secp_rec_scalars(const uint8_t *hashes, const uint8_t *sigs,
                                                                           u32 sig_len, u32 want_len, int chain_id,
                                                                           int special, u32 n, secp_rjob *jobs) {
    const size_t T = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    sc one = {{1, 0, 0, 0, 0, 0, 0, 0}}, r2 = sc_from(SECP_R2N);
    sc pre[SECP_BATCH];
#pragma unroll
    for (int k = 0; k < SECP_BATCH; k++) {
        size_t i = tid + k * T;
        sc rM = one;
        if (i < n) {
            rsig_in q;
            load_rsig(q, i, hashes, sigs, sig_len, want_len, chain_id, special);
            if (q.ok) rM = sc_from(q.r);
        }
        sc_mont_mul(rM, rM, r2);
        if (k == 0) pre[k] = rM; else sc_mont_mul(pre[k], pre[k - 1], rM);
    }
    sc inv;
    sc_mont_inv(inv, pre[SECP_BATCH - 1]);
#pragma unroll
    for (int k = SECP_BATCH - 1; k >= 0; k--) {
        size_t i = tid + k * T;
        sc rM = one;
        rsig_in q;
        q.ok = false;
        if (i < n) {
            load_rsig(q, i, hashes, sigs, sig_len, want_len, chain_id, special);
            if (q.ok) rM = sc_from(q.r);
        }
        sc_mont_mul(rM, rM, r2);
        sc wM;
        if (k > 0) sc_mont_mul(wM, inv, pre[k - 1]); else wM = inv;
        sc_mont_mul(inv, inv, rM);
        if (i < n) {
            secp_rjob j;
            sc u1, u2;
            sc_mont_mul(u1, sc_from(q.z), wM);             // z r^-1 (plain: the Montgomery factors cancel)
            if (!u256_is_zero(u1.v)) u256_sub(u1.v, SECP_N, u1.v);      // u1 = -z / r
            sc_mont_mul(u2, sc_from(q.s), wM);
            recode(j.d1, u1);
            u32 m1[8], m2[8];
            bool n1, n2;
            glv_split(m1, n1, m2, n2, u2.v);
            recode4(j.e1, m1, n1);
            recode4(j.e2, m2, n2);
            u64 c = 0;
#pragma unroll
            for (int l = 0; l < 8; l++) {                  // r + n < p was checked: no carry out
                c += (u64)q.r[l] + ((q.rec & 2) ? SECP_N[l] : 0u);
                j.x[l] = (u32)c;
                c >>= 32;
            }
            j.flags = (q.ok ? 1u : 0u) | ((q.rec & 1) ? 2u : 0u);
            jobs[i] = j;
        }
    }
}

// ------------------------------------------------------------------------------------------------ recovery
extern "C" __global__ void __launch_bounds__(SECP_BLOCK) k_secp_recover(const secp_rjob *jobs, u32 n,
                                                                       const secp_aff *g_table, secp_rpoint *out) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const secp_rjob *jp = jobs + i;
    secp_rpoint *op = out + i;
    const u32 flags = jp->flags;
    if (!(flags & 1u)) { op->ok = 0; return; }
    // R = (x, y) with y^2 = x^3 + 7 and the parity of the recovery id (secp256k1_ge_set_xo_var)
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
    // T[m - 1] = m R for m = 1..8; none is infinity (R has the odd prime order n)
    fe T[3 * SECP_RTAB];
    {
        secp_jac P, Q;
        jac_set_aff(P, x, y);
        T[0] = P.x; T[1] = P.y; T[2] = P.z;
        jac_dbl(Q, P);
        T[3] = Q.x; T[4] = Q.y; T[5] = Q.z;
#pragma unroll 1
        for (int m = 2; m < SECP_RTAB; m++) {
            jac_add_aff(Q, Q, x, y);
            T[3 * m] = Q.x; T[3 * m + 1] = Q.y; T[3 * m + 2] = Q.z;
        }
    }
    secp_jac acc;
    acc.inf = true;
    acc.x = acc.y = acc.z = fe_zero();
    const fe beta = fe_from(SECP_BETA);
    // u2 R = k1 R + k2 phi(R): from the top window down, four doublings, then the two halves' digits (one addition
    // site; h is uniform across the wave).  The additions keep every exceptional case (jac_add).
#pragma unroll 1
    for (int w = SECP_RWIN - 1; w >= 0; w--) {
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
    // + u1 G from the generator's comb table; the next window's entry is loaded while the current addition runs
    int dg = jp->d1[0];
    secp_aff eg = g_table[dg ? (dg < 0 ? -dg : dg) - 1 : 0];
#pragma unroll 1
    for (int w = 0; w < SECP_WIN; w++) {
        const int cg = dg;
        const secp_aff xg = eg;
        if (w + 1 < SECP_WIN) {
            dg = jp->d1[w + 1];
            eg = g_table[(w + 1) * SECP_TAB + (dg ? (dg < 0 ? -dg : dg) - 1 : 0)];
        }
        comb_add_entry(acc, xg, cg);
    }
    if (acc.inf) { op->ok = 0; return; }
    op->x = acc.x; op->y = acc.y; op->z = acc.z;
    op->ok = 1;
}

// ------------------------------------------------------------------------------------------------ finish
// affine Q -> 33-byte compressed key, address = Keccak-256(x || y)[12:] (ComputeAddress, DefaultCrypto.cs:197-200),
// accept = recovered and address == from (TransactionVerifier.cs:124-130).  Outputs may be null; a failed recovery
// writes zero bytes.
SDI u32 bswap32(u32 v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }
extern "C" __global__ void __launch_bounds__(SECP_BLOCK) k_secp_rec_finish(const secp_rpoint *pts, u32 n,
                                                                          uint8_t *pub33, uint8_t *addr20, uint8_t *ok_out,
                                                                          const uint8_t *from20, uint8_t *accept) {
    const size_t T = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
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
        fe x = fe_zero(), y = fe_zero();
        if (ok) {
            fe zi2;
            fe_sqr(zi2, zi);
            fe_mul(x, pts[i].x, zi2);
            fe_mul(zi2, zi2, zi);
            fe_mul(y, pts[i].y, zi2);
            x = fe_canon(x);
            y = fe_canon(y);
        }
        if (pub33) {
            uint8_t *o = pub33 + 33 * i;
            o[0] = ok ? (uint8_t)(2 + (y.v[0] & 1)) : 0;
#pragma unroll
            for (int b = 0; b < 32; b++) o[1 + b] = (uint8_t)(x.v[7 - b / 4] >> (8 * (3 - b % 4)));
        }
        if (ok_out) ok_out[i] = ok;
        if (addr20 || accept) {
            u64 s[25];
#pragma unroll
            for (int l = 0; l < 25; l++) s[l] = 0;
#pragma unroll
            for (int l = 0; l < 4; l++) {          // x || y big-endian, read as little-endian 64-bit lanes
                s[l] = (u64)bswap32(x.v[7 - 2 * l]) | ((u64)bswap32(x.v[6 - 2 * l]) << 32);
                s[4 + l] = (u64)bswap32(y.v[7 - 2 * l]) | ((u64)bswap32(y.v[6 - 2 * l]) << 32);
            }
            s[8] ^= 0x01;                          // Keccak padding (original domain byte) of a 64-byte message
            s[16] ^= 0x8000000000000000ULL;
            keccak_f1600(s);
            bool same = ok;
#pragma unroll
            for (int b = 0; b < 20; b++) {
                uint8_t a = ok ? (uint8_t)(s[(12 + b) / 8] >> (8 * ((12 + b) % 8))) : 0;
                if (addr20) addr20[20 * i + b] = a;
                if (from20) same = same && a == from20[20 * i + b];
            }
            if (accept) accept[i] = same && from20 != nullptr;
        }
    }
}

// ------------------------------------------------------------------------------------------------ Keccak-256
// message i = data[off[i] .. off[i + 1]); multi-block absorb at rate 136, padding 0x01 .. 0x80 (KeccakBytes)
extern "C" __global__ void __launch_bounds__(SECP_BLOCK) k_keccak256(const uint8_t *data, const u64 *off, u32 n,
                                                                    uint8_t *out32) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *m = data + off[i];
    const u64 len = off[i + 1] - off[i];
    const u64 blocks = len / 136 + 1;
    u64 s[25];
#pragma unroll
    for (int l = 0; l < 25; l++) s[l] = 0;
#pragma unroll 1
    for (u64 b = 0; b < blocks; b++) {
#pragma unroll
        for (int l = 0; l < 17; l++) {
            u64 v = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                u64 g = b * 136 + 8 * l + k;
                u32 byte = g < len ? m[g] : (g == len ? 0x01u : 0u);
                if (8 * l + k == 135 && b + 1 == blocks) byte ^= 0x80u;
                v |= (u64)byte << (8 * k);
            }
            s[l] ^= v;
        }
        keccak_f1600(s);
    }
#pragma unroll
    for (int k = 0; k < 32; k++) out32[32 * (size_t)i + k] = (uint8_t)(s[k / 8] >> (8 * (k % 8)));
}

// ------------------------------------------------------------------------------------------------ test hook
// one routine of secp.hpp / secp_comb.hpp / recode4 per lane on arbitrary operands (secp_debug.hpp has the layout)
#include "secp_debug.hpp"
extern "C" __global__ void __launch_bounds__(SECP_BLOCK) k_secp_debug(int op, const u32 *a, const u32 *b, u32 n,
                                                                     u32 *out) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 ia[SECP_DEBUG_IN], ib[SECP_DEBUG_IN], o[SECP_DEBUG_OUT];
#pragma unroll
    for (int k = 0; k < SECP_DEBUG_IN; k++) {
        ia[k] = a[(size_t)SECP_DEBUG_IN * i + k];
        ib[k] = b[(size_t)SECP_DEBUG_IN * i + k];
    }
    secp_debug_op(op, ia, ib, o);
#pragma unroll
    for (int k = 0; k < SECP_DEBUG_OUT; k++) out[(size_t)SECP_DEBUG_OUT * i + k] = o[k];
}

#ifndef SECP_HOST_EMULATION
// ---------------------------------------------------------------- host launch wrappers
static unsigned rec_blocks_for(size_t n) { return (unsigned)((n + SECP_BLOCK - 1) / SECP_BLOCK); }
extern "C" size_t lcbk_secp_rjob_bytes(void) { return sizeof(secp_rjob); }
extern "C" size_t lcbk_secp_rpoint_bytes(void) { return sizeof(secp_rpoint); }
extern "C" void lcbk_secp_rec_scalars(hipStream_t s, const uint8_t *hashes, const uint8_t *sigs, u32 sig_len,
                                      u32 want_len, int chain_id, int special, u32 n, void *jobs) {
    if (!n) return;
    size_t threads = (n + SECP_BATCH - 1) / SECP_BATCH;
    LCB_LAUNCH_GATED(k_secp_rec_scalars, dim3(rec_blocks_for(threads)), dim3(SECP_BLOCK), 0, s, hashes, sigs, sig_len,
                     want_len, chain_id, special, n, (secp_rjob *)jobs);
}
extern "C" void lcbk_secp_recover(hipStream_t s, const void *jobs, u32 n, const void *g_table, void *pts) {
    if (!n) return;
    LCB_LAUNCH_GATED(k_secp_recover, dim3(rec_blocks_for(n)), dim3(SECP_BLOCK), 0, s, (const secp_rjob *)jobs, n,
                     (const secp_aff *)g_table, (secp_rpoint *)pts);
}
extern "C" void lcbk_secp_rec_finish(hipStream_t s, const void *pts, u32 n, uint8_t *pub33, uint8_t *addr20,
                                     uint8_t *ok, const uint8_t *from20, uint8_t *accept) {
    if (!n) return;
    size_t threads = (n + SECP_BATCH - 1) / SECP_BATCH;
    LCB_LAUNCH_GATED(k_secp_rec_finish, dim3(rec_blocks_for(threads)), dim3(SECP_BLOCK), 0, s,
                     (const secp_rpoint *)pts, n, pub33, addr20, ok, from20, accept);
}
extern "C" void lcbk_keccak256(hipStream_t s, const uint8_t *data, const uint64_t *off, u32 n, uint8_t *out32) {
    if (!n) return;
    LCB_LAUNCH_GATED(k_keccak256, dim3(rec_blocks_for(n)), dim3(SECP_BLOCK), 0, s, data, (const u64 *)off, n, out32);
}
extern "C" size_t lcbk_secp_debug_in_words(void) { return SECP_DEBUG_IN; }
extern "C" size_t lcbk_secp_debug_out_words(void) { return SECP_DEBUG_OUT; }
extern "C" int lcbk_secp_debug_ops(void) { return SECP_DEBUG_OPS; }
extern "C" void lcbk_secp_debug(hipStream_t s, int op, const u32 *a, const u32 *b, u32 n, u32 *out) {
    if (!n) return;
    LCB_LAUNCH_GATED(k_secp_debug, dim3(rec_blocks_for(n)), dim3(SECP_BLOCK), 0, s, op, a, b, n, out);
}
#endif  // SECP_HOST_EMULATION
