// lachain_amd/csrc/secp_comb.hpp — pieces shared by the secp256k1 kernel files (k_secp.hip: header-signature checks and
// signing; k_secp_recover.hip: public-key recovery): launch shape, the comb tables' geometry, the signed-digit recoding
// of a scalar, one comb-table addition and DefaultCrypto's recovery-id arithmetic.
#pragma once
#include "secp.hpp"

#define SECP_BLOCK 256
#define SECP_WIN 33                  // signed 8-bit digits of a scalar < n: 32 bytes + the final carry
#define SECP_TAB 128                 // multiples 1..128 per window
#define SECP_BATCH 16                // signatures per thread in the batched inversion

// a -= n when a >= n (a < 2^256 < 2n: one subtraction reduces mod n)
SDI void sc_reduce_once(u32 *a) {
    if (!u256_lt(a, SECP_N)) {
        u32 br = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) { u64 d = (u64)a[k] - SECP_N[k] - br; a[k] = (u32)d; br = (u32)(d >> 32) & 1; }
    }
}
// RestoreEncodedRecIdFromSignatureBuffer (DefaultCrypto.cs:31-44) and recId = (enc - 36) / 2 / chainId; C and C# both
// truncate toward zero.  Returns the id in [0, 3], or -1 (chain id 0 is a DivideByZeroException in the reference)
SDI int secp_rec_id(const uint8_t *sg, u32 sig_len, int chain_id) {
    int enc = sig_len == 66 ? (int)sg[64] * 256 + (int)sg[65] : (int)sg[64];
    if (chain_id == 0) return -1;
    int rec = (enc - 36) / 2 / chain_id;
    return rec >= 0 && rec <= 3 ? rec : -1;
}
SDI void recode(int8_t *d, const sc &u) {
    u32 carry = 0;
#pragma unroll
    for (int w = 0; w < 32; w++) {
        u32 v = ((u.v[w >> 2] >> (8 * (w & 3))) & 0xffu) + carry;
        carry = v >= 128u;                                 // digits in [-128, 127]: int8 range
        d[w] = (int8_t)(int)(carry ? (int)v - 256 : (int)v);
    }
    d[32] = (int8_t)carry;
#pragma unroll
    for (int w = 33; w < 36; w++) d[w] = 0;
}
SDI void comb_add_entry(secp_jac &acc, const secp_aff &e, int d) {
    if (d == 0) return;
    fe y = e.y;
    if (d < 0) fe_neg(y, y);
    jac_add_aff(acc, acc, e.x, y);
}
