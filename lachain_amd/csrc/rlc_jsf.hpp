// lachain_amd/csrc/rlc_jsf.hpp — the Joint Sparse Form (Solinas, "Low-weight binary representations for pairs of
// integers", 2001) of the two 32-bit halves (a, b) of a batch exponent a + b lambda.  Plain C++, host and device: the
// wave-uniform ladder of rlc_common.hpp (g1_mul_ab_jsf) runs it once per wave on scalar registers, and
// tests/test_rlc_jsf.py compiles it with the host compiler.
//
// a = sum da_k 2^k, b = sum db_k 2^k with da_k, db_k in {-1, 0, 1}, k = 0..32 (one column more than the binary
// form), as four 64-bit column masks.  Of any three consecutive columns at least one is zero in both rows, and a
// column is nonzero (in either row) with probability 1/2 — 16.5 of the 33 — against 3/4 of the binary form's 32.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RLC_JSF_FN __host__ __device__ inline
#else
#define RLC_JSF_FN inline
#endif

#define RLC_JSF_COLS 33

struct rlc_jsf {
    uint64_t nz_a, neg_a;       // digit of a nonzero / negative, bit k = column k
    uint64_t nz_b, neg_b;       // the same for b
};

// one row's digit at a column: l = the row's remaining value (carry included), m = the other row's
RLC_JSF_FN int rlc_jsf_digit(uint64_t l, uint64_t m) {
    if (!(l & 1)) return 0;
    int u = 2 - (int)(l & 3);                                        // l mods 4: 1 -> 1, 3 -> -1
    if (((l & 7) == 3 || (l & 7) == 5) && (m & 3) == 2) u = -u;      // make the next column zero in both rows
    return u;
}

RLC_JSF_FN void rlc_jsf_recode(rlc_jsf &o, uint32_t a, uint32_t b) {
    uint64_t k0 = a, k1 = b;
    uint32_t d0 = 0, d1 = 0;                                         // the rows' carries
    o.nz_a = o.neg_a = o.nz_b = o.neg_b = 0;
    for (int j = 0; j < RLC_JSF_COLS; j++) {
        const uint64_t l0 = k0 + d0, l1 = k1 + d1;
        if (!(l0 | l1)) break;
        const int u0 = rlc_jsf_digit(l0, l1), u1 = rlc_jsf_digit(l1, l0);
        if (2 * (int)d0 == 1 + u0) d0 = 1 - d0;
        if (2 * (int)d1 == 1 + u1) d1 = 1 - d1;
        k0 >>= 1;
        k1 >>= 1;
        o.nz_a |= (uint64_t)(u0 != 0) << j;
        o.neg_a |= (uint64_t)(u0 < 0) << j;
        o.nz_b |= (uint64_t)(u1 != 0) << j;
        o.neg_b |= (uint64_t)(u1 < 0) << j;
    }
}
