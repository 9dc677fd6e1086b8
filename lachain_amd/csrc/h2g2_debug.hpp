// lachain_amd/csrc/h2g2_debug.hpp — TEST HOOK: one routine under hash-to-G2 (h2g2.hpp, field.hpp) or one point
// decoder (curve.hpp) on one item, for the edge-operand tests: the device kernel k_h2g2_debug (k_ptmul.hip;
// lcb_debug_h2g2_op, tests/test_gpu_h2g2_edges.py) runs it one lane per item, and every result is compared with Python
// integers (tests/pyref/bls12_381.py) at the operands of tests/h2g2_cases.py.  Included by k_ptmul.hip; no production
// kernel calls it.
//
// Item layout (u32 words).  In, H2G2_DEBUG_IN = 48; out, H2G2_DEBUG_OUT = 76: value words [0, 72), out[72] = the
// routine's flag, out[73] = 1 for a decoded point at infinity, the rest zero.  A field operand is the 12 Montgomery
// words the routine sees (a canonical residue, < p), an Fp2 operand a[12] b[12]; bytes are packed little-endian.
//   op 0   fp_sqrt(in[0..12))                 -> a^((p+1)/4) at [0, 12), flag: it is a root
//   op 1   fp2_sqrt(in[0..24))                -> root at [0, 24) (zero without one), flag: a root exists
//   op 2   fp2_sqrt_any                       -> the same layout; the root may be the negative of fp2_sqrt's
//   op 3   fp2_sqrt_normed                    -> root at [0, 24), flag: the norm is a square.  The norm and its fp_sqrt
//                                                root are formed as g2_calc_bn forms them; the routine runs only when
//                                                the flag is set (it is unspecified for non-squares: zero is written)
//   op 4   fp_inv_gcd(in[0..12))              -> [0, 12)
//   op 5   fp2_inv_g(in[0..24))               -> [0, 24)
//   op 6   fp_set_hash_digest(64 bytes)       -> t at [0, 12)
//   op 7   g2_calc_bn(t = in[0..24))          -> affine x at [0, 24), y at [24, 48) (zero on failure), flag: ok
//   op 8   g2_clear_cofactor_bp               of the affine twist point x = in[0..24), y = in[24..48)
//   op 9   g2_clear_cofactor_h2               of the same -> Jacobian (X, Y, Z) at [0, 72); Z = 0 is infinity
//   op 10  g1_decompress(48 bytes)            -> affine x at [0, 12), y at [12, 24), flag: ok, out[73]: infinity
//   op 11  g2_decompress(96 bytes)            -> affine x at [0, 24), y at [24, 48), flag: ok, out[73]: infinity
// lcb_debug_h2g2_op's op 12 is no routine of this switch: it runs k_mcl_g2_clear alone on each item (lcb_mcl.cpp).
#pragma once
#define H2G2_DEBUG_IN 48
#define H2G2_DEBUG_OUT 76
#define H2G2_DEBUG_OPS 12

DI fp h2g2_debug_fp(const u32 *p) {
    fp r;
    for (int j = 0; j < 12; j++) r.v[j] = p[j];
    return r;
}
DI void h2g2_debug_put(u32 *o, const fp &a) {
    for (int j = 0; j < 12; j++) o[j] = a.v[j];
}
DI void h2g2_debug_put2(u32 *o, const fp2 &a) {
    h2g2_debug_put(o, a.a);
    h2g2_debug_put(o + 12, a.b);
}
// the operations are calls (DN): the kernel's registers and scratch are those of its largest routine, not their sum
DN u32 h2g2_debug_sqrt(int op, const u32 *in, u32 *out) {
    fp2 x, y = fp2_zero();
    x.a = h2g2_debug_fp(in);
    x.b = h2g2_debug_fp(in + 12);
    bool ok = false;
    if (op == 0) {
        ok = fp_sqrt(y.a, x.a);
    } else if (op == 1) {
        ok = fp2_sqrt(y, x);
    } else if (op == 2) {
        ok = fp2_sqrt_any(y, x);
    } else {
        fp n, u, nr;
        fp_sqr(n, x.a);
        fp_sqr(u, x.b);
        fp_add(n, n, u);
        ok = fp_sqrt(nr, n);
        if (ok) fp2_sqrt_normed(y, x, nr);
    }
    if (op && !ok) y = fp2_zero();
    h2g2_debug_put2(out, y);
    return ok ? 1u : 0u;
}
DN void h2g2_debug_inv(int op, const u32 *in, u32 *out) {
    fp2 x, y = fp2_zero();
    x.a = h2g2_debug_fp(in);
    x.b = h2g2_debug_fp(in + 12);
    if (op == 4) fp_inv_gcd(y.a, x.a);
    else fp2_inv_g(y, x);
    h2g2_debug_put2(out, y);
}
DN u32 h2g2_debug_map(const u32 *in, u32 *out) {
    fp2 t;
    t.a = h2g2_debug_fp(in);
    t.b = h2g2_debug_fp(in + 12);
    g2 P;
    P.x = P.y = P.z = fp2_zero();
    const bool ok = g2_calc_bn(P, t);
    if (!ok) P.x = P.y = fp2_zero();
    h2g2_debug_put2(out, P.x);
    h2g2_debug_put2(out + 24, P.y);
    return ok ? 1u : 0u;
}
DN void h2g2_debug_clear(int op, const u32 *in, u32 *out) {
    g2 P, Q;
    P.x.a = h2g2_debug_fp(in);
    P.x.b = h2g2_debug_fp(in + 12);
    P.y.a = h2g2_debug_fp(in + 24);
    P.y.b = h2g2_debug_fp(in + 36);
    P.z = fp2_one();
    if (op == 8) g2_clear_cofactor_bp(Q, P);
    else g2_clear_cofactor_h2(Q, P);
    h2g2_debug_put2(out, Q.x);
    h2g2_debug_put2(out + 24, Q.y);
    h2g2_debug_put2(out + 48, Q.z);
}
DN u32 h2g2_debug_decode(int op, const u32 *in, u32 *out) {
    bool ok, inf;
    if (op == 10) {
        g1a a;
        a.x = a.y = fp_zero();
        a.inf = false;
        ok = g1_decompress(a, (const uint8_t *)in);
        if (!ok) { a.x = a.y = fp_zero(); a.inf = false; }
        h2g2_debug_put(out, a.x);
        h2g2_debug_put(out + 12, a.y);
        inf = a.inf;
    } else {
        g2a a;
        a.x = a.y = fp2_zero();
        a.inf = false;
        ok = g2_decompress(a, (const uint8_t *)in);
        if (!ok) { a.x = a.y = fp2_zero(); a.inf = false; }
        h2g2_debug_put2(out, a.x);
        h2g2_debug_put2(out + 24, a.y);
        inf = a.inf;
    }
    out[73] = inf ? 1u : 0u;
    return ok ? 1u : 0u;
}
// in: this item's H2G2_DEBUG_IN words (4-byte aligned: the decoders read words); out: its H2G2_DEBUG_OUT words
DI void h2g2_debug_op(int op, const u32 *in, u32 *out) {
    for (int i = 0; i < H2G2_DEBUG_OUT; i++) out[i] = 0;
    u32 flag = 0;
    switch (op) {
    case 0: case 1: case 2: case 3: flag = h2g2_debug_sqrt(op, in, out); break;
    case 4: case 5: h2g2_debug_inv(op, in, out); break;
    case 6: {
        fp t;
        fp_set_hash_digest(t, (const uint8_t *)in);
        h2g2_debug_put(out, t);
        break;
    }
    case 7: flag = h2g2_debug_map(in, out); break;
    case 8: case 9: h2g2_debug_clear(op, in, out); break;
    case 10: case 11: flag = h2g2_debug_decode(op, in, out); break;
    default: break;
    }
    out[72] = flag;
}
