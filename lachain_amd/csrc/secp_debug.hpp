// lachain_amd/csrc/secp_debug.hpp — TEST HOOK: one secp256k1 routine of secp.hpp / secp_comb.hpp / k_secp_recover.hip on
// one item, for the edge-operand tests.  The same function runs in three places, each compared with Python integers
// (tests/pyref/secp.py) at the operands of tests/secp_cases.py:
//   the device kernel k_secp_debug (k_secp_recover.hip; lcb_debug_secp_op, tests/test_gpu_secp_edges.py): the field
//     operations are the generated assembly of secp_asm.hpp there;
//   the host emulation (tools/emul/secp_recover_emul.cpp, emu_debug_secp_op, tests/test_secp_edges_emul.py): the C++
//     field operations;
//   and the assembly alone is simulated from its text by tests/test_secp_asm_sim.py.
// Included by k_secp_recover.hip after recode4; no production kernel calls it.
//
// Item layout (u32 words).  In, a and b alike, SECP_DEBUG_IN = 25: x[8] y[8] z[8] inf.  A field or scalar operand is x;
// a point is (x, y, z) Jacobian with inf != 0 for infinity; the affine operand of op 15 is (x, y) of b.
// Out, SECP_DEBUG_OUT = 44: x[8] y[8] z[8] inf flags digits[18].
//   ops 0..8    field: mul, sqr, add, sub, neg, dbl, canon, inv, sqrt of a.x (and b.x) -> x, as the routine leaves it
//   op 9        predicates -> flags: bit 0 fe_is_zero(a), bit 1 fe_is_odd(a), bit 2 fe_eq(a, b)
//   op 10, 11   sc_mont_mul(a, b), sc_mont_inv(a) -> x
//   op 12       glv_split(a) and recode4 of both halves: magnitudes -> x, y; flags bit 0 / 1: the first / second half is
//               negative; digits: e1[36] then e2[36] as signed bytes
//   op 13       the comb's recode(a) -> digits: d[36] as signed bytes
//   op 14..16   jac_dbl(a), jac_add_aff(a, b.x, b.y), jac_add(a, b) -> x, y, z, inf (the coordinates of an infinite
//               result are written as zero: the routines leave them unset)
#pragma once
#define SECP_DEBUG_IN 25
#define SECP_DEBUG_OUT 44
#define SECP_DEBUG_OPS 17

SDI secp_jac secp_debug_load(const u32 *p) {
    secp_jac r;
    r.x = fe_from(p); r.y = fe_from(p + 8); r.z = fe_from(p + 16);
    r.inf = p[24] != 0;
    return r;
}
SDI void secp_debug_digits(u32 *out, const int8_t *d, int n) {      // n signed bytes, four per word from the low byte
    for (int w = 0; w < n; w++) out[w >> 2] |= (u32)(uint8_t)d[w] << (8 * (w & 3));
}
SDI void secp_debug_op(int op, const u32 *a, const u32 *b, u32 *out) {
    for (int i = 0; i < SECP_DEBUG_OUT; i++) out[i] = 0;
    const secp_jac pa = secp_debug_load(a), pb = secp_debug_load(b);
    fe r = fe_zero();
    u32 flags = 0;
    switch (op) {
    case 0: fe_mul(r, pa.x, pb.x); break;
    case 1: fe_sqr(r, pa.x); break;
    case 2: fe_add(r, pa.x, pb.x); break;
    case 3: fe_sub(r, pa.x, pb.x); break;
    case 4: fe_neg(r, pa.x); break;
    case 5: fe_dbl(r, pa.x); break;
    case 6: r = fe_canon(pa.x); break;
    case 7: fe_inv(r, pa.x); break;
    case 8: fe_sqrt(r, pa.x); break;
    case 9:
        flags = (fe_is_zero(pa.x) ? 1u : 0u) | (fe_is_odd(pa.x) ? 2u : 0u) | (fe_eq(pa.x, pb.x) ? 4u : 0u);
        break;
    case 10: case 11: {
        sc s;
        if (op == 10) sc_mont_mul(s, sc_from(pa.x.v), sc_from(pb.x.v)); else sc_mont_inv(s, sc_from(pa.x.v));
        r = fe_from(s.v);
        break;
    }
    case 12: {
        u32 m1[8], m2[8];
        bool n1, n2;
        int8_t e[72];
        glv_split(m1, n1, m2, n2, pa.x.v);
        recode4(e, m1, n1);
        recode4(e + 36, m2, n2);
        r = fe_from(m1);
        for (int i = 0; i < 8; i++) out[8 + i] = m2[i];
        flags = (n1 ? 1u : 0u) | (n2 ? 2u : 0u);
        secp_debug_digits(out + 26, e, 72);
        break;
    }
    case 13: {
        int8_t d[36];
        recode(d, sc_from(pa.x.v));
        secp_debug_digits(out + 26, d, 36);
        break;
    }
    case 14: case 15: case 16: {
        secp_jac q;
        q.x = q.y = q.z = fe_zero();
        q.inf = false;
        if (op == 14) jac_dbl(q, pa);
        else if (op == 15) jac_add_aff(q, pa, pb.x, pb.y);
        else jac_add(q, pa, pb);
        if (q.inf) q.x = q.y = q.z = fe_zero();
        r = q.x;
        for (int i = 0; i < 8; i++) { out[8 + i] = q.y.v[i]; out[16 + i] = q.z.v[i]; }
        out[24] = q.inf ? 1u : 0u;
        break;
    }
    default: break;
    }
    for (int i = 0; i < 8; i++) out[i] = r.v[i];
    out[25] = flags;
}
