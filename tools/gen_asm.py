#!/usr/bin/env python3
"""tools/gen_asm.py — emits lachain_amd/csrc/asm_routines.hpp: hand-scheduled gfx950 assembly leaf
routines for the hot field arithmetic, with a custom register calling convention, plus the HIP wrappers
that call them.

Why: the pairing runs one lane per share with ~400 live VGPRs (one wave per SIMD).  A compiler-built
Montgomery multiply is a single dependent MAC chain (each v_mad_u64_u32 waits ~12 cycles for the previous
one: profiles/r01_valu_rates.jsonl), and passing Fp2 operands to a non-inlined function goes through
scratch (the AMDGPU ABI passes aggregates >16 registers in memory).  These routines instead take their
operands in fixed VGPRs (v0..), interleave 2-3 independent Montgomery products column by column so consecutive
MACs are independent, and give each product chain its own SGPR carry pair.  The inline asm that calls them tells
the compiler through register-tuple constraints and a clobber list exactly which registers move.

The emitters and their conventions (streams, operands, the accumulator ring, hazards, calls) are tools/asm_core.py's.
Here: the fused product-and-reduction of the eager routines (products, products_sqr), the routines, their HIP
wrappers, and the inline carry chains.  Modulus limbs live in VGPRs inside a routine (GFX9 VOP3 reads at most one
SGPR per instruction).  All routine outputs are fully reduced (< p); unreduced Karatsuba sums (< 2p) are valid
multiplicands because R > 4p.

Routines (label: inputs -> outputs, all 12-limb little-endian Montgomery):
  lcb_r_fp_mul      v[0:11]=a, v[12:23]=b                 -> v[0:11]=a*b
  lcb_r_fp_sqr      v[0:11]=a                             -> v[0:11]=a^2   (78 products for a*a)
  lcb_r_fp_mul2     v[0:11]=a0, v[12:23]=b0, v[24:35]=a1, v[36:47]=b1 -> v[0:11]=a0*b0, v[24:35]=a1*b1
  lcb_r_fp2_mul     v[0:23]=x, v[24:47]=y                 -> v[0:23]=x*y   (Karatsuba, 3 chains)
  lcb_r_fp2_sqr     v[0:23]=x                             -> v[0:23]=x^2   ((a+b)(a-b), 2ab: 2 chains)
  lcb_r_fp2_mul_fp  v[0:23]=x, v[24:35]=s                 -> v[0:23]=x*s   (2 chains)
"""
import os
import sys
from itertools import count

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asm_core import (N, P, PINV, PL, add_chain, c_quote, call_lines, clobbers, comba, condsub,  # noqa: E402
                      interleave_carry, library_header, limbs, merge, mov_regs, movs_const, ph, redc, ring, sub_chain)

S_PINV = 88
CARRY = [90, 92, 94]          # per-chain carry SGPR pairs
S_TMP = 96                    # scratch carry pair for add/sub chains (s[96:97])
S_TMP2 = 98                   # second scratch pair (s[98:99])
CLOBBER_SGPRS = [30, 31, S_PINV] + [c + d for c in CARRY for d in (0, 1)] + [S_TMP, S_TMP + 1, S_TMP2, S_TMP2 + 1]
RET = "s_setpc_b64 s[30:31]"


def vr(base):
    return list(range(base, base + N))


def load_p(preg):
    return movs_const(preg, PL) + [f"s_mov_b32 s{S_PINV}, 0x{PINV:08x}"]


def products(chains, preg):
    """Interleaved Montgomery products (product scanning / FIPS, the reduction's MACs in the product's columns):
    chains = [dict(a=[12 regs], b=[12 regs], m=[12 regs], acc=ring block, out=[12 regs])], chain t carrying in
    CARRY[t], p in preg.  out[j] may alias a[j] (written after a[j]'s last use).  Results are in [0, 2p)."""
    s = []
    a = s.append
    for c in chains:
        s += [f"v_mov_b32 v{c['acc']}, 0", f"v_mov_b32 v{c['acc'] + 1}, 0"]
    for k in range(2 * N - 1):
        lo = 0 if k < N else k - (N - 1)
        up = k if k < N else N - 1
        terms = []
        for i in range(lo, up + 1):
            terms.append(("ab", i, k - i))
            if i < k:
                terms.append(("mp", i, k - i))
        if k < N:
            terms.append(("m", k, 0))
        for n_t, (kind, i, j) in enumerate(terms):
            if kind == "m":
                for c in chains:
                    a(f"v_mul_lo_u32 v{c['m'][k]}, v{ring(c['acc'], k)[0]}, s{S_PINV}")
            for t, c in enumerate(chains):
                L, H, C = ring(c["acc"], k)
                x, y = (c["a"][i], c["b"][j]) if kind == "ab" else (c["m"][i], preg[j])
                a(f"v_mad_u64_u32 v[{L}:{H}], s[{CARRY[t]}:{CARRY[t] + 1}], v{x}, v{y}, v[{L}:{H}]")
            for t, c in enumerate(chains):
                L, H, C = ring(c["acc"], k)
                sc = f"s[{CARRY[t]}:{CARRY[t] + 1}]"
                a(f"v_addc_co_u32_e64 v{C}, {sc}, 0, {0 if n_t == 0 else 'v%d' % C}, {sc}")
        for c in chains:
            L, H, C = ring(c["acc"], k)
            if k >= N:
                a(f"v_mov_b32 v{c['out'][k - N]}, v{L}")
            if k == 2 * N - 2:
                a(f"v_mov_b32 v{c['out'][N - 1]}, v{H}")   # top carry word is 0: result < 2p < 2^384
            else:
                a(f"v_mov_b32 v{ring(c['acc'], k + 1)[0]}, v{H}")
    return s


# ------------------------------------------------------------------ routines
def r_fp_mul():
    P_, A, B, M = vr(40), vr(0), vr(12), vr(24)
    return (["lcb_r_fp_mul:"] + load_p(P_) + products([dict(a=A, b=B, m=M, acc=36, out=A)], P_) +
            condsub(A, P_, M, S_TMP) + [RET]), 52


def r_fp_mul2():
    P_ = vr(80)
    A0, B0, A1, B1, M0, M1 = vr(0), vr(12), vr(24), vr(36), vr(48), vr(60)
    s = ["lcb_r_fp_mul2:"] + load_p(P_)
    s += products([dict(a=A0, b=B0, m=M0, acc=72, out=A0), dict(a=A1, b=B1, m=M1, acc=76, out=A1)], P_)
    return s + condsub(A0, P_, M0, S_TMP) + condsub(A1, P_, M1, S_TMP) + [RET], 92


def products_sqr(A, F, E, M, acc, preg):
    """Montgomery square of A (FIPS as products(), one chain): a^2 = sum_i a_i 2^(32i) W_i with
    W_i = a_i 2^(32i) + 2 sum_{j>i} a_j 2^(32j), whose limbs are a_i (j = i), F[j] = a_j << 1 (j = i + 1) and
    E[j] = limb j of 2a = (a_j << 1) | (a_{j-1} >> 31) (j > i + 1; a_11 < 2^29, so no limb 12): 78 products
    instead of 144 for the a*a half.  F, E are indexed by limb (dicts); the result (< 2p) is written over A."""
    s = [f"v_mov_b32 v{acc}, 0", f"v_mov_b32 v{acc + 1}, 0"]
    a = s.append
    sc = f"s[{CARRY[0]}:{CARRY[0] + 1}]"
    for k in range(2 * N - 1):
        terms = []
        for i in range(max(0, k - (N - 1)), k // 2 + 1):
            j = k - i
            terms.append(("sq", A[i], A[i] if j == i else (F[j] if j == i + 1 else E[j])))
        lo = 0 if k < N else k - (N - 1)
        up = k if k < N else N - 1
        for i in range(lo, up + 1):
            if i < k:
                terms.append(("mp", M[i], preg[k - i]))
        if k < N:
            terms.append(("m", M[k], preg[0]))
        L, H, C = ring(acc, k)
        for n_t, (kind, x, y) in enumerate(terms):
            if kind == "m":
                a(f"v_mul_lo_u32 v{M[k]}, v{L}, s{S_PINV}")
            a(f"v_mad_u64_u32 v[{L}:{H}], {sc}, v{x}, v{y}, v[{L}:{H}]")
            a(f"v_addc_co_u32_e64 v{C}, {sc}, 0, {0 if n_t == 0 else 'v%d' % C}, {sc}")
        if k >= N:
            a(f"v_mov_b32 v{A[k - N]}, v{L}")      # A[k-N]'s last use (as a_i, i <= k - 12 ... ) was column k - 1
        if k == 2 * N - 2:
            a(f"v_mov_b32 v{A[N - 1]}, v{H}")
        else:
            a(f"v_mov_b32 v{ring(acc, k + 1)[0]}, v{H}")
    return s


def r_fp_sqr():
    P_, A = vr(50), vr(0)
    F = {j: 11 + j for j in range(1, N)}          # v12..v22
    E = {j: 21 + j for j in range(2, N)}          # v23..v32
    M = [33 + j for j in range(N)]                # v33..v44
    s = ["lcb_r_fp_sqr:"] + load_p(P_)
    s += [f"v_lshlrev_b32 v{F[j]}, 1, v{A[j]}" for j in range(1, N)]
    s += [f"v_alignbit_b32 v{E[j]}, v{A[j]}, v{A[j - 1]}, 31" for j in range(2, N)]
    return s + products_sqr(A, F, E, M, 46, P_) + condsub(A, P_, M, S_TMP) + [RET], 62


def r_fp2_sqr():
    P_ = vr(80)
    XA, XB, S, D, M0, M1 = vr(0), vr(12), vr(24), vr(36), vr(48), vr(60)
    s = ["lcb_r_fp2_sqr:"] + load_p(P_)
    s += add_chain(S, XA, XB, S_TMP)                                         # a + b   (< 2p)
    s += sub_chain(D, XA, XB, S_TMP) + add_chain(D, D, P_, S_TMP)            # a - b + p (< 2p)
    s += products([dict(a=S, b=D, m=M0, acc=72, out=S), dict(a=XA, b=XB, m=M1, acc=76, out=XA)], P_)
    s += condsub(S, P_, M0, S_TMP)                                           # r.a = a^2 - b^2
    s += condsub(XA, P_, M1, S_TMP)                                          # ab
    s += add_chain(XB, XA, XA, S_TMP) + condsub(XB, P_, M1, S_TMP)           # r.b = 2ab
    return s + mov_regs(XA, S) + [RET], 92


def r_fp2_mul_fp():
    P_ = vr(80)
    XA, XB, S, M0, M1 = vr(0), vr(12), vr(24), vr(36), vr(48)
    s = ["lcb_r_fp2_mul_fp:"] + load_p(P_)
    s += products([dict(a=XA, b=S, m=M0, acc=72, out=XA), dict(a=XB, b=S, m=M1, acc=76, out=XB)], P_)
    return s + condsub(XA, P_, M0, S_TMP) + condsub(XB, P_, M1, S_TMP) + [RET], 92


# ------------------------------------------------------------------ lazy (double-width) reduction
P2X4L = limbs(4 * P * P, 2 * N)     # 4p^2 < 2^764: keeps T0 - T1 + 4p^2 positive for multiplicands < 2p


def r_fp2_mul_lazy():
    """x*y in Fp2 with one Montgomery reduction per output coefficient (Karatsuba over double-width products):
    T0 = xa ya, T1 = xb yb, T2 = (xa + xb)(ya + yb) as 768-bit comba products (3 interleaved chains),
    U1 = T2 - T0 - T1, U0 = T0 - T1 + 4p^2, then REDC(U0), REDC(U1) (2 chains) and one conditional subtraction
    each: 3 x 144 + 2 x 156 = 744 MADs instead of 3 x 300 = 900, and no modular add/sub chains.
    Same contract as the eager routine: v[0:23] = x, v[24:47] = y in; v[0:23] = x*y out (fully reduced)."""
    P_ = vr(120)
    XA, XB, YA, YB, SA, SB = vr(0), vr(12), vr(24), vr(36), vr(48), vr(60)
    F0, F1, F2 = vr(72), vr(84), vr(96)
    T0 = F0[:11] + XA + [F0[11]]
    T1 = F1[:11] + XB + [F1[11]]
    T2 = F2[:11] + SA + [F2[11]]
    D = YA + YB                                   # b operands are dead after the products
    s = ["lcb_r_fp2_mul:"] + load_p(P_)
    s += merge([add_chain(SA, XA, XB, S_TMP), add_chain(SB, YA, YB, S_TMP2)])
    s += comba([dict(a=XA, b=YA, acc=108, out=T0, c=CARRY[0]),
                dict(a=XB, b=YB, acc=112, out=T1, c=CARRY[1]),
                dict(a=SA, b=SB, acc=116, out=T2, c=CARRY[2])])
    s += merge([sub_chain(T2, T2, T0, S_TMP), sub_chain(D, T0, T1, S_TMP2)])
    s += sub_chain(T2, T2, T1, S_TMP)             # U1 = T2 - T0 - T1  (>= 0)
    s += movs_const(T1, P2X4L)                    # 4p^2 into T1's registers
    s += add_chain(D, D, T1, S_TMP2)              # U0 = T0 - T1 + 4p^2  (> 0, mod 2^768)
    s += redc([dict(u=D, m=F0, acc=108, c=CARRY[0], out=D[N:]),
               dict(u=T2, m=F1, acc=112, c=CARRY[1], out=T2[N:])], P_, S_PINV)
    s += merge([condsub(D[N:], P_, SB, S_TMP, dst=XA), condsub(T2[N:], P_, F0, S_TMP2, dst=XB)])
    return s + [RET], 132


# ------------------------------------------------------------------ exponentiation by the field's constants
# lcb_r_fp_pow: v[0:11] = a, s84 = which (wave-uniform: 0 = p - 2, 1 = (p + 1)/4, 2 = (p - 1)/2, 3 = (p - 3)/4)
# -> v[0:11] = a^e.  The same sliding 4-bit windows as the compiled lcb_fp_pow_v (field.hpp), but the window table
# t1, t3, ..., t15 stays in VGPRs across the product calls: 12 caller-saved 8-register islands of the AMDGPU ABI from
# v64 (v64-71, v80-87, ..., v240-247), above every leaf routine's clobbers (<= v61), so neither this routine nor its
# callers save or reload it.  The compiled form kept the table in scratch (48 B reloaded per window, ~4.6 KB per
# exponentiation: most of the HBM traffic of every decompression lane, round 6).  The windows are known here, so
# each exponent is a straight-line program of steps `s_mov_b32 s82, cnt | idx << 16` + a call of lcb_r_fp_pow_step
# (cnt squarings, then one product by table entry idx; idx = 0xff: none).  Return addresses: s[80:81] (the
# routine), s[86:87] (the step); s83 counts.
POW_ISLANDS = [64 + 16 * k + j for k in range(12) for j in range(8)]           # v64-71, v80-87, ..., v240-247
POW_T = [POW_ISLANDS[12 * e:12 * e + 12] for e in range(8)]                     # t_(2e+1)
POW_EXPS = [P - 2, (P + 1) // 4, (P - 1) // 2, (P - 3) // 4]


def pow_program(e):
    """the sliding windows of field.hpp lcb_fp_pow_v for exponent e: (first table index, [(squarings, idx)])"""
    bit = lambda i: (e >> i) & 1
    i = e.bit_length() - 1
    first, steps, pend = None, [], 0
    while i >= 0:
        if not bit(i):
            pend += 1
            i -= 1
            continue
        j = max(i - 3, 0)
        while not bit(j):
            j += 1
        w = 0
        for b in range(i, j - 1, -1):
            w = (w << 1) | bit(b)
        if first is None:
            first = (w - 1) // 2
        else:
            steps.append((pend + i - j + 1, (w - 1) // 2))
        pend = 0
        i = j - 1
    if pend:
        steps.append((pend, 0xff))
    return first, steps


def pow_eval(a, e):
    """the program's value in plain integers (generator self-check)"""
    first, steps = pow_program(e)
    T = [pow(a, 2 * k + 1, P) for k in range(8)]
    acc = T[first]
    for cnt, idx in steps:
        for _ in range(cnt):
            acc = acc * acc % P
        if idx != 0xff:
            acc = acc * T[idx] % P
    return acc


def call(label):
    return call_lines(label, S_TMP)


def r_fp_pow():
    for ex in POW_EXPS:                         # generation-time check of the window programs
        assert pow_eval(7, ex) == pow(7, ex, P) and pow_eval(P - 3, ex) == pow(P - 3, ex, P)
    s = ["lcb_r_fp_pow:", "s_mov_b64 s[80:81], s[30:31]"]
    s += mov_regs(POW_T[0], vr(0))              # t1 = a
    s += call("lcb_r_fp_sqr")
    s += mov_regs(POW_T[7], vr(0))              # a^2, parked in t15's slot until t15 is formed
    for k in range(1, 8):
        s += mov_regs(vr(0), POW_T[k - 1]) + mov_regs(vr(12), POW_T[7]) + call("lcb_r_fp_mul")
        s += mov_regs(POW_T[k], vr(0))
    for w in range(len(POW_EXPS)):
        s += [f"s_cmp_eq_u32 s84, {w}", f"s_cbranch_scc1 lcb_r_fp_pow_e{w}"]
    s += ["s_branch lcb_r_fp_pow_e0"]
    for w, ex in enumerate(POW_EXPS):
        first, steps = pow_program(ex)
        s += [f"lcb_r_fp_pow_e{w}:"] + mov_regs(vr(0), POW_T[first])
        for cnt, idx in steps:
            s += [f"s_mov_b32 s82, {cnt | (idx << 16)}"] + call("lcb_r_fp_pow_step")
        s += ["s_setpc_b64 s[80:81]"]
    # the step: s82 = cnt | idx << 16
    s += ["lcb_r_fp_pow_step:", "s_mov_b64 s[86:87], s[30:31]", "s_and_b32 s83, s82, 0xffff",
          "lcb_r_fp_pow_sq:", "s_cmp_eq_u32 s83, 0", "s_cbranch_scc1 lcb_r_fp_pow_sel"]
    s += call("lcb_r_fp_sqr") + ["s_sub_u32 s83, s83, 1", "s_branch lcb_r_fp_pow_sq"]
    s += ["lcb_r_fp_pow_sel:", "s_lshr_b32 s83, s82, 16"]
    for k in range(8):
        s += [f"s_cmp_eq_u32 s83, {k}", f"s_cbranch_scc1 lcb_r_fp_pow_t{k}"]
    s += ["s_setpc_b64 s[86:87]"]               # idx 0xff: squarings only
    for k in range(8):
        s += [f"lcb_r_fp_pow_t{k}:"] + mov_regs(vr(12), POW_T[k]) + ["s_branch lcb_r_fp_pow_mul"]
    return s + ["lcb_r_fp_pow_mul:"] + call("lcb_r_fp_mul") + ["s_setpc_b64 s[86:87]"], 64


ROUTINES = [r_fp_mul, r_fp_sqr, r_fp_mul2, r_fp2_mul_lazy, r_fp2_sqr, r_fp2_mul_fp, r_fp_pow]


def clobber_list(nvgpr, keep):
    # scc: the call sequence's s_add_u32/s_addc_u32 write SCC; a compare the compiler hoisted above the call would
    # otherwise feed a stale SCC to the branch after it
    return clobbers(v=[i for i in range(nvgpr) if i not in keep], s=CLOBBER_SGPRS, flags=["scc"])


def pow_clobbers():
    return clobbers(v=list(range(12, 64)) + POW_ISLANDS, s=[30, 31, 80, 81, 82, 83, 86, 87] + CLOBBER_SGPRS[2:],
                    flags=["scc"])


def call_seq(label):
    return c_quote(call(label))


def render():
    streams, nv = [], {}
    for fn in ROUTINES:
        txt, n = fn()
        streams.append(txt)
        nv[fn.__name__] = n
    out = [library_header("gen_asm.py", "gfx950 assembly leaf routines with a register calling convention "
                          "(see the generator's docstring).",
                          "typedef uint32_t u32;\ntypedef u32 u32x12 __attribute__((ext_vector_type(12)));\n",
                          "LCB_ASM", streams)]
    # wrappers
    out.append(f"""// r = a*b
__device__ __forceinline__ u32x12 lcb_asm_fp_mul(u32x12 a, u32x12 b) {{
    asm({call_seq("lcb_r_fp_mul")}
        : "+{{v[0:11]}}"(a), "+{{v[12:23]}}"(b)
        :
        : {clobber_list(nv['r_fp_mul'], set(range(24)))});
    return a;
}}
// r = a^2 (78 + 144 products instead of 288)
__device__ __forceinline__ u32x12 lcb_asm_fp_sqr(u32x12 a) {{
    asm({call_seq("lcb_r_fp_sqr")}
        : "+{{v[0:11]}}"(a)
        :
        : {clobber_list(nv['r_fp_sqr'], set(range(12)))});
    return a;
}}
// (a0*b0, a1*b1)
__device__ __forceinline__ void lcb_asm_fp_mul2(u32x12 &a0, u32x12 b0, u32x12 &a1, u32x12 b1) {{
    asm({call_seq("lcb_r_fp_mul2")}
        : "+{{v[0:11]}}"(a0), "+{{v[12:23]}}"(b0), "+{{v[24:35]}}"(a1), "+{{v[36:47]}}"(b1)
        :
        : {clobber_list(nv['r_fp_mul2'], set(range(48)))});
}}
// x*y in Fp2: (xa, xb) <- (xa, xb) * (ya, yb); lazy reduction (one REDC per coefficient)
__device__ __forceinline__ void lcb_asm_fp2_mul(u32x12 &xa, u32x12 &xb, u32x12 ya, u32x12 yb) {{
    asm({call_seq("lcb_r_fp2_mul")}
        : "+{{v[0:11]}}"(xa), "+{{v[12:23]}}"(xb), "+{{v[24:35]}}"(ya), "+{{v[36:47]}}"(yb)
        :
        : {clobber_list(nv['r_fp2_mul_lazy'], set(range(48)))});
}}
// x^2 in Fp2
__device__ __forceinline__ void lcb_asm_fp2_sqr(u32x12 &xa, u32x12 &xb) {{
    asm({call_seq("lcb_r_fp2_sqr")}
        : "+{{v[0:11]}}"(xa), "+{{v[12:23]}}"(xb)
        :
        : {clobber_list(nv['r_fp2_sqr'], set(range(24)))});
}}
// a^e for e = p - 2, (p + 1)/4, (p - 1)/2, (p - 3)/4 (which = 0..3, wave-uniform): the window table in VGPR islands
__device__ __forceinline__ u32x12 lcb_asm_fp_pow(u32x12 a, int which) {{
    asm({call_seq("lcb_r_fp_pow")}
        : "+{{v[0:11]}}"(a)
        : "{{s84}}"(which)
        : {pow_clobbers()});
    return a;
}}
// x*s for x in Fp2, s in Fp
__device__ __forceinline__ void lcb_asm_fp2_mul_fp(u32x12 &xa, u32x12 &xb, u32x12 s) {{
    asm({call_seq("lcb_r_fp2_mul_fp")}
        : "+{{v[0:11]}}"(xa), "+{{v[12:23]}}"(xb), "+{{v[24:35]}}"(s)
        :
        : {clobber_list(nv['r_fp2_mul_fp'], set(range(36)))});
}}
""")
    out.append("\n// ------------------------------------------------------------------ inline carry chains\n")
    return "".join(out + [g() for g in INLINE])


# ------------------------------------------------------------------ inline add / sub (no call)
# Compiler-built 12-limb add/sub with C carries costs ~160 VALU instructions (64-bit adds + shifts); these
# are the 36-37 instruction carry chains.  Operands are separate u32 (r, temps, inputs) so the register allocator
# places them.  A single chain carries in VCC through VOP2 (e32) forms and pays `s_nop 1` on every carry link: one
# wave per SIMD has nothing else to issue in the hazard slots.  An Fp2 or Fp6-row operation has 2 or 3 independent
# chains; interleaving them (chain 0 in VCC, the others in compiler-chosen SGPR pairs through VOP3) puts the other
# chains' instructions in the slots and needs at most `s_nop 0` per link.
def chain_add_mod(r, t, a, b, pv, c):
    """r = a + b mod p (a, b < p): t = a + b; r = t - p; borrow -> keep t.  p sits in VGPRs pv: a VOP2 with carry-in
    already uses the constant bus (VCC)"""
    return add_chain(t[:N], a, b, c) + condsub(t[:N], pv, r, c, dst=r)


def chain_sub_mod(r, t, a, b, pv, c):
    """r = a - b mod p, or -a mod p for b None: t = a - b; t[12] = t0 - t0 - borrow = all-ones iff a < b;
    r = t + (p & t[12])"""
    x, y = (["0"] * N, a) if b is None else (a, b)
    s = sub_chain(t[:N], x, y, c) + sub_chain(t[N:], t[:1], t[:1], c, carry_in=True)
    s += [f"v_and_b32_e32 {r[j]}, 0x{PL[j]:08x}, {t[N]}" for j in range(N)]
    return s + add_chain(r, t[:N], r, c)


def operand_numbers():
    """-> take(n): the next n inline asm operands, as placeholders"""
    nxt = count()
    return lambda n: ph(next(nxt) for _ in range(n))


P_INPUTS = [f'"v"(0x{PL[j]:08x}u)' for j in range(N)]


def inline_fn(name, comment, reduced_doc, n_tmp, n_in, build, r_early=False, with_p=False):
    """one chain: r = op(a[, b]); operands r, t, a, b, p in that order"""
    take = operand_numbers()
    r, t, a, b = take(N), take(n_tmp), take(N), take(N)
    body = interleave_carry([build(r, t, a, b if n_in == 2 else None, take(N), "vcc")], [])
    outs = [f'"=&v"(r[{j}])' if r_early else f'"=v"(r[{j}])' for j in range(N)]
    outs += [f'"=&v"(t[{j}])' for j in range(n_tmp)]
    ins = [f'"v"({"ab"[k]}[{j}])' for k in range(n_in) for j in range(N)] + (P_INPUTS if with_p else [])
    txt = "\\n\\t".join(body)
    args = ", ".join(["u32 *r"] + [f"const u32 *{'ab'[k]}" for k in range(n_in)])
    tmp_decl = f"    u32 t[{n_tmp}];\n" if n_tmp else ""
    return (f"// {comment} ({reduced_doc})\n"
            f"__device__ __forceinline__ void {name}({args}) {{\n{tmp_decl}"
            f"    asm volatile(\"{txt}\"\n        : {', '.join(outs)}\n        : {', '.join(ins)}\n        : \"vcc\");\n}}\n")


def inline_fnk(name, comment, K, n_tmp, n_in, with_p, build, pair=False, cross=False):
    """K independent 12-limb chains in one asm block: r_k = op(x_k[, y_k]), or op(x_0, x_1) in every chain (cross).
    Operands: r_k, t_k, the K - 1 carry pairs, x_k, y_k, p.  The C identifiers are r0, t0, sc1, x0, ...; for the two
    components of an Fp2 (pair) ra, rb, ta, tb, sc, xa, ..."""
    take = operand_numbers()
    r, t, sops = [take(N) for _ in range(K)], [take(n_tmp) for _ in range(K)], take(K - 1)
    x = [take(N) for _ in range(K)]
    y = [take(N) for _ in range(K)] if n_in == 2 else [None] * K
    pv = take(N) if with_p else None
    body = interleave_carry([build(r[k], t[k], *((x[0], x[1]) if cross else (x[k], y[k])), pv, "%S" if k else "vcc")
                             for k in range(K)], sops)
    tags = "ab" if pair else [str(k) for k in range(K)]
    scs = ["sc"] if pair else [f"sc{k}" for k in range(1, K)]
    outs = [f'"=&v"(r{g}[{j}])' for g in tags for j in range(N)]
    outs += [f'"=&v"(t{g}[{j}])' for g in tags for j in range(n_tmp)] + [f'"=&s"({sc})' for sc in scs]
    ins = [f'"v"({v}{g}[{j}])' for v in "xy"[:n_in] for g in tags for j in range(N)] + (P_INPUTS if with_p else [])
    args = ", ".join([f"u32 *r{g}" for g in tags] + [f"const u32 *{v}{g}" for v in "xy"[:n_in] for g in tags])
    tdecl = [f"t{g}[{n_tmp}]" for g in tags]
    decl = f"    u32 {', '.join(tdecl)};\n" if pair else "".join(f"    u32 {d};\n" for d in tdecl)
    how = ("both Fp components in one interleaved pair of carry chains" if pair else
           f"{K} independent carry chains interleaved in one block")
    txt = "\\n\\t".join(body)
    return (f"// {comment}: {how}\n"
            f"__device__ __forceinline__ void {name}({args}) {{\n{decl}"
            f"    unsigned long long {', '.join(scs)};\n"
            f"    asm volatile(\"{txt}\"\n        : {', '.join(outs)}\n        : {', '.join(ins)}\n        : \"vcc\");\n}}\n")


def gen_add_mod():
    return inline_fn("lcb_fp_add_asm", "r = a + b mod p", "a, b < p -> r < p", N, 2, chain_add_mod,
                     r_early=True, with_p=True)


def gen_sub_mod():
    return inline_fn("lcb_fp_sub_asm", "r = a - b mod p", "a, b < p -> r < p", N + 1, 2, chain_sub_mod)


def gen_add_nr():
    return inline_fn("lcb_fp_add_nr_asm", "r = a + b, not reduced", "a, b < p -> r < 2p: multiplicand only", 0, 2,
                     lambda r, t, a, b, pv, c: add_chain(r, a, b, c), r_early=True)


def gen_neg():
    return inline_fn("lcb_fp_neg_asm", "r = -a mod p", "a < p -> r < p", N + 1, 1, chain_sub_mod)


def gen_fp2_add():
    return inline_fnk("lcb_fp2_add_asm", "(ra, rb) = (xa + ya, xb + yb) mod p", 2, N, 2, True, chain_add_mod, pair=True)


def gen_fp2_sub():
    return inline_fnk("lcb_fp2_sub_asm", "(ra, rb) = (xa - ya, xb - yb) mod p", 2, N + 1, 2, False, chain_sub_mod,
                      pair=True)


def gen_fp2_neg():
    return inline_fnk("lcb_fp2_neg_asm", "(ra, rb) = (-xa, -xb) mod p", 2, N + 1, 1, False, chain_sub_mod, pair=True)


def gen_fp2_mul_xi():
    # (a + b i)(1 + i) = (a - b) + (a + b) i: a subtraction chain and an addition chain side by side
    return inline_fnk("lcb_fp2_mul_xi_asm", "(ra, rb) = (xa - xb, xa + xb) mod p", 2, N + 1, 1, True,
                      lambda r, t, a, b, pv, c: (chain_sub_mod if c == "vcc" else chain_add_mod)(r, t, a, b, pv, c),
                      pair=True, cross=True)


def gen_fp3_add():
    return inline_fnk("lcb_fp3_add_asm", "r_k = x_k + y_k mod p, k = 0..2", 3, N, 2, True, chain_add_mod)


def gen_fp3_sub():
    return inline_fnk("lcb_fp3_sub_asm", "r_k = x_k - y_k mod p, k = 0..2", 3, N + 1, 2, False, chain_sub_mod)


INLINE = [gen_add_mod, gen_sub_mod, gen_add_nr, gen_neg, gen_fp2_add, gen_fp2_sub, gen_fp2_neg, gen_fp2_mul_xi,
          gen_fp3_add, gen_fp3_sub]


def main():
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lachain_amd", "csrc", "asm_routines.hpp")
    with open(dst, "w") as f:
        f.write(render())
    print("wrote", os.path.normpath(dst))


if __name__ == "__main__":
    main()
