#!/usr/bin/env python3
"""tools/gen_secp_asm.py — generates lachain_amd/csrc/secp_asm.hpp: gfx950 inline-assembly bodies of the secp256k1
field product and square (p = 2^256 - 2^32 - 977) used by k_secp.hip.

Each function is one asm block whose operands are pinned to v0..v15 (inputs / output); its temporaries are listed
as clobbers, so the compiler moves values in and out but never splits the carry chains.  Product: column (product)
scanning over the accumulator ring of tools/asm_core.py, at 8 limbs; it keeps its own emitter because its carries
ride in VCC through VOP2 (e32) forms, its zero is a VGPR and its top word leaves through the ring.  Square: the 28
cross products once, doubled by a 1-bit shift, plus the 8 squares.  Reduction: t = lo + hi * 977 + (hi << 32) column
by column, then the top word (< 2^34) folded once more by C = 2^32 + 977, and a final conditional + C if that wraps
(the result is < 2^256, congruent mod p: "weakly reduced", the representation secp.hpp uses).  977 and 0 live in
VGPRs (gfx9 VOP3 takes no literal operands, VOP2 needs a VGPR second source).

Verified at the edge operands of tests/secp_cases.py (every class of the reduction's tail and of the second correction
pass of the sum and the difference, which no ladder over random keys enters) in three places, each against Python
integers: the committed text of all four blocks interpreted on the CPU by tools/asm_sim.py (tests/test_secp_asm_sim.py,
which also holds every block to its outputs and clobbers), the C++ path the emulations compile instead
(tests/test_secp_edges_emul.py; tests/test_secp_emul.py on random operands), and the assembly on the device through
lcb_debug_secp_op (tests/test_gpu_secp_edges.py, word for word against the simulation).  The protocol tests
(tests/test_gpu_ecdsa.py and its siblings: every decision against the oracle) run it as the kernels do.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asm_core import c_quote, clobbers, ring  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lachain_amd", "csrc", "secp_asm.hpp")
ZERO = 41


def product(a, A, B, T, acc):
    """T[0..15] <- A[0..7] * B[0..7] (A, B, T register numbers), appended through a; acc: the ring block (even)"""
    rk = lambda k: ring(acc, k)                                                    # noqa: E731
    a(f"v_mov_b32 v{acc}, 0")
    a(f"v_mov_b32 v{acc + 1}, 0")
    for k in range(15):
        L, H, C = rk(k)
        terms = [(i, k - i) for i in range(8) if 0 <= k - i <= 7]
        for n, (i, j) in enumerate(terms):
            a(f"v_mad_u64_u32 v[{L}:{H}], vcc, v{A[i]}, v{B[j]}, v[{L}:{H}]")
            a(f"v_addc_co_u32_e32 v{C}, vcc, 0, v{C if n else ZERO}, vcc")
        a(f"v_mov_b32 v{T[k]}, v{L}")
        L2, H2, C2 = rk(k + 1)
        assert H2 == C
        a(f"v_mov_b32 v{L2}, v{H}")
    L, H, C = rk(15)
    a(f"v_mov_b32 v{T[15]}, v{L}")


def square(a, A, T, acc):
    """T <- A^2: cross products once (columns 1..13), doubled, plus the squares"""
    rk = lambda k: ring(acc, k)                                                    # noqa: E731
    a(f"v_mov_b32 v{T[0]}, 0")
    a(f"v_mov_b32 v{acc + 2}, 0")
    a(f"v_mov_b32 v{acc + 3}, 0")
    for k in range(1, 14):
        L, H, C = rk(k)
        terms = [(i, k - i) for i in range(8) if i < k - i <= 7]
        for n, (i, j) in enumerate(terms):
            a(f"v_mad_u64_u32 v[{L}:{H}], vcc, v{A[i]}, v{A[j]}, v[{L}:{H}]")
            a(f"v_addc_co_u32_e32 v{C}, vcc, 0, v{C if n else ZERO}, vcc")
        a(f"v_mov_b32 v{T[k]}, v{L}")
        L2, H2, C2 = rk(k + 1)
        a(f"v_mov_b32 v{L2}, v{H}")
    L, H, C = rk(14)
    a(f"v_mov_b32 v{T[14]}, v{L}")
    a(f"v_mov_b32 v{T[15]}, v{H}")                         # column 13's carry count: bits 480..511
    # double: T <<= 1 (top bit of T[14] goes to T[15])
    for k in range(15, 0, -1):
        a(f"v_alignbit_b32 v{T[k]}, v{T[k]}, v{T[k - 1]}, 31")
    a(f"v_lshlrev_b32 v{T[0]}, 1, v{T[0]}")
    # + squares: a_i^2 at columns 2i, 2i+1, carry chained through the whole 512 bits
    for i in range(8):                                     # the ring block as two pairs
        p0, p1 = (acc, acc + 1) if i % 2 == 0 else (acc + 2, acc + 3)
        a(f"v_mul_lo_u32 v{p0}, v{A[i]}, v{A[i]}")
        a(f"v_mul_hi_u32 v{p1}, v{A[i]}, v{A[i]}")
        if i == 0:
            a(f"v_add_co_u32_e32 v{T[0]}, vcc, v{T[0]}, v{p0}")
        else:
            a(f"v_addc_co_u32_e32 v{T[2 * i]}, vcc, v{T[2 * i]}, v{p0}, vcc")
        a(f"v_addc_co_u32_e32 v{T[2 * i + 1]}, vcc, v{T[2 * i + 1]}, v{p1}, vcc")


def reduce(a, T, R, X, K977):
    """R[0..7] <- T[0..15] mod p, weakly reduced.  X: 4 scratch registers (X[0] even); K977 holds 977."""
    L, H = X[0], X[1]
    # column k: t_k + 977 t_(8+k) + t_(7+k) (k >= 1) + carry; (L, H) = 64-bit column sum
    a(f"v_mov_b32 v{L}, v{T[0]}")
    a(f"v_mov_b32 v{H}, 0")
    for k in range(8):
        a(f"v_mad_u64_u32 v[{L}:{H}], vcc, v{T[8 + k]}, v{K977}, v[{L}:{H}]")   # < 2^64: no carry out
        if k >= 1:
            a(f"v_add_co_u32_e32 v{L}, vcc, v{L}, v{T[7 + k]}")
            a(f"v_addc_co_u32_e32 v{H}, vcc, 0, v{H}, vcc")
        a(f"v_mov_b32 v{R[k]}, v{L}")
        if k < 7:
            a(f"v_add_co_u32_e32 v{L}, vcc, v{H}, v{T[k + 1]}")
            a(f"v_addc_co_u32_e32 v{H}, vcc, 0, v{ZERO}, vcc")
    # k8 = carry + t_15 (the (hi << 32) term at limb 8), as (L, H) with H <= 1
    a(f"v_add_co_u32_e32 v{L}, vcc, v{H}, v{T[15]}")
    a(f"v_addc_co_u32_e32 v{H}, vcc, 0, v{ZERO}, vcc")
    # R += k8 C = k8 977 + (k8 << 32): limb 0 lo(L 977), limb 1 hi(L 977) + H 977 + L, limb 2 H
    P0, P1 = X[2], X[3]
    a(f"v_mul_lo_u32 v{P0}, v{L}, v{K977}")
    a(f"v_mul_hi_u32 v{P1}, v{L}, v{K977}")
    a(f"v_mad_u32_u24 v{P1}, v{H}, v{K977}, v{P1}")        # < 2^11: no overflow
    a(f"v_add_co_u32_e32 v{R[0]}, vcc, v{R[0]}, v{P0}")
    a(f"v_addc_co_u32_e32 v{R[1]}, vcc, v{R[1]}, v{P1}, vcc")
    a(f"v_addc_co_u32_e32 v{R[2]}, vcc, v{R[2]}, v{H}, vcc")
    for k in range(3, 8):
        a(f"v_addc_co_u32_e32 v{R[k]}, vcc, 0, v{R[k]}, vcc")
    a(f"v_addc_co_u32_e32 v{P0}, vcc, 0, v{ZERO}, vcc")      # wrap of the first chain (0 / 1)
    a(f"v_add_co_u32_e32 v{R[1]}, vcc, v{R[1]}, v{L}")
    for k in range(2, 8):
        a(f"v_addc_co_u32_e32 v{R[k]}, vcc, 0, v{R[k]}, vcc")
    a(f"v_addc_co_u32_e32 v{P0}, vcc, v{P0}, v{ZERO}, vcc")  # total wraps w (at most one: the sum added is < 2^67)
    # R += w C (the value is < 2^67 after a wrap: no further carry out)
    a(f"v_mul_u32_u24 v{P1}, v{P0}, v{K977}")
    a(f"v_add_co_u32_e32 v{R[0]}, vcc, v{R[0]}, v{P1}")
    a(f"v_addc_co_u32_e32 v{R[1]}, vcc, v{R[1]}, v{P0}, vcc")
    for k in range(2, 8):
        a(f"v_addc_co_u32_e32 v{R[k]}, vcc, 0, v{R[k]}, vcc")


def addsub_lines(sub):
    """inline asm with compiler-allocated operands: %0..%7 r (early clobber), %8 t, %9 u, %10 z (temps),
    %11..%18 a, %19..%26 b.  add: r = a + b, then + C per carry out (twice at most); sub: r = a - b, then - C
    (= + p mod 2^256) per borrow (twice at most) — the same values as secp.hpp's C++ fe_add / fe_sub."""
    R = [f"%{i}" for i in range(8)]
    T, U, Z = "%8", "%9", "%10"
    A = [f"%{11 + i}" for i in range(8)]
    B = [f"%{19 + i}" for i in range(8)]
    op0, opc = ("v_sub_co_u32_e32", "v_subb_co_u32_e32") if sub else ("v_add_co_u32_e32", "v_addc_co_u32_e32")
    L = [f"v_mov_b32 {Z}, 0", f"{op0} {R[0]}, vcc, {A[0]}, {B[0]}"]
    for k in range(1, 8):
        L.append(f"{opc} {R[k]}, vcc, {A[k]}, {B[k]}, vcc")
    for _ in range(2):
        L.append(f"v_addc_co_u32_e32 {T}, vcc, 0, {Z}, vcc")       # t = carry / borrow (0 / 1)
        L.append(f"v_mul_u32_u24_e32 {U}, 977, {T}")
        L.append(f"{op0} {R[0]}, vcc, {R[0]}, {U}")
        L.append(f"{opc} {R[1]}, vcc, {R[1]}, {T}, vcc")
        for k in range(2, 8):
            L.append(f"{opc} {R[k]}, vcc, {R[k]}, {Z}, vcc")
    return L


def block(lines):
    return "        " + c_quote(lines, end_last=True)


def addsub_fn(name, sub, comment):
    body = block(addsub_lines(sub))
    outs = ", ".join(f'"=&v"(r.v[{i}])' for i in range(8)) + ', "=&v"(t), "=&v"(u), "=&v"(z)'
    ins = ", ".join(f'"v"(a.v[{i}])' for i in range(8)) + ", " + ", ".join(f'"v"(b.v[{i}])' for i in range(8))
    return "\n".join([
        f"// {comment}",
        f"__device__ __forceinline__ void {name}(fe &r, const fe &a, const fe &b) {{",
        "    u32 t, u, z;",
        "    asm volatile(",
        body,
        f"        : {outs}",
        f"        : {ins}",
        '        : "vcc");',
        "}",
    ])


def emit():
    """-> (header text, instructions of the product, of the square)"""
    A = list(range(0, 8))
    B = list(range(8, 16))
    T = list(range(16, 32))
    ACC = 32
    X = [36, 37, 38, 39]
    K = 40
    m = [f"v_mov_b32 v{K}, 977", f"v_mov_b32 v{ZERO}, 0"]
    product(m.append, A, B, T, ACC)
    reduce(m.append, T, A, X, K)
    s = [f"v_mov_b32 v{K}, 977", f"v_mov_b32 v{ZERO}, 0"]
    square(s.append, A, T, ACC)
    reduce(s.append, T, A, X, K)
    clob = clobbers(v=range(16, 42), flags=["vcc"])
    clob_sq = clobbers(v=range(8, 42), flags=["vcc"])
    out = [
        "// GENERATED by tools/gen_secp_asm.py — do not edit.",
        "// secp256k1 field product / square (p = 2^256 - 2^32 - 977) as gfx950 inline assembly; see the generator.",
        "#pragma once",
        "#include <stdint.h>",
        "typedef uint32_t u32;",
        "typedef u32 u32x8 __attribute__((ext_vector_type(8)));",
        "",
        "// a * b, weakly reduced (< 2^256, congruent mod p)",
        "__device__ __forceinline__ u32x8 secp_asm_mul(u32x8 a, u32x8 b) {",
        "    asm volatile(",
        block(m),
        '        : "+{v[0:7]}"(a), "+{v[8:15]}"(b)',
        "        :",
        f"        : {clob});",
        "    return a;",
        "}",
        addsub_fn("secp_asm_add", False, "r = a + b, weakly reduced (fe_add)"),
        addsub_fn("secp_asm_sub", True, "r = a - b mod p, weakly reduced (fe_sub)"),
        "// a^2, weakly reduced",
        "__device__ __forceinline__ u32x8 secp_asm_sqr(u32x8 a) {",
        "    asm volatile(",
        block(s),
        '        : "+{v[0:7]}"(a)',
        "        :",
        f"        : {clob_sq});",
        "    return a;",
        "}",
        "",
    ]
    return "\n".join(out), len(m), len(s)


def render():
    return emit()[0]


def main():
    text, n_mul, n_sqr = emit()
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote", OUT, n_mul, "/", n_sqr, "instructions")


if __name__ == "__main__":
    main()
