#!/usr/bin/env python3
"""tools/asm_core.py — the emitter core shared by the assembly generators gen_asm.py (asm_routines.hpp),
gen_tower_asm.py (asm_tower.hpp) and gen_secp_asm.py (secp_asm.hpp).  The generators define routines; what the
routines are written with lives here, once.

Conventions
  Stream.    An instruction stream is a plain list of strings, one instruction or `label:` per entry, without
             indentation.  Emitters return lists; callers concatenate them.
  Operands.  A register operand is an int (VGPR number, printed `v12`) or a string passed through as it is: an inline
             asm placeholder (`%7`, see ph()) or a literal (`0`).  A carry operand is an int (first SGPR of an aligned
             pair, printed `s[96:97]`, VOP3 / e64 forms) or a string: `vcc` (VOP2 / e32 forms) or a placeholder (e64).
  Limbs.     Field elements are 12 x 32-bit little-endian limbs in Montgomery form, R = 2^384; per MAC one
             `v_mad_u64_u32 acc, carry, x, y, acc` and one `v_addc_co_u32 hi, carry, 0, hi, carry`.
  Ring.      A column accumulator is an even-aligned 64-bit pair (v_mad_u64_u32 needs aligned pairs on gfx950) plus a
             carry word, rotated through four registers so the 32-bit shift between columns is one v_mov: ring().
             The first carry add of a column writes the fresh carry word (0 + 0 + carry), so nothing is zeroed.
  Calls.     Routines are reached with `s_swappc_b64` through a scratch SGPR pair (call_lines) and return with
             `s_setpc_b64` of their return pair.

Hazards (gfx940+)
  A VALU write of VCC or an SGPR pair needs two wait states before a VALU reads that register as carry-in or select
  mask, and a `v_accvgpr_write` needs two before a `v_accvgpr_read` of the same AGPR.  A wait state is one issued
  instruction; `s_nop n` counts n + 1.  Two formulations exist because they pad differently and the generated text
  is fixed: interleave_carry() schedules K carry chains of an inline asm block round-robin and pads per chain as it
  goes; hazard_fix() is a pass over a finished routine that tracks every SGPR pair and AGPR.
"""
import re

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
N = 12
PINV = (-pow(P, -1, 1 << 32)) % (1 << 32)


def limbs(x, n=N):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


PL = limbs(P)


# ------------------------------------------------------------------ operands
def vreg(x):
    return f"v{x}" if isinstance(x, int) else x


def sp(c):
    return f"s[{c}:{c + 1}]" if isinstance(c, int) else c


def _enc(c):
    return "e32" if c == "vcc" else "e64"


def ph(numbers):
    """inline asm placeholders %n for compiler-allocated operands"""
    return [f"%{i}" for i in numbers]


def ring(acc, k):
    """(low, high, carry word) of column k in the 4-register accumulator block at acc (even)"""
    return (acc, acc + 1, acc + 3) if k % 2 == 0 else (acc + 2, acc + 3, acc + 1)


# ------------------------------------------------------------------ moves and linear chains
def movs_const(r, vals):
    return [f"v_mov_b32 v{r[j]}, 0x{vals[j]:08x}" for j in range(len(r))]


def mov_regs(dst, src):
    return [f"v_mov_b32 v{d}, v{x}" for d, x in zip(dst, src)]


def _chain(first, link, r, x, y, c, carry_in):
    cs = sp(c)
    return [f"{link if j or carry_in else first}_{_enc(c)} {vreg(r[j])}, {cs}, {vreg(x[j])}, {vreg(y[j])}" +
            (f", {cs}" if j or carry_in else "") for j in range(len(r))]


def add_chain(r, x, y, c, carry_in=False):
    """r = x + y (+ the carry in c) over len(r) words; carry out in c"""
    return _chain("v_add_co_u32", "v_addc_co_u32", r, x, y, c, carry_in)


def sub_chain(r, x, y, c, carry_in=False):
    """r = x - y (- the borrow in c) over len(r) words; borrow out in c"""
    return _chain("v_sub_co_u32", "v_subb_co_u32", r, x, y, c, carry_in)


def select(r, x, y, c):
    """r = c ? y : x, word by word"""
    return [f"v_cndmask_b32_{_enc(c)} {vreg(r[j])}, {vreg(x[j])}, {vreg(y[j])}, {sp(c)}" for j in range(len(r))]


def condsub(r, kp, tmp, c, dst=None):
    """dst (default r) <- r - kp if r >= kp else r: tmp = r - kp; borrow ? r : tmp"""
    return sub_chain(tmp, r, kp, c) + select(r if dst is None else dst, tmp, r, c)


# ------------------------------------------------------------------ column products and Montgomery reduction
def comba(chains):
    """interleaved plain products T = a*b (24 words): chains = [dict(a, b, acc, out, c)], acc the ring block, c the
    chain's carry pair.  out[k] is written at the end of column k and may alias a[k-11] (k >= 11: a[k-11]'s last use
    is column k) — that is how the 24-word products fit in the registers the operands free."""
    s = []
    for ch in chains:
        s += [f"v_mov_b32 v{ch['acc']}, 0", f"v_mov_b32 v{ch['acc'] + 1}, 0"]
    for k in range(2 * N - 1):
        terms = [(i, k - i) for i in range(max(0, k - (N - 1)), min(k, N - 1) + 1)]
        for n_t, (i, j) in enumerate(terms):
            for ch in chains:
                L, H, C = ring(ch["acc"], k)
                s.append(f"v_mad_u64_u32 v[{L}:{H}], {sp(ch['c'])}, v{ch['a'][i]}, v{ch['b'][j]}, v[{L}:{H}]")
            for ch in chains:
                L, H, C = ring(ch["acc"], k)
                s.append(f"v_addc_co_u32_e64 v{C}, {sp(ch['c'])}, 0, {0 if n_t == 0 else 'v%d' % C}, {sp(ch['c'])}")
        for ch in chains:
            L, H, C = ring(ch["acc"], k)
            s.append(f"v_mov_b32 v{ch['out'][k]}, v{L}")
            if k == 2 * N - 2:
                s.append(f"v_mov_b32 v{ch['out'][2 * N - 1]}, v{H}")   # top word; the carry word is 0 (T < 2^768)
            else:
                s.append(f"v_mov_b32 v{ring(ch['acc'], k + 1)[0]}, v{H}")
    return s


def redc(chains, preg, s_pinv):
    """interleaved Montgomery reductions (U + m p) / 2^384 of 24-word U, product scanning: chains =
    [dict(u, m, acc, c[, out])], p in the VGPRs preg, -1/p mod 2^32 in SGPR s_pinv.  The result (< 2p for
    U < 9.84 p^2) lands in out, by default u[12:24] (u[k] is consumed at the start of column k)."""
    s = []
    for ch in chains:
        s += [f"v_mov_b32 v{ch['acc']}, 0", f"v_mov_b32 v{ch['acc'] + 1}, 0"]
    for k in range(2 * N):
        for ch in chains:                       # acc += U_k (the column's carry word starts fresh here)
            L, H, C = ring(ch["acc"], k)
            s.append(f"v_add_co_u32_e64 v{L}, {sp(ch['c'])}, v{L}, v{ch['u'][k]}")
        for ch in chains:
            L, H, C = ring(ch["acc"], k)
            s.append(f"v_addc_co_u32_e64 v{H}, {sp(ch['c'])}, v{H}, 0, {sp(ch['c'])}")
        for ch in chains:
            L, H, C = ring(ch["acc"], k)
            s.append(f"v_addc_co_u32_e64 v{C}, {sp(ch['c'])}, 0, 0, {sp(ch['c'])}")
        terms = [(i, k - i) for i in range(max(0, k - (N - 1)), min(k - 1, N - 1) + 1)]
        if k < N:
            terms.append((k, 0))
        for i, j in terms:
            if (i, j) == (k, 0):                # m_k = acc * (-1/p) mod 2^32, then acc += m_k p_0
                for ch in chains:
                    s.append(f"v_mul_lo_u32 v{ch['m'][k]}, v{ring(ch['acc'], k)[0]}, s{s_pinv}")
            for ch in chains:
                L, H, C = ring(ch["acc"], k)
                s.append(f"v_mad_u64_u32 v[{L}:{H}], {sp(ch['c'])}, v{ch['m'][i]}, v{preg[j]}, v[{L}:{H}]")
            for ch in chains:
                L, H, C = ring(ch["acc"], k)
                s.append(f"v_addc_co_u32_e64 v{C}, {sp(ch['c'])}, 0, v{C}, {sp(ch['c'])}")
        for ch in chains:
            L, H, C = ring(ch["acc"], k)
            if k >= N:
                s.append(f"v_mov_b32 v{ch.get('out', ch['u'][N:])[k - N]}, v{L}")
            if k < 2 * N - 1:
                s.append(f"v_mov_b32 v{ring(ch['acc'], k + 1)[0]}, v{H}")
    return s


# ------------------------------------------------------------------ interleaving and hazard padding
def merge(streams):
    """round-robin interleave of independent instruction lists"""
    out, idx = [], [0] * len(streams)
    while any(idx[k] < len(streams[k]) for k in range(len(streams))):
        for k in range(len(streams)):
            if idx[k] < len(streams[k]):
                out.append(streams[k][idx[k]])
                idx[k] += 1
    return out


_CARRY_OPS = ("v_add_co_u32", "v_addc_co_u32", "v_sub_co_u32", "v_subb_co_u32")


def interleave_carry(seqs, sops):
    """Round-robin over the K carry chains of one inline asm block (chain 0 carries in VCC, chain c > 0 in the SGPR
    pair operand sops[c-1], written `%S` in its lines), padding with s_nop where a chain's carry read would come
    < 2 wait states after its carry write (chains of unequal length, or one chain alone, get `s_nop 1` links)."""
    out, last_w = [], [None] * len(seqs)
    idx = [0] * len(seqs)
    c = 0
    while any(idx[k] < len(seqs[k]) for k in range(len(seqs))):
        while idx[c] >= len(seqs[c]):
            c = (c + 1) % len(seqs)
        line = seqs[c][idx[c]]
        idx[c] += 1
        if line.endswith((", vcc", ", %S")) and last_w[c] is not None:
            gap = len(out) - last_w[c] - 1          # instructions issued since the chain's carry write
            if gap < 2:
                out.append(f"s_nop {1 - gap}")
        if line.startswith(_CARRY_OPS):
            last_w[c] = len(out)
        out.append(line if c == 0 else line.replace("%S", sops[c - 1]))
        c = (c + 1) % len(seqs)
    return out


_SREAD_E64 = ("v_addc_co_u32_e64", "v_subb_co_u32_e64", "v_cndmask_b32_e64")
_SWRITE = ("v_mad_u64_u32", "v_add_co_u32_e64", "v_addc_co_u32_e64", "v_sub_co_u32_e64", "v_subb_co_u32_e64")


def _sgpr_pairs(txt):
    return [(int(a), int(b)) for a, b in re.findall(r"s\[(\d+):(\d+)\]", txt)]


def hazard_fix(lines):
    """insert s_nop into a finished routine so that (1) a VALU read of an SGPR pair comes >= 2 wait states after a
    VALU wrote it and (2) an AGPR read comes >= 2 wait states after its write"""
    out = []
    last_sw = {}     # sgpr pair -> position (in wait-state units) of the last VALU write
    last_aw = {}     # agpr -> position of last write
    pos = 0
    for ln in lines:
        mn = ln.split()[0] if ln.strip() else ""
        ops = ln[len(mn):].split(",")
        need = 0
        if mn in _SREAD_E64:
            for pr in _sgpr_pairs(ops[-1]):
                if pr in last_sw:
                    need = max(need, 2 - (pos - last_sw[pr] - 1))
        if mn == "v_accvgpr_read_b32":
            a = int(re.search(r"a(\d+)", ops[1]).group(1))
            if a in last_aw:
                need = max(need, 2 - (pos - last_aw[a] - 1))
        if need > 0:
            out.append(f"s_nop {need - 1}")
            pos += need
        out.append(ln)
        if mn in _SWRITE:
            for pr in _sgpr_pairs(ops[1]):
                last_sw[pr] = pos
        if mn == "v_accvgpr_write_b32":
            last_aw[int(re.search(r"a(\d+)", ops[0]).group(1))] = pos
        pos += int(ln.split()[1]) + 1 if mn == "s_nop" else 1
    return out


# ------------------------------------------------------------------ calls, C quoting, headers
def call_lines(label, scratch, ret=30):
    """call `label` through the scratch pair s[scratch:scratch+1]; the return address goes to s[ret:ret+1].  The
    two SALU adds write SCC."""
    return [f"s_getpc_b64 s[{scratch}:{scratch + 1}]",
            f"s_add_u32 s{scratch}, s{scratch}, {label}@rel32@lo+4",
            f"s_addc_u32 s{scratch + 1}, s{scratch + 1}, {label}@rel32@hi+12",
            f"s_swappc_b64 s[{ret}:{ret + 1}], s[{scratch}:{scratch + 1}]"]


def c_quote(lines, end_last=False):
    """the lines as adjacent C string pieces for an asm statement, one per source line (`\\n\\t` after each but,
    unless end_last, the last)"""
    q = [f'"{ln}\\n\\t"' for ln in lines]
    if not end_last:
        q[-1] = f'"{lines[-1]}"'
    return "\n        ".join(q)


def clobbers(v=(), a=(), s=(), flags=()):
    """an asm clobber list: VGPR, AGPR and SGPR numbers, then flags such as scc, vcc"""
    return ", ".join([f'"v{i}"' for i in v] + [f'"a{i}"' for i in a] + [f'"s{i}"' for i in s] +
                     [f'"{x}"' for x in flags])


def library_header(generator, about, typedefs, stem, routines):
    """the head of a routine-library header: banner, includes, typedefs, the `<stem>_LIBRARY(tag)` kernel macro (one
    per translation unit; never launched, it only hosts the routines' code) and the routines' text, escaped, as the
    `<stem>_LIBRARY_TEXT` macro.  routines: instruction streams, each starting with its label."""
    lib = "\n".join("  .p2align 8\n" + "\n".join(ln if ln.endswith(":") else "  " + ln for ln in r) for r in routines)
    esc = lib.replace("\\", "\\\\").replace('"', '\\"')
    return (f"// GENERATED by tools/{generator} — do not edit.\n// {about}\n"
            "#pragma once\n#include <hip/hip_runtime.h>\n#include <stdint.h>\n\n" + typedefs + "\n"
            f"#define {stem}_LIBRARY(tag) \\\n"
            f'extern "C" __global__ void __launch_bounds__(64) {stem.lower()}_library_##tag() {{ \\\n'
            f"    asm volatile({stem}_LIBRARY_TEXT); \\\n}}\n\n"
            f'#define {stem}_LIBRARY_TEXT \\\n    "  s_endpgm\\n" \\\n' +
            "".join(f'    "{ln}\\n" \\\n' for ln in esc.split("\n")) + '    ""\n\n')
