#!/usr/bin/env python3
"""tools/asm_sim.py — single-lane interpreter for the generated gfx950 routine libraries (asm_routines.hpp,
asm_tower.hpp) and for the inline blocks of secp_asm.hpp (tests/test_secp_asm_sim.py: VOP2 forms with their carries
in VCC).

Executes a library's text (the subset of VOP3 / SOP / global / LDS instructions the generators emit) for one lane
with Python integers: registers, SCC, labels, branches, calls with a return stack, global memory (a dict of 32-bit
words keyed by byte address) and LDS.  The generators' arithmetic and their register contract (which registers a
routine may write) are checked with it on the CPU by tests/test_asm_routines.py and tests/test_asm_tower.py.
"""
import functools
import os
import re

M32 = (1 << 32) - 1
HERE = os.path.dirname(os.path.abspath(__file__))
HPP = os.path.join(HERE, "..", "lachain_amd", "csrc", "asm_routines.hpp")
TOWER_HPP = os.path.join(HERE, "..", "lachain_amd", "csrc", "asm_tower.hpp")


def load_program(path=TOWER_HPP, macro="LCB_ASM_TOWER_LIBRARY_TEXT"):
    """-> (instructions [(mnemonic, [operands])], {label: index}) parsed from the library text macro.  The
    `.p2align` in front of every routine stays in the stream as an instruction that raises: a routine that runs off
    its end stops there instead of sliding into the next one."""
    src = open(path).read()
    body = src[src.index("#define " + macro):]
    body = body[:body.index('    ""\n')]
    prog, labels = [], {}
    for raw in re.findall(r'"(.*?)\\n"', body):
        line = raw.strip()
        if not line or (line.startswith(".") and not line.startswith(".p2align")):
            continue
        if line.endswith(":"):
            labels[line[:-1]] = len(prog)
            continue
        mn, _, rest = line.partition(" ")
        ops = [o.strip() for o in rest.split(",")] if rest else []
        prog.append((mn, ops))
    return prog, labels


def load_library(path=HPP, macro="LCB_ASM_LIBRARY_TEXT"):
    return load_program(path, macro)


@functools.lru_cache(maxsize=None)
def _regs(op):
    """'v12' -> ('v', [12]); 'v[36:37]' -> ('v', [36, 37]); 's[90:91]' -> ('s', [90, 91])"""
    m = re.fullmatch(r"([vsa])(\d+)", op)
    if m:
        return m.group(1), [int(m.group(2))]
    m = re.fullmatch(r"([vsa])\[(\d+):(\d+)\]", op)
    if m:
        lo, hi = int(m.group(2)), int(m.group(3))
        return m.group(1), list(range(lo, hi + 1))
    return None, None


class ProgLane:
    def __init__(self):
        self.v, self.s, self.a = {}, {}, {}
        self.written_v, self.written_s, self.written_a = set(), set(), set()
        self.counts = {}
        self.mem, self.lds, self.scc = {}, {}, 0
        self.vcc, self.vcc_written = None, False      # this lane's bit of VCC (the inline blocks of secp_asm.hpp)

    def get(self, op):
        if op == "vcc":
            if self.vcc is None:
                raise KeyError("read of undefined vcc")
            return self.vcc
        kind, rr = _regs(op)
        if kind is None:
            return int(op, 0) & M32
        f = {"v": self.v, "s": self.s, "a": self.a}[kind]
        val = 0
        for k, r in enumerate(rr):
            if r not in f:
                raise KeyError(f"read of undefined {kind}{r}")
            val |= f[r] << (32 * k)
        return val

    def getmask(self, op):  # a lane-mask SGPR pair: this lane's bit
        return self.get(op) & 1

    def put(self, op, val):
        if op == "vcc":
            self.vcc, self.vcc_written = val & 1, True
            return
        kind, rr = _regs(op)
        f, w = {"v": (self.v, self.written_v), "s": (self.s, self.written_s), "a": (self.a, self.written_a)}[kind]
        if kind == "v" and len(rr) == 2 and rr[0] % 2:
            raise ValueError(f"misaligned 64-bit VGPR pair {op}")
        for k, r in enumerate(rr):
            f[r] = (val >> (32 * k)) & M32
            w.add(r)

    def load(self, addr, n):
        out = 0
        for k in range(n):
            a = addr + 4 * k
            if a not in self.mem:
                raise KeyError(f"load of unwritten memory 0x{a:x}")
            out |= self.mem[a] << (32 * k)
        return out

    def store(self, addr, val, n):
        for k in range(n):
            self.mem[addr + 4 * k] = (val >> (32 * k)) & M32


def _split_off(op):
    """'v[72:75] offset:1024' -> ('v[72:75]', 1024)"""
    m = re.fullmatch(r"(\S+)\s+offset:(\d+)", op)
    return (m.group(1), int(m.group(2))) if m else (op, 0)


def _vop2(mn, ops):
    """the VOP2 (e32) encodings take their carries in VCC only and a VGPR as the second source"""
    if mn.endswith("_e32") and "_co_" in mn:
        if ops[1] != "vcc" or (len(ops) > 4 and ops[4] != "vcc"):
            raise ValueError(f"{mn}: the e32 form carries through vcc only: {ops}")
    if mn.endswith("_e32") and _regs(ops[-2 if len(ops) > 4 else -1])[0] != "v":
        raise ValueError(f"{mn}: the second source of an e32 form is a VGPR: {ops}")


def run_program(prog, labels, entry, lane, max_steps=50_000_000):
    """run from label `entry` until the `s_setpc_b64` that returns from it"""
    pc, stack, target = labels[entry], [], None
    g = lane.get
    for _ in range(max_steps):
        mn, ops = prog[pc]
        pc += 1
        lane.counts[mn] = lane.counts.get(mn, 0) + 1
        if mn == "v_mad_u64_u32":
            r = g(ops[2]) * g(ops[3]) + g(ops[4])
            lane.put(ops[0], r & ((1 << 64) - 1)); lane.put(ops[1], r >> 64)
        elif mn in ("v_add_co_u32_e64", "v_addc_co_u32_e64"):
            r = g(ops[2]) + g(ops[3]) + (lane.getmask(ops[4]) if mn == "v_addc_co_u32_e64" else 0)
            lane.put(ops[0], r & M32); lane.put(ops[1], r >> 32)
        elif mn in ("v_sub_co_u32_e64", "v_subb_co_u32_e64"):
            r = g(ops[2]) - g(ops[3]) - (lane.getmask(ops[4]) if mn == "v_subb_co_u32_e64" else 0)
            lane.put(ops[0], r & M32); lane.put(ops[1], 1 if r < 0 else 0)
        elif mn in ("v_add_co_u32_e32", "v_addc_co_u32_e32"):       # VOP2: carry out (and in) through VCC
            _vop2(mn, ops)
            r = g(ops[2]) + g(ops[3]) + (lane.getmask(ops[4]) if mn == "v_addc_co_u32_e32" else 0)
            lane.put(ops[0], r & M32); lane.put(ops[1], r >> 32)
        elif mn in ("v_sub_co_u32_e32", "v_subb_co_u32_e32"):
            _vop2(mn, ops)
            r = g(ops[2]) - g(ops[3]) - (lane.getmask(ops[4]) if mn == "v_subb_co_u32_e32" else 0)
            lane.put(ops[0], r & M32); lane.put(ops[1], 1 if r < 0 else 0)
        elif mn == "v_mul_hi_u32":
            lane.put(ops[0], (g(ops[1]) * g(ops[2])) >> 32)
        elif mn == "v_mad_u32_u24":                                  # 24-bit sources, 32-bit sum
            lane.put(ops[0], ((g(ops[1]) & 0xFFFFFF) * (g(ops[2]) & 0xFFFFFF) + g(ops[3])) & M32)
        elif mn in ("v_mul_u32_u24", "v_mul_u32_u24_e32"):
            if mn.endswith("_e32"):
                _vop2(mn, ops)
            lane.put(ops[0], ((g(ops[1]) & 0xFFFFFF) * (g(ops[2]) & 0xFFFFFF)) & M32)
        elif mn == "v_cndmask_b32_e64":
            lane.put(ops[0], g(ops[2]) if lane.getmask(ops[3]) else g(ops[1]))
        elif mn == "v_mul_lo_u32":
            lane.put(ops[0], (g(ops[1]) * g(ops[2])) & M32)
        elif mn == "v_alignbit_b32":
            lane.put(ops[0], (((g(ops[1]) << 32) | g(ops[2])) >> (g(ops[3]) & 31)) & M32)
        elif mn == "v_lshlrev_b32":
            lane.put(ops[0], (g(ops[2]) << (g(ops[1]) & 31)) & M32)
        elif mn == "s_and_b32":
            r = g(ops[1]) & g(ops[2])
            lane.put(ops[0], r); lane.scc = 1 if r else 0
        elif mn == "s_lshr_b32":
            r = g(ops[1]) >> (g(ops[2]) & 31)
            lane.put(ops[0], r); lane.scc = 1 if r else 0
        elif mn in ("v_mov_b32", "s_mov_b32", "s_mov_b64", "v_accvgpr_read_b32", "v_accvgpr_write_b32"):
            lane.put(ops[0], g(ops[1]))
        elif mn == "s_add_u32":
            if "@" in ops[2]:
                target = ops[2].split("@")[0]
            else:
                r = g(ops[1]) + g(ops[2])
                lane.put(ops[0], r & M32); lane.scc = r >> 32
        elif mn == "s_addc_u32":
            if "@" not in ops[2]:
                r = g(ops[1]) + g(ops[2]) + lane.scc
                lane.put(ops[0], r & M32); lane.scc = r >> 32
        elif mn == "s_sub_u32":
            r = g(ops[1]) - g(ops[2])
            lane.put(ops[0], r & M32); lane.scc = 1 if r < 0 else 0
        elif mn == "s_mul_i32":
            lane.put(ops[0], (g(ops[1]) * g(ops[2])) & M32)
        elif mn == "s_cmp_eq_u32":
            lane.scc = 1 if g(ops[0]) == g(ops[1]) else 0
        elif mn == "s_cmp_lg_u32":
            lane.scc = 1 if g(ops[0]) != g(ops[1]) else 0
        elif mn == "s_branch":
            pc = labels[ops[0]]
        elif mn in ("s_cbranch_scc1", "s_cbranch_scc0"):
            if lane.scc == (1 if mn.endswith("1") else 0):
                pc = labels[ops[0]]
        elif mn in ("s_nop", "s_waitcnt", "s_getpc_b64"):
            pass
        elif mn == "s_swappc_b64":
            stack.append(pc)
            pc = labels[target]
        elif mn == "s_setpc_b64":
            if not stack:
                return
            pc = stack.pop()
        elif mn in ("global_load_dwordx4", "global_store_dwordx4"):
            last, off = _split_off(ops[2])
            if last == "off":                       # 64-bit VGPR address
                addr = g(ops[1] if mn == "global_load_dwordx4" else ops[0]) + off
            else:                                   # SGPR base + 32-bit VGPR offset
                addr = g(last) + g(ops[1] if mn == "global_load_dwordx4" else ops[0]) + off
            if mn == "global_load_dwordx4":
                lane.put(ops[0], lane.load(addr, 4))
            else:
                lane.store(addr, g(ops[1]), 4)
        elif mn in ("ds_write_b128", "ds_read_b128"):
            if mn == "ds_write_b128":
                src, off = _split_off(ops[1])
                a = g(ops[0]) + off
                for k in range(4):
                    lane.lds[a + 4 * k] = (g(src) >> (32 * k)) & M32
            else:
                addr, off = _split_off(ops[1])
                a = g(addr) + off
                lane.put(ops[0], sum(lane.lds[a + 4 * k] << (32 * k) for k in range(4)))
        elif mn == ".p2align":
            raise RuntimeError(f"{entry}: a routine fell off its end without s_setpc_b64")
        else:
            raise NotImplementedError(mn)
    raise RuntimeError("step limit")


def call(lib, label, inputs, agprs=None):
    """run routine `label` of lib = (prog, labels) on a fresh lane.  inputs: {first VGPR: 12-limb integer}; agprs:
    {first AGPR: 12-limb integer}.  Returns (lane, reader(first VGPR) -> integer)."""
    lane = ProgLane()
    for f, vals in ((lane.v, inputs), (lane.a, agprs or {})):
        for base, val in vals.items():
            for j in range(12):
                f[base + j] = (val >> (32 * j)) & M32
    run_program(*lib, label, lane)

    def read(base):
        return sum(lane.v[base + j] << (32 * j) for j in range(12))
    return lane, read
