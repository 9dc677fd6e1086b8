"""The committed secp256k1 field assembly (lachain_amd/csrc/secp_asm.hpp) run on the CPU by tools/asm_sim.py, at the
edge operands of tests/secp_cases.py, against Python integers.  TEST INFRASTRUCTURE.

The four `asm volatile` blocks are parsed out of the header's text (tests/test_generated_headers.py ties that text to
tools/gen_secp_asm.py), their operands bound the way the constraints bind them (v[0:7] / v[8:15] for the product and
the square, %0..%26 for the sum and the difference) and every instruction interpreted for one lane.  Checked:
  * the catalogue itself: every class of the reduction's tail and of the correction passes has its members
    (secp_cases.coverage, from the written definition of the reduction), so the rare branches are really entered;
  * every pair (mul / add / sub) and every operand (sqr) gives a value below 2^256 congruent to the integer result;
  * every register a block writes is one of its outputs or clobbers, VCC included, and the add / sub outputs are
    early-clobber (they are written while inputs are still to be read);
  * the model (tests/pyref/secp.py) agrees with the oracle.
tests/test_gpu_secp_edges.py compares the device's words with the words computed here.
"""
import functools
import os
import re
import sys

import pytest

import secp_cases as C
from pyref import secp as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_sim  # noqa: E402

HEADER = os.path.join(ROOT, "lachain_amd", "csrc", "secp_asm.hpp")
P = S.P


class AsmBlock:
    """one `asm volatile` block: instructions [(mnemonic, [operands])], output / input constraints [(constraint,
    expression)], clobbers [name]"""

    def __init__(self, name, body):
        self.name = name
        lines = re.findall(r'"([^"]*?)\\n\\t"', body)
        tail = body[body.rindex('\\n\\t"') + 5:]
        parts = re.split(r"\n\s*:", tail)
        assert len(parts) == 4 and lines, name
        self.outputs = re.findall(r'"([^"]+)"\(([^()]*(?:\[[^\]]*\])?)\)', parts[1])
        self.inputs = re.findall(r'"([^"]+)"\(([^()]*(?:\[[^\]]*\])?)\)', parts[2])
        self.clobbers = re.findall(r'"([^"]+)"', parts[3])
        self.text = lines

    def program(self, bind=None):
        """the instruction list with %k replaced by bind[k]"""
        prog = []
        for line in self.text:
            if bind is not None:
                line = re.sub(r"%(\d+)", lambda m: bind[int(m.group(1))], line)
            mn, _, rest = line.partition(" ")
            prog.append((mn, [o.strip() for o in rest.split(",")]))
        return prog + [("s_setpc_b64", [])]


@functools.lru_cache(maxsize=None)
def blocks():
    """{function name: AsmBlock} of the committed header"""
    src = open(HEADER).read()
    out = {}
    for chunk in src.split("__device__ __forceinline__")[1:]:
        name = re.search(r"(secp_asm_\w+)\(", chunk).group(1)
        body = chunk[chunk.index("asm volatile(") + len("asm volatile("):]
        out[name] = AsmBlock(name, body[:body.index(");\n")])
    assert sorted(out) == ["secp_asm_add", "secp_asm_mul", "secp_asm_sqr", "secp_asm_sub"]
    return out


def pinned(block):
    """[(first, last)] of the v[lo:hi] ranges the constraints of a product / square block pin"""
    return [tuple(int(x) for x in re.fullmatch(r"\+\{v\[(\d+):(\d+)\]\}", c).groups()) for c, _ in block.outputs]


@functools.lru_cache(maxsize=None)
def _mul_program(name):
    return blocks()[name].program()


ADDSUB_BASE = 50                     # %k -> v(50 + k): any 27 distinct registers do, the constraints are plain "v"


@functools.lru_cache(maxsize=None)
def _addsub_program(name):
    b = blocks()[name]
    assert len(b.outputs) == 11 and len(b.inputs) == 16
    return b.program([f"v{ADDSUB_BASE + k}" for k in range(27)])


def run_block(name, a, b=None):
    """-> (result, lane) of secp_asm_<name> on 256-bit a (and b)"""
    lane = asm_sim.ProgLane()
    if name in ("mul", "sqr"):
        prog = _mul_program("secp_asm_" + name)
        ranges = pinned(blocks()["secp_asm_" + name])
        for (lo, _), val in zip(ranges, (a, b)):
            for k, w in enumerate(C.words(val)):
                lane.v[lo + k] = w
        out = ranges[0][0]
    else:
        prog = _addsub_program("secp_asm_" + name)
        for k, w in enumerate(C.words(a) + C.words(b)):
            lane.v[ADDSUB_BASE + 11 + k] = w
        out = ADDSUB_BASE
    asm_sim.run_program(prog, {"entry": 0}, "entry", lane)
    return C.from_words([lane.v[out + k] for k in range(8)]), lane


@functools.lru_cache(maxsize=None)
def sim_table(name):
    """the simulated result of every catalogue pair (mul / add / sub: {(i, j): value}) or operand (sqr: {i: value});
    shared by the tests here and by tests/test_gpu_secp_edges.py"""
    if name == "sqr":
        return {i: run_block("sqr", a)[0] for i, (_, a) in enumerate(C.FIELD)}
    return {(i, j): run_block(name, C.FIELD[i][1], C.FIELD[j][1])[0] for i, j in C.FIELD_PAIRS}


# ------------------------------------------------------------------------------------------------ the catalogue
def test_catalogue_reaches_every_branch():
    cov = C.coverage()
    assert len(C.FIELD) >= 88 and len(C.FIELD_PAIRS) == len(C.FIELD) ** 2
    for cls, floor in C.COVERAGE_FLOOR.items():
        assert floor >= 4 and len(cov.get(cls, ())) >= floor, (cls, len(cov.get(cls, ())), floor)
    lo, hi = C.edge_xs()
    assert lo == [1, 2, 3, 4, 6, 8] and [P - x for x in hi] == [3, 4, 10, 12, 13, 16]
    assert {c for c, _, _ in C.jac_pairs()} >= {
        "P+P same form", "P+P different Z", "P-P same Z", "P-P different Z", "inf+Q", "P+inf", "inf+inf", "generic",
        "x equal mod p only: P+P", "x equal mod p only: P-P", "2P+P", "kG+(k+1)G"}
    for cls, a, b in C.jac_pairs() + C.aff_pairs():
        for j in (a, b):                                     # every operand is the point its name says
            assert j.inf == (j.aff is None) and (j.inf or S.from_jacobian(j.x, j.y, j.z) == j.aff), (cls, j.name)
    names = [n for n, _ in C.scalars()]
    for must in ("0", "n-1", "(n+1)/2", "lambda", "lambda+1", "n-lambda", "2^129-1", "a1", "-b1-1", "a2+1"):
        assert must in names, must
    for items in (C.FIELD_PAIRS, C.jac_pairs(), C.aff_pairs(), C.jac_operands(), C.scalars(), C.scalar_pairs(),
                  list(range(5)), list(range(7)), list(range(64)), list(range(128))):
        idx = C.spread(items)
        assert len(idx) % 64 != 0 and set(idx) == set(range(len(items)))
        lanes = {}
        for pos, i in enumerate(idx):
            lanes.setdefault(i, set()).add(pos % 64)
        assert all(len(v) > 1 for v in lanes.values())


def test_model_matches_the_oracle():
    import oracle as o
    lam, _ = C.glv()
    for k in (1, 2, 3, 7, S.N - 1, S.N - 2, (S.N + 1) // 2, lam, lam * lam % S.N, 1 << 128, (1 << 128) - 1, 0xDEADBEEF):
        pt = S.pt_mul(k, S.G)
        c33, u65 = o.ecdsa_pubkey(k.to_bytes(32, "big"))
        assert S.compress(pt) == c33 and S.uncompressed(pt) == u65, hex(k)
        assert S.on_curve(pt) and S.pt_add(pt, S.pt_neg(pt)) is None
    assert S.pt_mul(S.N, S.G) is None and S.pt_add(None, S.G) == S.G


# ------------------------------------------------------------------------------------------------ the arithmetic
@pytest.mark.parametrize("name", ["mul", "add", "sub"])
def test_every_pair(name):
    table = sim_table(name)
    want = {"mul": lambda a, b: a * b, "add": lambda a, b: a + b, "sub": lambda a, b: a - b}[name]
    bad = []
    for (i, j), got in table.items():
        (na, a), (nb, b) = C.FIELD[i], C.FIELD[j]
        if not (0 <= got < C.W and got % P == want(a, b) % P):
            bad.append((na, nb, hex(got)))
    assert not bad, (len(bad), bad[:8])


def test_every_square():
    bad = [(na, hex(got)) for (na, a), got in zip(C.FIELD, sim_table("sqr").values())
           if not (0 <= got < C.W and got % P == a * a % P)]
    assert not bad, bad[:8]


def test_sum_and_difference_are_the_written_corrections():
    """the words, not only the residue: + C per carry and - C per borrow, as secp.hpp's C++ fe_add / fe_sub"""
    add, sub = sim_table("add"), sim_table("sub")
    for i, j in C.FIELD_PAIRS:
        a, b = C.FIELD[i][1], C.FIELD[j][1]
        assert add[i, j] == C.add_class(a, b)[1] and sub[i, j] == C.sub_class(a, b)[1], (C.FIELD[i][0], C.FIELD[j][0])
    for i, j in C.FIELD_PAIRS[::97]:
        assert sim_table("mul")[i, j] == C.product_class(C.FIELD[i][1], C.FIELD[j][1]).result


# ------------------------------------------------------------------------------------------------ the register contract
def test_writes_stay_within_outputs_and_clobbers():
    hi = C.W - 1
    for name in ("mul", "sqr"):
        b = blocks()["secp_asm_" + name]
        allowed = {r for lo, up in pinned(b) for r in range(lo, up + 1)}
        allowed |= {int(c[1:]) for c in b.clobbers if re.fullmatch(r"v\d+", c)}
        for a, c in ((hi, hi), (P - 2, C.W - (1 << 33)), (0, 0)):
            lane = run_block(name, a, c)[1]
            assert lane.written_v <= allowed, (name, sorted(lane.written_v - allowed))
            assert lane.vcc_written and "vcc" in b.clobbers
            assert not lane.written_s and not lane.written_a
        assert pinned(b)[0] == (0, 7) and (name == "sqr" or pinned(b)[1] == (8, 15))
    for name in ("add", "sub"):
        b = blocks()["secp_asm_" + name]
        outs = {ADDSUB_BASE + k for k in range(len(b.outputs))}
        for a, c in ((hi, hi), (0, hi), (C.C - 1, C.C), (0, 0)):
            lane = run_block(name, a, c)[1]
            assert lane.written_v <= outs, (name, sorted(lane.written_v - outs))
            assert lane.vcc_written and b.clobbers == ["vcc"]
        # the outputs are written before the last input is read: each must be early-clobber, the inputs plain VGPRs
        assert [c for c, _ in b.outputs] == ["=&v"] * 11
        assert [c for c, _ in b.inputs] == ["v"] * 16
        assert [e for _, e in b.outputs[:8]] == [f"r.v[{k}]" for k in range(8)]
        assert [e for _, e in b.inputs] == [f"a.v[{k}]" for k in range(8)] + [f"b.v[{k}]" for k in range(8)]


def test_simulator_keeps_its_habits():
    """an undefined read raises, VCC included; a misaligned 64-bit pair raises; an e32 form with a carry outside VCC
    or a constant second source raises"""
    def run(lines, v=None):
        lane = asm_sim.ProgLane()
        lane.v.update(v or {})
        prog = [(ln.partition(" ")[0], [o.strip() for o in ln.partition(" ")[2].split(",")]) for ln in lines]
        asm_sim.run_program(prog + [("s_setpc_b64", [])], {"e": 0}, "e", lane)
        return lane
    with pytest.raises(KeyError):
        run(["v_addc_co_u32_e32 v1, vcc, 0, v0, vcc"], {0: 1})
    with pytest.raises(KeyError):
        run(["v_add_co_u32_e32 v1, vcc, v0, v2"], {0: 1})
    with pytest.raises(ValueError):
        run(["v_mad_u64_u32 v[3:4], vcc, v0, v0, v[3:4]"], {0: 1, 3: 0, 4: 0})
    with pytest.raises(ValueError):
        run(["v_add_co_u32_e32 v1, s[2:3], v0, v0"], {0: 1})
    with pytest.raises(ValueError):
        run(["v_add_co_u32_e32 v1, vcc, v0, 5"], {0: 1})
    lane = run(["v_sub_co_u32_e32 v1, vcc, v0, v2", "v_subb_co_u32_e32 v3, vcc, v0, v0, vcc", "v_mul_hi_u32 v4, v2, v2",
                "v_mad_u32_u24 v5, v2, v2, v0", "v_mul_u32_u24_e32 v6, 977, v2"], {0: 1, 2: 0xFF000003})
    assert [lane.v[k] for k in (1, 3, 4, 5, 6)] == [(1 - 0xFF000003) % 2 ** 32, 0xFFFFFFFF, 0xFF000003 ** 2 >> 32, 10, 977 * 3]
