"""The secp256k1 device code at the edge operands of tests/secp_cases.py, through lcb_debug_secp_op (k_secp_debug in
k_secp_recover.hip: one routine of secp.hpp / secp_comb.hpp / recode4 per lane), against the big-integer model
tests/pyref/secp.py.  On the device fe_mul / fe_sqr / fe_add / fe_sub are the generated assembly of secp_asm.hpp, whose
reduction tail and second correction pass no ladder over random keys enters; the catalogue does (its coverage is
asserted on the CPU by tests/test_secp_asm_sim.py).

The comparisons are those of tests/secp_edges.py, shared with the CPU emulation of the C++ path
(tests/test_secp_edges_emul.py); all are exact: integers mod p or n, or words.  mul / sqr / add / sub must also give
the very words the CPU simulation of the same instructions gives (tests/test_secp_asm_sim.py), so a disagreement can
be attributed to the simulator or to the hardware.  No launch is a whole number of waves, and every case runs on more
than one lane (secp_cases.spread)."""
import pytest

import secp_edges as E
from helpers import gpu_native
from test_secp_asm_sim import sim_table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    nat = gpu_native()
    assert nat.SECP_DEBUG_OPS == E.OPS and (nat.SECP_DEBUG_IN, nat.SECP_DEBUG_OUT) == (E.IN_WORDS, E.OUT_WORDS)
    return nat.debug_secp_op


@pytest.mark.parametrize("op", ["mul", "add", "sub"])
def test_field_pairs(run, op):
    bad = E.check_field_pairs(run, op, sim_table(op))
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("op", ["sqr", "neg", "dbl", "canon", "inv", "sqrt"])
def test_field_unary(run, op):
    bad = E.check_field_unary(run, op, sim_table("sqr") if op == "sqr" else None)
    assert not bad, (len(bad), bad[:8])


def test_predicates(run):
    bad = E.check_predicates(run)
    assert not bad, (len(bad), bad[:8])


def test_scalar_montgomery(run):
    bad = E.check_sc_mont_mul(run) + E.check_sc_mont_inv(run)
    assert not bad, (len(bad), bad[:8])


def test_split_and_digits(run):
    bad = E.check_split(run) + E.check_comb_recode(run)
    assert not bad, (len(bad), bad[:4])


def test_doubling(run):
    bad = E.check_jac_dbl(run)
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("affine", [True, False], ids=["jac_add_aff", "jac_add"])
def test_addition(run, affine):
    bad = E.check_jac_add(run, affine)
    assert not bad, (len(bad), bad[:8])


def test_hook_rejects_bad_arguments():
    import ctypes
    nat = gpu_native()
    lib = nat.lib()
    a = (ctypes.c_uint32 * E.IN_WORDS)()
    out = (ctypes.c_uint32 * E.OUT_WORDS)()
    assert lib.lcb_debug_secp_op(0, a, None, 1, out) == -1           # the product needs b
    assert lib.lcb_debug_secp_op(len(E.OPS), a, a, 1, out) == -1
    assert lib.lcb_debug_secp_op(-1, a, a, 1, out) == -1
    assert lib.lcb_debug_secp_op(1, a, None, 0, out) == -1
    assert lib.lcb_debug_secp_op(1, a, None, 65537, out) == -1
    assert lib.lcb_debug_secp_op(1, a, None, 1, out) == 0 and not any(out)
