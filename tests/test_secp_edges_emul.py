"""The C++ path of the secp256k1 device code at the edge operands of tests/secp_cases.py: the routine switch of
lachain_amd/csrc/secp_debug.hpp compiled for the host by tools/emul/secp_recover_emul.cpp (emu_debug_secp_op; the C++
fe_mul / fe_sqr / fe_add / fe_sub of secp.hpp, not the assembly) against the model tests/pyref/secp.py, with the
comparisons of tests/secp_edges.py that tests/test_gpu_secp_edges.py runs on the device.  Three implementations must
agree with the integers: this one, the assembly simulated (tests/test_secp_asm_sim.py) and the assembly on the device.
TEST INFRASTRUCTURE."""
import ctypes

import pytest

import secp_edges as E
from test_secp_recover_emul import emu  # noqa: F401  (the fixture that builds and loads the emulation)


@pytest.fixture(scope="module")
def run(emu):  # noqa: F811
    fn = emu.emu_debug_secp_op
    fn.restype = None
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t,
                   ctypes.POINTER(ctypes.c_uint32)]

    def run_(op, a_items, b_items=None):
        n = len(a_items)
        a = (ctypes.c_uint32 * (E.IN_WORDS * n))(*[w for v in a_items for w in v])
        b = None if b_items is None else (ctypes.c_uint32 * (E.IN_WORDS * n))(*[w for v in b_items for w in v])
        out = (ctypes.c_uint32 * (E.OUT_WORDS * n))()
        fn(E.OPS[op], a, b, n, out)
        return [list(out[E.OUT_WORDS * i:E.OUT_WORDS * (i + 1)]) for i in range(n)]
    return run_


@pytest.mark.parametrize("op", ["mul", "add", "sub"])
def test_field_pairs(run, op):
    bad = E.check_field_pairs(run, op)
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("op", ["sqr", "neg", "dbl", "canon", "inv", "sqrt"])
def test_field_unary(run, op):
    bad = E.check_field_unary(run, op)
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
