"""Register and scratch gate for the raw-transaction ingress kernels of the built library (CPU test; no GPU needed):
k_rawtx_decode and k_rawtx_long hold the decoded fields and a Keccak sponge in registers, so they must not spill, must
not use scratch and use no LDS (tools/kernel_resources.py reads the code object's metadata).  This gate is what decided
that decode and hashing stay one kernel."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "lachain_amd", "liblachain_bls.so")


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(SO):
        pytest.skip("liblachain_bls.so not built")
    if not shutil.which("llvm-objdump", path="/opt/rocm/lib/llvm/bin"):
        pytest.skip("llvm-objdump not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    return kernel_resources(SO)


@pytest.mark.parametrize("kernel", ["k_rawtx_decode", "k_rawtx_long", "k_rawtx_finish"])
def test_no_spills_no_scratch_no_lds(resources, kernel):
    assert kernel in resources, kernel
    r = resources[kernel]
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["group_segment_fixed_size"] == 0, r
