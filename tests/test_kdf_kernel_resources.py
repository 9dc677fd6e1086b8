"""Register and scratch gate for the TPKE keystream kernel of the built library (CPU test; no GPU needed): like every
Keccak kernel here, k_kdf_xor keeps its sponge in registers, so it must not spill, must not use scratch and uses no LDS
(tools/kernel_resources.py reads the code object's metadata)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "lachain_amd", "liblachain_bls.so")

KERNELS = ["k_kdf_xor", "k_tpke_ids_to_x"]


@pytest.fixture(scope="module")
def resources():
    assert os.path.exists(SO), "liblachain_bls.so is not built"
    if not shutil.which("llvm-objdump", path="/opt/rocm/lib/llvm/bin"):
        pytest.skip("llvm-objdump not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    return kernel_resources(SO)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch_no_lds(resources, kernel):
    assert kernel in resources, kernel
    r = resources[kernel]
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["group_segment_fixed_size"] == 0, r
