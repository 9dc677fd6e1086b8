"""Register and scratch gate for the state-trie kernels of the built library (CPU test; no GPU needed): like every
Keccak kernel here, the trie's hashing kernels keep their sponge in registers, so they must not spill, must not use
scratch and use no LDS (tools/kernel_resources.py reads the code object's metadata).  The root builder's plumbing
kernels are held to the same."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "lachain_amd", "liblachain_bls.so")

HASHING = ["k_trie_flat", "k_trie_flat_listed", "k_trie_level", "k_trie_items", "k_trie_merge"]
PLUMBING = ["k_trie_sort_key", "k_trie_order", "k_trie_heads", "k_trie_roots_init", "k_trie_roots_write"]


@pytest.fixture(scope="module")
def resources():
    assert os.path.exists(SO), "liblachain_bls.so is not built"
    if not shutil.which("llvm-objdump", path="/opt/rocm/lib/llvm/bin"):
        pytest.skip("llvm-objdump not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    return kernel_resources(SO)


@pytest.mark.parametrize("kernel", HASHING + PLUMBING)
def test_no_spills_no_scratch_no_lds(resources, kernel):
    assert kernel in resources, kernel
    r = resources[kernel]
    assert r["vgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    assert r["group_segment_fixed_size"] == 0, r
