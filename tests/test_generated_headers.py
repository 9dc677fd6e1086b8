"""CPU check that the committed generated headers under lachain_amd/csrc are exactly what their generators under
tools/ produce: each generator's render() against the file(s) it writes, byte for byte.  Nothing is written.
"""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

GENERATORS = [("gen_asm", ["asm_routines.hpp"]),
              ("gen_tower_asm", ["asm_tower.hpp"]),
              ("gen_secp_asm", ["secp_asm.hpp"]),
              ("gen_constants", ["bls_constants.hpp", "bls_constants_host.h"]),
              ("gen_fpmul", ["fp_mul_gen.hpp"])]


@pytest.mark.parametrize("module,headers", GENERATORS, ids=[g for g, _ in GENERATORS])
def test_render_matches_committed_header(module, headers):
    texts = importlib.import_module(module).render()
    if isinstance(texts, str):
        texts = (texts,)
    assert len(texts) == len(headers)
    for name, text in zip(headers, texts):
        with open(os.path.join(ROOT, "lachain_amd", "csrc", name), "rb") as f:
            committed = f.read()
        assert text.encode("utf-8") == committed, f"{name} is not what tools/{module}.py renders"
