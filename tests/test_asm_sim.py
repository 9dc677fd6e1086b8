"""CPU check of what tools/asm_sim.py guarantees the routine tests: a read of an undefined register raises, a
misaligned 64-bit VGPR pair raises, written registers are tracked, and a routine that runs off its end raises instead
of sliding into the next one.  A four-routine library text stands in for a generated header.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_sim  # noqa: E402

ROUTINES = [["r_ok:", "v_mov_b32 v12, v0", "s_mov_b32 s40, 5", "s_setpc_b64 s[30:31]"],
            ["r_undefined:", "v_mov_b32 v12, v13", "s_setpc_b64 s[30:31]"],
            ["r_misaligned:", "v_mad_u64_u32 v[1:2], s[90:91], v0, v0, v[1:2]", "s_setpc_b64 s[30:31]"],
            ["r_no_return:", "v_mov_b32 v12, v0"],
            ["r_next:", "v_mov_b32 v13, v0", "s_setpc_b64 s[30:31]"]]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lines = ["  s_endpgm"]
    for r in ROUTINES:
        lines += ["  .p2align 8", r[0]] + ["  " + ln for ln in r[1:]]
    path = tmp_path_factory.mktemp("asm_sim") / "lib.hpp"
    path.write_text("#define T_TEXT \\\n" + "".join(f'    "{ln}\\n" \\\n' for ln in lines) + '    ""\n\n')
    return asm_sim.load_library(str(path), "T_TEXT")


def test_written_registers_are_tracked(lib):
    lane, rd = asm_sim.call(lib, "r_ok", {0: 7})
    assert lane.v[12] == 7 and lane.s[40] == 5
    assert lane.written_v == {12} and lane.written_s == {40} and lane.written_a == set()


def test_undefined_read_raises(lib):
    with pytest.raises(KeyError, match="undefined v13"):
        asm_sim.call(lib, "r_undefined", {0: 7})


def test_misaligned_pair_raises(lib):
    with pytest.raises(ValueError, match="misaligned"):
        asm_sim.call(lib, "r_misaligned", {0: 7})


def test_running_off_the_end_raises(lib):
    with pytest.raises(RuntimeError, match="fell off its end"):
        asm_sim.call(lib, "r_no_return", {0: 7})
