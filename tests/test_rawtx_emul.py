"""CPU check of the raw-transaction lane (lachain_amd/csrc/rawtx_lane.hpp, the body of k_rawtx.hip's k_rawtx_decode and
k_rawtx_long) compiled for the host by tools/emul/rawtx_emul.cpp: a stand-alone program built with
-fsanitize=address,undefined that runs the cases of tests/rawtx_cases.py, every item from an exact-size heap buffer
that ends at the last aligned word holding one of its bytes.  Status, detail bits 0-1 and every decoded byte must equal
the restatement's (tests/pyref/rawtx.py), and there must be no sanitizer report.  TEST INFRASTRUCTURE: a decoder that
misreads hostile bytes is found here, under the sanitizer, before tests/test_gpu_rawtx.py runs the same cases on the
device."""
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rawtx_cases as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emul", "rawtx_emul.cpp")
EXE = os.path.join(ROOT, "tools", "emul", "rawtx_emul")
CSRC = os.path.join(ROOT, "lachain_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("rawtx_lane.hpp", "txhash_lane.hpp", "rbc_lane.hpp", "keccak.hpp")]


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-o", EXE, SRC], check=True)
    return EXE


def run(exe, tmp_path, raw, off, new, chain):
    """the emulator's outputs as pyref.rawtx.Ingested tuples (accept is not the lane's: 0)"""
    n = len(off) - 1
    L = 66 if new else 65
    cases, results = tmp_path / "cases.bin", tmp_path / "results.bin"
    cases.write_bytes(struct.pack("<IIII", n, L, chain, 0) + struct.pack("<%dQ" % (n + 1), *off) + raw)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, str(cases), str(results)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    got = results.read_bytes()
    size = 2 + 104 + 16 + L + 64
    assert len(got) == size * n
    res = []
    for i in range(n):
        g = got[size * i:size * (i + 1)]
        res.append(C.W.Ingested(0, g[0], g[1], g[2:106], struct.unpack("<QQ", g[106:122]), g[122:122 + L],
                                g[122 + L:154 + L], g[154 + L:186 + L]))
    return res


def check(exe, tmp_path, cases, new, chain, aligned=()):
    raw, off, items = C.pack(cases, aligned)
    want = C.expected(items, off, new, chain, recover=False)
    got = run(exe, tmp_path, raw, off, new, chain)
    bad = [(i, items[i].note, len(items[i].wire), off[i] % 8) for i in range(len(items)) if got[i] != want[i]]
    assert not bad, (bad[:10], got[bad[0][0]], want[bad[0][0]])
    return want


def test_six_vectors(exe, tmp_path):
    for wire, new, chain, _, _ in C.kats():
        want = check(exe, tmp_path, [C.Case(wire, "kat")], new, chain, aligned={0})
        assert {(w.status, w.detail) for w in want if w.status == 0} == {(0, 3)}


@pytest.mark.parametrize("new,chain", C.CALLS)
def test_round_trip_sweep(exe, tmp_path, new, chain):
    want = check(exe, tmp_path, C.roundtrip(new, chain), new, chain)
    assert sum(w.status == 0 for w in want) > 200


@pytest.mark.parametrize("new", [False, True])
def test_hostile_items(exe, tmp_path, new):
    cases, chain = C.hostile(new)
    want = check(exe, tmp_path, cases, new, chain)
    assert {w.status for w in want} == {0, 1, 2, 3, 4, 5}
    base, _ = C.base_vector(new)
    assert all(w.status != 0 for w in want[1:1 + len(base)])               # every prefix is refused


@pytest.mark.parametrize("new", [False, True])
def test_every_start_alignment(exe, tmp_path, new):
    cases, chain = C.hostile(new)
    pick = [c for c in cases if not c.note.startswith(("byte ", "prefix "))]
    pick += [c for c in cases if c.note.startswith("prefix ")][::7]
    check(exe, tmp_path, pick, new, chain, aligned=set(range(len(pick))))
