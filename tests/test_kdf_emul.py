"""CPU check of the TPKE keystream lane (lachain_amd/csrc/kdf_lane.hpp, the body of k_kdf_xor) compiled for the host by
tools/emul/kdf_emul.cpp: a stand-alone program built with -fsanitize=address,undefined that runs the cases of
tests/kdf_cases.py, every item from exact-size heap buffers at its packed alignment.  It must agree with the oracle
(oracle.drg_bytes / oracle.xor_with_hash) and leave no sanitizer report.  TEST INFRASTRUCTURE: catches logic errors,
stray word loads and stray byte stores in the device code without a GPU; the kernel itself is covered by
tests/test_gpu_tpke_kdf.py, which shares the cases."""
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kdf_cases as C  # noqa: E402
import oracle as o  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emul", "kdf_emul.cpp")
EXE = os.path.join(ROOT, "tools", "emul", "kdf_emul")
CSRC = os.path.join(ROOT, "lachain_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("kdf_lane.hpp", "rbc_lane.hpp", "keccak.hpp")]


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-o", EXE, SRC], check=True)
    return EXE


@pytest.fixture(scope="module")
def batch():
    items = C.items()
    return items, C.expected(o, items)


def run(exe, tmp_path, items, data_align=0, seed_align=0, out_align=None, in_place=False, ok=None) -> list:
    cases, results = tmp_path / "cases.bin", tmp_path / "results.bin"
    n = len(items)
    soff, doff = C.offsets([s for s, _ in items]), C.offsets([d for _, d in items])
    out_align = 8 if in_place else data_align if out_align is None else out_align
    body = struct.pack("<IIII", n, data_align, seed_align, out_align)
    body += struct.pack("<%dI" % (n + 1), *soff) + struct.pack("<%dI" % (n + 1), *doff)
    body += bytes(ok if ok is not None else [1] * n)
    body += b"".join(s for s, _ in items) + b"".join(d for _, d in items)
    cases.write_bytes(body)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, str(cases), str(results)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    got = results.read_bytes()
    assert len(got) == doff[-1]
    return [got[doff[i]:doff[i + 1]] for i in range(n)]


def mismatches(items, got, want):
    return [(i, len(items[i][0]), len(items[i][1])) for i in range(len(items)) if got[i] != want[i]]


def test_reference_vector(exe, tmp_path):
    seed, data, want = C.reference_vector()
    assert o.drg_bytes(seed, 32) == want                      # the oracle itself stands on the reference's vector
    assert run(exe, tmp_path, [(seed, data)]) == [want]


@pytest.mark.parametrize("align", C.ALIGNMENTS)
def test_cases_at_every_alignment(exe, tmp_path, batch, align):
    """every length at each start alignment; the seeds at another phase than the data"""
    items, want = batch
    got = run(exe, tmp_path, items, data_align=align, seed_align=(3 * align + 1) % 8)
    assert not mismatches(items, got, want)
    assert got[C.reference_index()] == C.reference_vector()[2]


@pytest.mark.parametrize("align", C.ALIGNMENTS)
def test_output_at_another_alignment_than_the_data(exe, tmp_path, batch, align):
    """the stores follow the output's boundaries, the loads the data's"""
    items, want = batch
    assert not mismatches(items, run(exe, tmp_path, items, data_align=(5 * align + 3) % 8, out_align=align), want)


@pytest.mark.parametrize("align", C.ALIGNMENTS)
def test_in_place(exe, tmp_path, batch, align):
    items, want = batch
    assert not mismatches(items, run(exe, tmp_path, items, data_align=align, in_place=True), want)


def test_ok_zero_writes_zero_bytes(exe, tmp_path, batch):
    items, _ = batch
    ok = [i % 3 != 1 for i in range(len(items))]
    want = C.expected(o, items, ok)
    for align in (0, 5):
        assert not mismatches(items, run(exe, tmp_path, items, data_align=align, ok=ok), want)


def test_g1_seed_equals_xor_with_hash(exe, tmp_path):
    """the TPKE paths' shape: a 48-byte seed is Utils.XorWithHash of a serialised G1 point"""
    items = [(C.rnd("g1 %d" % n, 48), C.rnd("payload %d" % n, n)) for n in C.DATA_LENS]
    got = run(exe, tmp_path, items)
    assert got == [o.xor_with_hash(s, d) for s, d in items]
    assert got[0] == b"" and run(exe, tmp_path, [(bytes(48), bytes(40))]) == [o.xor_with_hash(bytes(48), bytes(40))]
