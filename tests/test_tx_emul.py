"""CPU check of the transaction-hash lane (lachain_amd/csrc/txhash_lane.hpp, the body of k_txhash.hip's k_tx_hash)
compiled for the host by tools/emul/txhash_emul.cpp: a stand-alone program built with -fsanitize=address,undefined
that runs the reference's known answers and the sweep of tests/tx_cases.py, every item from exact-size heap buffers.
It must agree with the restatement (tests/pyref/txhash.py) and leave no sanitizer report.  TEST INFRASTRUCTURE: catches
logic errors and stray loads in the device code without a GPU; the kernel itself is covered by
tests/test_gpu_tx_hash.py, which shares the cases."""
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tx_cases as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emul", "txhash_emul.cpp")
EXE = os.path.join(ROOT, "tools", "emul", "txhash_emul")
CSRC = os.path.join(ROOT, "lachain_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("txhash_lane.hpp", "rbc_lane.hpp", "keccak.hpp")]


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-o", EXE, SRC], check=True)
    return EXE


def run(exe, tmp_path, items, new, chain_id, claimed=None, with_sigs=True):
    recs, inv, off, sigs = C.flatten(items)
    n = len(items)
    sig_len = (66 if new else 65) if with_sigs else 0
    claimed = claimed if claimed is not None else bytes(32 * n)
    cases, results = tmp_path / "cases.bin", tmp_path / "results.bin"
    cases.write_bytes(struct.pack("<IIII", n, sig_len, chain_id, 0) + recs + struct.pack("<%dQ" % (n + 1), *off) + inv +
                      (sigs if with_sigs else b"") + claimed)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, str(cases), str(results)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    got = results.read_bytes()
    assert len(got) == 65 * n
    return (b"".join(got[65 * i:65 * i + 32] for i in range(n)), b"".join(got[65 * i + 32:65 * i + 64] for i in range(n)),
            bytes(got[65 * i + 64] for i in range(n)))


@pytest.mark.parametrize("new", [False, True])
def test_kats(exe, tmp_path, new):
    kats = C.kat_cases(new)
    items = [C.Item(tx, sig, 0, "kat") for tx, sig, _, _ in kats]
    chain = C.K["chain_id"]["new" if new else "old"]
    claimed = b"".join(h for _, _, h, _ in kats)
    raw, full, match = run(exe, tmp_path, items, new, chain, claimed)
    assert full == claimed and match == b"\x01" * len(kats)
    assert (raw, full) == C.expected(items, chain)
    if not new:
        import oracle as o
        assert raw[32:] == o.keccak256(bytes.fromhex(C.K["unsigned"][0]["rlp"]))


@pytest.mark.parametrize("new,chain", C.CALLS)
def test_sweep(exe, tmp_path, new, chain):
    items = C.sweep(new, chain)
    want_raw, want_full = C.expected(items, chain)
    claimed = bytearray(want_full)
    for i in range(1, len(items), 2):                      # every second claimed hash is off by one bit
        claimed[32 * i + (i % 32)] ^= 1 << (i % 8)
    raw, full, match = run(exe, tmp_path, items, new, chain, bytes(claimed))
    bad = [(i, items[i].note, items[i].align, len(items[i].tx[5])) for i in range(len(items))
           if raw[32 * i:32 * i + 32] != want_raw[32 * i:32 * i + 32] or full[32 * i:32 * i + 32] != want_full[32 * i:32 * i + 32]]
    assert not bad, bad[:10]
    assert match == bytes((i + 1) % 2 for i in range(len(items)))


def test_raw_only(exe, tmp_path):
    items = C.sweep(False, 25)[:40]
    raw, full, match = run(exe, tmp_path, items, False, 25, with_sigs=False)
    assert raw == C.expected(items, 25)[0] and full == bytes(32 * len(items)) and match == bytes(len(items))
