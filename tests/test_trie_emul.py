"""CPU check of the state-trie lane (lachain_amd/csrc/trie_lane.hpp, the bodies of k_trie.hip's hashing kernels)
compiled for the host by tools/emul/trie_emul.cpp: a stand-alone program built with -fsanitize=address,undefined that
runs the cases of tests/trie_cases.py, every item from exact-size heap buffers.  It must agree with the restatement
(tests/pyref/trie.py) and leave no sanitizer report.  TEST INFRASTRUCTURE: catches logic errors and stray loads in the
device code without a GPU; the kernels themselves are covered by tests/test_gpu_trie.py, which shares the cases."""
import os
import random
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trie_cases as C  # noqa: E402
from pyref import trie as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emul", "trie_emul.cpp")
EXE = os.path.join(ROOT, "tools", "emul", "trie_emul")
CSRC = os.path.join(ROOT, "lachain_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("trie_lane.hpp", "rbc_lane.hpp", "keccak.hpp")]


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-o", EXE, SRC], check=True)
    return EXE


def run(exe, tmp_path, mode, n, n_literals, body: bytes) -> bytes:
    cases, results = tmp_path / "cases.bin", tmp_path / "results.bin"
    cases.write_bytes(struct.pack("<IIII", mode, n, n_literals, 0) + body)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, str(cases), str(results)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    return results.read_bytes()


def u64s(vals):
    return struct.pack("<%dQ" % len(vals), *vals)


def run_flat(exe, tmp_path, nodes):
    recs, data, off = C.flatten(nodes)
    got = run(exe, tmp_path, 0, len(nodes), 0, recs + u64s(off) + data)
    assert len(got) == 32 * len(nodes)
    return got


def test_flat_cases(exe, tmp_path):
    nodes = C.flat_cases()
    got = run_flat(exe, tmp_path, nodes)
    bad = [(i, n.note, len(n.data)) for i, n in enumerate(nodes) if got[32 * i:32 * i + 32] != C.expected_hash(n)]
    assert not bad, bad[:10]


def test_long_leaves(exe, tmp_path):
    """whole rate blocks inside the item (the straight-load path) at every alignment"""
    d = C.Drbg(b"long leaves")
    nodes = C.align([(C.leaf(d, v), a) for a in range(8) for v in (136 * 2 + a, 136 * 3 - 36 + a, 5000 + 17 * a)])
    got = run_flat(exe, tmp_path, nodes)
    assert got == b"".join(C.expected_hash(n) for n in nodes)


def test_items(exe, tmp_path):
    rng = random.Random(3)
    hashes = C.crafted_pool(rng, 40, 50) + [C.craft([1] * 51), C.craft([1] * 51, 1), C.craft([1] * 51, 1), bytes(32),
                                           b"\xff" * 32, C.craft(range(51))]
    values = [bytes(rng.randrange(256) for _ in range(v)) for v in list(C.VALUE_LENS) + [96, 97, 98, 102, 103, 104, 231, 232]]
    values += [bytes([i]) * (i % 9) for i in range(len(hashes) - len(values))]
    n = len(hashes)
    off = [0]
    for v in values:
        off.append(off[-1] + len(v))
    got = run(exe, tmp_path, 1, n, 0, b"".join(hashes) + u64s(off) + b"".join(values))
    assert len(got) == 167 * n
    prev = None
    for i, (h, v) in enumerate(zip(hashes, values)):
        rec = got[167 * i:167 * i + 167]
        frags = [R.hash_fragment(h, f) for f in range(51)]
        assert list(rec[:51]) == frags and list(rec[83:134]) == frags, i
        bits = "".join(format(f, "05b") for f in frags) + str(h[31] >> 7)
        assert int.from_bytes(rec[51:83], "little") == int(bits, 2), i
        assert rec[134:166] == R.leaf_hash(h, v), (i, len(v))
        if prev is None:
            assert rec[166] == 255
        else:
            pf = [R.hash_fragment(prev, f) for f in range(51)]
            lcp = next((f for f in range(51) if pf[f] != frags[f]), 51)
            assert rec[166] == lcp, i
        prev = h


def rehash_body(records, items, children, literals, order):
    off, coff = [0], [0]
    for it in items:
        off.append(off[-1] + len(it))
    for c in children:
        coff.append(coff[-1] + len(c))
    refs = [r for c in children for r in c]
    return (records + u64s(off) + b"".join(items) + u64s(coff) + struct.pack("<%dq" % len(refs), *refs) +
            b"".join(literals) + u64s(order))


def children_first(children):
    """an order with every in-batch child before its parents"""
    n, done, order = len(children), set(), []
    while len(order) < n:
        for i in range(n):
            if i not in done and all(r < 0 or r in done for r in children[i]):
                done.add(i)
                order.append(i)
    return order


@pytest.mark.parametrize("k", [1, 7, 50])
def test_rehash_chain(exe, tmp_path, k):
    t, root = C.chain_trie(k, [(C.craft([9 + j], fill=j), bytes(j)) for j in range(5)])
    records, items, children, literals, want = C.export(t, root, random.Random(k))
    got = run(exe, tmp_path, 2, len(items), 0, rehash_body(records, items, children, literals, children_first(children)))
    assert got == want


def test_rehash_with_literals(exe, tmp_path):
    rng = random.Random(11)
    t, root = R.TrieHashMap(), 0
    for h in C.crafted_pool(rng, 40, 6):
        root = t.add_by_hash(root, h, bytes(rng.randrange(256) for _ in range(rng.randrange(80))))
    records, items, children, literals, want = C.export(t, root, rng, lambda i, n: i % 3 == 0 and i != root)
    assert literals and any(r >= 0 for c in children for r in c)
    got = run(exe, tmp_path, 2, len(items), len(literals),
              rehash_body(records, items, children, literals, children_first(children)))
    assert got == want
