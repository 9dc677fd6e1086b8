"""The cases the TPKE keystream (Utils.XorWithHash: lachain_amd/csrc/kdf_lane.hpp, k_kdf_xor) is checked on, shared by
the CPU emulation (tests/test_kdf_emul.py) and the GPU tests (tests/test_gpu_tpke_kdf.py).  Not a test module.

One batch of items (seed material, data), more than one wave and fewer than two:
  * every data length of DATA_LENS: the ends of the write-out (0, 1, 7, 8, 9), the 32-byte state (31 .. 33, 63 .. 65),
    the seed's cycles, which take effect at bytes 288 and 608 (287 .. 289, 320, 607 .. 609), and a long item (1000);
  * every seed length of SEED_LENS: 0 is valid, 48 is the G1 point of the TPKE paths, 104 makes `m || seed` exactly one
    rate block, 103 / 105 lie around it and 240 takes two absorb permutations;
  * the reference's own vector (CryptographyTest.cs:103-113, kdf_deadbeef_32 of tests/golden/reference_kats.json);
  * zero-length items between non-empty neighbours.
The items are packed back to back, so item i starts at the sum of the lengths before it; running the batch from a base
of every alignment in ALIGNMENTS puts every item, hence every length, at each start alignment."""
import hashlib
import json
import os

DATA_LENS = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 287, 288, 289, 320, 607, 608, 609, 1000]
SEED_LENS = [0, 4, 48, 103, 104, 105, 240]
ALIGNMENTS = list(range(8))

_HERE = os.path.dirname(os.path.abspath(__file__))


def rnd(tag: str, n: int) -> bytes:
    return hashlib.shake_256(tag.encode()).digest(n) if n else b""


def reference_vector():
    """(seed, data, expected) of the reference's test"""
    with open(os.path.join(_HERE, "golden", "reference_kats.json")) as f:
        k = json.load(f)["kdf_deadbeef_32"]
    return bytes.fromhex("deadbeef"), bytes(32), bytes.fromhex(k["hex"])


def items():
    """[(seed material, data)]: the batch"""
    out = []
    for s in (48, 0, 105):                       # every data length, under three seed lengths
        for n in DATA_LENS:
            out.append((rnd("seed %d %d" % (s, n), s), rnd("data %d %d" % (s, n), n)))
    for s in SEED_LENS:                          # every seed length, one state and across both cycles
        for n in (33, 609):
            out.append((rnd("sweep seed %d %d" % (s, n), s), rnd("sweep data %d %d" % (s, n), n)))
    seed, data, _ = reference_vector()
    out.append((seed, data))
    # zero-length items between non-empty neighbours (DATA_LENS' own 0 follows the item before it, too)
    for k in range(3):
        out.append((rnd("z seed %d" % k, 48), b""))
        out.append((rnd("nz seed %d" % k, 48), rnd("nz data %d" % k, 5 + 11 * k)))
    assert 64 < len(out) < 128
    return out


def reference_index():
    return 3 * len(DATA_LENS) + 2 * len(SEED_LENS)


def offsets(chunks, start=0):
    off = [start]
    for c in chunks:
        off.append(off[-1] + len(c))
    return off


def expected(oracle, batch, ok=None):
    """the outputs by the oracle: data ^ DigestRandomGenerator(seed) bytes; zero bytes where ok[i] == 0"""
    out = []
    for i, (seed, data) in enumerate(batch):
        if ok is not None and not ok[i]:
            out.append(bytes(len(data)))
        else:
            ks = oracle.drg_bytes(seed, len(data)) if data else b""
            out.append(bytes(a ^ b for a, b in zip(data, ks)))
    return out
