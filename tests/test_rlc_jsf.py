"""The Joint Sparse Form recoding of the batch exponents' halves (lachain_amd/csrc/rlc_jsf.hpp, CPU test).

The wave-uniform ladder of the TPKE batch check (rlc_common.hpp g1_mul_ab_jsf) walks the signed digits this header
gives for (a, b).  The header is plain C++: it is compiled here with the host compiler into a small shared object and
compared with a pure-Python JSF written below.  For every case: the digits reproduce a and b, lie in {-1, 0, 1}, set
no bit above column 32, and of any three consecutive columns at least one is zero in both rows; over 10,000 seeded
random pairs the mean count of nonzero columns stays below 17.5 (the form's density is 1/2: 16.5 of 33 columns,
against 24 of 32 for the plain binary joint form)."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lachain_amd", "csrc")
M32 = 2 ** 32 - 1

SHIM = r"""
#include "rlc_jsf.hpp"
extern "C" void jsf_many(const uint32_t *ab, uint64_t n, uint64_t *out) {
    for (uint64_t i = 0; i < n; i++) {
        rlc_jsf j;
        rlc_jsf_recode(j, ab[2 * i], ab[2 * i + 1]);
        out[4 * i] = j.nz_a; out[4 * i + 1] = j.neg_a; out[4 * i + 2] = j.nz_b; out[4 * i + 3] = j.neg_b;
    }
}
"""


@pytest.fixture(scope="module")
def recode(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++ or clang++) on PATH"
    d = tmp_path_factory.mktemp("jsf")
    src, so = str(d / "jsf_shim.cpp"), str(d / "libjsf_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC, "-o", so, src],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.jsf_many.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.jsf_many.restype = None

    def run(pairs):
        flat = (ctypes.c_uint32 * (2 * len(pairs)))(*[w for p in pairs for w in p])
        out = (ctypes.c_uint64 * (4 * len(pairs)))()
        lib.jsf_many(flat, len(pairs), out)
        return [tuple(out[4 * i:4 * i + 4]) for i in range(len(pairs))]
    return run


def jsf_model(a, b):
    """Solinas' algorithm on Python integers -> (digits of a, digits of b), least significant first"""
    k, d, rows = [a, b], [0, 0], ([], [])
    while k[0] + d[0] > 0 or k[1] + d[1] > 0:
        l = [k[0] + d[0], k[1] + d[1]]
        u = [0, 0]
        for i in (0, 1):
            if l[i] % 2:
                u[i] = 2 - l[i] % 4
                if l[i] % 8 in (3, 5) and l[1 - i] % 4 == 2:
                    u[i] = -u[i]
        for i in (0, 1):
            if 2 * d[i] == 1 + u[i]:
                d[i] = 1 - d[i]
            k[i] //= 2
            rows[i].append(u[i])
    return rows


def digits(nz, neg):
    assert neg & ~nz == 0, "a sign bit on a zero digit"
    return [((nz >> k) & 1) * (1 - 2 * ((neg >> k) & 1)) for k in range(64)]


def check(pair, masks):
    """the properties of one recoding; returns its count of nonzero columns"""
    a, b = pair
    nz_a, neg_a, nz_b, neg_b = masks
    assert (nz_a | nz_b | neg_a | neg_b) >> 33 == 0, (pair, "a bit above column 32")
    da, db = digits(nz_a, neg_a), digits(nz_b, neg_b)
    assert set(da) | set(db) <= {-1, 0, 1}
    assert sum(d << k for k, d in enumerate(da)) == a, pair
    assert sum(d << k for k, d in enumerate(db)) == b, pair
    col = nz_a | nz_b
    for k in range(31):
        assert (col >> k) & 7 != 7, (pair, k, "three consecutive nonzero columns")
    ma, mb = jsf_model(a, b)
    assert da[:len(ma)] == ma and not any(da[len(ma):]), pair
    assert db[:len(mb)] == mb and not any(db[len(mb):]), pair
    return bin(col).count("1")


FIXED = [(0, 0), (1, 0), (0, 1), (1, 1), (M32, M32), (M32, 1), (0x55555555, 0xAAAAAAAA), (0x80000000, 0x7FFFFFFF)]


def test_fixed_pairs(recode):
    for pair, masks in zip(FIXED, recode(FIXED)):
        check(pair, masks)
    assert recode([(0, 0)]) == [(0, 0, 0, 0)]
    assert recode([(1, 0)]) == [(1, 0, 0, 0)] and recode([(0, 1)]) == [(0, 0, 1, 0)]
    nz_a, neg_a, nz_b, neg_b = recode([(M32, M32)])[0]       # 2^32 - 1 twice: column 32 leads, -1 at column 0
    assert (nz_a, neg_a, nz_b, neg_b) == ((1 << 32) | 1, 1, (1 << 32) | 1, 1)


def test_equal_and_triple_operands(recode):
    rng = random.Random(0x15F)
    bs = [1, 2, 3, 5, 0x55555555, M32 // 3, 0x2AAAAAAA] + [rng.randrange(1, M32 // 3 + 1) for _ in range(500)]
    same = [(v, v) for v in bs] + [(rng.randrange(2 ** 32),) * 2 for _ in range(500)] + [(M32, M32)]
    for pair, masks in zip(same, recode(same)):
        check(pair, masks)
        assert masks[0] == masks[2] and masks[1] == masks[3]          # a = b: the two rows are one
    triple = [(3 * v, v) for v in bs]
    assert all(a <= M32 for a, _ in triple)
    for pair, masks in zip(triple, recode(triple)):
        check(pair, masks)


def test_random_pairs_and_density(recode):
    rng = random.Random(2001)
    pairs = [(rng.randrange(2 ** 32), rng.randrange(2 ** 32)) for _ in range(10000)]
    cols = [check(pair, masks) for pair, masks in zip(pairs, recode(pairs))]
    mean = sum(cols) / len(cols)
    binary = sum(bin(a | b).count("1") for a, b in pairs) / len(pairs)
    print("mean nonzero columns: JSF %.3f, binary joint form %.3f" % (mean, binary))
    assert mean < 17.5, mean
