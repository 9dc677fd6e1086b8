"""Host-pointer forms of every host file, back to back on one thread's implicit context.

The host-pointer entry points take their transient device buffers from one shared set of staging slots (HostCall,
lachain_amd/csrc/host_call.hpp), in request order: what was a ciphertext buffer in one call is an offset array in the
next.  This test runs one form of every host file in sequence at small sizes, then at sizes that make every slot grow
(300 items cross a 256-lane block), then small again in reverse order, so each call finds slots that other calls left
larger, smaller or differently typed.  Every result is compared with the reference its own feature test uses (oracle,
tests/pyref), never with the library itself."""
import ctypes
import os
import random
import sys

import pytest

import oracle as o
import trie_cases as TC
import tx_cases as XC
from helpers import Drbg, R, gpu_native
from pyref import rbc_merkle as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ecies_emul import ref_ecdh  # noqa: E402
from test_gpu_mcl_surface import _mul_vec  # noqa: E402

pytestmark = pytest.mark.gpu

MULVEC_COOP_MAX = 512            # lcb_mcl.cpp: above it mclBnG1_mulVec stages its terms for the one-lane kernels
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
U8 = ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


@pytest.fixture(scope="module")
def mcl(nat):
    from lachain_amd import mcl as m
    return m


def buf(data: bytes):
    b = (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    return b, ctypes.cast(b, U8)


# ------------------------------------------------------------------ one step per entry point: inputs and the reference's
# answer are made once, the returned function calls the library and compares
def step_g1_mul(nat, n, seed):
    d = Drbg(b"interleaved mul %d" % seed)
    ks = [d.fr() for _ in range(n)]
    want = [o.g1_mul(o.g1_gen(), k) for k in ks]
    return lambda: nat.mul_batch(1, None, ks, generator=True) == want


def step_tpke(nat):
    """2 ciphertexts x 4 shares, one share corrupted (lcb_tpke_verify_shares)"""
    coeffs = [o.fr(17), o.fr(23)]
    x = [o.fr_eval_poly(coeffs, o.fr(i + 1)) for i in range(4)]
    y = o.g1_mul(o.g1_gen(), o.fr_eval_poly(coeffs, o.fr(0)))
    yi = [o.g1_mul(o.g1_gen(), xi) for xi in x]
    cts = [o.tpke_encrypt(y, b"interleaved payload %d" % c, o.fr(99 + c)) for c in range(2)]
    shares = [(c, i, o.tpke_decrypt(*cts[c], x[i])) for c in range(2) for i in range(4)]
    c, i, ui = shares[5]
    shares[5] = (c, i, o.g1_add(ui, o.g1_gen()))
    want = [o.tpke_verify_share(yi[i], *cts[c], ui) == 1 for c, i, ui in shares]
    assert want == [k != 5 for k in range(8)]
    return lambda: nat.tpke_verify_shares(yi, cts, shares) == want


def step_mul_vec(mcl):
    """mclBnG1_mulVec just above MULVEC_COOP_MAX: the staged path (terms, block sums)"""
    Fr, G1 = mcl.Fr, mcl.G1
    n, m = MULVEC_COOP_MAX + 1, 6
    d = Drbg(b"interleaved mulvec")
    base = [G1.Generator() * Fr.FromBytes(d.fr()) for _ in range(m)]
    pts = [base[i % m] for i in range(n)]
    scs = [Fr.FromBytes(d.fr()) for _ in range(n)]
    fold = [0] * m
    for i in range(n):
        fold[i % m] = (fold[i % m] + int.from_bytes(scs[i].ToBytes(), "little")) % R
    want = G1.Zero().ToBytes()
    for j in range(m):
        want = o.g1_add(want, o.g1_mul(base[j].ToBytes(), fold[j].to_bytes(32, "little")))
    return lambda: _mul_vec(mcl, pts, scs).ToBytes() == want


def step_eval_poly(nat, n, seed):
    d = Drbg(b"interleaved poly %d" % seed)
    coeffs = [o.g1_mul(o.g1_gen(), d.fr()) for _ in range(3)]
    xs = list(range(seed, seed + n))
    want = [o.g1_eval_poly(coeffs, o.fr(x)) for x in xs]
    return lambda: nat.g1_eval_poly_batch(coeffs, xs) == want


def step_pubkey(nat, n, seed):
    rng = random.Random(100 + seed)
    privs = [rng.randrange(1, SECP_N).to_bytes(32, "big") for _ in range(n)]
    want = b"".join(o.ecdsa_pubkey(p)[0] for p in privs)
    return lambda: nat.ecdsa_pubkey_batch(b"".join(privs)) == (want, b"\x01" * n)


def step_keccak(nat, n, seed):
    """lengths 0, 135, 136 and 137 (around the 136-byte rate), then random ones up to n messages"""
    rng = random.Random(200 + seed)
    msgs = [rng.randbytes(ln) for ln in (0, 135, 136, 137)] + [rng.randbytes(rng.randrange(300)) for _ in range(n - 4)]
    want = b"".join(o.keccak256(m) for m in msgs)
    return lambda: nat.keccak256_batch(msgs) == want


def step_merkle_root(nat, n, seed):
    """trees of 1 and 3 hashes first"""
    rng = random.Random(300 + seed)
    trees = [[rng.randbytes(32) for _ in range(c)] for c in ([1, 3] + [1 + k % 5 for k in range(n)])[:max(2, n)]]
    want = [M.compute_root(t) for t in trees]
    return lambda: nat.merkle_root_batch(trees) == want


def step_rs_encode(nat, shard_size, seed):
    """4 shards, 2 erasures"""
    data = random.Random(400 + seed).randbytes(2 * shard_size)
    want = o.rs_encode_shards(data, 4, 2)
    return lambda: nat.rs_encode(data, 4, 2) == want


def step_ecdh(nat, n, seed):
    """n items over a few distinct keys and scalars (the Python reference multiplies once per distinct pair)"""
    rng = random.Random(500 + seed)
    scalars = [rng.randrange(1, SECP_N).to_bytes(32, "big") for _ in range(min(n, 3))]
    pubs = [o.ecdsa_pubkey(rng.randrange(1, SECP_N).to_bytes(32, "big"))[0] for _ in range(min(n, 4))]
    who = [rng.randrange(len(scalars)) for _ in range(n)]
    pub = [pubs[i % len(pubs)] for i in range(n)]
    keys = [ref_ecdh(pub[i], scalars[who[i]]) for i in range(n)]
    assert all(k is not None for k in keys)
    want = (b"".join(keys), b"\x01" * n)
    return lambda: nat.secp_ecdh_batch(b"".join(pub), b"".join(scalars), who) == want


_tx = {}


def step_tx_hash(nat, n, seed):
    """n items of the transaction sweep (old chain id), starting at item `seed`"""
    chain = XC.K["chain_id"]["old"]
    if not _tx:
        items = XC.sweep(False, chain)
        raw, full = XC.expected(items, chain)
        _tx["items"], _tx["raw"], _tx["full"] = items, raw, full
    pool = _tx["items"]
    pick = [(seed + k) % len(pool) for k in range(n)]
    recs, inv, off, sigs = XC.flatten([pool[k] for k in pick])
    invs = [inv[off[k]:off[k + 1]] for k in range(n)]
    want = (b"".join(_tx["raw"][32 * k:32 * k + 32] for k in pick), b"".join(_tx["full"][32 * k:32 * k + 32] for k in pick))
    return lambda: nat.tx_hash_batch(recs, invs, sigs, 65, False, chain) == want


def step_trie(nat, n, seed):
    """lcb_trie_node_hash_batch with only out32, then with only accept (one expected hash spoiled)"""
    nodes = TC.batch_of(n, b"interleaved trie %d" % seed)
    recs, data, off = TC.flatten(nodes)
    want = b"".join(TC.expected_hash(x) for x in nodes)
    spoiled = bytearray(want)
    spoiled[32 * (n - 1)] ^= 1
    want_acc = b"\x01" * (n - 1) + b"\x00"
    offs = (ctypes.c_uint64 * (n + 1))(*off)

    def run():
        fn = nat.lib().lcb_trie_node_hash_batch
        (kr, pr), (kd, pd), (ke, pe) = buf(recs), buf(data), buf(bytes(spoiled))
        (out, po), (acc, pa) = buf(bytes(32 * n)), buf(b"\xee" * n)
        if fn(po, None, pr, pd, offs, None, n) != 0 or bytes(out)[:32 * n] != want:
            return False
        return fn(None, pa, pr, pd, offs, pe, n) == 0 and bytes(acc)[:n] == want_acc
    return run


def sequence(nat, mcl, tpke, mul_vec, sizes, seed):
    """one step per host file's form, in the files' order; sizes: (a, b, c) item counts, rotated over the steps"""
    a, b, c = sizes
    return [
        ("lcb_g1_mul_batch", step_g1_mul(nat, min(a, 3), seed)),                 # lcb_host.cpp (BLS: stays small)
        ("lcb_tpke_verify_shares", tpke),
        ("mclBnG1_mulVec", mul_vec),                                              # lcb_mcl.cpp
        ("lcb_g1_eval_poly_batch", step_eval_poly(nat, min(b, 3), seed)),         # lcb_dkg.cpp (BLS: stays small)
        ("lcb_ecdsa_pubkey_batch", step_pubkey(nat, c, seed)),                    # lcb_ecdsa.cpp
        ("lcb_keccak256_batch", step_keccak(nat, max(a, 4), seed)),
        ("lcb_merkle_root_batch", step_merkle_root(nat, b, seed)),                # lcb_rbc.cpp
        ("lcb_rs_encode", step_rs_encode(nat, c, seed)),
        ("lcb_secp_ecdh_batch", step_ecdh(nat, a, seed)),                         # lcb_ecies.cpp
        ("lcb_tx_hash_batch", step_tx_hash(nat, b, seed)),                        # lcb_txhash.cpp
        ("lcb_trie_node_hash_batch", step_trie(nat, c, seed)),                    # lcb_trie.cpp
    ]


def test_host_forms_interleaved(nat, mcl):
    tpke, mul_vec = step_tpke(nat), step_mul_vec(mcl)
    small = sequence(nat, mcl, tpke, mul_vec, (1, 2, 3), 1)
    large = sequence(nat, mcl, tpke, mul_vec, (300, 300, 300), 2)
    again = sequence(nat, mcl, tpke, mul_vec, (3, 1, 2), 3)
    for phase, steps in (("small", small), ("large", large), ("small, reversed", again[::-1])):
        for name, run in steps:
            assert run(), (phase, name, nat.last_error())
