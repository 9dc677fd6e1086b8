"""GPU transaction hashing (k_txhash.hip's k_tx_hash through lcb_tx_hash_batch / lcb_tx_hash_dev /
lcb_ctx_tx_hash_dev) against the reference's known answers (tests/golden/tx_kats.json) and the plain-Python
restatement (tests/pyref/txhash.py over o.keccak256), bit for bit.  The sweep (tests/tx_cases.py, shared with the host
emulation in tests/test_tx_emul.py) is one call per (signature width, chain id): every 64-bit field and value edge, To
present and empty, invocation lengths up to 65,536 at each of the 8 byte alignments, the Keccak block edges of both
encodings, short and long list headers, stripped r / s / v and the zero signatures.  Every buffer handed to the
library carries a guard pattern on both sides that must be intact afterwards."""
import ctypes

import pytest

import oracle as o
import tx_cases as C
from helpers import gpu_native

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xA5
_expected = {}


@pytest.fixture(scope="module")
def nat():
    return gpu_native()


def expected(new, chain):
    """the restatement's hashes of one call's sweep: computed once, shared by the host and device forms"""
    if (new, chain) not in _expected:
        items = C.sweep(new, chain)
        _expected[new, chain] = (items,) + C.expected(items, chain)
    return _expected[new, chain]


def guarded(data: bytes):
    """(buffer, pointer to the data inside it)"""
    buf = (ctypes.c_uint8 * (2 * GUARD + len(data))).from_buffer_copy(bytes([PATTERN]) * GUARD + data + bytes([PATTERN]) * GUARD)
    return buf, ctypes.cast(ctypes.byref(buf, GUARD), ctypes.POINTER(ctypes.c_uint8))


def inner(buf) -> bytes:
    raw = bytes(buf)
    assert raw[:GUARD] == bytes([PATTERN]) * GUARD and raw[-GUARD:] == bytes([PATTERN]) * GUARD, "guard overwritten"
    return raw[GUARD:-GUARD]


def host_call(nat, items, new, chain, with_sigs=True):
    recs, inv, off, sigs = C.flatten(items)
    n = len(items)
    b_rec, p_rec = guarded(recs)
    b_inv, p_inv = guarded(inv)
    b_sig, p_sig = guarded(sigs)
    b_raw, p_raw = guarded(bytes(32 * n))
    b_full, p_full = guarded(bytes(32 * n))
    offs = (ctypes.c_uint64 * (n + 1))(*off)
    rc = nat.lib().lcb_tx_hash_batch(p_raw, p_full, p_rec, p_inv, offs, p_sig if with_sigs else None, 66 if new else 65, n,
                                     int(new), chain)
    assert rc == 0, nat.last_error()
    assert (inner(b_rec), inner(b_inv), inner(b_sig)) == (recs, inv, sigs)
    return inner(b_raw), inner(b_full)


@pytest.mark.parametrize("new", [False, True])
def test_kats(nat, new):
    kats = C.kat_cases(new)
    items = [C.Item(tx, sig, 0, "kat") for tx, sig, _, _ in kats]
    chain = C.K["chain_id"]["new" if new else "old"]
    raw, full = host_call(nat, items, new, chain)
    assert full == b"".join(h for _, _, h, _ in kats)
    assert raw == C.expected(items, chain)[0]
    if not new:
        assert raw[32:] == o.keccak256(bytes.fromhex(C.K["unsigned"][0]["rlp"]))


@pytest.mark.parametrize("new,chain", C.CALLS)
def test_sweep_host_form(nat, new, chain):
    items, want_raw, want_full = expected(new, chain)
    raw, full = host_call(nat, items, new, chain)
    bad = [(i, items[i].note, items[i].align, len(items[i].tx[5])) for i in range(len(items))
           if raw[32 * i:32 * i + 32] != want_raw[32 * i:32 * i + 32] or full[32 * i:32 * i + 32] != want_full[32 * i:32 * i + 32]]
    assert not bad, bad[:10]


def test_raw_only_without_signatures(nat):
    items, want_raw, _ = expected(False, 25)
    raw, full = host_call(nat, items, False, 25, with_sigs=False)
    assert raw == want_raw and full == bytes(32 * len(items))       # full32_out is not written


@pytest.mark.parametrize("new,chain", C.CALLS)
def test_sweep_device_form(nat, new, chain):
    import torch
    items, want_raw, want_full = expected(new, chain)
    recs, inv, off, sigs = C.flatten(items)
    n = len(items)
    dev = torch.device("cuda:0")
    pad = bytes([PATTERN]) * GUARD

    def dbuf(data):
        return torch.frombuffer(bytearray(pad + data + pad), dtype=torch.uint8).to(dev)

    lib = nat.lib()
    d_rec, d_inv, d_sig = dbuf(recs), dbuf(inv), dbuf(sigs)
    d_off = torch.tensor(off, dtype=torch.int64, device=dev)
    with nat.Context() as ctx:
        for c in (None, ctx.ptr):
            d_raw, d_full = dbuf(bytes(32 * n)), dbuf(bytes(32 * n))
            pre = (c,) if c else ()
            fn = lib.lcb_ctx_tx_hash_dev if c else lib.lcb_tx_hash_dev
            assert fn(*pre, d_raw.data_ptr() + GUARD, d_full.data_ptr() + GUARD, d_rec.data_ptr() + GUARD,
                      d_inv.data_ptr() + GUARD, d_off.data_ptr(), d_sig.data_ptr() + GUARD, 66 if new else 65, n, int(new),
                      chain, torch.cuda.current_stream().cuda_stream) == 0, lib.lcb_last_error()
            torch.cuda.synchronize()
            for t, want in ((d_raw, want_raw), (d_full, want_full), (d_rec, recs), (d_inv, inv), (d_sig, sigs)):
                assert bytes(t.cpu().numpy()) == pad + want + pad
    ms = nat.tx_phase_ms()
    assert len(ms) == 3 and ms[0] >= 0


def test_bad_arguments_fail_the_call(nat):
    items = C.sweep(False, 25)[:4]
    recs, inv, off, sigs = C.flatten(items)
    lib = nat.lib()
    n = len(items)
    out = (ctypes.c_uint8 * (32 * n))()
    po = ctypes.cast(out, ctypes.POINTER(ctypes.c_uint8))

    def call(recs=recs, off=off, sig_len=65, new=0, chain=25, inv_ptr=True):
        (b_rec, pr), (b_inv, pi), (b_sig, ps) = guarded(recs), guarded(inv), guarded(sigs)     # buffers held until return
        offs = (ctypes.c_uint64 * len(off))(*off)
        return lib.lcb_tx_hash_batch(po, po, pr, pi if inv_ptr else None, offs, ps, sig_len, n, new, chain)

    assert call() == 0
    assert call(sig_len=66) == -1 and call(new=1) == -1 and call(inv_ptr=False) == -1 and call(chain=-1) == -1
    assert call(off=[5, 4, 4, 4, 4]) == -1                              # decreasing offsets
    assert call(off=[0, 2 ** 31, 2 ** 31, 2 ** 31, 2 ** 31]) == -1       # an item of 2^31 bytes: refused before any read
    bad_to = bytearray(recs)
    bad_to[96] = 19
    assert call(recs=bytes(bad_to)) == -1
    assert "to_len" in nat.last_error()
