"""GPU parity of the level driver's overlap rule (lcb_set_busy_coop_max, lcb_set_level_mode): a batched
TPKE verify that overlaps another one on its device runs a level's final exponentiation on the one-lane kernel above
the busy threshold instead of the nine-lane kernel.  Both kernels leave the same canonical values, so no decision may
change.

10 decryptors (F = 3), 7 ciphertexts, 70 shares: seven level-1 groups.  set_level_mode(2) makes every call count as
overlapped, set_busy_coop_max(0) sends every level dispatch to the one-lane kernel and set_fe_pair_min(2) forces the
pair stage, so its two passes, level 2 and the single checks behind it all run one-lane at these sizes.  Every decision
must equal the oracle's per-share decision and the decisions of the same call with set_level_mode(1) (never
overlapped: the nine-lane kernels), and the dispatch counters must show which kernel ran: one dispatch for pass 1, one
for pass 2 when it has jobs, one per further level (each is a single chunk here); the census chain is not counted."""
import threading

import numpy as np
import pytest

from test_gpu_batched import Batch, run_dev, up

pytestmark = pytest.mark.gpu
N, F, C = 10, 3, 7
CT = np.repeat(np.arange(C, dtype=np.uint32), N)
DEC = np.tile(np.arange(N, dtype=np.uint32), C)


@pytest.fixture(scope="module")
def nat():
    from helpers import gpu_native
    return gpu_native()


@pytest.fixture(scope="module")
def tdev():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def batch():
    return Batch(b"gpu-level-mode", N, F, C)


@pytest.fixture(autouse=True)
def settings(nat):
    """every setting a test here changes is restored afterwards"""
    default = nat.busy_coop_max()
    yield default
    nat.set_level_mode(0)
    nat.set_busy_coop_max(default)
    nat.set_fe_pair_min(None)
    nat.set_batch_census(16384)


def shares_of(b, bad):
    shares = [(b.bad if (int(c), int(j)) in bad else b.good)[c][j] for c, j in zip(CT, DEC)]
    expect = np.array([b.expect(int(c), int(j), s) for c, j, s in zip(CT, DEC, shares)], dtype=np.uint8)
    return shares, expect


def run_mode(nat, tdev, b, shares, mode):
    """decisions, level-kernel stats and the number of level dispatches the call's own counters imply"""
    nat.set_level_mode(mode)
    got = run_dev(nat, tdev, b, CT, DEC, shares)
    levels, _ = nat.tpke_batched_stats()
    _, _, pass1, pass2 = nat.tpke_fe_pair_stats()
    assert pass1 >= 1                                  # the pair stage ran
    dispatches = 1 + (1 if pass2 else 0) + sum(1 for v in levels[1:] if v)
    return got, nat.tpke_level_kernel_stats(), dispatches


CASES = {
    "all_valid": [],
    "one_wrong": [(1, 7)],
    "two_wrong": [(3, 2), (3, 6)],
    "three_wrong": [(5, 1), (5, 4), (5, 8)],
    "every_group_one": [(c, (3 * c) % N) for c in range(C)],
    "every_group_two": [(c, (3 * c + d) % N) for c in range(C) for d in (0, 4)],
    "every_group_three": [(c, (3 * c + d) % N) for c in range(C) for d in (0, 4, 5)],
}


def forced_pair(nat, tdev, b, bad):
    shares, expect = shares_of(b, set(bad))
    nat.set_busy_coop_max(0)
    nat.set_fe_pair_min(2)
    busy, st_busy, n_busy = run_mode(nat, tdev, b, shares, 2)
    lat, st_lat, n_lat = run_mode(nat, tdev, b, shares, 1)
    assert np.array_equal(busy, expect), (busy.tolist(), expect.tolist())
    assert np.array_equal(lat, busy)
    # forced busy: every level dispatch one-lane, each of them because of the rule (all are far below set_coop_max)
    assert st_busy[:3] == [n_busy, 0, n_busy], (st_busy, n_busy)
    # forced latency: the nine-lane kernel throughout
    assert st_lat[:3] == [0, n_lat, 0], (st_lat, n_lat)


@pytest.mark.parametrize("case", sorted(CASES))
def test_level_mode_forced_busy_cases(nat, tdev, batch, case):
    forced_pair(nat, tdev, batch, CASES[case])


def test_level_mode_forced_busy_suspect_key_singles(nat, tdev, batch):
    """decryptor 2's share is wrong in every ciphertext: with a census its key is suspect, so level 1 holds the six
    remaining groups and, beside them, its other shares as exact singles; one more bad share fails a group.  The
    census chain keeps its kernels and is not counted."""
    bad = {(c, 2) for c in range(C)} | {(4, 7)}
    nat.set_batch_census(64)
    forced_pair(nat, tdev, batch, bad)
    assert nat.batched_census() == [17, 1, 6, 11]


def test_level_mode_default_threshold_keeps_small_levels(nat, tdev, batch, settings):
    """a queue-sized flush that overlaps another one keeps the latency kernels: the committed default never reaches
    levels this small (a one-lane final exponentiation takes about 12 ms however few checks it has)"""
    assert settings >= 1024 and nat.busy_coop_max() == settings
    shares, expect = shares_of(batch, {(1, 7), (5, 1), (5, 4), (5, 8)})
    nat.set_fe_pair_min(2)
    got, st, n = run_mode(nat, tdev, batch, shares, 2)
    assert np.array_equal(got, expect)
    assert st[:3] == [0, n, 0], (st, n)


def test_level_mode_overlapped_calls(nat, tdev, batch):
    """two contexts on two streams, called from two threads at once in auto mode: both decide correctly whichever form
    either saw, and the in-flight count returns to 0, also after a call that fails its argument checks"""
    torch, dev = tdev
    lib = nat.lib()
    b = batch
    bads = [{(0, 4), (3, 2), (3, 6)}, {(c, (3 * c) % N) for c in range(C)}]
    d_y = up(torch, dev, b"".join(b.yi))
    d_u = up(torch, dev, b"".join(ct[0] for ct in b.cts))
    d_w = up(torch, dev, b"".join(ct[2] for ct in b.cts))
    d_v = up(torch, dev, b"".join(ct[1] for ct in b.cts))
    d_voff = up(torch, dev, np.arange(0, 32 * (C + 1), 32, dtype=np.uint32))
    d_ct, d_dec = up(torch, dev, CT), up(torch, dev, DEC)
    lanes = []
    for bad in bads:
        shares, expect = shares_of(b, bad)
        lanes.append(dict(ctx=nat.Context(), stream=torch.cuda.Stream(dev), expect=expect,
                          sh=up(torch, dev, b"".join(shares)),
                          acc=torch.full((len(shares),), 7, dtype=torch.uint8, device=dev), rc=None))
    torch.cuda.synchronize(dev)
    nat.set_level_mode(0)
    nat.set_busy_coop_max(0)
    nat.set_fe_pair_min(2)
    assert nat.batched_inflight(0) == 0
    gate = threading.Barrier(len(lanes))

    def one(ln, n_cts=C):
        return lib.lcb_ctx_tpke_verify_shares_batched_dev(
            ln["ctx"].ptr, ln["acc"].data_ptr(), len(CT), d_y.data_ptr(), N, d_u.data_ptr(), d_w.data_ptr(),
            d_v.data_ptr(), d_voff.data_ptr(), n_cts, d_ct.data_ptr(), d_dec.data_ptr(), ln["sh"].data_ptr(),
            ln["stream"].cuda_stream)

    def work(ln):
        gate.wait()
        ln["rc"] = one(ln)

    threads = [threading.Thread(target=work, args=(ln,)) for ln in lanes]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    try:
        assert [ln["rc"] for ln in lanes] == [0, 0], nat.last_error()
        assert nat.batched_inflight(0) == 0
        torch.cuda.synchronize(dev)
        for ln in lanes:
            got = ln["acc"].cpu().numpy()
            assert np.array_equal(got, ln["expect"]), (got.tolist(), ln["expect"].tolist())
            st = nat.tpke_level_kernel_stats(ln["ctx"])
            assert st[0] + st[1] >= 1 and 1 <= st[3] <= 2, st        # (which form either call saw is timing)
        assert one(lanes[0], n_cts=1 << 32) == -1                     # refused before anything is launched
        assert nat.batched_inflight(0) == 0
    finally:
        torch.cuda.synchronize(dev)
        for ln in lanes:
            ln["ctx"].close()
