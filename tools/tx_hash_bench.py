#!/usr/bin/env python3
"""Throughput of device transaction hashing and receipt verification (k_txhash.hip) on one GPU, one process.

Workload (a): n receipts (default 2^20) with invocations of 0, 36 and 68 bytes in equal thirds under 4,096 keys, signed
on the GPU (new chain id).  Workload (b): the same with 1 % of the items carrying a 24 KB invocation (what lane
divergence costs).  Measured in one session, each after 3 warm-up calls, median / min / max of 10 calls, HIP events on
the stream the kernels run on:
  * lcb_tx_hash_dev alone (RawHash and FullHash from the fields);
  * lcb_receipts_verify_dev with its three kernel phases (lcb_tx_phase_ms);
  * for (a), what a caller could assemble without the fused kernel: lcb_keccak256_dev over the same 2 n messages,
    pre-encoded on the host by the restatement (tests/pyref/txhash.py), and lcb_tx_verify_dev on ready hashes;
  * a CPU leg: the restatement (pure Python RLP + the oracle's Keccak) on 16 processes.  It is interpreter-bound, not a
    tuned implementation.
The expectation for (a) is fused hashing <= 1.5 x the pre-encoded Keccak time; the tool reports the ratio and does not
adjust it.  Writes profiles/txhash/<source_hash>.json (or --out) and prints the same JSON.
"""
import argparse
import json
import multiprocessing
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHAIN, NEW, L = 225, True, 66
REC = 104


def _encode(job):
    """worker: the restatement's two RLPs (and, with hash=True, their hashes) of a slice of items"""
    from pyref import txhash as T
    recs, invs, sigs, do_hash = job
    out = []
    for k in range(len(invs)):
        r = recs[REC * k:REC * k + REC]
        tx = (int.from_bytes(r[0:8], "little"), int.from_bytes(r[8:16], "little"), int.from_bytes(r[16:24], "little"),
              r[56:76] if r[96] == 20 else b"", r[24:56], invs[k])
        sig = sigs[L * k:L * k + L]
        if do_hash:
            out.append(T.raw_hash(*tx, CHAIN) + T.full_hash(*tx, sig))
        else:
            out.append((T.rlp(*tx, CHAIN), T.rlp_with_signature(*tx, sig)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--cpu-sample", type=int, default=1 << 16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pool = multiprocessing.get_context("fork").Pool(16)       # forked before the GPU is opened: CPU work only
    import numpy as np
    import torch
    import oracle as o
    from bench import source_hash
    from lachain_amd import native as nat
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    lib = nat.lib()
    n, nk = args.n, args.keys
    rng = np.random.default_rng(20240801)
    N = o.SECP_N
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    med = statistics.median

    def stat(ms):
        return {"median": med(ms), "min": min(ms), "max": max(ms)}

    def timed(call, phases=None):
        ms, ph = [], []
        for k in range(args.warmup + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            rc = call()
            e1.record(st)
            e1.synchronize()
            if rc != 0:
                raise SystemExit("call failed: " + lib.lcb_last_error().decode())
            if k >= args.warmup:
                ms.append(e0.elapsed_time(e1))
                if phases:
                    ph.append(phases())
        return ms, ph

    privs = np.frombuffer(b"".join((int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1).to_bytes(32, "big")
                                   for _ in range(nk)), dtype=np.uint8).reshape(nk, 32)
    idx = rng.integers(0, nk, size=n)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def workload(lens):
        """records, invocations, offsets, signatures, claimed hashes on the device; From = the signer's address"""
        recs = np.zeros((n, REC), dtype=np.uint8)
        recs[:, 0:8] = np.arange(n, dtype="<u8").view(np.uint8).reshape(n, 8)                    # nonce
        recs[:, 8:16] = np.full(n, 1, dtype="<u8").view(np.uint8).reshape(n, 8)                  # gas price
        recs[:, 16:24] = rng.integers(21000, 10 ** 8, size=n).astype("<u8").view(np.uint8).reshape(n, 8)
        recs[:, 47:56] = np.frombuffer(rng.bytes(9 * n), dtype=np.uint8).reshape(n, 9)            # a 72-bit value
        recs[:, 56:76] = np.frombuffer(rng.bytes(20 * n), dtype=np.uint8).reshape(n, 20)          # To
        recs[:, 96] = 20
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens.astype(np.uint64))
        inv = np.frombuffer(rng.bytes(int(off[-1])), dtype=np.uint8)
        d = {"rec": up(recs.reshape(-1)), "inv": up(inv) if len(inv) else torch.zeros(8, dtype=torch.uint8, device=dev),
             "off": up(off.view(np.int64)), "raw": torch.zeros(32 * n, dtype=torch.uint8, device=dev),
             "full": torch.zeros(32 * n, dtype=torch.uint8, device=dev)}
        assert lib.lcb_tx_hash_dev(d["raw"].data_ptr(), None, d["rec"].data_ptr(), d["inv"].data_ptr(), d["off"].data_ptr(),
                                   None, L, n, int(NEW), CHAIN, st.cuda_stream) == 0, lib.lcb_last_error()
        raw = d["raw"].cpu().numpy().tobytes()
        nonces = np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
        nonces[:, 0] &= 0x7f
        sigs, sok = nat.ecdsa_sign_hashed_batch(raw, privs[idx].tobytes(), nonces.tobytes(), NEW, CHAIN)
        assert sok == b"\x01" * n
        d["sig"] = up(np.frombuffer(sigs, dtype=np.uint8))
        addr = torch.zeros(20 * n, dtype=torch.uint8, device=dev)
        ok = torch.zeros(n, dtype=torch.uint8, device=dev)
        assert lib.lcb_ecdsa_recover_hashed_dev(None, addr.data_ptr(), ok.data_ptr(), d["raw"].data_ptr(), d["sig"].data_ptr(),
                                                L, n, int(NEW), CHAIN, st.cuda_stream) == 0, lib.lcb_last_error()
        torch.cuda.synchronize()
        assert bool((ok == 1).all())
        recs[:, 76:96] = addr.cpu().numpy().reshape(n, 20)
        d["rec"] = up(recs.reshape(-1))
        d["addr"] = addr
        d["host"] = (recs, inv, off, sigs)
        return d

    def measure(d):
        acc = torch.zeros(n, dtype=torch.uint8, device=dev)
        det = torch.zeros(n, dtype=torch.uint8, device=dev)
        hash_ms, _ = timed(lambda: lib.lcb_tx_hash_dev(d["raw"].data_ptr(), d["full"].data_ptr(), d["rec"].data_ptr(),
                                                       d["inv"].data_ptr(), d["off"].data_ptr(), d["sig"].data_ptr(), L, n,
                                                       int(NEW), CHAIN, st.cuda_stream))
        rv_ms, rv_ph = timed(lambda: lib.lcb_receipts_verify_dev(acc.data_ptr(), det.data_ptr(), d["rec"].data_ptr(),
                                                                 d["inv"].data_ptr(), d["off"].data_ptr(), d["sig"].data_ptr(),
                                                                 L, d["full"].data_ptr(), n, int(NEW), CHAIN, st.cuda_stream),
                             nat.tx_phase_ms)
        assert bool((acc == 1).all()) and bool((det == 7).all())
        ph = [med(p[k] for p in rv_ph) for k in range(3)]
        return {"tx_hash_ms": stat(hash_ms), "tx_hash_per_s": n / (med(hash_ms) * 1e-3),
                "receipts_verify_ms": stat(rv_ms), "receipts_verify_per_s": n / (med(rv_ms) * 1e-3),
                "phase_ms": {"hashing": ph[0], "recovery": ph[1], "roots": ph[2]}}

    def slices(d, m, do_hash, parts=64):
        recs, inv, off, sigs = d["host"]
        jobs = []
        for p in range(parts):
            a, b = m * p // parts, m * (p + 1) // parts
            jobs.append((recs[a:b].tobytes(), [inv[int(off[k]):int(off[k + 1])].tobytes() for k in range(a, b)],
                         sigs[L * a:L * b], do_hash))
        return jobs

    # ---- workload (a)
    lens_a = np.array([0, 36, 68], dtype=np.int64)[np.arange(n) % 3]
    da = workload(lens_a)
    res_a = measure(da)
    enc = [e for part in pool.map(_encode, slices(da, n, False)) for e in part]
    msgs = [m for pair in enc for m in pair]                                     # raw, full, raw, full, ...
    moff = np.zeros(2 * n + 1, dtype=np.uint64)
    moff[1:] = np.cumsum(np.fromiter((len(m) for m in msgs), dtype=np.uint64, count=2 * n))
    dmsg = up(np.frombuffer(b"".join(msgs), dtype=np.uint8))
    dmoff = up(moff.view(np.int64))
    dout = torch.zeros(64 * n, dtype=torch.uint8, device=dev)
    kec_ms, _ = timed(lambda: lib.lcb_keccak256_dev(dout.data_ptr(), dmsg.data_ptr(), dmoff.data_ptr(), 2 * n, st.cuda_stream))
    both = dout.cpu().numpy().reshape(n, 2, 32)
    assert np.array_equal(both[:, 0].reshape(-1), da["raw"].cpu().numpy()), "fused RawHash differs from Keccak of the RLP"
    assert np.array_equal(both[:, 1].reshape(-1), da["full"].cpu().numpy()), "fused FullHash differs from Keccak of the RLP"
    acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    txv_ms, _ = timed(lambda: lib.lcb_tx_verify_dev(acc.data_ptr(), da["raw"].data_ptr(), da["sig"].data_ptr(), L,
                                                    da["addr"].data_ptr(), n, int(NEW), CHAIN, st.cuda_stream))
    assert bool((acc == 1).all())
    ratio = res_a["tx_hash_ms"]["median"] / med(kec_ms)
    res_a.update({"keccak256_preencoded_ms": stat(kec_ms), "preencoded_bytes": int(moff[-1]),
                  "fused_over_preencoded": ratio, "expectation": "fused <= 1.5 x pre-encoded Keccak",
                  "expectation_met": ratio <= 1.5, "tx_verify_ready_hashes_ms": stat(txv_ms)})
    # ---- the CPU leg: the restatement's two hashes per item, 16 processes
    m = min(n, args.cpu_sample)
    t0 = time.perf_counter()
    cpu = [e for part in pool.map(_encode, slices(da, m, True)) for e in part]
    cpu_dt = time.perf_counter() - t0
    assert b"".join(c[:32] for c in cpu) == da["raw"].cpu().numpy().tobytes()[:32 * m]
    pool.close()
    del da, dmsg, dout, enc, msgs
    torch.cuda.empty_cache()
    # ---- workload (b)
    lens_b = lens_a.copy()
    lens_b[rng.choice(n, size=max(1, n // 100), replace=False)] = 24 * 1024
    db = workload(lens_b)
    res_b = measure(db)
    res_b["invocation_bytes"] = int(lens_b.sum())
    res = {"tool": "tools/tx_hash_bench.py", "source_hash": source_hash(), "device": torch.cuda.get_device_name(0),
           "n": n, "keys": nk, "warmup": args.warmup, "repeats": args.repeats, "a": res_a, "b": res_b,
           "b_over_a_tx_hash": res_b["tx_hash_ms"]["median"] / res_a["tx_hash_ms"]["median"],
           "cpu_receipts_hashed_per_s": m / cpu_dt, "cpu_processes": 16, "cpu_sample": m,
           "cpu_leg": "tests/pyref/txhash.py (pure Python RLP, the oracle's Keccak) on 16 processes: interpreter-bound, "
                      "not a tuned implementation"}
    out = args.out or os.path.join(ROOT, "profiles", "txhash", res["source_hash"] + ".json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
