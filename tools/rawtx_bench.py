#!/usr/bin/env python3
"""Throughput of the raw-transaction ingress (k_rawtx.hip) on one GPU, one process.

Workload (a) is tools/tx_hash_bench.py's: n transactions (default 2^20) with invocations of 0, 36 and 68 bytes in equal
thirds under 4,096 keys, signed on the GPU (new chain id), here encoded to the wire by the restatement
(tests/pyref/txhash.py).  Workload (b): the same with 1 % of the items carrying a 24 KB invocation.  Measured in one
session, each after 3 warm-up calls, median / min / max of 10 calls, HIP events on the stream the kernels run on:
  * lcb_raw_txs_ingest_dev, the whole call with every output, and its three phases (lcb_rawtx_phase_ms);
  * its decode-and-hash form (accept == NULL) against lcb_tx_hash_dev on the same transactions as fields;
  * lcb_receipts_verify_dev on the same transactions as fields, against the whole call;
  * a CPU leg for (a): the restatement's decode (tests/pyref/rawtx.py, pure Python) on 16 processes.  It is
    interpreter-bound, not a tuned implementation.
Expectations, reported and not adjusted: decode-and-hash <= 2 x lcb_tx_hash_dev; the whole call within a few per cent of
lcb_receipts_verify_dev.  Writes profiles/rawtx/<source_hash>.json (or --out) and prints the same JSON.
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
    """worker: the wire bytes of a slice of items"""
    from pyref import txhash as T
    recs, invs, sigs = job
    out = []
    for k in range(len(invs)):
        r = recs[REC * k:REC * k + REC]
        out.append(T.rlp_with_signature(int.from_bytes(r[0:8], "little"), int.from_bytes(r[8:16], "little"),
                                        int.from_bytes(r[16:24], "little"), r[56:76] if r[96] == 20 else b"", r[24:56],
                                        invs[k], sigs[L * k:L * k + L]))
    return out


def _decode(wires):
    """worker: the restatement's decode of a slice of items; the count it accepts"""
    from pyref import rawtx as W
    return sum(W.decode(w, NEW, CHAIN).status == W.OK for w in wires)


def note(*a):
    print(*a, file=sys.stderr, flush=True)


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

    def zeros(k):
        return torch.zeros(k, dtype=torch.uint8, device=dev)

    def workload(lens):
        """the transactions as fields (tools/tx_hash_bench.py's workload) and as wire bytes, on the device"""
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
        d = {"rec": up(recs.reshape(-1)), "inv": up(inv) if len(inv) else zeros(8), "off": up(off.view(np.int64)),
             "raw": zeros(32 * n), "full": zeros(32 * n)}
        assert lib.lcb_tx_hash_dev(d["raw"].data_ptr(), None, d["rec"].data_ptr(), d["inv"].data_ptr(), d["off"].data_ptr(),
                                   None, L, n, int(NEW), CHAIN, st.cuda_stream) == 0, lib.lcb_last_error()
        raw = d["raw"].cpu().numpy().tobytes()
        nonces = np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
        nonces[:, 0] &= 0x7f
        sigs, sok = nat.ecdsa_sign_hashed_batch(raw, privs[idx].tobytes(), nonces.tobytes(), NEW, CHAIN)
        assert sok == b"\x01" * n
        d["sig"] = up(np.frombuffer(sigs, dtype=np.uint8))
        addr, ok = zeros(20 * n), zeros(n)
        assert lib.lcb_ecdsa_recover_hashed_dev(None, addr.data_ptr(), ok.data_ptr(), d["raw"].data_ptr(), d["sig"].data_ptr(),
                                                L, n, int(NEW), CHAIN, st.cuda_stream) == 0, lib.lcb_last_error()
        torch.cuda.synchronize()
        assert bool((ok == 1).all())
        recs[:, 76:96] = addr.cpu().numpy().reshape(n, 20)
        d["rec"] = up(recs.reshape(-1))
        note("signed", n, "transactions; encoding to the wire")
        parts, jobs = 256, []
        blank = recs.copy()
        for p in range(parts):
            a, b = n * p // parts, n * (p + 1) // parts
            jobs.append((blank[a:b].tobytes(), [inv[int(off[k]):int(off[k + 1])].tobytes() for k in range(a, b)],
                         sigs[L * a:L * b]))
        wires = [w for part in pool.map(_encode, jobs) for w in part]
        woff = np.zeros(n + 1, dtype=np.uint64)
        woff[1:] = np.cumsum(np.fromiter((len(w) for w in wires), dtype=np.uint64, count=n))
        d["wire"] = up(np.frombuffer(b"".join(wires), dtype=np.uint8))
        d["woff"] = up(woff.view(np.int64))
        d["wire_bytes"] = int(woff[-1])
        d["wires"] = wires
        note("encoded", d["wire_bytes"], "wire bytes")
        return d

    def measure(d):
        acc, stt, det = zeros(n), zeros(n), zeros(n)
        txs, span, sigs, raw32, full32 = zeros(REC * n), zeros(16 * n), zeros(L * n), zeros(32 * n), zeros(32 * n)

        def ingest(with_accept):
            return lib.lcb_raw_txs_ingest_dev(acc.data_ptr() if with_accept else None, stt.data_ptr(), det.data_ptr(),
                                              txs.data_ptr(), span.data_ptr(), sigs.data_ptr(), raw32.data_ptr(),
                                              full32.data_ptr(), d["wire"].data_ptr(), d["woff"].data_ptr(), n, int(NEW),
                                              CHAIN, st.cuda_stream)

        dh_ms, _ = timed(lambda: ingest(False))
        assert bool((stt == 0).all()) and bool((det == 3).all())
        all_ms, all_ph = timed(lambda: ingest(True), nat.rawtx_phase_ms)
        assert bool((acc == 1).all()) and bool((det == 7).all())
        assert torch.equal(txs, d["rec"]) and torch.equal(sigs, d["sig"]), "decoded fields differ from the signed ones"
        hash_ms, _ = timed(lambda: lib.lcb_tx_hash_dev(d["raw"].data_ptr(), d["full"].data_ptr(), d["rec"].data_ptr(),
                                                       d["inv"].data_ptr(), d["off"].data_ptr(), d["sig"].data_ptr(), L, n,
                                                       int(NEW), CHAIN, st.cuda_stream))
        assert torch.equal(raw32, d["raw"]) and torch.equal(full32, d["full"]), "hashes differ from lcb_tx_hash_dev's"
        acc2, det2 = zeros(n), zeros(n)
        rv_ms, _ = timed(lambda: lib.lcb_receipts_verify_dev(acc2.data_ptr(), det2.data_ptr(), d["rec"].data_ptr(),
                                                             d["inv"].data_ptr(), d["off"].data_ptr(), d["sig"].data_ptr(),
                                                             L, d["full"].data_ptr(), n, int(NEW), CHAIN, st.cuda_stream))
        assert bool((acc2 == 1).all())
        ph = [med(p[k] for p in all_ph) for k in range(3)]
        r_dh, r_all = med(dh_ms) / med(hash_ms), med(all_ms) / med(rv_ms)
        return {"wire_bytes": d["wire_bytes"], "ingest_ms": stat(all_ms), "ingest_per_s": n / (med(all_ms) * 1e-3),
                "phase_ms": {"decode_and_hashing": ph[0], "recovery": ph[1], "finish": ph[2]},
                "decode_and_hash_form_ms": stat(dh_ms), "tx_hash_ms": stat(hash_ms), "decode_and_hash_over_tx_hash": r_dh,
                "expectation_decode_and_hash": "<= 2 x lcb_tx_hash_dev", "expectation_decode_and_hash_met": r_dh <= 2.0,
                "receipts_verify_ms": stat(rv_ms), "ingest_over_receipts_verify": r_all,
                "expectation_ingest": "within a few per cent of lcb_receipts_verify_dev"}

    lens_a = np.array([0, 36, 68], dtype=np.int64)[np.arange(n) % 3]
    da = workload(lens_a)
    res_a = measure(da)
    note("measured (a)")
    m = min(n, args.cpu_sample)
    parts = 64
    t0 = time.perf_counter()
    good = sum(pool.map(_decode, [da["wires"][m * p // parts:m * (p + 1) // parts] for p in range(parts)]))
    cpu_dt = time.perf_counter() - t0
    assert good == m
    del da
    torch.cuda.empty_cache()
    lens_b = lens_a.copy()
    lens_b[rng.choice(n, size=max(1, n // 100), replace=False)] = 24 * 1024
    db = workload(lens_b)
    pool.close()
    res_b = measure(db)
    res = {"tool": "tools/rawtx_bench.py", "source_hash": source_hash(), "device": torch.cuda.get_device_name(0),
           "n": n, "keys": nk, "warmup": args.warmup, "repeats": args.repeats, "a": res_a, "b": res_b,
           "b_over_a_decode_and_hash": res_b["decode_and_hash_form_ms"]["median"] / res_a["decode_and_hash_form_ms"]["median"],
           "cpu_decoded_per_s": m / cpu_dt, "cpu_processes": 16, "cpu_sample": m,
           "cpu_leg": "tests/pyref/rawtx.py's decode (pure Python, no hashing) on 16 processes: interpreter-bound, not a "
                      "tuned implementation"}
    out = args.out or os.path.join(ROOT, "profiles", "rawtx", res["source_hash"] + ".json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
