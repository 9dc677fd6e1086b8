#!/usr/bin/env python3
"""Throughput of batched secp256k1 public-key recovery (k_secp_recover.hip) on one GPU.

Inputs: n signatures (default 2^20) of random hashes by 4,096 random keys, signed on the GPU
(lcb_ecdsa_sign_hashed_batch, new chain id).  Measured in one session, each after warm-up, median of the repeats, HIP
events on the stream the kernels run on:
  * lcb_ecdsa_recover_hashed_dev (key + address) with its three kernel phases (lcb_ecdsa_recover_phase_ms);
  * lcb_tx_verify_dev (recover, address, compare with From);
  * lcb_ecdsa_verify_hashed_dev on the same signatures against the 4,096 keys' resident comb tables;
  * a CPU leg: o.ecdsa_recover (the oracle, libsecp256k1 semantics) over 16 threads for at least 2 s.
Field products per recovery are counted by the host emulation (tools/emul/secp_recover_emul.cpp) on a sample of the
same inputs; the recovery kernel's fraction of the INT32 peak is products x 72 MAC x rate / 3.93e13, the way DESIGN.md
prices k_secp_verify.  Writes profiles/ecdsa_recover/<source_hash>.json (or --out) and prints the same JSON.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

MAC_PER_PRODUCT = 72
INT32_PEAK = 3.93e13
CHAIN, NEW, L = 225, True, 66


def product_count(hashes, sigs, m):
    src = os.path.join(ROOT, "tools", "emul", "secp_recover_emul.cpp")
    lib_path = os.path.join(ROOT, "tools", "emul", "libsecp_recover_emul.so")
    if not os.path.exists(lib_path) or os.path.getmtime(lib_path) < os.path.getmtime(src):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", lib_path, src], check=True)
    emu = ctypes.CDLL(lib_path)
    emu.emu_recover.restype = ctypes.c_ulonglong
    pub, addr, ok = (ctypes.create_string_buffer(k * m) for k in (33, 20, 1))
    p3 = (ctypes.c_ulonglong * 3)()
    emu.emu_recover(pub, addr, ok, None, hashes[:32 * m], sigs[:L * m], L, None, m, 0, int(NEW), CHAIN, p3)
    assert ok.raw == b"\x01" * m
    return [p / m for p in p3]


def cpu_leg(o, hashes, sigs, n, threads=16, seconds=2.0):
    lib = o.lib()
    f = lib.orc_ecdsa_recover
    f.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    counts = [0] * threads
    stop = time.perf_counter() + seconds

    def work(t):
        out = ctypes.create_string_buffer(33)
        i, done = t, 0
        while time.perf_counter() < stop or done == 0:
            v = int.from_bytes(sigs[L * i + 64:L * i + 66], "big")
            rec = (v - 36) // 2 // CHAIN
            assert f(out, hashes[32 * i:32 * i + 32], sigs[L * i:L * i + 64], rec) == 0
            done += 1
            i = (i + threads) % n
        counts[t] = done

    t0 = time.perf_counter()
    ts = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    return sum(counts) / dt, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import oracle as o
    from bench import source_hash
    from lachain_amd import native as nat
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    lib = nat.lib()
    n, nk = args.n, args.keys
    rng = np.random.default_rng(20240601)
    N = o.SECP_N

    def scalars(m):
        return b"".join((int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1).to_bytes(32, "big") for _ in range(m))

    privs = np.frombuffer(scalars(nk), dtype=np.uint8).reshape(nk, 32)
    keys, kok = nat.ecdsa_pubkey_batch(privs.tobytes())
    assert kok == b"\x01" * nk
    idx = rng.integers(0, nk, size=n).astype(np.int32)
    hashes = rng.bytes(32 * n)
    nonces = np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    nonces[:, 0] &= 0x7f                                   # below n, and nonzero with overwhelming probability
    sigs, sok = nat.ecdsa_sign_hashed_batch(hashes, privs[idx].tobytes(), nonces.tobytes(), NEW, CHAIN)
    assert sok == b"\x01" * n
    want_keys = np.frombuffer(keys, dtype=np.uint8).reshape(nk, 33)[idx]

    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    dh = torch.frombuffer(bytearray(hashes), dtype=torch.uint8).to(dev)
    ds = torch.frombuffer(bytearray(sigs), dtype=torch.uint8).to(dev)
    di = torch.from_numpy(idx).to(dev)
    pub = torch.zeros(33 * n, dtype=torch.uint8, device=dev)
    addr = torch.zeros(20 * n, dtype=torch.uint8, device=dev)
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    acc = torch.zeros(n, dtype=torch.uint8, device=dev)

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

    rec_ms, rec_ph = timed(lambda: lib.lcb_ecdsa_recover_hashed_dev(pub.data_ptr(), addr.data_ptr(), ok.data_ptr(),
                                                                     dh.data_ptr(), ds.data_ptr(), L, n, int(NEW), CHAIN,
                                                                     st.cuda_stream), nat.ecdsa_recover_phase_ms)
    assert bool((ok == 1).all())
    assert np.array_equal(pub.cpu().numpy().reshape(n, 33), want_keys), "recovered keys differ from the signers'"
    tx_ms, _ = timed(lambda: lib.lcb_tx_verify_dev(acc.data_ptr(), dh.data_ptr(), ds.data_ptr(), L, addr.data_ptr(), n,
                                                   int(NEW), CHAIN, st.cuda_stream))
    assert bool((acc == 1).all())
    ks = nat.EcdsaKeySet(keys, 33)
    try:
        ver_ms, _ = timed(lambda: lib.lcb_ecdsa_verify_hashed_dev(acc.data_ptr(), dh.data_ptr(), ds.data_ptr(), L,
                                                                  di.data_ptr(), n, ks.h, int(NEW), CHAIN,
                                                                  st.cuda_stream))
        assert bool((acc == 1).all())
    finally:
        ks.close()
    sample = min(n, 4096)                                 # a whole block of finish threads (16 points each)
    prod = product_count(hashes, sigs, sample)
    cpu_rate, cpu_dt = cpu_leg(o, hashes, sigs, n)

    med = statistics.median
    phases = [med(p[k] for p in rec_ph) for k in range(3)]
    rate = n / (med(rec_ms) * 1e-3)
    kernel_rate = n / (phases[1] * 1e-3)
    ver_rate = n / (med(ver_ms) * 1e-3)
    res = {
        "tool": "tools/ecdsa_recover_bench.py", "source_hash": source_hash(), "device": torch.cuda.get_device_name(0),
        "n": n, "keys": nk, "warmup": args.warmup, "repeats": args.repeats,
        "recover_per_s": rate, "recover_ms": {"median": med(rec_ms), "min": min(rec_ms), "max": max(rec_ms)},
        "phase_ms": {"scalars": phases[0], "recovery": phases[1], "finish": phases[2]},
        "tx_verify_per_s": n / (med(tx_ms) * 1e-3), "tx_verify_ms": {"median": med(tx_ms), "min": min(tx_ms), "max": max(tx_ms)},
        "verify_hashed_per_s": ver_rate, "verify_hashed_ms": {"median": med(ver_ms), "min": min(ver_ms), "max": max(ver_ms)},
        "recover_over_verify": rate / ver_rate,
        "field_products_per_recovery": {"scalars": prod[0], "recovery": prod[1], "finish": prod[2], "sample": sample},
        "recovery_kernel_int32_fraction": kernel_rate * prod[1] * MAC_PER_PRODUCT / INT32_PEAK,
        "mac_per_product": MAC_PER_PRODUCT, "int32_peak_mac_per_s": INT32_PEAK,
        "cpu_recover_per_s": cpu_rate, "cpu_threads": 16, "cpu_seconds": cpu_dt,
        "cpu_leg": "o.ecdsa_recover (oracle/secp.c) on the same inputs, 16 threads",
        "gpu_over_cpu": rate / cpu_rate,
    }
    assert rate > cpu_rate, "the GPU path must beat the 16-thread CPU leg"
    out = args.out or os.path.join(ROOT, "profiles", "ecdsa_recover", res["source_hash"] + ".json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
