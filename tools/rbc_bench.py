#!/usr/bin/env python3
"""The reliable broadcast's byte work for one era at N = 256, F = 85 on one GPU (k_rbc.hip, batched k_rs.hip).

Workload: B = 256 RBC instances of a 180-byte payload and of a 64 KiB payload.  Measured in one process and one
session, each figure after 3 warm-up calls, median / min / max of at least 10 timed calls:
  * echo checks per second: all 65,536 (instance, shard) echoes through lcb_rbc_check_echo_dev, HIP events on the
    stream the kernel runs on;
  * lcb_rbc_val_batch and lcb_rbc_decode_batch, wall milliseconds per 256 instances (host pointers in and out), and
    beside each the same work put together from the single-instance entry points: 256 lcb_rs_encode / lcb_rs_decode
    calls, one lcb_keccak256_batch over the leaves, tree and proofs on the host with o.keccak256;
  * a CPU leg: the plain-Python echo check (tests/pyref/rbc_merkle.py over o.keccak256) on 16 threads, same items;
  * the echo kernel's roofline: Keccak permutations per second x VALU instructions per permutation (counted in the
    disassembly of the library that ran: the round loop's body x 24) over the VALU issue rate (one wave64 instruction
    per 2 cycles per SIMD, 4 SIMDs x 256 CUs at 2.4 GHz).  Keccak is bitwise work; the INT32-MAC peak does not apply.
Writes profiles/rbc/<source_hash>.json (or --out) and prints the same JSON.
"""
import argparse
import glob
import json
import os
import random
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, F = 256, 85
K = N - 2 * F
B = 256
VALU_WAVE_INSTR_PER_S = 256 * 4 * 2.4e9 / 2
LLVM = "/opt/rocm/lib/llvm/bin"


def valu_per_permutation(so_path):
    """VALU instructions of one Keccak-f[1600] in k_rbc_echo: its round loops are counted by a scalar register stepping
    8 bytes through the 24 round constants, one round per trip; returns (per round, per permutation, loops found)"""
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "lib.so")
        shutil.copy(so_path, so)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=td, check=True, capture_output=True)
        text = ""
        for co in sorted(glob.glob(os.path.join(td, "lib.so.*gfx950"))):
            out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--disassemble-symbols=k_rbc_echo", co],
                                 capture_output=True, text=True).stdout
            if "\tv_" in out:
                text = out
    ins = []
    for line in text.splitlines():
        m = re.match(r"\s+(\S+)\s.*//\s*([0-9A-F]+):", line)
        if m:
            ins.append((int(m.group(2), 16), m.group(1), line))
    if not ins:
        raise SystemExit("k_rbc_echo not found in " + so_path)
    at = {a: i for i, (a, _, _) in enumerate(ins)}
    rounds = []
    for i, (a, op, line) in enumerate(ins):
        m = re.search(r"<k_rbc_echo\+0x([0-9a-f]+)>", line)
        if op != "s_cbranch_scc1" or not m:
            continue
        target = ins[0][0] + int(m.group(1), 16)
        if target > a:
            continue
        body = ins[at[target]:i + 1]
        if any(b[1] == "s_cmpk_lg_i32" and "0xc0" in b[2] for b in body):      # 24 constants x 8 bytes
            rounds.append(sum(1 for b in body if b[1].startswith("v_")))
    if not rounds:
        raise SystemExit("no 24-trip round loop found in k_rbc_echo's disassembly")
    return max(rounds), 24 * max(rounds), len(rounds)


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import oracle as o
    from bench import source_hash
    from lachain_amd import native as nat
    from pyref import rbc_merkle as R
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    if args.repeats < 10 or args.warmup < 3:
        raise SystemExit("at least 3 warm-up and 10 timed calls")
    lib = nat.lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    depth = nat.rbc_tree_depth(N)
    T = 1 << depth

    def wall(call):
        ms = []
        for k in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            r = call()
            dt = (time.perf_counter() - t0) * 1e3
            if k >= args.warmup:
                ms.append(dt)
        return ms, r

    def host_tree(leaves):
        nodes = [bytes(32)] * T + [leaves[32 * i:32 * i + 32] for i in range(N)] + [bytes(32)] * (T - N)
        for i in range(T - 1, 0, -1):
            nodes[i] = o.keccak256(nodes[2 * i] + nodes[2 * i + 1])
        return nodes

    def composed_val(payloads, S):
        """the single-instance entry points: encode per instance, one flat Keccak over all leaves, host trees / proofs"""
        shards = [nat.rs_encode(R.augment(p, N, F), N, 2 * F) for p in payloads]
        leaves = nat.keccak256_batch([sh[i * S:(i + 1) * S] for sh in shards for i in range(N)])
        roots, proofs = [], []
        for b in range(B):
            nodes = host_tree(leaves[32 * N * b:32 * N * (b + 1)])
            roots.append(nodes[1])
            proofs.append(b"".join(b"".join(R.branch(nodes, i)) for i in range(N)))
        return b"".join(shards), b"".join(roots), b"".join(proofs)

    def composed_decode(echos, S):
        shards = [nat.rs_decode(e, S, N, 2 * F) for e in echos]
        leaves = nat.keccak256_batch([sh[i * S:(i + 1) * S] for sh in shards for i in range(N)])
        roots = [host_tree(leaves[32 * N * b:32 * N * (b + 1)])[1] for b in range(B)]
        return b"".join(shards), b"".join(roots)

    res = {"tool": "tools/rbc_bench.py", "source_hash": source_hash(), "device": torch.cuda.get_device_name(0),
           "n": N, "f": F, "instances": B, "warmup": args.warmup, "repeats": args.repeats, "workloads": {}}
    per_round, per_perm, loops = valu_per_permutation(nat.LIB_PATH)
    res["echo_kernel_isa"] = {"valu_per_round": per_round, "valu_per_permutation": per_perm, "round_loops": loops,
                              "valu_wave_instr_per_s": VALU_WAVE_INSTR_PER_S}
    rng = random.Random(20241019)
    for name, plen in (("payload_180", 180), ("payload_64KiB", 65536)):
        payloads = [rng.randbytes(plen) for _ in range(B)]
        S = nat.rbc_shard_size(plen, N, F)
        val_ms, (shards, roots, proofs) = wall(lambda: nat.rbc_val_batch(payloads, N, F))
        cval_ms, cval = wall(lambda: composed_val(payloads, S))
        assert cval == (shards, roots, proofs), "val_batch differs from the composed single-instance calls"
        # decode: N - 2F echoes per instance, shard 0 always kept (two erased shards 0 and 255 share an evaluation point)
        echos = []
        for b in range(B):
            keep = [0] + rng.sample(range(1, N), K - 1)
            rng.shuffle(keep)
            echos.append([(j, shards[(b * N + j) * S:(b * N + j + 1) * S]) for j in keep])
        flat = b"".join(d for e in echos for _, d in e)
        off = [b * K * S for b in range(B + 1)]
        frm = [j for e in echos for j, _ in e]
        dec_ms, dec = wall(lambda: nat.rbc_decode_batch(flat, off, frm, roots, N, F))
        assert dec == (shards, b"\x01" * B, b"\x01" * B, roots), "decode_batch did not restore the shards and roots"
        cdec_ms, cdec = wall(lambda: composed_decode(echos, S))
        assert cdec == (shards, roots)
        # echo checks: every (instance, shard) of the era, device pointers
        n_items = B * N
        dd = torch.frombuffer(bytearray(shards), dtype=torch.uint8).to(dev)
        dr = torch.from_numpy(np.repeat(np.frombuffer(roots, dtype=np.uint8).reshape(B, 32), N, axis=0).copy()).to(dev)
        dp = torch.frombuffer(bytearray(proofs), dtype=torch.uint8).to(dev)
        ddo = torch.arange(0, (n_items + 1) * S, S, dtype=torch.int64, device=dev)
        dpo = torch.arange(0, (n_items + 1) * depth, depth, dtype=torch.int64, device=dev)
        dfr = torch.from_numpy(np.tile(np.arange(N, dtype=np.int32), B)).to(dev)
        acc = torch.zeros(n_items, dtype=torch.uint8, device=dev)
        echo_ms = []
        for k in range(args.warmup + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            rc = lib.lcb_rbc_check_echo_dev(acc.data_ptr(), dd.data_ptr(), ddo.data_ptr(), dfr.data_ptr(), dr.data_ptr(),
                                            dp.data_ptr(), dpo.data_ptr(), n_items, N, st.cuda_stream)
            e1.record(st)
            e1.synchronize()
            if rc != 0:
                raise SystemExit("call failed: " + lib.lcb_last_error().decode())
            if k >= args.warmup:
                echo_ms.append(e0.elapsed_time(e1))
        assert bool((acc == 1).all()), "an honest echo was rejected"
        # CPU leg: the plain-Python check on 16 threads over the same items for at least 2 s
        threads, counts = 16, [0] * 16
        stop = time.perf_counter() + 2.0

        def work(t):
            i, done = t, 0
            while time.perf_counter() < stop or done == 0:
                b, j = divmod(i, N)
                base = 32 * depth * i
                proof = [proofs[base + 32 * q:base + 32 * q + 32] for q in range(depth)]
                assert R.check_echo(shards[i * S:(i + 1) * S], j, roots[32 * b:32 * b + 32], proof, N)
                done += 1
                i = (i + threads) % n_items
            counts[t] = done

        t0 = time.perf_counter()
        ts = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        cpu_rate = sum(counts) / (time.perf_counter() - t0)
        med = statistics.median(echo_ms)
        perms = n_items * (S // 136 + 1 + depth)
        perm_rate = perms / (med * 1e-3)
        res["workloads"][name] = {
            "payload_bytes": plen, "shard_bytes": S,
            "echo_items": n_items, "echo_ms": stats(echo_ms), "echo_checks_per_s": n_items / (med * 1e-3),
            "echo_permutations_per_item": S // 136 + 1 + depth, "echo_permutations_per_s": perm_rate,
            "echo_valu_issue_fraction": perm_rate * per_perm / 64 / VALU_WAVE_INSTR_PER_S,
            "cpu_echo_checks_per_s": cpu_rate, "cpu_threads": threads,
            "cpu_leg": "tests/pyref/rbc_merkle.py check_echo over o.keccak256, Python threads",
            "val_batch_ms": stats(val_ms), "val_composed_ms": stats(cval_ms),
            "val_composed_over_batch": statistics.median(cval_ms) / statistics.median(val_ms),
            "decode_batch_ms": stats(dec_ms), "decode_composed_ms": stats(cdec_ms),
            "decode_composed_over_batch": statistics.median(cdec_ms) / statistics.median(dec_ms),
        }
    res["composed"] = ("256 lcb_rs_encode / lcb_rs_decode calls, one lcb_keccak256_batch over the 65,536 leaves, tree and "
                       "proofs on the host with o.keccak256")
    out = args.out or os.path.join(ROOT, "profiles", "rbc", res["source_hash"] + ".json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
