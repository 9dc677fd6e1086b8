#!/usr/bin/env python3
"""The state-trie layer on one GPU (k_trie.hip): flat checks, roots from key/value sets, the deferred commit.

Measured in one process and one session, each device figure after 3 warm-up calls, median / min / max of at least 10
timed calls (HIP events on the stream the kernels run on); the host-driven and CPU legs are interpreter-bound, take
seconds per call and are timed over --host-repeats calls after one warm-up, which the record says:
  (i)   the flat consistency check (lcb_trie_node_hash_dev with expected hashes) over 2^20 nodes of a fast-sync-like
        mix, 31 leaves with 32-byte values per 32-child internal node, with its internal nodes in a launch of their own
        (the default) and in one mixed launch (LCB_TRIE_MIXED=1), against lcb_keccak256_dev over the same messages
        assembled beforehand; Keccak permutations per second as a fraction of the vector issue rate (one wave64
        instruction per 2 cycles per SIMD, 4 SIMDs x 256 CUs at 2.4 GHz), the VALU count of a permutation read from the
        disassembly of the library that ran;
  (ii)  lcb_trie_root_dev over 2^20 keys and over a six-trie state of about 2^20 keys, against what a caller could
        assemble before this layer: the same construction on the host, one lcb_keccak256_batch call per depth; and a
        CPU leg: the restatement's canonical build (tests/pyref/trie.py over o.keccak256) on 16 processes;
  (iii) the deferred commit: 2^16 updates into a 2^20-key trie through the mirror (lachain_amd/trie.py) with one rehash
        call, against the eagerly hashing restatement doing the same updates.
Writes profiles/trie/<source_hash>.json (or --out) and prints the same JSON.
"""
import argparse
import glob
import json
import multiprocessing
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

VALU_WAVE_INSTR_PER_S = 256 * 4 * 2.4e9 / 2
LLVM = "/opt/rocm/lib/llvm/bin"
STATE_SIZES = (1 << 17, 1 << 10, 1 << 19, 1 << 18, 1 << 17, 22)    # Balances, Contracts, Storage, Transactions, Events, Validators


def valu_per_permutation(so_path, kernel):
    """VALU instructions of one Keccak-f[1600] in `kernel`: its round loop is a backward branch whose body steps through
    the 24 round constants (the innermost such loop: the block loop around it holds the same compare); returns
    (per round, per permutation) or None when no such loop is found"""
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "lib.so")
        shutil.copy(so_path, so)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=td, check=True, capture_output=True)
        text = ""
        for co in sorted(glob.glob(os.path.join(td, "lib.so.*gfx950"))):
            out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--disassemble-symbols=" + kernel, co],
                                 capture_output=True, text=True).stdout
            if "\tv_" in out:
                text = out
    ins = []
    for line in text.splitlines():
        m = re.match(r"\s+(\S+)\s.*//\s*([0-9A-F]+):", line)
        if m:
            ins.append((int(m.group(2), 16), m.group(1), line))
    if not ins:
        return None
    at = {a: i for i, (a, _, _) in enumerate(ins)}
    rounds = []
    for i, (a, op, line) in enumerate(ins):
        m = re.search(r"<%s\+0x([0-9a-f]+)>" % re.escape(kernel), line)
        if not op.startswith("s_cbranch") or not m:
            continue
        target = ins[0][0] + int(m.group(1), 16)
        if target > a or target not in at:
            continue
        body = ins[at[target]:i + 1]
        if any(b[1] == "s_cmpk_lg_i32" and "0xc0" in b[2] for b in body):      # 24 constants x 8 bytes
            rounds.append(sum(1 for b in body if b[1].startswith("v_")))
    if not rounds:
        return None
    return min(rounds), 24 * min(rounds)


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "calls": len(ms)}


def path_keys(np, kh):
    """(n, 32) uint8 key hashes -> (n, 32) uint8 path keys, big-endian: fragments 0 .. 50 most significant bit first,
    then bit 255"""
    bits = np.unpackbits(kh, axis=1, bitorder="little")
    frag = bits[:, :255].reshape(-1, 51, 5)[:, :, ::-1].reshape(-1, 255)
    return np.packbits(np.concatenate([frag, bits[:, 255:]], axis=1), axis=1, bitorder="big")


def host_driven_roots(np, nat, kh, values, trie_of, n_tries, clock):
    """what a caller could assemble before this layer: sort and prefix lengths on the host (numpy), then the canonical
    trie bottom-up with one lcb_keccak256_batch call for the leaves and one per depth.  clock[0] collects the seconds
    spent inside the library."""
    n = len(values)
    roots = [bytes(32)] * n_tries
    if not n:
        return roots
    pk = path_keys(np, kh)
    order = np.lexsort([pk.view("S32").ravel(), trie_of])
    pk, tr = pk[order], trie_of[order]
    x = np.unpackbits(pk[1:] ^ pk[:-1], axis=1)
    lcp = np.where(x.any(axis=1), x.argmax(axis=1) // 5, 51)
    lcp = np.concatenate([[-1], np.where(tr[1:] == tr[:-1], lcp, -1)]).tolist()
    t0 = time.perf_counter()
    lh = nat.keccak256_batch([b"\x20\0\0\0" + bytes(kh[i]) + values[i] for i in order.tolist()])
    clock[0] += time.perf_counter() - t0
    pkint = [int.from_bytes(bytes(p), "big") for p in pk]
    entries = [(lh[32 * s:32 * s + 32], s, False, lcp[s]) for s in range(n)]        # hash, first key, internal, boundary
    for d in range(max(lcp), -1, -1):
        groups, msgs = [], []
        for e in entries:
            if e[3] == d:
                groups[-1].append(e)
            else:
                groups.append([e])
        for g in groups:
            if len(g) >= 2 or g[0][2]:
                msgs.append(b"".join(bytes([(pkint[e[1]] >> (251 - 5 * d)) & 31]) + e[0] for e in g))
        t0 = time.perf_counter()
        hs = nat.keccak256_batch(msgs) if msgs else b""
        clock[0] += time.perf_counter() - t0
        entries, k = [], 0
        for g in groups:
            if len(g) >= 2 or g[0][2]:
                entries.append((hs[32 * k:32 * k + 32], g[0][1], True, g[0][3]))
                k += 1
            else:
                entries.append(g[0])
    for h, s, _, _ in entries:
        roots[int(tr[s])] = h
    return roots


def cpu_subroot(arg):
    """one worker of the CPU leg: the restatement's canonical build of the keys under one label at depth 1"""
    from pyref import trie as R
    label, items = arg
    if len(items) == 1:
        return label, R.leaf_hash(*items[0])
    return label, R.canonical_root(items, 1)


def cpu_root(pool, items):
    from pyref import trie as R
    by = {}
    for k, v in items:
        by.setdefault(R.hash_fragment(k, 0), []).append((k, v))
    if len(items) < 2:
        return R.canonical_root(items)
    subs = dict(pool.map(cpu_subroot, sorted(by.items()), chunksize=1))
    labels = sorted(subs)
    return R.internal_hash(sum(1 << f for f in labels), [subs[f] for f in labels])


def build_canonical(trie, node_types, items, depth=0):
    """the canonical trie over items (key hash, value) as nodes of `trie`, each hashed once; returns the root id"""
    Leaf, Internal, fragment = node_types
    if len(items) == 1:
        return trie._new(Leaf(*items[0]))
    by = {}
    for kv in items:
        by.setdefault(fragment(kv[0], depth), []).append(kv)
    labels = sorted(by)
    kids = [build_canonical(trie, node_types, by[f], depth + 1) for f in labels]
    return trie._new(Internal(sum(1 << f for f in labels), kids, [trie.nodes[c].Hash for c in kids]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--log-nodes", type=int, default=20)
    ap.add_argument("--log-keys", type=int, default=20)
    ap.add_argument("--log-updates", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import source_hash
    from lachain_amd import native as nat
    from lachain_amd import trie as T
    from pyref import trie as R
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    if args.repeats < 10 or args.warmup < 3:
        raise SystemExit("at least 3 warm-up and 10 timed calls")
    lib = nat.lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    rng = np.random.default_rng(20241020)

    def timed(call, check=None):
        ms = []
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
        if check:
            check()
        return ms

    def wall(call, repeats):
        ms, r = [], None
        for k in range(1 + repeats):
            t0 = time.perf_counter()
            r = call()
            if k:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms, r

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    res = {"tool": "tools/trie_bench.py", "source_hash": source_hash(), "device": torch.cuda.get_device_name(0),
           "warmup": args.warmup, "repeats": args.repeats, "host_repeats": args.host_repeats,
           "valu_wave_instr_per_s": VALU_WAVE_INSTR_PER_S}
    isa = valu_per_permutation(nat.LIB_PATH, "k_trie_flat")
    isa_from = "k_trie_flat"
    if isa is None:
        isa, isa_from = valu_per_permutation(nat.LIB_PATH, "k_rbc_echo"), "k_rbc_echo (the same keccak_f1600)"
    res["isa"] = {"kernel": isa_from, "valu_per_round": isa and isa[0], "valu_per_permutation": isa and isa[1]}

    # ---------------------------------------------------------------- (i) the flat check
    n = 1 << args.log_nodes
    groups = n // 32
    leaves = rng.integers(0, 256, (groups, 31, 64), dtype=np.uint8)
    kids = rng.integers(0, 256, (groups, 32, 32), dtype=np.uint8)
    data = np.concatenate([leaves.reshape(groups, -1), kids.reshape(groups, -1)], axis=1).ravel()
    lens = np.tile(np.array([64] * 31 + [1024], dtype=np.int64), groups)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    recs = np.zeros((n, 4), dtype=np.uint32)
    recs[:, 2] = 32
    recs[31::32] = (1, 0xffffffff, 0, 0)
    # the same messages assembled beforehand: prefix || leaf bytes; label || child hash
    lmsg = np.concatenate([np.broadcast_to(np.array([32, 0, 0, 0], dtype=np.uint8), (groups, 31, 4)), leaves], axis=2)
    imsg = np.concatenate([np.broadcast_to(np.arange(32, dtype=np.uint8)[None, :, None], (groups, 32, 1)), kids], axis=2)
    msgs = np.concatenate([lmsg.reshape(groups, -1), imsg.reshape(groups, -1)], axis=1).ravel()
    moff = np.concatenate([[0], np.cumsum(np.tile(np.array([68] * 31 + [1056], dtype=np.int64), groups))]).astype(np.int64)
    d_data, d_off, d_recs, d_msgs, d_moff = to_dev(data), to_dev(off), to_dev(recs), to_dev(msgs), to_dev(moff)
    d_ref = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    d_acc = torch.zeros(n, dtype=torch.uint8, device=dev)
    pre_ms = timed(lambda: lib.lcb_keccak256_dev(d_ref.data_ptr(), d_msgs.data_ptr(), d_moff.data_ptr(), n, st.cuda_stream))
    sample = bytes(d_ref[:32 * 64].cpu().numpy())
    for i in (0, 30, 31, 63):
        m = bytes(msgs[moff[i]:moff[i + 1]])
        want = R.leaf_hash(m[4:36], m[36:]) if i % 32 != 31 else R.internal_hash(0xffffffff, [m[33 * j + 1:33 * j + 33] for j in range(32)])
        assert sample[32 * i:32 * i + 32] == want, "the assembled messages are not the nodes' messages"

    def flat_call():
        return lib.lcb_trie_node_hash_dev(d_out.data_ptr(), d_acc.data_ptr(), d_recs.data_ptr(), d_data.data_ptr(),
                                          d_off.data_ptr(), d_ref.data_ptr(), n, st.cuda_stream)

    def flat_check():
        assert bool((d_acc == 1).all()) and bool((d_out == d_ref).all()), "the flat check disagrees with Keccak of the messages"
        d_out.zero_()
        d_acc.zero_()

    os.environ.pop("LCB_TRIE_MIXED", None)
    split_ms = timed(flat_call, flat_check)
    os.environ["LCB_TRIE_MIXED"] = "1"
    mixed_ms = timed(flat_call, flat_check)
    os.environ.pop("LCB_TRIE_MIXED", None)
    perms = groups * (31 + 8)
    rate = lambda ms: perms / (statistics.median(ms) * 1e-3)
    frac = lambda ms: isa and rate(ms) * isa[1] / 64 / VALU_WAVE_INSTR_PER_S
    res["flat"] = {
        "nodes": n, "mix": "31 leaves (32-byte key hash, 32-byte value) per 32-child internal node", "permutations": perms,
        "split_launch_ms": stats(split_ms), "mixed_launch_ms": stats(mixed_ms), "preassembled_keccak_ms": stats(pre_ms),
        "split_over_preassembled": statistics.median(split_ms) / statistics.median(pre_ms),
        "mixed_over_split": statistics.median(mixed_ms) / statistics.median(split_ms),
        "nodes_per_s": n / (statistics.median(split_ms) * 1e-3),
        "permutations_per_s": {"split": rate(split_ms), "mixed": rate(mixed_ms), "preassembled": rate(pre_ms)},
        "valu_issue_fraction": {"split": frac(split_ms), "mixed": frac(mixed_ms), "preassembled": frac(pre_ms)},
        "against": "lcb_keccak256_dev over the same 2^20 messages assembled beforehand",
    }
    del d_data, d_msgs, d_ref, d_out, d_acc
    print("flat check done", file=sys.stderr, flush=True)

    # ---------------------------------------------------------------- (ii) roots from key/value sets
    pool = multiprocessing.get_context("spawn").Pool(16)
    res["roots"] = {}
    nk = 1 << args.log_keys
    shapes = {"one_trie": (nk,), "six_trie_state": tuple(max(1, s * nk >> 20) for s in STATE_SIZES)}
    for name, sizes in shapes.items():
        total = sum(sizes)
        kh = rng.integers(0, 256, (total, 32), dtype=np.uint8)
        val = rng.integers(0, 256, (total, 32), dtype=np.uint8)
        toff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        ioff = np.arange(0, 32 * (total + 1), 32, dtype=np.int64)
        d_k, d_v, d_io, d_to = to_dev(kh.ravel()), to_dev(val.ravel()), to_dev(ioff), to_dev(toff)
        B = len(sizes)
        d_roots = torch.zeros(32 * B, dtype=torch.uint8, device=dev)
        d_stat = torch.zeros(B, dtype=torch.uint8, device=dev)
        dev_ms = timed(lambda: lib.lcb_trie_root_dev(d_roots.data_ptr(), d_stat.data_ptr(), d_k.data_ptr(), d_io.data_ptr(),
                                                     d_v.data_ptr(), d_io.data_ptr(), d_to.data_ptr(), B, total, 1,
                                                     st.cuda_stream))
        got = bytes(d_roots.cpu().numpy())
        got = [got[32 * b:32 * b + 32] for b in range(B)]
        assert bytes(d_stat.cpu().numpy()) == b"\x01" * B
        values = [bytes(v) for v in val]
        trie_of = np.repeat(np.arange(B), sizes)
        clock = [0.0]
        host_ms, host_roots = wall(lambda: host_driven_roots(np, nat, kh, values, trie_of, B, clock), args.host_repeats)
        assert host_roots == got, "the device roots differ from the host-driven construction"
        items = [(bytes(k), v) for k, v in zip(kh, values)]
        cpu_ms, cpu_roots = wall(lambda: [cpu_root(pool, items[toff[b]:toff[b + 1]]) for b in range(B)], 1)
        assert cpu_roots == got, "the device roots differ from the restatement"
        res["roots"][name] = {
            "keys": total, "tries": list(sizes), "value_bytes": 32,
            "device_ms": stats(dev_ms), "keys_per_s": total / (statistics.median(dev_ms) * 1e-3),
            "host_driven_ms": stats(host_ms), "host_driven_library_ms_per_call": clock[0] * 1e3 / (1 + args.host_repeats),
            "host_driven_over_device": statistics.median(host_ms) / statistics.median(dev_ms),
            "cpu_restatement_ms": stats(cpu_ms), "cpu_processes": 16,
            "cpu_over_device": statistics.median(cpu_ms) / statistics.median(dev_ms),
        }
        if name == "six_trie_state":
            assert T.StateHash(got) == R.state_hash(got)
        print("roots done:", name, file=sys.stderr, flush=True)
    res["roots"]["host_driven"] = ("numpy sort and prefix lengths, the canonical trie bottom-up in Python, one "
                                   "lcb_keccak256_batch call for the leaves and one per depth; interpreter-bound")
    res["roots"]["cpu_leg"] = ("tests/pyref/trie.py canonical_root over o.keccak256, the 32 depth-1 subtrees on 16 "
                               "processes, one timed call; interpreter-bound")
    pool.close()
    pool.join()

    # ---------------------------------------------------------------- (iii) the deferred commit
    nk, nu = 1 << args.log_keys, 1 << args.log_updates
    kh = [bytes(k) for k in rng.integers(0, 256, (nk, 32), dtype=np.uint8)]
    items = [(k, bytes(8)) for k in kh]
    eager = R.TrieHashMap()
    root = build_canonical(eager, (lambda k, v: R.LeafNode(k, v), lambda m, c, h: R.InternalNode(m, c, h), R.hash_fragment), items)
    mirror = T.TrieHashMap()                               # the same nodes, hashes known: a clean trie
    mirror.version = eager.version
    for i, node in eager.nodes.items():
        mirror.nodes[i] = (T.LeafNode(node.KeyHash, node.Value, node.Hash) if node.Type == R.LEAF
                           else T.InternalNode(node.ChildrenMask, node.Children, node.Hash))
    picks = rng.choice(nk, nu, replace=False).tolist()
    updates = [(kh[i], int(j).to_bytes(8, "little")) for j, i in enumerate(picks, 1)]
    inside = [0.0]
    real_rehash = nat.trie_rehash_batch

    def clocked(*a):
        t0 = time.perf_counter()
        r = real_rehash(*a)
        inside[0] += time.perf_counter() - t0
        return r
    nat.trie_rehash_batch = clocked

    def deferred():
        r = root
        for k, v in updates:
            r = mirror.update_by_hash(r, k, v)
        return mirror.GetHash(r)

    def eagerly():
        r = root
        for k, v in updates:
            r = eager.update_by_hash(r, k, v)
        return eager.GetHash(r)

    # every call starts from the clean root, so each repeats the whole commit (old roots stay valid in both)
    def_ms, def_root = wall(deferred, args.host_repeats)
    nat.trie_rehash_batch = real_rehash
    eag_ms, eag_root = wall(eagerly, args.host_repeats)
    assert def_root == eag_root, "the deferred commit's root differs from the eager restatement's"
    res["commit"] = {
        "keys": nk, "updates": nu, "deferred_ms": stats(def_ms), "eager_restatement_ms": stats(eag_ms),
        "eager_over_deferred": statistics.median(eag_ms) / statistics.median(def_ms),
        "rehash_call_ms_per_commit": inside[0] * 1e3 / (1 + args.host_repeats),
        "note": "both legs run their structural edits in the Python interpreter; rehash_call_ms_per_commit is the wall "
                "time inside the one lcb_trie_rehash_batch call (argument marshalling included)",
    }
    out = args.out or os.path.join(ROOT, "profiles", "trie", res["source_hash"] + ".json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
