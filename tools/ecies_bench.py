#!/usr/bin/env python3
"""Throughput of the batched secp256k1 ECIES envelope (k_ecies.hip) on one GPU.

Measured in one session and one process, each after 3 warm-up calls, 10 timed calls, medians with min-max, every output
checked:
  1. ECDH: n items (default 2^20) whose scalars are picked by index among 4,096 (lcb_secp_ecdh_dev), with the kernel
     phases (lcb_ecies_phase_ms) and k_ecdh_mul's share of the INT32 peak = field products per multiplication (counted
     by the host emulation, tools/emul/ecies_emul.cpp) x 72 MAC x rate / 3.93e13, the arithmetic DESIGN.md §15 uses.
     For the comparison with public-key recovery, lcb_ecdsa_recover_hashed_dev runs at the same n in the same session.
  2. The N = 256, F = 85 node load of one trustless key generation: 65,536 value decrypts under one key, 65,536 value
     encrypts to 256 recipients, 256 row envelopes of 2,752 B each way; device-pointer and host-pointer forms.
  3. A CPU leg on the same items over 16 threads: OpenSSL (EC_POINT_mul, SHA256, EVP_aes_256_gcm with a 16-byte IV,
     the calls of tests/golden/make_ecies_kats.py) where libcrypto loads, otherwise the host emulation of the kernels.
     The record names which one ran.  Neither is libsecp256k1 / BouncyCastle, the reference's own libraries.
Writes profiles/ecies/<source_hash>.json (or --out) and prints the same JSON.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

MAC_PER_PRODUCT = 72
INT32_PEAK = 3.93e13
N_NODES, F = 256, 85
ROW_BYTES = 32 * (F + 1)
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
u8p = ctypes.POINTER(ctypes.c_uint8)


def emulation():
    src = os.path.join(ROOT, "tools", "emul", "ecies_emul.cpp")
    lib_path = os.path.join(ROOT, "tools", "emul", "libecies_emul.so")
    deps = [src] + [os.path.join(ROOT, "lachain_amd", "csrc", f) for f in ("k_ecies.hip", "ecies_lane.hpp")]
    if not os.path.exists(lib_path) or os.path.getmtime(lib_path) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", lib_path, src], check=True)
    emu = ctypes.CDLL(lib_path)
    emu.emu_ecdh.restype = ctypes.c_ulonglong
    return emu


def product_count(emu, pubs, scalars, m):
    key, ok = ctypes.create_string_buffer(32 * m), ctypes.create_string_buffer(m)
    p = emu.emu_ecdh(key, ok, pubs[:33 * m], scalars[:32 * m], None, m, m)
    assert ok.raw == b"\x01" * m
    return p / m, key.raw


def threaded(work, n_items, threads=16, seconds=2.0):
    """items per second of work(i) over `threads` threads for at least `seconds` (foreign calls release the GIL)"""
    counts = [0] * threads
    stop = time.perf_counter() + seconds

    def run(t):
        i, done = t, 0
        while time.perf_counter() < stop or done == 0:
            work(i)
            done += 1
            i = (i + threads) % n_items
        counts[t] = done

    t0 = time.perf_counter()
    ts = [threading.Thread(target=run, args=(t,)) for t in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return sum(counts) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--scalars", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import source_hash
    from lachain_amd import native as nat
    from pyref import ecies as E
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    lib = nat.lib()
    n, ns = args.n, args.scalars
    rng = np.random.default_rng(20261019)
    med = statistics.median
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()

    def scalars(m):
        raw = np.frombuffer(rng.bytes(32 * m), dtype=np.uint8).reshape(m, 32).copy()
        raw[:, 0] &= 0x7f                                  # below n, and nonzero with overwhelming probability
        return raw

    def to_dev(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

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

    def wall(call):
        ms = []
        for k in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            rc = call()
            dt = (time.perf_counter() - t0) * 1e3
            if rc != 0:
                raise SystemExit("call failed: " + lib.lcb_last_error().decode())
            if k >= args.warmup:
                ms.append(dt)
        return ms

    def stats(ms):
        return {"median": med(ms), "min": min(ms), "max": max(ms)}

    # ---------------------------------------------------------------- 1. ECDH at n items under ns scalars
    d = scalars(ns)
    a = scalars(n)
    pubs_a, ok_a = nat.ecdsa_pubkey_batch(a.tobytes())            # P_i = a_i G
    pubs_d, ok_d = nat.ecdsa_pubkey_batch(d.tobytes())            # D_j = d_j G
    assert ok_a == b"\x01" * n and ok_d == b"\x01" * ns
    idx = rng.integers(0, ns, size=n).astype(np.int32)
    dp, dd, di = to_dev(pubs_a), to_dev(d.tobytes()), torch.from_numpy(idx).to(dev)
    keys = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    ecdh_ms, ecdh_ph = timed(lambda: lib.lcb_secp_ecdh_dev(keys.data_ptr(), ok.data_ptr(), dp.data_ptr(), dd.data_ptr(),
                                                           di.data_ptr(), ns, n, st.cuda_stream), nat.ecies_phase_ms)
    assert bool((ok == 1).all())
    got = keys.cpu().numpy().reshape(n, 32)
    # every output: d_j (a_i G) must equal a_i (d_j G), computed with the roles of point and scalar exchanged
    dp2 = to_dev(np.frombuffer(pubs_d, dtype=np.uint8).reshape(ns, 33)[idx].tobytes())
    da = to_dev(a.tobytes())
    keys2 = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    assert lib.lcb_secp_ecdh_dev(keys2.data_ptr(), ok.data_ptr(), dp2.data_ptr(), da.data_ptr(), None, n, n,
                                 st.cuda_stream) == 0
    st.synchronize()
    assert bool((ok == 1).all()) and np.array_equal(keys2.cpu().numpy().reshape(n, 32), got), "ECDH is not symmetric"
    for i in range(0, n, max(1, n // 16)):                       # and a sample against the pure-Python restatement
        assert E.ecdh(pubs_a[33 * i:33 * i + 33], d[idx[i]].tobytes()) == got[i].tobytes(), i
    emu = emulation()
    sample = min(n, 1024)
    products, emu_keys = product_count(emu, pubs_a, d[idx[:sample]].tobytes(), sample)
    assert emu_keys == got[:sample].tobytes()

    # public-key recovery at the same n, same session (condition (b) of DESIGN.md §19)
    hashes = rng.bytes(32 * n)
    sigs, sok = nat.ecdsa_sign_hashed_batch(hashes, d[idx].tobytes(), scalars(n).tobytes(), True, 225)
    assert sok == b"\x01" * n
    dh, dsg = to_dev(hashes), to_dev(sigs)
    pub = torch.zeros(33 * n, dtype=torch.uint8, device=dev)
    rec_ms, rec_ph = timed(lambda: lib.lcb_ecdsa_recover_hashed_dev(pub.data_ptr(), None, ok.data_ptr(), dh.data_ptr(),
                                                                     dsg.data_ptr(), 66, n, 1, 225, st.cuda_stream),
                           nat.ecdsa_recover_phase_ms)
    assert bool((ok == 1).all())
    assert np.array_equal(pub.cpu().numpy().reshape(n, 33), np.frombuffer(pubs_d, dtype=np.uint8).reshape(ns, 33)[idx])
    del dh, dsg, pub, keys2, dp2, da
    phases = [med(p[k] for p in ecdh_ph) for k in range(4)]
    rec_phase = med(p[1] for p in rec_ph)
    mul_rate = n / (phases[1] * 1e-3)

    # ---------------------------------------------------------------- 2. the N = 256, F = 85 node load
    node_priv = scalars(N_NODES)
    node_pub, nok = nat.ecdsa_pubkey_batch(node_priv.tobytes())
    assert nok == b"\x01" * N_NODES
    node_pub = np.frombuffer(node_pub, dtype=np.uint8).reshape(N_NODES, 33)
    load = {}

    def envelope_leg(name, m, plen, recipients, dec_idx):
        """m envelopes of plen bytes to recipients[i]; decrypted with node key dec_idx[i]"""
        pt = rng.bytes(plen * m)
        eph, nonce = scalars(m).tobytes(), rng.bytes(16 * m)
        rp = node_pub[recipients].tobytes()
        off = np.arange(m + 1, dtype=np.int64) * plen
        coff = np.arange(m + 1, dtype=np.int64) * (plen + 65)
        d_rp, d_eph, d_nonce, d_pt = to_dev(rp), to_dev(eph), to_dev(nonce), to_dev(pt)
        d_off, d_coff = torch.from_numpy(off).to(dev), torch.from_numpy(coff).to(dev)
        d_env = torch.zeros((plen + 65) * m, dtype=torch.uint8, device=dev)
        d_ok = torch.zeros(m, dtype=torch.uint8, device=dev)
        enc_ms, enc_ph = timed(lambda: lib.lcb_secp256k1_encrypt_dev(
            d_env.data_ptr(), d_ok.data_ptr(), d_rp.data_ptr(), d_eph.data_ptr(), d_nonce.data_ptr(), d_pt.data_ptr(),
            d_off.data_ptr(), m, st.cuda_stream), nat.ecies_phase_ms)
        assert bool((d_ok == 1).all())
        env = bytes(d_env.cpu().numpy())
        d_priv = to_dev(node_priv.tobytes())
        d_idx = torch.from_numpy(dec_idx.astype(np.int32)).to(dev)
        d_back = torch.zeros(plen * m, dtype=torch.uint8, device=dev)
        dec_ms, dec_ph = timed(lambda: lib.lcb_secp256k1_decrypt_dev(
            d_back.data_ptr(), d_ok.data_ptr(), d_priv.data_ptr(), d_idx.data_ptr(), N_NODES, d_env.data_ptr(),
            d_coff.data_ptr(), m, st.cuda_stream), nat.ecies_phase_ms)
        assert bool((d_ok == 1).all()) and bytes(d_back.cpu().numpy()) == pt, name + ": round trip"
        for i in (0, m // 2, m - 1):                             # a sample against the pure-Python restatement
            e = env[(plen + 65) * i:(plen + 65) * (i + 1)]
            assert E.secp256k1_encrypt(rp[33 * i:33 * i + 33], eph[32 * i:32 * i + 32], nonce[16 * i:16 * i + 16],
                                       pt[plen * i:plen * (i + 1)]) == e, (name, i)
        # host-pointer forms (wall clock: staging copies and the synchronisation included)
        hb = lambda b: ctypes.cast((ctypes.c_uint8 * len(b)).from_buffer_copy(b), u8p)
        h_out, h_ok = (ctypes.c_uint8 * ((plen + 65) * m))(), (ctypes.c_uint8 * m)()
        h_rp, h_eph, h_nonce, h_pt, h_env, h_priv = hb(rp), hb(eph), hb(nonce), hb(pt), hb(env), hb(node_priv.tobytes())
        h_off = (ctypes.c_uint64 * (m + 1))(*off.tolist())
        h_coff = (ctypes.c_uint64 * (m + 1))(*coff.tolist())
        h_idx = (ctypes.c_uint32 * m)(*dec_idx.tolist())
        henc_ms = wall(lambda: lib.lcb_secp256k1_encrypt_batch(ctypes.cast(h_out, u8p), ctypes.cast(h_ok, u8p), h_rp, h_eph,
                                                               h_nonce, h_pt, h_off, m))
        assert bytes(h_out) == env and bytes(h_ok) == b"\x01" * m
        h_back = (ctypes.c_uint8 * (plen * m))()
        hdec_ms = wall(lambda: lib.lcb_secp256k1_decrypt_batch(ctypes.cast(h_back, u8p), ctypes.cast(h_ok, u8p), h_priv,
                                                               h_idx, N_NODES, h_env, h_coff, m))
        assert bytes(h_back) == pt and bytes(h_ok) == b"\x01" * m
        load[name] = {
            "items": m, "plaintext_bytes": plen,
            "encrypt_dev_ms": stats(enc_ms), "encrypt_dev_per_s": m / (med(enc_ms) * 1e-3),
            "encrypt_dev_phase_ms": [med(p[k] for p in enc_ph) for k in range(4)],
            "decrypt_dev_ms": stats(dec_ms), "decrypt_dev_per_s": m / (med(dec_ms) * 1e-3),
            "decrypt_dev_phase_ms": [med(p[k] for p in dec_ph) for k in range(4)],
            "encrypt_host_ms": stats(henc_ms), "encrypt_host_per_s": m / (med(henc_ms) * 1e-3),
            "decrypt_host_ms": stats(hdec_ms), "decrypt_host_per_s": m / (med(hdec_ms) * 1e-3),
        }
        return env, pt

    m_val = N_NODES * N_NODES
    # HandleCommit: N values to the N validators per commit; HandleSendValue: every value opened with the node's key.
    # One message set serves both: the decryption runs under the key the envelope was made for
    val_env, val_pt = envelope_leg("values", m_val, 32, np.arange(m_val) % N_NODES, np.arange(m_val) % N_NODES)
    one = np.zeros(m_val, dtype=np.int64)
    envelope_leg("values_one_key", m_val, 32, one, one)           # 65,536 decrypts under one key
    envelope_leg("rows", N_NODES, ROW_BYTES, np.arange(N_NODES), np.arange(N_NODES))

    # ---------------------------------------------------------------- 3. CPU leg, 16 threads
    try:
        import make_ecies_kats as ossl
        ossl.self_check()
        cpu_name = "OpenSSL libcrypto through ctypes (EC_POINT_mul + SHA256; EVP_aes_256_gcm, 16-byte IV), 16 threads"

        def cpu_ecdh(i):
            assert ossl.ecdh(pubs_a[33 * i:33 * i + 33], d[idx[i]].tobytes()) == got[i].tobytes()

        def cpu_value(i):
            e = val_env[97 * i:97 * i + 97]
            key = ossl.ecdh(e[:33], node_priv[i % N_NODES].tobytes())
            p, _ = ossl.gcm(key, e[33:49], e[49:81])              # CTR is its own inverse; the tag costs the same
            assert p == val_pt[32 * i:32 * i + 32]
    except (OSError, AssertionError, AttributeError) as e:
        cpu_name = "host emulation of the kernels (tools/emul/ecies_emul.cpp), 16 threads; libcrypto: %s" % e

        def cpu_ecdh(i):
            key, okb = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1)
            emu.emu_ecdh(key, okb, pubs_a[33 * i:33 * i + 33], d[idx[i]].tobytes(), None, 1, 1)
            assert key.raw == got[i].tobytes()

        def cpu_value(i):
            back, okb = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1)
            emu.emu_secp256k1_decrypt(back, okb, node_priv[i % N_NODES].tobytes(), None, 1, val_env[97 * i:97 * i + 97],
                                      (ctypes.c_uint64 * 2)(0, 97), 1)
            assert back.raw == val_pt[32 * i:32 * i + 32]
    cpu_ecdh_rate = threaded(cpu_ecdh, n)
    cpu_value_rate = threaded(cpu_value, m_val)

    rate = n / (med(ecdh_ms) * 1e-3)
    res = {
        "tool": "tools/ecies_bench.py", "source_hash": source_hash(), "device": torch.cuda.get_device_name(0),
        "n": n, "scalars": ns, "warmup": args.warmup, "repeats": args.repeats,
        "ecdh_per_s": rate, "ecdh_ms": stats(ecdh_ms),
        "phase_ms": {"scalars": phases[0], "multiplication": phases[1], "finish": phases[2], "gcm": phases[3]},
        "field_products_per_ecdh_mul": products, "field_products_sample": sample,
        "ecdh_mul_int32_fraction": mul_rate * products * MAC_PER_PRODUCT / INT32_PEAK,
        "mac_per_product": MAC_PER_PRODUCT, "int32_peak_mac_per_s": INT32_PEAK,
        "ecdh_mul_ns_per_item": phases[1] * 1e6 / n,
        "recover_kernel_ns_per_item": rec_phase * 1e6 / n, "recover_ms": stats(rec_ms),
        "condition_b_mul_not_slower_than_recover": phases[1] <= rec_phase,
        "node_load_n256_f85": load,
        "cpu_leg": cpu_name, "cpu_threads": 16,
        "cpu_ecdh_per_s": cpu_ecdh_rate, "cpu_value_decrypt_per_s": cpu_value_rate,
        "gpu_over_cpu_ecdh": rate / cpu_ecdh_rate,
        "gpu_over_cpu_value_decrypt": load["values"]["decrypt_dev_per_s"] / cpu_value_rate,
    }
    out = args.out or os.path.join(ROOT, "profiles", "ecies", res["source_hash"] + ".json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
