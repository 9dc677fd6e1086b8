#!/usr/bin/env python3
"""tests/golden/make_rawtx_kats.py — extracts the six signed raw transactions the reference's own tests hold into
tests/golden/rawtx_kats.json: the wire bytes, the chain id their v decodes to, and what the reference pins about each.

Usage: make_rawtx_kats.py <reference checkout> [output].  Run where the reference's sources are at hand; it is never run
where the GPU tests run.  The JSON is data only (hex vectors, numbers and the file:line they come from).
Sources:
  test/Lachain.CoreTest/IntegrationTests/TransactionsTest.cs  the signed RLPs whose Keccak is the receipt's hash, under
      the old and the new chain id; the recovered address is From
  test/Lachain.CryptoTest/CryptographyTest.cs  Test_TxHash2's two signed RLPs with their full hashes, the string
      Test_External_Signature2 decodes with LegacyTransactionChainId, and the address Test_SignRoundTrip pins for the
      key that signed the first five
  test/Lachain.CoreTest/RPC/HTTP/Web3/Web3TransactionTests.cs  the string VerifyRawTransaction answers with a hash
The chain id is (v - 35) // 2 of the string's own v.  No reference line pins the sixth string's sender: the script
recovers it with the repository's oracle and marks it as such.
"""
import json
import os
import re
import sys

TT = "test/Lachain.CoreTest/IntegrationTests/TransactionsTest.cs"
CT = "test/Lachain.CryptoTest/CryptographyTest.cs"
WT = "test/Lachain.CoreTest/RPC/HTTP/Web3/Web3TransactionTests.cs"
HERE = os.path.dirname(os.path.abspath(__file__))


def v_of(raw: bytes) -> bytes:
    """the seventh top-level string of one RLP list of strings"""
    off = 1 + (raw[0] - 0xf7 if raw[0] >= 0xf8 else 0)
    for k in range(7):
        h = raw[off]
        if h < 0x80:
            item, off = raw[off:off + 1], off + 1
        elif h <= 0xb7:
            item, off = raw[off + 1:off + 1 + h - 0x80], off + 1 + h - 0x80
        else:
            ll = h - 0xb7
            n = int.from_bytes(raw[off + 1:off + 1 + ll], "big")
            item, off = raw[off + 1 + ll:off + 1 + ll + n], off + 1 + ll + n
    return item


def main(out, ref):
    files = {f: open(os.path.join(ref, f)).read().splitlines() for f in (TT, CT, WT)}

    def find(f, pat, start=0):
        for i in range(start, len(files[f])):
            if re.search(pat, files[f][i]):
                return i
        raise KeyError(pat)

    def hex_at(f, i):
        return re.search(r'"0x([0-9a-fA-F]+)"', files[f][i]).group(1).lower()

    def src(f, i):
        return f"{f}:{i + 1}"

    addr = find(CT, r'var address = "0x6Bc32575')
    key = find(CT, r'var privateKey = "0xD95D6DB6')
    signer = {"address": hex_at(CT, addr), "address_source": src(CT, addr), "private_key": hex_at(CT, key),
              "private_key_source": src(CT, key)}
    vectors = []

    def add(f, pat, pins, full_hash_pat=None, from_pinned=True, after=None):
        i = find(f, pat, find(f, after) if after else 0)
        raw = bytes.fromhex(hex_at(f, i))
        v = v_of(raw)
        e = {"raw": raw.hex(), "source": src(f, i), "use_new_chain_id": len(v) == 2,
             "chain_id": (int.from_bytes(v, "big") - 35) // 2, "pinned": pins,
             "from": signer["address"] if from_pinned else None, "from_pinned": from_pinned}
        if full_hash_pat:
            j = find(f, full_hash_pat)
            e["full_hash"], e["full_hash_source"] = hex_at(f, j), src(f, j)
        vectors.append(e)

    add(TT, r'"0xf86f8085174876e8', "receipt.Hash == Keccak(raw); the recovered address is From")
    add(TT, r'"0xf8718085174876e8', "receipt.Hash == Keccak(raw); the recovered address is From")
    add(CT, r'"0xf88d01018405f5e1', "RlpWithSignature and FullHash", r'"0x4f0da38b')
    add(CT, r'"0xf88f01018405f5e1', "RlpWithSignature and FullHash", r'"0x0d3515b2')
    add(CT, r'"0xf86d808504a817c8', "decoded by LegacyTransactionChainId in Test_External_Signature2",
        after=r"public void Test_External_Signature2\(\)")
    add(WT, r'var rawTx = "0xf8848001832e1a30', "VerifyRawTransaction returns the hash", r'"0x2ad6261b', from_pinned=False,
        after=r"public void Test_VerifyRawTransaction_Valid_txn\(\)")
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"), os.path.dirname(HERE)]
    from pyref import rawtx as W                        # the sixth sender: recovered, not pinned
    last = vectors[-1]
    got = W.ingest(bytes.fromhex(last["raw"]), 0, last["use_new_chain_id"], last["chain_id"])
    assert got.accept == 1
    last["from"] = got.record[76:96].hex()
    with open(out, "w") as fo:
        json.dump({"signer": signer, "vectors": vectors}, fo, indent=1, sort_keys=True)
        fo.write("\n")
    print("wrote", out, "with", len(vectors), "raw transactions")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit("usage: make_rawtx_kats.py <reference checkout> [output]")
    main(sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "rawtx_kats.json"), sys.argv[1])
