#!/usr/bin/env python3
"""tests/golden/make_tx_kats.py — extracts the transaction-encoding known answers the reference's own tests hold
into tests/golden/tx_kats.json: the fields of the two transactions, the five RLP strings and the four full hashes.

Usage: make_tx_kats.py <reference checkout> [output].  Run where the reference's sources are at hand; it is never run
where the GPU tests run.  The JSON is data only (numbers, hex vectors and the file:line they come from).
Source: test/Lachain.CryptoTest/CryptographyTest.cs
  :208-232 Test_TxHash: a transfer with nonce 0, gas price 0, gas limit 0 under the two zero signatures (65 and 66
           zero bytes, SignatureUtils.ZeroOld / ZeroNew): two signed RLPs, two full hashes
  :234-274 Test_TxHash2: nonce 1, gas price 1, gas limit 100000000, a 36-byte invocation: the unsigned RLP under the
           old chain id, and the signed RLPs and full hashes the reference's signer produced under both chain ids
The signatures of Test_TxHash2 are read back out of the signed RLPs (r, s left-padded to 32 bytes, v to the trailer's
width).  The chain ids (25 old, 225 new) are the ones the signed RLPs' v values decode to: v = 2 * chain + 35 + recId.
"""
import json
import os
import re
import sys

SRC = "test/Lachain.CryptoTest/CryptographyTest.cs"


def rlp_items(b):
    """top-level items of one RLP list of strings"""
    off = 1 + (b[0] - 0xf7 if b[0] >= 0xf8 else 0)
    out = []
    while off < len(b):
        h = b[off]
        if h < 0x80:
            out.append(bytes([h])); off += 1
        elif h <= 0xb7:
            n = h - 0x80; out.append(b[off + 1:off + 1 + n]); off += 1 + n
        else:
            ll = h - 0xb7; n = int.from_bytes(b[off + 1:off + 1 + ll], "big")
            out.append(b[off + 1 + ll:off + 1 + ll + n]); off += 1 + ll + n
    return out


def main(out, ref):
    lines = open(os.path.join(ref, SRC)).read().splitlines()

    def find(pat, start=0):
        for i in range(start, len(lines)):
            if re.search(pat, lines[i]):
                return i
        raise KeyError(pat)

    def hex_at(i):
        return re.search(r'"0x([0-9a-fA-F]+)"', lines[i]).group(1).lower()

    def src(i):
        return f"{SRC}:{i + 1}"

    def fields(start, end):
        """the object initialiser between two lines: Nonce, GasPrice, GasLimit (absent: 0), To, Value, Invocation"""
        body = "\n".join(lines[start:end])

        def num(name):
            m = re.search(name + r"\s*=\s*(?:\(ulong\)\s*)?(\d+)", body)
            return int(m.group(1)) if m else 0

        to = re.search(r'To = "0x([0-9a-fA-F]{40})"', body).group(1).lower()
        money = int(re.search(r'Value = Money.Parse\("(\d+)"\)', body).group(1))
        inv = re.search(r'"0x([0-9a-fA-F]+)"\.HexToBytes\(\)\s*\)', body, flags=re.S)
        frm = re.search(r'fromAddress = "0x([0-9a-fA-F]{40})"', body)
        return {"nonce": num("Nonce"), "gas_price": num("GasPrice"), "gas_limit": num("GasLimit"), "to": to,
                "value": (money * 10 ** 18).to_bytes(32, "big").hex(),        # Money: 18 decimals (Money.cs)
                "invocation": inv.group(1).lower() if inv else "",
                "from": frm.group(1).lower() if frm else "00" * 20,           # UInt160Utils.Zero
                "source": f"{src(start)}-{end}"}

    t1 = find(r"public void Test_TxHash\(\)")
    t2 = find(r"public void Test_TxHash2\(\)")
    k = {"transactions": {"transfer": fields(t1, find(r"\};", t1) + 1), "invoke": fields(t2, find(r"\};", t2) + 1)}}
    cases = []
    for new, rl, fh in ((False, find(r'"0xe58000', t1), find(r'"0xe115bce0', t1)),
                        (True, find(r'"0xe78000', t1), find(r'"0xad0a8811', t1))):
        cases.append({"tx": "transfer", "use_new_chain_id": new, "sig": "00" * (66 if new else 65),
                      "sig_note": "SignatureUtils.ZeroNew" if new else "SignatureUtils.ZeroOld",
                      "rlp_with_signature": hex_at(rl), "full_hash": hex_at(fh), "source": f"{src(rl)}, {src(fh)}"})
    chain = {}
    for new, rl, fh in ((False, find(r'"0xf88d0101', t2), find(r'"0x4f0da38b', t2)),
                        (True, find(r'"0xf88f0101', t2), find(r'"0x0d3515b2', t2))):
        signed = bytes.fromhex(hex_at(rl))
        v, r, s = rlp_items(signed)[6:9]
        chain[new] = (int.from_bytes(v, "big") - 35) // 2
        sig = r.rjust(32, b"\0") + s.rjust(32, b"\0") + v.rjust(2 if new else 1, b"\0")
        cases.append({"tx": "invoke", "use_new_chain_id": new, "sig": sig.hex(), "sig_note": "read out of the signed RLP",
                      "rlp_with_signature": signed.hex(), "full_hash": hex_at(fh), "source": f"{src(rl)}, {src(fh)}"})
    u = find(r'"0xf84d0101', t2)
    k["chain_id"] = {"old": chain[False], "new": chain[True]}
    k["signed"] = cases
    k["unsigned"] = [{"tx": "invoke", "use_new_chain_id": False, "rlp": hex_at(u), "source": src(u)}]
    pk = find(r'new EcdsaKeyPair\("0x', t2)
    k["invoke_private_key"] = {"hex": hex_at(pk), "source": src(pk)}
    with open(out, "w") as fo:
        json.dump(k, fo, indent=1, sort_keys=True)
        fo.write("\n")
    print("wrote", out, "with", len(cases) + 1, "RLP strings and", len(cases), "hashes")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit("usage: make_tx_kats.py <reference checkout> [output]")
    main(sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "tx_kats.json"),
         sys.argv[1])
