"""CPU check of the transaction-encoding restatement (tests/pyref/txhash.py) against every string and hash the
reference's own tests hold (tests/golden/tx_kats.json, from CryptographyTest.cs:208-274), and of the shared case
builders the emulation and GPU tests use.  TEST INFRASTRUCTURE: the restatement is the yardstick of
tests/test_tx_emul.py, tests/test_gpu_tx_hash.py and tests/test_gpu_tx_receipts.py."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle as o  # noqa: E402
from pyref import txhash as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = json.load(open(os.path.join(ROOT, "tests", "golden", "tx_kats.json")))


def kat_tx(name):
    t = K["transactions"][name]
    return (t["nonce"], t["gas_price"], t["gas_limit"], bytes.fromhex(t["to"]), bytes.fromhex(t["value"]),
            bytes.fromhex(t["invocation"]))


def chain_of(new):
    return K["chain_id"]["new" if new else "old"]


def test_file_holds_five_strings_and_four_hashes():
    assert len(K["signed"]) == 4 and len(K["unsigned"]) == 1
    assert K["chain_id"] == {"old": 25, "new": 225}
    assert all(c["source"].startswith("test/Lachain.CryptoTest/CryptographyTest.cs:") for c in K["signed"] + K["unsigned"])


def test_unsigned_rlp():
    for u in K["unsigned"]:
        assert T.rlp(*kat_tx(u["tx"]), chain_of(u["use_new_chain_id"])).hex() == u["rlp"]


def test_signed_rlp_and_full_hash():
    for c in K["signed"]:
        sig = bytes.fromhex(c["sig"])
        assert T.rlp_with_signature(*kat_tx(c["tx"]), sig).hex() == c["rlp_with_signature"], c["source"]
        assert T.full_hash(*kat_tx(c["tx"]), sig).hex() == c["full_hash"], c["source"]


def test_zero_fields_pinned_by_the_transfer():
    """e5 80 00 00 94...: nonce 0 is empty, gas price and gas limit 0 are the byte 00; ...80 00 80 80 / 80 82 00 00 80 80"""
    old, new = (bytes.fromhex(c["rlp_with_signature"]) for c in K["signed"][:2])
    assert old[:4] == bytes.fromhex("e5800000") and old[-4:] == bytes.fromhex("80008080")
    assert new[-6:] == bytes.fromhex("808200008080")


def test_signed_kats_recover_to_from():
    """Test_TxHash2's two receipts pass VerifyTransactionImmediately; the zero signatures fail it with the hash right"""
    for c in K["signed"]:
        tx, sig, new = kat_tx(c["tx"]), bytes.fromhex(c["sig"]), c["use_new_chain_id"]
        frm = bytes.fromhex(K["transactions"][c["tx"]]["from"])
        got = T.verify_receipt(tx, sig, bytes.fromhex(c["full_hash"]), frm, new, chain_of(new))
        assert got == ((1, 7) if c["tx"] == "invoke" else (0, 1)), c["source"]
    pk = o.ecdsa_pubkey(bytes.fromhex(K["invoke_private_key"]["hex"]))[0]
    assert T.address_of(pk).hex() == K["transactions"]["invoke"]["from"]


def test_mirror_host_encoders_reproduce_the_reference_strings():
    """lachain_amd/transactions.py's Rlp / RlpWithSignature are host byte code: no device needed"""
    from lachain_amd import transactions as M
    if M.TransactionUtils.ChainId(False) == 0:
        M.TransactionUtils.SetChainId(K["chain_id"]["old"], K["chain_id"]["new"])
    assert (M.TransactionUtils.ChainId(False), M.TransactionUtils.ChainId(True)) == (25, 225)

    def mirror_tx(name):
        nonce, gp, gl, to, value, inv = kat_tx(name)
        return M.Transaction(To=to, Value=value, From=bytes.fromhex(K["transactions"][name]["from"]), Nonce=nonce,
                             GasPrice=gp, GasLimit=gl, Invocation=inv)

    for u in K["unsigned"]:
        assert M.TransactionUtils.Rlp(mirror_tx(u["tx"]), u["use_new_chain_id"]).hex() == u["rlp"]
    for c in K["signed"]:
        got = M.TransactionUtils.RlpWithSignature(mirror_tx(c["tx"]), bytes.fromhex(c["sig"]), c["use_new_chain_id"])
        assert got.hex() == c["rlp_with_signature"], c["source"]
    with pytest.raises(RuntimeError):
        M.TransactionUtils.SetChainId(1, 2)


def test_element_rules():
    assert T.encode_element(b"") == b"\x80" and T.encode_element(b"\0") == b"\0" and T.encode_element(b"\x7f") == b"\x7f"
    assert T.encode_element(b"\x80") == b"\x81\x80"
    assert T.encode_element(bytes(55))[:1] == b"\xb7" and T.encode_element(bytes(56))[:2] == b"\xb8\x38"
    assert T.encode_element(bytes(65536))[:4] == b"\xba\x01\x00\x00"
    assert T.encode_list([bytes(55)])[:1] == b"\xf7" and T.encode_list([bytes(56)])[:2] == b"\xf8\x38"
    assert T.big_endian(0) == b"\0" and T.big_endian(0x100) == b"\x01\x00" and T.big_endian(2 ** 64 - 1) == b"\xff" * 8
    assert T.trim_leading_zeros(bytes(2)) == bytes(2) and T.trim_leading_zeros(b"\0\x01\0") == b"\x01\0"


def test_sweep_covers_what_it_claims():
    import tx_cases as C
    assert {c for _, c in C.CALLS} == {1, 25, 127, 128, 225, 2 ** 31 - 1}
    for new, chain in C.CALLS:
        items = C.sweep(new, chain)
        assert 350 <= len(items) <= 550, len(items)
        encs = [(T.rlp(*it.tx, chain), T.rlp_with_signature(*it.tx, it.sig)) for it in items]
        for k in (0, 1):
            assert set(C.EDGES) <= {len(e[k]) for e in encs}
            assert {0xc0 + 55, 0xf8} <= {e[k][0] for e in encs} and any(e[k][:2] == b"\xf8\x38" for e in encs)
        for ln in (0, 1, 2, 55, 56, 255, 256, 1023, 1024, 65535, 65536):
            assert {it.align for it in items if len(it.tx[5]) == ln and it.note == "invocation"} == set(range(8)), ln
        for edge in C.EDGES:
            assert {it.align for it, e in zip(items, encs) if it.note == "edge" and edge in (len(e[0]), len(e[1]))} \
                == set(range(8))
        pos = 0
        for it in items:
            assert it.align == pos % 8
            pos += len(it.tx[5])
        assert {len(it.tx[3]) for it in items} == {0, 20}
