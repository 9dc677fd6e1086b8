"""Plain Python restatement of the reference's transaction encoding and hashes, over the oracle's Keccak-256
(o.keccak256).  TEST INFRASTRUCTURE: the yardstick of tests/test_tx_pyref.py, tests/test_tx_emul.py and the GPU
transaction tests; the library is never compared with itself.

Reference: src/Lachain.Crypto/TransactionUtils.cs:30-105 (GetEthTx, Rlp, LAEncodeSigned, RlpWithSignature, RawHash,
FullHash), src/Lachain.Utility/Utils/HexUtils.cs:88-92 (TrimLeadingZeros leaves an all-zero array whole), Nethereum's
RLP.EncodeElement / EncodeList, and TransactionVerifier.cs:109-143 (VerifyTransactionImmediately)."""
import oracle as o


def trim_leading_zeros(b: bytes) -> bytes:
    """HexUtils.TrimLeadingZeros: strips leading zero bytes, but returns an all-zero (or empty) array unchanged"""
    for i, v in enumerate(b):
        if v:
            return b[i:]
    return b


def big_endian(v: int) -> bytes:
    """new BigInteger(v).ToByteArray().Reverse().TrimLeadingZeros() for a non-negative v: minimal big-endian, zero is
    the one byte 00 (ToByteArray gives at least one byte, and a sign byte that the trim removes)"""
    return v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")


def _length(n: int, base: int) -> bytes:
    if n < 56:
        return bytes([base + n])
    be = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([base + 55 + len(be)]) + be


def encode_element(b: bytes) -> bytes:
    """Nethereum RLP.EncodeElement: an empty (or null) string is 80, one byte below 80 is itself (a single 00 too)"""
    if len(b) == 0:
        return b"\x80"
    if len(b) == 1 and b[0] < 0x80:
        return bytes(b)
    return _length(len(b), 0x80) + bytes(b)


def encode_list(items) -> bytes:
    payload = b"".join(items)
    return _length(len(payload), 0xc0) + payload


def six_fields(nonce, gas_price, gas_limit, to, value32, invocation):
    """the first six elements of GetEthTx's data: nonce empty when zero; gasPrice / gasLimit minimal with zero as 00;
    To as it is (20 bytes or none); Value = UInt256.ToBytes(false, true): the 32 buffer bytes, leading zeros stripped,
    nothing left for zero; the invocation as it is"""
    assert len(to) in (0, 20) and len(value32) == 32
    return [b"" if nonce == 0 else big_endian(nonce), big_endian(gas_price), big_endian(gas_limit), bytes(to),
            bytes(value32).lstrip(b"\0"), bytes(invocation)]


def rlp(nonce, gas_price, gas_limit, to, value32, invocation, chain_id: int) -> bytes:
    """Transaction.Rlp(useNewId): [six fields, chainId, "", ""] (RLPSigner.GetRLPEncodedRaw)"""
    data = six_fields(nonce, gas_price, gas_limit, to, value32, invocation) + [big_endian(chain_id), b"", b""]
    return encode_list([encode_element(d) for d in data])


def signature_fields(sig: bytes):
    """(v, r, s) as GetEthTx hands them to RLPSigner: each half and the tail through TrimLeadingZeros"""
    assert len(sig) in (65, 66)
    return trim_leading_zeros(sig[64:]), trim_leading_zeros(sig[:32]), trim_leading_zeros(sig[32:64])


def rlp_with_signature(nonce, gas_price, gas_limit, to, value32, invocation, sig: bytes) -> bytes:
    """Transaction.RlpWithSignature: LAEncodeSigned over the six fields, then V, R, S.  SignedData.IsSigned() needs a
    non-null V, which every encoded signature has.  R and S go through the RLPSigner constructor, whose zero check
    (R, S both all zero -> unsigned: three empty elements would be Nethereum >= 4's choice) the reference's own
    encoder avoids (TransactionUtils.cs:85-89): with R = S = 0 it writes V as it is and two empty strings, which
    CryptographyTest.cs:221-225 pins.  A single zero half is not pinned anywhere; the same rule is applied to it."""
    v, r, s = signature_fields(sig)
    r = b"" if not any(r) else r
    s = b"" if not any(s) else s
    data = six_fields(nonce, gas_price, gas_limit, to, value32, invocation) + [v, r, s]
    return encode_list([encode_element(d) for d in data])


def raw_hash(nonce, gas_price, gas_limit, to, value32, invocation, chain_id: int) -> bytes:
    return o.keccak256(rlp(nonce, gas_price, gas_limit, to, value32, invocation, chain_id))


def full_hash(nonce, gas_price, gas_limit, to, value32, invocation, sig: bytes) -> bytes:
    return o.keccak256(rlp_with_signature(nonce, gas_price, gas_limit, to, value32, invocation, sig))


P = 2 ** 256 - 2 ** 32 - 977


def _tdiv(a: int, b: int) -> int:
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def rec_id(sig: bytes, chain_id: int, use_new_chain_id: bool):
    """recId = (enc - 36) / 2 / chainId (DefaultCrypto.cs:155-158; C# truncates), or None where the reference throws"""
    if len(sig) != (66 if use_new_chain_id else 65) or chain_id == 0:
        return None
    rec = _tdiv(_tdiv(int.from_bytes(sig[64:], "big") - 36, 2), chain_id)
    return rec if 0 <= rec <= 3 else None


def address_of(pub33: bytes) -> bytes:
    """ComputeAddress (DefaultCrypto.cs:197-200): keccak256(x || y)[12:]"""
    x = int.from_bytes(pub33[1:], "big")
    y = pow((x ** 3 + 7) % P, (P + 1) // 4, P)
    if (y & 1) != (pub33[0] & 1):
        y = P - y
    return o.keccak256(x.to_bytes(32, "big") + y.to_bytes(32, "big"))[12:]


def recover_address(hash32: bytes, sig: bytes, use_new_chain_id: bool, chain_id: int):
    """receipt.RecoverPublicKey + GetAddress over o.ecdsa_recover (no low-s rule): the address, or None"""
    rec = rec_id(sig, chain_id, use_new_chain_id)
    pk = o.ecdsa_recover(hash32, sig[:64], rec) if rec is not None else None
    return address_of(pk) if pk else None


def verify_receipt(tx, sig: bytes, claimed_hash: bytes, from20: bytes, use_new_chain_id: bool, chain_id: int):
    """VerifyTransactionImmediately(receipt, useNewChainId, cacheEnabled: false) as (accept, detail): detail bit 0 =
    Hash == FullHash, bit 1 = the signature recovers from RawHash, bit 2 = the recovered address is From.
    tx = (nonce, gas_price, gas_limit, to, value32, invocation)."""
    detail = int(full_hash(*tx, sig) == claimed_hash)
    addr = recover_address(raw_hash(*tx, chain_id), sig, use_new_chain_id, chain_id)
    if addr is not None:
        detail |= 2
        if addr == from20:
            detail |= 4
    return int(detail == 7), detail
