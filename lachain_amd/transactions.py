"""lachain_amd/transactions.py — the transaction's encoding, hashes, signing and verification under the reference's
names, over the batched entry points of liblachain_bls.so (lachain_amd/native.py): a receipt goes in as fields, and
RawHash, FullHash, the hash check, the sender recovery and the From comparison run on the device in one call.

Reference: src/Lachain.Crypto/TransactionUtils.cs (GetEthTx, Rlp, RlpWithSignature, RawHash, FullHash),
src/Lachain.Core/Blockchain/Operations/TransactionSigner.cs and TransactionVerifier.cs (VerifyTransactionImmediately,
VerifyTransactions and the public-key cache), and src/Lachain.Core/RPC/HTTP/Web3/TransactionServiceWeb3.cs:69-82, :184-254
(MakeTransaction, SendRawTransaction and its batch forms: wire bytes in, decoded on the device).  Rlp and RlpWithSignature are host byte code (wire use and tests); every
hash and every curve operation is the library's.
"""
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

from . import native


class Transaction(NamedTuple):
    """Lachain.Proto.Transaction: To is 20 bytes or empty, Value the 32-byte big-endian UInt256 buffer"""
    To: bytes
    Value: bytes
    From: bytes
    Nonce: int = 0
    GasPrice: int = 0
    GasLimit: int = 0
    Invocation: bytes = b""

    def record(self) -> bytes:
        return native.tx_fields(self.Nonce, self.GasPrice, self.GasLimit, self.To, self.Value, self.From)


class TransactionReceipt(NamedTuple):
    Transaction: Transaction
    Hash: bytes
    Signature: bytes          # r || s || v, 65 bytes under the old chain id and 66 under the new one


def _signature_size(use_new_chain_id: bool) -> int:
    return 66 if use_new_chain_id else 65


def _trim_leading_zeros(b: bytes) -> bytes:
    """HexUtils.TrimLeadingZeros (HexUtils.cs:88-92): an all-zero array stays whole"""
    for i, v in enumerate(b):
        if v:
            return b[i:]
    return b


def _big_endian(v: int) -> bytes:
    return v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")


def _rlp_length(n: int, base: int) -> bytes:
    if n < 56:
        return bytes([base + n])
    be = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([base + 55 + len(be)]) + be


def _rlp_element(b: bytes) -> bytes:
    if len(b) == 1 and b[0] < 0x80:
        return bytes(b)
    return _rlp_length(len(b), 0x80) + bytes(b)


def _rlp_list(items) -> bytes:
    body = b"".join(_rlp_element(i) for i in items)
    return _rlp_length(len(body), 0xc0) + body


class TransactionUtils:
    """ChainId(useNewId) is the pair given to SetChainId, once, as in the reference"""
    _old = 0
    _new = 0

    @classmethod
    def SetChainId(cls, old_chain_id: int, new_chain_id: int) -> None:
        if cls._old or cls._new:
            raise RuntimeError("trying to set chainId second time.")
        cls._old, cls._new = old_chain_id, new_chain_id

    @classmethod
    def ChainId(cls, use_new_id: bool) -> int:
        return cls._new if use_new_id else cls._old

    @staticmethod
    def _six(t: Transaction):
        return [b"" if t.Nonce == 0 else _big_endian(t.Nonce), _big_endian(t.GasPrice), _big_endian(t.GasLimit),
                bytes(t.To), bytes(t.Value).lstrip(b"\0"), bytes(t.Invocation)]

    @classmethod
    def Rlp(cls, t: Transaction, use_new_id: bool) -> bytes:
        return _rlp_list(cls._six(t) + [_big_endian(cls.ChainId(use_new_id)), b"", b""])

    @classmethod
    def RlpWithSignature(cls, t: Transaction, s: bytes, use_new_id: bool) -> bytes:
        r, ss, v = _trim_leading_zeros(s[:32]), _trim_leading_zeros(s[32:64]), _trim_leading_zeros(s[64:])
        return _rlp_list(cls._six(t) + [v, r if any(r) else b"", ss if any(ss) else b""])

    @classmethod
    def RawHashes(cls, txs: Sequence[Transaction], use_new_id: bool) -> List[bytes]:
        raw, _ = native.tx_hash_batch(b"".join(t.record() for t in txs), [t.Invocation for t in txs], None,
                                      _signature_size(use_new_id), use_new_id, cls.ChainId(use_new_id))
        return [raw[32 * i:32 * i + 32] for i in range(len(txs))]

    @classmethod
    def FullHashes(cls, txs: Sequence[Transaction], sigs: Sequence[bytes], use_new_id: bool) -> List[bytes]:
        size = _signature_size(use_new_id)
        if any(len(s) != size for s in sigs):
            raise ValueError("a signature of the wrong size for this chain id")
        _, full = native.tx_hash_batch(b"".join(t.record() for t in txs), [t.Invocation for t in txs], b"".join(sigs),
                                       size, use_new_id, cls.ChainId(use_new_id))
        return [full[32 * i:32 * i + 32] for i in range(len(txs))]

    @classmethod
    def RawHash(cls, t: Transaction, use_new_id: bool) -> bytes:
        return cls.RawHashes([t], use_new_id)[0]

    @classmethod
    def FullHash(cls, t: Transaction, s: bytes, use_new_id: bool) -> bytes:
        return cls.FullHashes([t], [s], use_new_id)[0]


class Signer:
    """TransactionSigner.Sign with caller-given nonces (lcb_ecdsa_sign_hashed_batch; not RFC 6979)"""

    @staticmethod
    def SignBatch(txs: Sequence[Transaction], private_keys: Sequence[bytes], nonces: Sequence[bytes],
                  use_new_chain_id: bool) -> List[TransactionReceipt]:
        chain = TransactionUtils.ChainId(use_new_chain_id)
        size = _signature_size(use_new_chain_id)
        raw = b"".join(TransactionUtils.RawHashes(txs, use_new_chain_id))
        sigs, ok = native.ecdsa_sign_hashed_batch(raw, b"".join(private_keys), b"".join(nonces), use_new_chain_id, chain)
        if ok != b"\x01" * len(txs):
            raise ValueError("a private key or nonce outside [1, n), or a zero r / s")
        sigs = [sigs[size * i:size * (i + 1)] for i in range(len(txs))]
        full = TransactionUtils.FullHashes(txs, sigs, use_new_chain_id)
        return [TransactionReceipt(t, h, s) for t, h, s in zip(txs, full, sigs)]

    @staticmethod
    def Sign(transaction: Transaction, private_key: bytes, use_new_chain_id: bool, nonce: bytes) -> TransactionReceipt:
        return Signer.SignBatch([transaction], [private_key], [nonce], use_new_chain_id)[0]


class TransactionVerifier:
    """VerifyTransactionImmediately / VerifyTransactions with the reference's public-key cache (address -> key)"""

    def __init__(self):
        self._publicKeyCache: Dict[bytes, bytes] = {}

    def VerifyTransactionImmediately(self, receipt: TransactionReceipt, use_new_chain_id: bool,
                                     cache_enabled: bool) -> bool:
        return self.VerifyTransactions([receipt], use_new_chain_id, cache_enabled)[0]

    def VerifyTransactions(self, receipts: Sequence[TransactionReceipt], use_new_chain_id: bool,
                           cache_enabled: bool) -> List[bool]:
        """the decisions of the reference's sequential loop over `receipts`, in list order.  Without the cache: one
        receipts call.  With it: the hashes and one recovery call over every receipt whose From is not cached at the
        start, a host walk in order (a sender enters the cache at its first accepted receipt), then one
        VerifySignatureHashed call (low s enforced, as in the reference's cached branch) for the receipts the walk found
        cached at their turn."""
        n = len(receipts)
        if not n:
            return []
        chain = TransactionUtils.ChainId(use_new_chain_id)
        size = _signature_size(use_new_chain_id)
        records = b"".join(r.Transaction.record() for r in receipts)
        invs = [r.Transaction.Invocation for r in receipts]
        # a signature of another size throws in the reference wherever it is decoded: the receipt is rejected
        sized = [len(r.Signature) == size for r in receipts]
        sigs = [r.Signature if good else bytes(size) for r, good in zip(receipts, sized)]
        hashes = b"".join(r.Hash if good else bytes(32) for r, good in zip(receipts, sized))
        if not cache_enabled:
            accept, _ = native.receipts_verify_batch(records, invs, b"".join(sigs), size, hashes, use_new_chain_id, chain)
            return [bool(a) and good for a, good in zip(accept, sized)]
        raw, full = native.tx_hash_batch(records, invs, b"".join(sigs), size, use_new_chain_id, chain)
        raw = [raw[32 * i:32 * i + 32] for i in range(n)]
        hash_ok = [sized[i] and full[32 * i:32 * i + 32] == receipts[i].Hash for i in range(n)]
        miss = [i for i in range(n) if receipts[i].Transaction.From not in self._publicKeyCache]
        recovered = {}
        if miss:
            pub, addr, ok = native.ecdsa_recover_hashed_batch(b"".join(raw[i] for i in miss),
                                                              b"".join(sigs[i] for i in miss), size, use_new_chain_id, chain)
            for k, i in enumerate(miss):
                recovered[i] = (pub[33 * k:33 * k + 33], addr[20 * k:20 * k + 20]) if ok[k] else None
        out = [False] * n
        cached = []                                     # (receipt index, key) of the cached branch
        for i, r in enumerate(receipts):
            if not hash_ok[i]:
                continue
            frm = r.Transaction.From
            key = self._publicKeyCache.get(frm)
            if key is not None:
                cached.append((i, key))
                continue
            rec = recovered[i]
            if rec is not None and rec[1] == frm:
                out[i] = True
                self._publicKeyCache[frm] = rec[0]
        if cached:
            keys = sorted({k for _, k in cached})
            acc = native.ecdsa_verify_hashed_batch(b"".join(raw[i] for i, _ in cached), b"".join(sigs[i] for i, _ in cached),
                                                   size, b"".join(keys), 33, [keys.index(k) for _, k in cached],
                                                   use_new_chain_id, chain)
            for (i, _), a in zip(cached, acc):
                out[i] = bool(a)
        return out


RAWTX_STATUS_NAMES = ("Ok", "NotList", "ListLength", "Element", "Count", "Width")


def MakeTransactions(raws: Sequence[bytes], use_new_chain_id: bool) -> List[Optional[Tuple[Transaction, bytes]]]:
    """TransactionServiceWeb3.MakeTransaction (:69-82) and the padded signature of SendRawTransaction (:189-198) for each
    signed wire transaction, from one lcb_raw_txs_ingest_batch call: (Transaction, r || s || v), or None where the strict
    decoder refuses the item.  From is the sender recovered on the device where the pool's signature check would pass
    (native.RawTxs.accept) and 20 zero bytes otherwise: the reference takes it from Nethereum's own recovery."""
    return [None if m is None else (m[0], m[1]) for m in _ingest(raws, use_new_chain_id)[0]]


def _ingest(raws, use_new_chain_id):
    chain = TransactionUtils.ChainId(use_new_chain_id)
    size = _signature_size(use_new_chain_id)
    joined = b"".join(raws)
    got = native.raw_txs_ingest_batch(raws, use_new_chain_id, chain)
    made = []
    for i in range(len(raws)):
        if got.status[i] != native.RAWTX_OK:
            made.append(None)
            continue
        rec = got.records[104 * i:104 * (i + 1)]
        at, ln = got.spans[i]
        t = Transaction(To=rec[56:56 + int.from_bytes(rec[96:100], "little")], Value=rec[24:56], From=rec[76:96],
                        Nonce=int.from_bytes(rec[0:8], "little"), GasPrice=int.from_bytes(rec[8:16], "little"),
                        GasLimit=int.from_bytes(rec[16:24], "little"), Invocation=joined[at:at + ln])
        made.append((t, got.sigs[size * i:size * (i + 1)], got.full32[32 * i:32 * i + 32]))
    return made, got


def SendRawTransactionBatch(raw_txs: Sequence[bytes], use_new_chain_id: bool,
                            pool_add: Callable[[Transaction, bytes], str]) -> List[str]:
    """la_sendRawTransactionBatch (TransactionServiceWeb3.cs:217-235): SendRawTransaction (:184-215) per item, in list
    order, over one device call.  Per item: "0x" + FullHash where the transaction entered the pool; "BadChainId" (:203);
    "InvalidSignature" where TransactionPool.Add's signature check fails (TransactionPool.cs:130-143); the string
    pool_add returned where it is not "Ok"; "Refused: <status>" where the strict decoder turns the bytes down (the
    caller sends those down its host path).  pool_add(transaction, signature) stands for the pool's own state checks
    (nonce, balance, gas, duplicates) and returns an OperatingError name; it is called only for items whose signature
    check passed."""
    made, got = _ingest(raw_txs, use_new_chain_id)
    out = []
    for i, m in enumerate(made):
        if m is None:
            out.append("Refused: " + RAWTX_STATUS_NAMES[got.status[i]])
        elif not got.detail[i] & native.RAWTX_CHAIN_OK:
            out.append("BadChainId")
        elif not got.accept[i]:
            out.append("InvalidSignature")
        else:
            result = pool_add(m[0], m[1])
            out.append("0x" + m[2].hex() if result == "Ok" else result)
    return out
