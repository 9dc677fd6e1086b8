"""Plain Python restatement of the raw-transaction ingress (lcb_raw_txs_ingest_*): the strict RLP decode
of a signed wire transaction, the decoded record and signature, RawHash / FullHash of the decoded fields (through
tests/pyref/txhash.py over the oracle's Keccak-256) and the pool's signature decision.  TEST INFRASTRUCTURE: the
yardstick of tests/test_rawtx_pyref.py, tests/test_rawtx_emul.py and tests/test_gpu_rawtx.py; the library is never
compared with itself.

Reference: TransactionServiceWeb3.cs:184-215 (SendRawTransaction), :69-82 (MakeTransaction), TransactionPool.cs:130-143
(Add), SignatureUtils.cs:27 (ToSignature's width check).  What Nethereum's decoder does with malformed or non-canonical
RLP is pinned by nothing: the decoder below is strict, and whatever it refuses it reports as a status."""
import collections
import struct

from pyref import txhash as T

OK, NOT_LIST, LIST_LENGTH, ELEMENT, COUNT, WIDTH = range(6)
SAME_ENCODING, CHAIN_OK, RECOVERS = 1, 2, 4

# tx = (nonce, gas_price, gas_limit, to, value32, invocation) as tests/pyref/txhash.py takes it; span = (offset of the
# invocation in the item, its length); detail holds bits 0 and 1 only
Decoded = collections.namedtuple("Decoded", "status detail tx sig span")
REFUSED = {s: Decoded(s, 0, None, None, (0, 0)) for s in range(1, 6)}


def sig_len(use_new_chain_id: bool) -> int:
    return 66 if use_new_chain_id else 65


def decode(item: bytes, use_new_chain_id: bool, chain_id: int) -> Decoded:
    """the first failing check, in this order, gives the status"""
    n = len(item)
    # 1. a list
    if n == 0 or item[0] < 0xc0:
        return REFUSED[NOT_LIST]
    # 2. its header: header plus payload is the item exactly
    if item[0] <= 0xf7:
        hdr, payload = 1, item[0] - 0xc0
    else:
        ll = item[0] - 0xf7
        if ll > 4 or 1 + ll > n or item[1] == 0:
            return REFUSED[LIST_LENGTH]
        payload = int.from_bytes(item[1:1 + ll], "big")
        if payload < 56:
            return REFUSED[LIST_LENGTH]
        hdr = 1 + ll
    if hdr + payload != n:
        return REFUSED[LIST_LENGTH]
    # 3. nine strings, one after the other; a tenth is never parsed
    pos, elems = hdr, []
    for _ in range(9):
        if pos >= n:
            return REFUSED[COUNT]
        b = item[pos]
        if b < 0x80:
            at, k = pos, 1
        elif b <= 0xb7:
            at, k = pos + 1, b - 0x80
            if at + k > n or (k == 1 and item[at] < 0x80):
                return REFUSED[ELEMENT]
        elif b <= 0xbf:
            ll = b - 0xb7
            if ll > 4 or pos + 1 + ll > n or item[pos + 1] == 0:
                return REFUSED[ELEMENT]
            k = int.from_bytes(item[pos + 1:pos + 1 + ll], "big")
            at = pos + 1 + ll
            if k < 56 or at + k > n:
                return REFUSED[ELEMENT]
        else:
            return REFUSED[ELEMENT]
        elems.append((at, k))
        pos = at + k
    if pos != n:
        return REFUSED[COUNT]
    # 4. widths
    L = sig_len(use_new_chain_id)
    w = [k for _, k in elems]
    if (w[0] > 8 or w[1] > 8 or w[2] > 8 or w[3] not in (0, 20) or w[4] > 32 or w[6] != L - 64 or w[7] > 32
            or w[8] > 32):
        return REFUSED[WIDTH]
    e = [item[at:at + k] for at, k in elems]
    nonce, gas_price, gas_limit = (int.from_bytes(x, "big") for x in e[:3])
    v = int.from_bytes(e[6], "big")
    detail = 0
    lead = [len(x) > 0 and x[0] == 0 for x in e]
    if not (lead[0] or len(e[1]) == 0 or len(e[2]) == 0 or (len(e[1]) >= 2 and lead[1]) or (len(e[2]) >= 2 and lead[2])
            or lead[4]):
        detail |= SAME_ENCODING
    if v in (2 * chain_id + 35, 2 * chain_id + 36):
        detail |= CHAIN_OK
    tx = (nonce, gas_price, gas_limit, e[3], e[4].rjust(32, b"\0"), e[5])
    sig = e[7].rjust(32, b"\0") + e[8].rjust(32, b"\0") + e[6]
    return Decoded(OK, detail, tx, sig, elems[5])


def record(tx, from20: bytes = bytes(20)) -> bytes:
    """lcb_tx_fields (104 B) of decoded fields"""
    nonce, gas_price, gas_limit, to, value, _ = tx
    return struct.pack("<QQQ32s20s20sII", nonce, gas_price, gas_limit, value, to.ljust(20, b"\0"), from20, len(to), 0)


Ingested = collections.namedtuple("Ingested", "accept status detail record span sig raw32 full32")


def ingest(item: bytes, item_off: int, use_new_chain_id: bool, chain_id: int, recover: bool = True) -> Ingested:
    """every output of the call for one item that starts at item_off in the call's raw buffer; with recover False
    (accept == NULL) detail holds bits 0 and 1 only and From stays zero"""
    L = sig_len(use_new_chain_id)
    d = decode(item, use_new_chain_id, chain_id)
    if d.status != OK:
        return Ingested(0, d.status, 0, bytes(104), (0, 0), bytes(L), bytes(32), bytes(32))
    raw32 = T.raw_hash(*d.tx, chain_id)
    full32 = T.full_hash(*d.tx, d.sig)
    detail, accept, frm = d.detail, 0, bytes(20)
    if recover:
        addr = T.recover_address(raw32, d.sig, use_new_chain_id, chain_id)
        if addr is not None:
            detail |= RECOVERS
        accept = int(detail == 7)
        if accept:
            frm = addr
    return Ingested(accept, OK, detail, record(d.tx, frm), (item_off + d.span[0], d.span[1]), d.sig, raw32, full32)
