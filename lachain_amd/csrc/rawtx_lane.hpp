// lachain_amd/csrc/rawtx_lane.hpp — the per-lane pieces of the raw-transaction ingress (k_rawtx.hip): the strict RLP
// decode of one signed wire transaction, its decoded record, signature and invocation span, and RawHash / FullHash of
// the decoded fields through tx_hash (txhash_lane.hpp), whose invocation pointer stays inside the wire bytes.  No LDS,
// no barriers, so tools/emul/rawtx_emul.cpp (RBC_HOST_EMULATION) runs the lane on the CPU.
//
// Reference: TransactionServiceWeb3.cs:184-215 (SendRawTransaction), :69-82 (MakeTransaction), SignatureUtils.cs:27
// (ToSignature), TransactionUtils.cs:30-48 (Lachain's own encoding of elements 0-5).  tests/pyref/rawtx.py restates the
// rules; DESIGN.md §24 has them in words.
//
// Every byte of the item is hostile.  A length read from the bytes is compared, in 64-bit arithmetic, with the item's
// end before anything it describes is read; the decode reads single bytes at indices below the item's length, and the
// hashing reads the invocation, which by then lies inside the item, by tx_put_six's aligned words.
#pragma once
#include "txhash_lane.hpp"

#define RAWTX_OK 0
#define RAWTX_NOT_LIST 1
#define RAWTX_LIST_LENGTH 2
#define RAWTX_ELEMENT 3
#define RAWTX_COUNT 4
#define RAWTX_WIDTH 5
#define RAWTX_SAME_ENCODING 1
#define RAWTX_CHAIN_OK 2
#define RAWTX_RECOVERS 4
// an invocation of this many bytes or more is hashed by k_rawtx_long (k_txhash.hip's TXH_LONG, for the same reason)
#define RAWTX_LONG 1024

// the big-endian value of p[at .. at + k), k <= 8 (the caller has checked at + k against the item's end)
SDI u64 rawtx_be(const uint8_t *p, u64 at, u32 k) {
    u64 v = 0;
#pragma unroll 1
    for (u32 b = 0; b < k; b++) v = (v << 8) | p[at + b];
    return v;
}
// p[at .. at + k), k <= 32, left-padded to 32 bytes, in memory order (four little-endian words)
SDI void rawtx_pad32(u64 m[4], const uint8_t *p, u64 at, u32 k) {
    u64 w3 = 0, w2 = 0, w1 = 0, w0 = 0;                // the bytes as one 256-bit number
#pragma unroll 1
    for (u32 b = 0; b < k; b++) {
        w3 = (w3 << 8) | (w2 >> 56);
        w2 = (w2 << 8) | (w1 >> 56);
        w1 = (w1 << 8) | (w0 >> 56);
        w0 = (w0 << 8) | p[at + b];
    }
    m[0] = tx_bswap64(w3);
    m[1] = tx_bswap64(w2);
    m[2] = tx_bswap64(w1);
    m[3] = tx_bswap64(w0);
}

// the nine elements' bodies: at[e] is the body's index in the item, n[e] its length
struct rawtx_elems {
    u64 at[9], n[9];
};
// checks 1 - 3 of DESIGN.md §24: the list, its header, nine strings that fill the payload exactly
SDI u32 rawtx_parse(rawtx_elems &e, const uint8_t *p, u64 len) {
#pragma unroll
    for (int k = 0; k < 9; k++) e.at[k] = e.n[k] = 0;
    if (len == 0 || p[0] < 0xc0) return RAWTX_NOT_LIST;
    u64 hdr = 1, payload = p[0] - 0xc0;
    if (p[0] > 0xf7) {
        const u32 ll = p[0] - 0xf7;
        if (ll > 4 || 1 + (u64)ll > len || p[1] == 0) return RAWTX_LIST_LENGTH;
        payload = rawtx_be(p, 1, ll);
        if (payload < 56) return RAWTX_LIST_LENGTH;
        hdr = 1 + ll;
    }
    if (hdr + payload != len) return RAWTX_LIST_LENGTH;
    u64 pos = hdr;
    u32 st = RAWTX_OK;
#pragma unroll
    for (int k = 0; k < 9; k++) {                      // unrolled: at[] and n[] are registers; one failure ends the rest
        if (st != RAWTX_OK) continue;
        if (pos >= len) { st = RAWTX_COUNT; continue; }
        const u32 b = p[pos];
        u64 at = pos, n = 1;
        if (b >= 0xc0) {
            st = RAWTX_ELEMENT;
        } else if (b >= 0xb8) {
            const u32 ll = b - 0xb7;
            if (ll > 4 || pos + 1 + ll > len || p[pos + 1] == 0) {
                st = RAWTX_ELEMENT;
            } else {
                n = rawtx_be(p, pos + 1, ll);          // below 2^32: the sum below cannot wrap
                at = pos + 1 + ll;
                if (n < 56 || at + n > len) st = RAWTX_ELEMENT;
            }
        } else if (b >= 0x80) {
            n = b - 0x80;
            at = pos + 1;
            if (at + n > len || (n == 1 && p[at] < 0x80)) st = RAWTX_ELEMENT;
        }
        if (st != RAWTX_OK) continue;
        e.at[k] = at;
        e.n[k] = n;
        pos = at + n;
    }
    if (st == RAWTX_OK && pos != len) st = RAWTX_COUNT;
    return st;
}
// check 4: the widths MakeTransaction's conversions and ToSignature accept
SDI bool rawtx_widths_ok(const rawtx_elems &e, u32 sig_len) {
    return e.n[0] <= 8 && e.n[1] <= 8 && e.n[2] <= 8 && (e.n[3] == 0 || e.n[3] == 20) && e.n[4] <= 32 &&
           e.n[6] == sig_len - 64 && e.n[7] <= 32 && e.n[8] <= 32;
}
// an element with a leading zero byte
SDI bool rawtx_lead_zero(const rawtx_elems &e, int k, const uint8_t *p) { return e.n[k] != 0 && p[e.at[k]] == 0; }

// Lane i of a call: the item raw[off[i] .. off[i + 1]).  Outputs, each but status nullable: status[i], detail[i] (bits
// 0 and 1), the record txs + 104 i (From zero; 8-byte aligned), span[2 i] = span_base + off[i] + the invocation's index
// and span[2 i + 1] = its length, the signature sigs + sig_len i (r || s || v), raw32 and full32 (32 bytes per item).  A
// refused item gets its status and zero bytes everywhere else.  With defer_long an accepted item whose invocation has
// RAWTX_LONG bytes or more is decoded but not hashed: the lane returns true and the caller lists it for a lane of
// k_rawtx_long, which runs it again without the flag.
SDI bool rawtx_lane(size_t i, const uint8_t *raw, const u64 *off, u64 span_base, u32 sig_len, u32 chain_id,
                    bool defer_long, uint8_t *status, uint8_t *detail, uint8_t *txs, u64 *span, uint8_t *sigs,
                    uint8_t *raw32, uint8_t *full32) {
    const uint8_t *p = raw + off[i];
    const u64 len = off[i + 1] - off[i];
    rawtx_elems e;
    u32 st = rawtx_parse(e, p, len);
    if (st == RAWTX_OK && !rawtx_widths_ok(e, sig_len)) st = RAWTX_WIDTH;
    const bool ok = st == RAWTX_OK, two = sig_len == 66;

    tx_item t;
    u64 r[4] = {0, 0, 0, 0}, s[4] = {0, 0, 0, 0}, to[4] = {0, 0, 0, 0};
    u32 b0 = 0, b1 = 0, det = 0;
    t.nonce = t.gas_price = t.gas_limit = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) t.value[j] = 0;
    t.has_to = false;
    t.inv = p;
    t.inv_len = 0;
    t.first = 0;
    if (ok) {
        t.nonce = rawtx_be(p, e.at[0], (u32)e.n[0]);
        t.gas_price = rawtx_be(p, e.at[1], (u32)e.n[1]);
        t.gas_limit = rawtx_be(p, e.at[2], (u32)e.n[2]);
        rawtx_pad32(to, p, e.at[3], (u32)e.n[3]);
        rawtx_pad32(t.value, p, e.at[4], (u32)e.n[4]);
        rawtx_pad32(r, p, e.at[7], (u32)e.n[7]);
        rawtx_pad32(s, p, e.at[8], (u32)e.n[8]);
        t.has_to = e.n[3] == 20;
        t.inv = p + e.at[5];
        t.inv_len = e.n[5];
        t.first = t.inv_len ? t.inv[0] : 0;
        const u32 v = (u32)rawtx_be(p, e.at[6], (u32)e.n[6]);
        b0 = two ? v >> 8 : v;
        b1 = two ? v & 0xff : 0;
        const bool other = rawtx_lead_zero(e, 0, p) || e.n[1] == 0 || e.n[2] == 0 ||
                           (e.n[1] >= 2 && rawtx_lead_zero(e, 1, p)) || (e.n[2] >= 2 && rawtx_lead_zero(e, 2, p)) ||
                           rawtx_lead_zero(e, 4, p);
        det = (other ? 0 : RAWTX_SAME_ENCODING) | ((v == 2 * chain_id + 35 || v == 2 * chain_id + 36) ? RAWTX_CHAIN_OK : 0);
    }
    // To's 20 bytes are the last 20 of the padded 32
    t.to[0] = (to[1] >> 32) | (to[2] << 32);
    t.to[1] = (to[2] >> 32) | (to[3] << 32);
    t.to[2] = to[3] >> 32;

    status[i] = (uint8_t)st;
    if (detail) detail[i] = (uint8_t)det;
    if (txs) {                                         // lcb_tx_fields: words 0-2 the integers, 3-6 value, 7-9 to (and
        u64 *q = (u64 *)(txs + TX_REC_BYTES * i);      // From's first four bytes), 10-11 From, 12 to_len | reserved
        q[0] = t.nonce;
        q[1] = t.gas_price;
        q[2] = t.gas_limit;
#pragma unroll
        for (int j = 0; j < 4; j++) q[3 + j] = t.value[j];
        q[7] = t.to[0];
        q[8] = t.to[1];
        q[9] = t.to[2];
        q[10] = 0;
        q[11] = 0;
        q[12] = t.has_to ? 20 : 0;
    }
    if (span) {
        span[2 * i] = ok ? span_base + off[i] + e.at[5] : 0;
        span[2 * i + 1] = t.inv_len;
    }
    if (sigs) {
        uint8_t *sig = sigs + (size_t)sig_len * i;
        rbc_store_hash(sig, r);
        rbc_store_hash(sig + 32, s);
        sig[64] = (uint8_t)b0;
        if (two) sig[65] = (uint8_t)b1;
    }
    if (ok && defer_long && t.inv_len >= RAWTX_LONG) return true;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        const bool full = pass == 1;
        uint8_t *out = full ? full32 : raw32;
        if (!out) continue;
        u64 h[4] = {0, 0, 0, 0};
        if (ok) tx_hash(h, t, full, chain_id, r, s, b0, b1, two);
        rbc_store_hash(out + 32 * i, h);
    }
    return false;
}

// The decision of one item after the recovery: detail gains bit 2 where the signature recovered, accept = status 0 and
// all three bits, From = the recovered address where accepted (the decode left it zero)
SDI void rawtx_finish(size_t i, const uint8_t *status, const uint8_t *rec_ok, const uint8_t *addr20, const uint8_t *det_in,
                      uint8_t *accept, uint8_t *detail, uint8_t *txs) {
    const bool ok = status[i] == RAWTX_OK;
    const uint8_t d = ok ? (uint8_t)((det_in[i] & 3) | (rec_ok[i] ? RAWTX_RECOVERS : 0)) : 0;
    const bool acc = d == 7;
    accept[i] = acc;
    if (detail) detail[i] = d;
    if (txs && acc)
        for (int b = 0; b < 20; b++) txs[TX_REC_BYTES * i + TX_REC_FROM + b] = addr20[20 * i + b];
}
