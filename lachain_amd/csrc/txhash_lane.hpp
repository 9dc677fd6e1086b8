// lachain_amd/csrc/txhash_lane.hpp — the per-lane pieces of the transaction hashing kernel (k_txhash.hip): the RLP of a
// transaction is never materialised; a lane forms the list header and every element prefix in registers and feeds
// them, the field bytes and the invocation (streamed from global memory) into one Keccak-256 sponge kept in registers.
// No LDS, no barriers, so tools/emul/txhash_emul.cpp (RBC_HOST_EMULATION) runs the lane on the CPU.
//
// Reference: TransactionUtils.cs:30-105 (GetEthTx, Rlp, LAEncodeSigned, RawHash, FullHash), HexUtils.cs:88-92
// (TrimLeadingZeros leaves an all-zero array whole), Nethereum RLP.EncodeElement / EncodeList.
//   RawHash  = Keccak-256(list[nonce, gasPrice, gasLimit, to, value, invocation, chainId, "", ""])
//   FullHash = Keccak-256(list[nonce, gasPrice, gasLimit, to, value, invocation, v, r, s])
// nonce: empty when 0; gasPrice, gasLimit, chainId: minimal big-endian, zero is the byte 00; to: 20 bytes or none;
// value, r, s: 32 bytes with leading zeros stripped, nothing left when zero; v: sig[64 .. sig_len) stripped unless all
// zero (then whole).  One pass per hash: the two encodings differ in the list header, so their streams may run at
// different byte phases; a second pass re-reads the invocation.
#pragma once
#include "rbc_lane.hpp"

// lcb_tx_fields (include/lachain_bls.h), 104 bytes, 8-byte aligned
#define TX_REC_BYTES 104
#define TX_REC_FROM 76

// ------------------------------------------------------------------------------------------------ the sponge
// s: the state; acc: the stream's current, partly filled word (nb bytes, low byte first); w: the word of the rate block
// that acc will go to.  A full word is XORed into its place through a select chain, so the state is never indexed by a
// register and stays in VGPRs.  The permutation is inlined at two places only (the invocation loop and the finish), so
// the three stretches of the stream place their words differently:
//   TXS_HEAD    the list header and the elements before the invocation's bytes: at most 91 bytes, always inside the
//               first block, no permutation
//   TXS_BODY    the invocation's bytes: a permutation whenever the block is full (tx_put_six's loop)
//   TXS_TAIL    the elements after the invocation: at most 69 bytes, which cross at most one block boundary; words
//               past the block wait in ov[] until the finish has permuted
#define TXS_HEAD 0
#define TXS_BODY 1
#define TXS_TAIL 2
struct tx_sponge {
    u64 s[25];
    u64 ov[9];
    u64 acc;
    u32 nb, w;
};
SDI void txs_init(tx_sponge &p) {
#pragma unroll
    for (int l = 0; l < 25; l++) p.s[l] = 0;
#pragma unroll
    for (int l = 0; l < 9; l++) p.ov[l] = 0;
    p.acc = 0;
    p.nb = 0;
    p.w = 0;
}
template <int PART> SDI void txs_xor_word(tx_sponge &p, u64 v) {
#pragma unroll
    for (int l = 0; l < (PART == TXS_HEAD ? 12 : 17); l++) p.s[l] ^= (p.w == (u32)l) ? v : 0;
    if (PART == TXS_TAIL) {
#pragma unroll
        for (int l = 0; l < 9; l++) p.ov[l] ^= (p.w == (u32)(17 + l)) ? v : 0;
    }
}
template <int PART> SDI void txs_emit(tx_sponge &p, u64 v) {
    txs_xor_word<PART>(p, v);
    p.w++;                                             // TXS_BODY: the caller permutes when this reaches 17
}
// k stream bytes (1 .. 8) held in the low bytes of v, first byte lowest; the bytes of v above k must be zero
template <int PART> SDI void txs_put(tx_sponge &p, u64 v, u32 k) {
    const u32 sh = 8 * p.nb;
    p.acc |= v << sh;
    u32 t = p.nb + k;
    if (t >= 8) {
        txs_emit<PART>(p, p.acc);
        p.acc = (v >> 1) >> (63 - sh);                 // the bytes that did not fit (none when nb was 0)
        t -= 8;
    }
    p.nb = t;
}
// the original Keccak padding (0x01 .. 0x80, rate 136) and the last one or two permutations; the hash is s[0 .. 3]
SDI void txs_finish(tx_sponge &p) {
    txs_xor_word<TXS_TAIL>(p, p.acc | ((u64)0x01 << (8 * p.nb)));
    u32 blocks = p.w >= 17 ? 2 : 1;
#pragma unroll 1
    for (;;) {
        if (blocks == 1) p.s[16] ^= 0x8000000000000000ULL;
        keccak_f1600(p.s);
        if (--blocks == 0) break;
#pragma unroll
        for (int l = 0; l < 9; l++) p.s[l] ^= p.ov[l];
    }
}

// ------------------------------------------------------------------------------------------------ lengths
SDI u32 tx_clz64(u64 x) {
#ifdef RBC_HOST_EMULATION
    return x ? (u32)__builtin_clzll(x) : 64;
#else
    return x ? (u32)__clzll((long long)x) : 64;
#endif
}
SDI u32 tx_ctz64(u64 x) {
#ifdef RBC_HOST_EMULATION
    return x ? (u32)__builtin_ctzll(x) : 64;
#else
    return x ? (u32)(__ffsll((unsigned long long)x) - 1) : 64;
#endif
}
SDI u64 tx_bswap64(u64 x) {
    x = ((x & 0x00ff00ff00ff00ffULL) << 8) | ((x >> 8) & 0x00ff00ff00ff00ffULL);
    x = ((x & 0x0000ffff0000ffffULL) << 16) | ((x >> 16) & 0x0000ffff0000ffffULL);
    return (x << 32) | (x >> 32);
}
SDI u32 tx_be_bytes(u64 x) { return (64 - tx_clz64(x) + 7) / 8; }          // minimal big-endian width, 0 for 0
// the string header's (or, with base 0xc0, the list header's) width for a body of n bytes
SDI u32 tx_hdr_len(u64 n) { return n < 56 ? 1 : 1 + tx_be_bytes(n); }
template <int PART> SDI void tx_put_hdr(tx_sponge &p, u64 n, u32 base) {
    if (n < 56) {
        txs_put<PART>(p, base + n, 1);
    } else {
        const u32 ll = tx_be_bytes(n);
        txs_put<PART>(p, base + 55 + ll, 1);
        txs_put<PART>(p, tx_bswap64(n) >> (8 * (8 - ll)), ll);
    }
}

// an integer element: minimal big-endian; zero is the empty string (nonce) or the byte 00 (everything else)
SDI u32 tx_int_len(u64 x) {                            // one byte for zero either way
    const u32 L = tx_be_bytes(x);
    return (L == 0 || (L == 1 && x < 0x80)) ? 1 : 1 + L;
}
template <int PART> SDI void tx_put_int(tx_sponge &p, u64 x, bool empty_when_zero) {
    const u32 L = tx_be_bytes(x);
    if (L == 0) {
        txs_put<PART>(p, empty_when_zero ? 0x80 : 0x00, 1);
    } else if (L == 1 && x < 0x80) {
        txs_put<PART>(p, x, 1);
    } else {
        txs_put<PART>(p, 0x80 + L, 1);
        txs_put<PART>(p, tx_bswap64(x) >> (8 * (8 - L)), L);
    }
}

// a 32-byte big-endian string in memory order (four little-endian words) with its leading zero bytes stripped; all
// zero gives the empty string (value: UInt256.ToBytes(false, true); r, s: TrimLeadingZeros, then the zero check)
SDI u32 tx_lead_zero32(const u64 v[4]) {
    u32 z = 0;
    bool run = true;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const u32 zj = tx_ctz64(v[j]) / 8;
        z += run ? zj : 0;
        run = run && zj == 8;
    }
    return z;
}
SDI u32 tx_str32_len(const u64 v[4]) {
    const u32 L = 32 - tx_lead_zero32(v);
    return (L == 0 || (L == 1 && (v[3] >> 56) < 0x80)) ? 1 : 1 + L;
}
template <int PART> SDI void tx_put_str32(tx_sponge &p, const u64 v[4]) {
    const u32 skip = tx_lead_zero32(v), L = 32 - skip;
    if (L == 0) { txs_put<PART>(p, 0x80, 1); return; }
    if (!(L == 1 && (v[3] >> 56) < 0x80)) txs_put<PART>(p, 0x80 + L, 1);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (skip >= 8u * j + 8) continue;
        if (skip <= 8u * j) txs_put<PART>(p, v[j], 8);
        else txs_put<PART>(p, v[j] >> (8 * (skip - 8u * j)), 8u * j + 8 - skip);
    }
}

// v = sig[64 .. sig_len), one or two bytes: leading zeros stripped unless every byte is zero (then whole)
SDI u32 tx_v_len(u32 b0, u32 b1, bool two) {
    if (!two) return b0 < 0x80 ? 1 : 2;
    if (b0) return 3;
    if (!b1) return 3;                                  // 82 00 00
    return b1 < 0x80 ? 1 : 2;
}
template <int PART> SDI void tx_put_v(tx_sponge &p, u32 b0, u32 b1, bool two) {
    if (two && (b0 || !b1)) { txs_put<PART>(p, 0x82 | (b0 << 8) | (b1 << 16), 3); return; }
    const u32 b = two ? b1 : b0;
    if (b < 0x80) txs_put<PART>(p, b, 1);
    else txs_put<PART>(p, 0x81 | (b << 8), 2);
}

// ------------------------------------------------------------------------------------------------ one transaction
struct tx_item {
    u64 nonce, gas_price, gas_limit;
    u64 value[4];
    u64 to[3];          // 20 bytes in memory order; to[2] holds four
    bool has_to;
    const uint8_t *inv; // the invocation's bytes, any alignment
    u64 inv_len;
    u32 first;          // its first byte (a one-byte invocation below 0x80 is its own encoding)
};
SDI void tx_load(tx_item &t, const uint8_t *rec, const uint8_t *inv, u64 inv_len) {
    const u64 *q = (const u64 *)rec;                   // words 0-2 the integers, 3-6 value, 7-9 to (and From's first
    t.nonce = q[0];                                    // four bytes), 12 to_len
    t.gas_price = q[1];
    t.gas_limit = q[2];
#pragma unroll
    for (int j = 0; j < 4; j++) t.value[j] = q[3 + j];
    t.to[0] = q[7];
    t.to[1] = q[8];
    t.to[2] = q[9] & 0xffffffffULL;
    t.has_to = (u32)q[12] == 20;
    t.inv = inv;
    t.inv_len = inv_len;
    t.first = inv_len ? inv[0] : 0;
}
// the six shared elements' encoded length
SDI u64 tx_six_len(const tx_item &t) {
    u64 n = tx_int_len(t.nonce) + tx_int_len(t.gas_price) + tx_int_len(t.gas_limit);
    n += t.has_to ? 21 : 1;
    n += tx_str32_len(t.value);
    if (t.inv_len == 0 || (t.inv_len == 1 && t.first < 0x80)) n += 1;
    else n += tx_hdr_len(t.inv_len) + t.inv_len;
    return n;
}
// the list header and the six shared elements: whole words of the invocation by rbc_load64 (two aligned loads and a
// funnel shift; both words hold bytes of the item), the last 1 .. 7 bytes one by one
SDI void tx_put_six(tx_sponge &p, const tx_item &t, u64 payload) {
    tx_put_hdr<TXS_HEAD>(p, payload, 0xc0);
    tx_put_int<TXS_HEAD>(p, t.nonce, true);
    tx_put_int<TXS_HEAD>(p, t.gas_price, false);
    tx_put_int<TXS_HEAD>(p, t.gas_limit, false);
    if (t.has_to) {
        txs_put<TXS_HEAD>(p, 0x94, 1);
        txs_put<TXS_HEAD>(p, t.to[0], 8);
        txs_put<TXS_HEAD>(p, t.to[1], 8);
        txs_put<TXS_HEAD>(p, t.to[2], 4);
    } else {
        txs_put<TXS_HEAD>(p, 0x80, 1);
    }
    tx_put_str32<TXS_HEAD>(p, t.value);
    if (t.inv_len == 0) { txs_put<TXS_HEAD>(p, 0x80, 1); return; }
    if (!(t.inv_len == 1 && t.first < 0x80)) tx_put_hdr<TXS_HEAD>(p, t.inv_len, 0x80);
    u64 g = 0;
#pragma unroll 1
    for (;;) {                                         // one inlined permutation for whole blocks, words and tail alike
        bool full, last = false;
        if (p.w == 0 && g + 136 <= t.inv_len) {        // a whole rate block at the stream's byte phase, words in place
            const u32 sh = 8 * p.nb;
#pragma unroll
            for (int l = 0; l < 17; l++) {
                const u64 v = rbc_load64(t.inv + g + 8 * l);
                p.s[l] ^= p.acc | (v << sh);
                p.acc = (v >> 1) >> (63 - sh);
            }
            g += 136;
            full = true;
        } else {
            u64 v = 0;
            u32 k = 8;
            if (g + 8 <= t.inv_len) {
                v = rbc_load64(t.inv + g);
            } else {
                k = (u32)(t.inv_len - g);
                for (u32 b = 0; b < k; b++) v |= (u64)t.inv[g + b] << (8 * b);
                last = true;
            }
            if (k) txs_put<TXS_BODY>(p, v, k);
            g += 8;
            full = p.w == 17;
        }
        if (full) {
            keccak_f1600(p.s);
            p.w = 0;
        }
        if (last) break;
    }
}

// One hash of transaction t: RawHash (full = false; chain_id is TransactionUtils.ChainId(useNewId), a positive int) or
// FullHash (full = true; r, s: the signature's halves in memory order, b0 / b1: its one or two trailing bytes)
SDI void tx_hash(u64 out[4], const tx_item &t, bool full, u32 chain_id, const u64 r[4], const u64 s[4], u32 b0, u32 b1,
                 bool two) {
    tx_sponge p;
    txs_init(p);
    const u64 six = tx_six_len(t);
    tx_put_six(p, t, six + (full ? tx_v_len(b0, b1, two) + tx_str32_len(r) + tx_str32_len(s)
                                 : tx_int_len(chain_id) + 2));
    if (!full) {
        tx_put_int<TXS_TAIL>(p, chain_id, false);
        txs_put<TXS_TAIL>(p, 0x8080, 2);
    } else {
        tx_put_v<TXS_TAIL>(p, b0, b1, two);
        tx_put_str32<TXS_TAIL>(p, r);
        tx_put_str32<TXS_TAIL>(p, s);
    }
    txs_finish(p);
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = p.s[j];
}

// Lane i of a call: txs + 104 i, invocation bytes inv[off[i] .. off[i + 1]), signature sigs + sig_len i (sigs may be
// null: RawHash only).  Outputs, each nullable: raw32, full32 (32 bytes per item) and match[i] = FullHash equals
// claimed + 32 i.
SDI void tx_lane(size_t i, const uint8_t *txs, const uint8_t *inv, const u64 *off, const uint8_t *sigs, u32 sig_len,
                 const uint8_t *claimed, u32 chain_id, uint8_t *raw32, uint8_t *full32, uint8_t *match) {
    tx_item t;
    tx_load(t, txs + TX_REC_BYTES * i, inv + off[i], off[i + 1] - off[i]);
    u64 r[4] = {0, 0, 0, 0}, s[4] = {0, 0, 0, 0};
    u32 b0 = 0, b1 = 0;
    const bool two = sig_len == 66;
    if (sigs) {
        const uint8_t *sig = sigs + (size_t)sig_len * i;
        rbc_load_hash(r, sig);
        rbc_load_hash(s, sig + 32);
        b0 = sig[64];
        b1 = two ? sig[65] : 0;
    }
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        const bool full = pass == 1;
        if (full ? (!sigs || (!full32 && !match)) : !raw32) continue;
        u64 h[4];
        tx_hash(h, t, full, chain_id, r, s, b0, b1, two);
        if (!full) {
            rbc_store_hash(raw32 + 32 * i, h);
        } else {
            if (full32) rbc_store_hash(full32 + 32 * i, h);
            if (match) {
                u64 c[4];
                rbc_load_hash(c, claimed + 32 * i);
                match[i] = h[0] == c[0] && h[1] == c[1] && h[2] == c[2] && h[3] == c[3];
            }
        }
    }
}
