// lachain_amd/csrc/kdf_lane.hpp — the per-lane pieces of the TPKE keystream (k_kdf.hip): Utils.XorWithHash, i.e.
// BouncyCastle's DigestRandomGenerator(Sha3Digest) seeded once and XORed over a payload.  One item per lane, one
// sponge per lane in registers, no LDS, no barriers, so tools/emul/kdf_emul.cpp (RBC_HOST_EMULATION) runs it item by
// item on the CPU.
//
// Reference: TPKE/Utils.cs:12-19 (XorWithHash), pinned by CryptographyTest.cs:103-113; host restatement host_sha3.hpp.
// SHA3-256: rate 136, padding byte 0x06, final byte 0x80.  A hash is four little-endian 64-bit words.
//   seed = state = 0^32, seed_ctr = state_ctr = 1
//   AddSeedMaterial(m):  seed = SHA3(m || seed)                              (|m| + 32) / 136 + 1 permutations
//   GenerateState:       state = SHA3(le64(state_ctr++) || state || seed)    one permutation; afterwards, when
//                        state_ctr % 10 == 0, seed = SHA3(seed || le64(seed_ctr++))
//   NextBytes(n):        GenerateState up front, 32 bytes per state, GenerateState again when a further byte is needed
// The chain is sequential within an item (each state hashes the one before), so the item is the unit of parallelism.
//
// Memory discipline.  Items lie at any byte alignment and their neighbours belong to other lanes.
//   reads   whole aligned words by rbc_load64 (each holds at least one byte of the item), bytes in a last partial word
//   writes  bytes up to the first 8-byte boundary of the output range and after the last one, aligned words in
//           between; no byte outside the range is written and no word shared with a neighbour is read and written back
// out == data (in place, the same packing) works: word t of an item is read before any store reaches it, because the
// stores trail the loads by the output's distance to its first boundary.  Any other overlap of out and data is not
// supported.
#pragma once
#include "rbc_lane.hpp"

// AddSeedMaterial on the initial (zero) seed: sd = SHA3-256(m[0 .. len) || sd).  Message words by rbc_load64; behind
// the message the 32 seed bytes and the padding byte follow at the message's byte phase, taken from a five-word queue
// that shifts by one word per step (no register array is indexed by a register).
SDI void kdf_add_seed(u64 sd[4], const uint8_t *m, u64 len) {
    u64 s[25];
#pragma unroll
    for (int l = 0; l < 25; l++) s[l] = 0;
    const u32 nb = (u32)(len & 7);                     // message bytes in the word the message ends in
    u64 t0 = sd[0], t1 = sd[1], t2 = sd[2], t3 = sd[3], t4 = 0x06;
    u64 prev = 0;                                      // the bytes before the queue's head, in the top nb bytes
    for (u32 k = 0; k < nb; k++) prev |= (u64)m[len - nb + k] << (8 * (8 - nb + k));
    const u64 blocks = (len + 32) / 136 + 1;
#pragma unroll 1
    for (u64 b = 0; b < blocks; b++) {
        const u64 base = b * 136;
        if (base + 136 <= len) {                       // a whole rate block inside the message
#pragma unroll
            for (int l = 0; l < 17; l++) s[l] ^= rbc_load64(m + base + 8 * l);
        } else {
#pragma unroll
            for (int l = 0; l < 17; l++) {
                const u64 g = base + 8 * l;
                u64 v;
                if (g + 8 <= len) v = rbc_load64(m + g);
                else {                                 // nb bytes of what came before, then 8 - nb of the queue's head
                    v = ((prev >> 1) >> (63 - 8 * nb)) | (t0 << (8 * nb));
                    prev = t0; t0 = t1; t1 = t2; t2 = t3; t3 = t4; t4 = 0;
                }
                s[l] ^= v;
            }
        }
        if (b + 1 == blocks) s[16] ^= 0x8000000000000000ULL;
        keccak_f1600(s);
    }
#pragma unroll
    for (int w = 0; w < 4; w++) sd[w] = s[w];
}

// GenerateState: st = SHA3-256(le64(ctr) || st || sd), 72 bytes in one block
SDI void kdf_generate_state(u64 st[4], const u64 sd[4], u64 ctr) {
    u64 s[25];
    s[0] = ctr;
#pragma unroll
    for (int w = 0; w < 4; w++) { s[1 + w] = st[w]; s[5 + w] = sd[w]; }
    s[9] = 0x06;
#pragma unroll
    for (int l = 10; l < 25; l++) s[l] = 0;
    s[16] = 0x8000000000000000ULL;
    keccak_f1600(s);
#pragma unroll
    for (int w = 0; w < 4; w++) st[w] = s[w];
}
// the seed's cycle: sd = SHA3-256(sd || le64(ctr)), 40 bytes in one block
SDI void kdf_cycle_seed(u64 sd[4], u64 ctr) {
    u64 s[25];
#pragma unroll
    for (int w = 0; w < 4; w++) s[w] = sd[w];
    s[4] = ctr;
    s[5] = 0x06;
#pragma unroll
    for (int l = 6; l < 25; l++) s[l] = 0;
    s[16] = 0x8000000000000000ULL;
    keccak_f1600(s);
#pragma unroll
    for (int w = 0; w < 4; w++) sd[w] = s[w];
}

// The write-out.  Output word t (bytes 8t .. 8t + 8 of the item) is produced in order; with h = the bytes up to the
// output's first 8-byte boundary (0 .. 7), an aligned store covers item bytes [8t - 8 + h, 8t + h): the top 8 - h
// bytes of the word before and the low h bytes of this one.
SDI void kdf_put(uint8_t *o, u32 h, u64 t, u64 prev, u64 cur) {
    if (h == 0) *(u64 *)(o + 8 * t) = cur;
    else if (t == 0) {
        for (u32 k = 0; k < h; k++) o[k] = (uint8_t)(cur >> (8 * k));
    } else *(u64 *)(o + 8 * t - 8 + h) = (prev >> (8 * h)) | (cur << (64 - 8 * h));
}
// the end of the item: T whole words were put, cur holds the last c (0 .. 7) bytes
SDI void kdf_finish(uint8_t *o, u32 h, u64 T, u64 prev, u64 cur, u32 c) {
    u32 from = 0;                                      // the bytes of cur still to store: from .. c
    if (h != 0 && T != 0) {                            // the top 8 - h bytes of prev are pending
        if (c >= h) {
            *(u64 *)(o + 8 * T - 8 + h) = (prev >> (8 * h)) | (cur << (64 - 8 * h));
            from = h;
        } else {
            for (u32 k = h; k < 8; k++) o[8 * T - 8 + k] = (uint8_t)(prev >> (8 * k));
        }
    }
    for (u32 k = from; k < c; k++) o[8 * T + k] = (uint8_t)(cur >> (8 * k));
}

// out[0 .. n) = data[0 .. n) ^ keystream(seed material m[0 .. mlen)); live == false writes n zero bytes instead and
// reads nothing.  n == 0 touches no memory (the up-front state of an empty NextBytes is never used).
SDI void kdf_xor_item(uint8_t *out, const uint8_t *m, u64 mlen, const uint8_t *data, u64 n, bool live) {
    if (n == 0) return;
    u64 sd[4] = {0, 0, 0, 0}, st[4] = {0, 0, 0, 0};
    if (live) kdf_add_seed(sd, m, mlen);
    const u32 h = (u32)((8 - ((uintptr_t)out & 7)) & 7);
    const u64 T = n >> 3, blocks = (n + 31) >> 5;
    const u32 c = (u32)(n & 7);
    u64 state_ctr = 1, seed_ctr = 1;
    u32 until = 9;                                     // states until state_ctr is a multiple of 10
    u64 prev = 0, last = 0;
#pragma unroll 1
    for (u64 b = 0; b < blocks; b++) {
        if (live) {
            kdf_generate_state(st, sd, state_ctr++);
            if (--until == 0) {
                kdf_cycle_seed(sd, seed_ctr++);
                until = 10;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64 t = 4 * b + j;
            if (t < T) {
                const u64 cur = live ? rbc_load64(data + 8 * t) ^ st[j] : 0;
                kdf_put(out, h, t, prev, cur);
                prev = cur;
            } else if (t == T && c != 0 && live) {
                u64 v = 0;
                for (u32 k = 0; k < c; k++) v |= (u64)data[8 * T + k] << (8 * k);
                last = v ^ st[j];
            }
        }
    }
    kdf_finish(out, h, T, prev, last, c);
}
