// lachain_amd/csrc/keccak.hpp — the Keccak-f[1600] permutation, one state per lane (25 x 64-bit words in registers).
// Shared by the secp256k1 translation units (header hashes, addresses, k_keccak256: included through secp.hpp) and the
// reliable-broadcast Merkle kernels (k_rbc.hip).  Compiles for the host when the including file defines __device__ /
// __forceinline__ / __constant__ away (tools/emul).
#pragma once
#include <stdint.h>

typedef uint32_t u32;
typedef uint64_t u64;
#ifndef SDI
#define SDI __device__ __forceinline__
#endif

// ------------------------------------------------------------------------------------------------ Keccak-f[1600]
__constant__ static const u64 SECP_KRC[24] = {
    0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
    0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
    0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
    0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
    0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
    0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
SDI u64 rotl64(u64 v, int r) { return r ? (v << r) | (v >> (64 - r)) : v; }
SDI void keccak_f1600(u64 *s) {
    const int rot[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    for (int round = 0; round < 24; round++) {
        u64 C[5], D[5], B[25];
#pragma unroll
        for (int x = 0; x < 5; x++) C[x] = s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) D[x] = C[(x + 4) % 5] ^ rotl64(C[(x + 1) % 5], 1);
#pragma unroll
        for (int i = 0; i < 25; i++) s[i] ^= D[i % 5];
#pragma unroll
        for (int x = 0; x < 5; x++)
#pragma unroll
            for (int y = 0; y < 5; y++) B[y + 5 * ((2 * x + 3 * y) % 5)] = rotl64(s[x + 5 * y], rot[x + 5 * y]);
#pragma unroll
        for (int x = 0; x < 5; x++)
#pragma unroll
            for (int y = 0; y < 5; y++) s[x + 5 * y] = B[x + 5 * y] ^ ((~B[(x + 1) % 5 + 5 * y]) & B[(x + 2) % 5 + 5 * y]);
        s[0] ^= SECP_KRC[round];
    }
}
