// lachain_amd/csrc/k_kdf.hip — gfx950 kernel: the TPKE keystream, Utils.XorWithHash for a batch (TPKE/Utils.cs:12-19).
// The per-lane generator and its memory discipline live in kdf_lane.hpp.
//
//   k_kdf_xor   one item per lane, the sponge in registers, no LDS, no scratch.  Item i: seed material
//               seeds[seed_off[i] .. seed_off[i + 1]) (seed_off == null: seeds[stride i .. stride (i + 1)), the TPKE
//               paths' 48-byte G1 points), data[data_off[i] .. data_off[i + 1]), out packed as data.  ok (nullable):
//               a lane with ok[i] == 0 writes zero bytes and reads neither seed nor data.
// The chain of an item is sequential (one permutation per 32 bytes), so a wave runs as long as its longest item; blocks
// of one wave keep a long item from holding back more than its 63 neighbours.
#include "kdf_lane.hpp"
#include "gate.hpp"

#define KDF_BLOCK 64

extern "C" __global__ void __launch_bounds__(KDF_BLOCK) k_kdf_xor(uint8_t *out, const uint8_t *seeds, const u32 *seed_off,
                                                                u32 seed_stride, const uint8_t *data, const u32 *data_off,
                                                                const uint8_t *ok, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 d0 = data_off[i], d1 = data_off[i + 1];
    const uint8_t *m = seed_off ? seeds + seed_off[i] : seeds + (size_t)seed_stride * i;
    const u64 mlen = seed_off ? seed_off[i + 1] - seed_off[i] : seed_stride;
    kdf_xor_item(out + d0, m, mlen, data + d0, d1 - d0, ok ? ok[i] != 0 : true);
}

// PublicKey.FullDecrypt's evaluation points (TPKE/PublicKey.cs:74-84): xs[e] = Fr.FromInt(ids[e] + 1), 32 bytes little-endian;
// a negative value is r minus its magnitude (at most 2^31, below r's lowest word: no borrow)
extern "C" __global__ void __launch_bounds__(256) k_tpke_ids_to_x(const int *ids, u32 ne, u64 *xs) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const long long v = (long long)ids[e] + 1;
    u64 w[4] = {(u64)v, 0, 0, 0};
    if (v < 0) {
        w[0] = 0xffffffff00000001ULL - (u64)(-v);
        w[1] = 0x53bda402fffe5bfeULL;
        w[2] = 0x3339d80809a1d805ULL;
        w[3] = 0x73eda753299d7d48ULL;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) xs[4 * (size_t)e + k] = w[k];
}

// ---------------------------------------------------------------- host launch wrappers
static unsigned kdf_blocks(u32 n) { return (n + KDF_BLOCK - 1) / KDF_BLOCK; }
extern "C" void lcbk_tpke_ids_to_x(hipStream_t s, const int32_t *ids, u32 ne, uint8_t *xs) {
    if (!ne) return;
    LCB_LAUNCH_GATED(k_tpke_ids_to_x, dim3((ne + 255) / 256), dim3(256), 0, s, (const int *)ids, ne, (u64 *)xs);
}
extern "C" void lcbk_kdf_xor(hipStream_t s, uint8_t *out, const uint8_t *seeds, const uint32_t *seed_off, const uint8_t *data,
                             const uint32_t *data_off, const uint8_t *ok, u32 n) {
    if (!n) return;
    LCB_LAUNCH_GATED(k_kdf_xor, dim3(kdf_blocks(n)), dim3(KDF_BLOCK), 0, s, out, seeds, seed_off, 0u, data, data_off, ok, n);
}
extern "C" void lcbk_kdf_xor_strided(hipStream_t s, uint8_t *out, const uint8_t *seeds, u32 seed_stride, const uint8_t *data,
                                     const uint32_t *data_off, const uint8_t *ok, u32 n) {
    if (!n) return;
    LCB_LAUNCH_GATED(k_kdf_xor, dim3(kdf_blocks(n)), dim3(KDF_BLOCK), 0, s, out, seeds, (const u32 *)nullptr, seed_stride,
                     data, data_off, ok, n);
}
