// tools/emul/rbc_emul.cpp — TEST INFRASTRUCTURE: compiles the per-lane pieces of the reliable-broadcast Merkle kernels
// (lachain_amd/csrc/rbc_lane.hpp: Keccak-256 of a byte range, the 64-byte node hash, CheckEchoMessage's walk,
// ComputeRoot's pairing) for the CPU and runs them one lane at a time, so the CPU suite checks them against
// tests/pyref/rbc_merkle.py without a GPU.  The tree kernel's barrier structure is not emulated: its levels are replayed
// here by plain loops over the same per-lane functions.  The product path never loads this library.
#define RBC_HOST_EMULATION
#include <stdint.h>
#include <string.h>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#define __constant__
#include "../../lachain_amd/csrc/rbc_lane.hpp"

extern "C" {
// Keccak-256 of n byte ranges data[off[i] .. off[i + 1])
void emu_rbc_absorb(uint8_t *out32, const uint8_t *data, const uint64_t *off, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
        u64 h[4];
        rbc_keccak_range(h, data + off[i], off[i + 1] - off[i]);
        rbc_store_hash(out32 + 32 * i, h);
    }
}
void emu_rbc_node(uint8_t *out32, const uint8_t *l32, const uint8_t *r32) {
    u64 l[4], r[4], h[4];
    rbc_load_hash(l, l32);
    rbc_load_hash(r, r32);
    rbc_node_hash(h, l, r);
    rbc_store_hash(out32, h);
}
int emu_rbc_depth(int n) { return rbc_depth(n); }
// the echo kernel, item by item
void emu_rbc_echo(uint8_t *accept, const uint8_t *data, const uint64_t *doff, const int32_t *from, const uint8_t *roots,
                  const uint8_t *proofs, const uint64_t *poff, uint32_t n_items, int n) {
    for (uint32_t t = 0; t < n_items; t++) {
        u64 leaf[4];
        rbc_keccak_range(leaf, data + doff[t], doff[t + 1] - doff[t]);
        accept[t] = rbc_echo_walk(leaf, from[t], n, proofs + 32 * poff[t], poff[t + 1] - poff[t], roots + 32 * (size_t)t);
    }
}
// the root kernel's levels for one tree of count hashes; returns 0 for no hashes
int emu_merkle_root(uint8_t *root32, const uint8_t *hashes, uint64_t count) {
    if (!count) { memset(root32, 0, 32); return 0; }
    std::vector<uint8_t> cur(hashes, hashes + 32 * count), nxt;
    while (count > 1) {
        uint64_t p = (count + 1) / 2;
        nxt.assign(32 * p, 0);
        for (uint64_t i = 0; i < p; i++) {
            u64 h[4];
            rbc_root_pair(h, cur.data(), i, count);
            rbc_store_hash(nxt.data() + 32 * i, h);
        }
        cur.swap(nxt);
        count = p;
    }
    memcpy(root32, cur.data(), 32);
    return 1;
}
}
