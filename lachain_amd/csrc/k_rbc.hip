// lachain_amd/csrc/k_rbc.hip — gfx950 kernels: the Keccak-256 Merkle layer of the reliable broadcast (SURVEY.md §8f
// row 3) and the block transaction root.
//
// Reference: ReliableBroadcast.cs:296-309 (CheckEchoMessage), :311-319 (AugmentInput), :366-386 (MerkleTreeBranch,
// ConstructMerkleTree); MerkleTree.cs:139-191 (ComputeRoot).  The per-lane hashing lives in rbc_lane.hpp.
//
//   k_rbc_augment   AugmentInput: int32 LE length | payload | zero padding, written as the k data shards of each instance
//   k_rbc_tree      one workgroup per instance: leaf hashes (one lane per shard), the 2T-node heap in LDS, one barrier
//                   per level; writes the whole tree, or the root and the N branches
//   k_rbc_echo      one lane per ECHO: leaf hash, <= log2(T) node hashes, compare with the claimed root
//   k_merkle_root   one workgroup per tree of any size: levels ping-pong in a workspace, odd last node paired with itself
#include "rbc_lane.hpp"
#include "gate.hpp"

#define RBC_BLOCK 256
#define RBC_MAX_T 256
typedef unsigned long long ull;

// instance b = blockIdx.y: payload[poff[b] .. poff[b + 1]) -> the first k * S bytes of its shard area at
// shards + soff[b] (n * S bytes, S = (soff[b + 1] - soff[b]) / n); one lane per byte
extern "C" __global__ void __launch_bounds__(RBC_BLOCK) k_rbc_augment(const uint8_t *payload, const ull *poff,
                                                                     uint8_t *shards, const ull *soff, int n, int k) {
    const size_t b = blockIdx.y;
    const u64 len = poff[b + 1] - poff[b];
    const u64 S = (soff[b + 1] - soff[b]) / (u64)n;
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= S * (u64)k) return;
    uint8_t v = 0;
    if (g < 4) v = (uint8_t)(len >> (8 * g));
    else if (g - 4 < len) v = payload[poff[b] + g - 4];
    shards[soff[b] + g] = v;
}

// instance b = blockIdx.x: n shards of S = (soff[b + 1] - soff[b]) / n bytes at shards + soff[b].  node[T + i] =
// Keccak(shard i), zero for i >= n; node[i] = Keccak(node[2i] || node[2i + 1]); node[0] = 0.  Outputs (each may be
// null): trees b x 2T hashes; roots b x 1; proofs b x n x depth, proofs[b][i][j] = node[((i + T) >> j) ^ 1].
// Every thread reaches every barrier: the block-wide loops bound work by index, nothing returns early.
extern "C" __global__ void __launch_bounds__(RBC_BLOCK) k_rbc_tree(const uint8_t *shards, const ull *soff, int n, int depth,
                                                                  u64 *trees, u64 *roots, u64 *proofs) {
    __shared__ u64 node[2 * RBC_MAX_T * 4];
    const int T = 1 << depth;
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const u64 S = (soff[b + 1] - soff[b]) / (u64)n;
    for (int i = tid; i < T; i += RBC_BLOCK) {
        u64 h[4] = {0, 0, 0, 0};
        if (i < n) rbc_keccak_range(h, shards + soff[b] + (u64)i * S, S);
#pragma unroll
        for (int w = 0; w < 4; w++) node[4 * (T + i) + w] = h[w];
    }
    if (tid < 4) node[tid] = 0;
    for (int w = T >> 1; w >= 1; w >>= 1) {
        __syncthreads();
        for (int i = w + tid; i < 2 * w; i += RBC_BLOCK) {
            u64 h[4];
            rbc_node_hash(h, &node[8 * i], &node[8 * i + 4]);
#pragma unroll
            for (int q = 0; q < 4; q++) node[4 * i + q] = h[q];
        }
    }
    __syncthreads();
    if (trees)
        for (int t = tid; t < 8 * T; t += RBC_BLOCK) trees[b * 8 * T + t] = node[t];
    if (roots && tid < 4) roots[4 * b + tid] = node[4 + tid];
    if (proofs)
        for (int t = tid; t < n * depth * 4; t += RBC_BLOCK) {
            const int q = t & 3, j = (t >> 2) % depth, i = (t >> 2) / depth;
            proofs[(b * n * depth) * 4 + t] = node[4 * (((i + T) >> j) ^ 1) + q];
        }
}

// item t: data[doff[t] .. doff[t + 1]) claimed to be shard from[t] under roots[t] with proof hashes
// proofs[poff[t] .. poff[t + 1]) (offsets in hashes).  accept[t] = CheckEchoMessage.  Items are independent: lengths
// and proof lengths may differ from lane to lane.
extern "C" __global__ void __launch_bounds__(RBC_BLOCK) k_rbc_echo(uint8_t *accept, const uint8_t *data, const ull *doff,
                                                                  const int *from, const uint8_t *roots,
                                                                  const uint8_t *proofs, const ull *poff, u32 n_items,
                                                                  int n) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_items) return;
    u64 leaf[4];
    rbc_keccak_range(leaf, data + doff[t], doff[t + 1] - doff[t]);
    accept[t] = rbc_echo_walk(leaf, from[t], n, proofs + 32 * poff[t], poff[t + 1] - poff[t], roots + 32 * (size_t)t);
}

// tree t = blockIdx.x: hashes[off[t] .. off[t + 1]) (offsets in hashes).  0 hashes: status 0, root zero; 1 hash: itself;
// otherwise MerkleTree.Build level by level.  The levels alternate between two areas of the tree's own slice of the
// workspace, ws + 32 * off[t]: c / 2 rounded up nodes, then c / 4 rounded up, which together never exceed c.  The level
// count is uniform over the block, so every thread reaches every barrier.
extern "C" __global__ void __launch_bounds__(RBC_BLOCK) k_merkle_root(uint8_t *roots, uint8_t *status, const uint8_t *hashes,
                                                                     const ull *off, uint8_t *ws) {
    const size_t t = blockIdx.x;
    const int tid = threadIdx.x;
    u64 c = off[t + 1] - off[t];
    const uint8_t *cur = hashes + 32 * off[t];
    uint8_t *bufa = ws + 32 * off[t], *bufb = bufa + 32 * ((c + 1) / 2);
    if (tid == 0) status[t] = c != 0;
    if (c == 0) {
        if (tid < 32) roots[32 * t + tid] = 0;
        return;
    }
    uint8_t *nxt = bufa;
    while (c > 1) {
        const u64 p = (c + 1) / 2;
        for (u64 i = tid; i < p; i += RBC_BLOCK) {
            u64 h[4];
            rbc_root_pair(h, cur, i, c);
            rbc_store_hash(nxt + 32 * i, h);
        }
        __syncthreads();
        cur = nxt;
        nxt = nxt == bufa ? bufb : bufa;
        c = p;
    }
    if (tid == 0) {
        u64 h[4];
        rbc_load_hash(h, cur);
        rbc_store_hash(roots + 32 * t, h);
    }
}

// ---------------------------------------------------------------- host launch wrappers
extern "C" void lcbk_rbc_augment(hipStream_t s, const uint8_t *payload, const uint64_t *poff, uint8_t *shards,
                                 const uint64_t *soff, int n, int k, size_t max_bytes, unsigned B) {
    if (!B || !max_bytes) return;
    LCB_LAUNCH_GATED(k_rbc_augment, dim3((unsigned)((max_bytes + RBC_BLOCK - 1) / RBC_BLOCK), B), dim3(RBC_BLOCK), 0, s,
                     payload, (const ull *)poff, shards, (const ull *)soff, n, k);
}
extern "C" void lcbk_rbc_tree(hipStream_t s, const uint8_t *shards, const uint64_t *soff, int n, int depth, void *trees,
                              void *roots, void *proofs, unsigned B) {
    if (!B) return;
    LCB_LAUNCH_GATED(k_rbc_tree, dim3(B), dim3(RBC_BLOCK), 0, s, shards, (const ull *)soff, n, depth, (u64 *)trees,
                     (u64 *)roots, (u64 *)proofs);
}
extern "C" void lcbk_rbc_echo(hipStream_t s, uint8_t *accept, const uint8_t *data, const uint64_t *doff, const int *from,
                              const uint8_t *roots, const uint8_t *proofs, const uint64_t *poff, u32 n_items, int n) {
    if (!n_items) return;
    LCB_LAUNCH_GATED(k_rbc_echo, dim3((n_items + RBC_BLOCK - 1) / RBC_BLOCK), dim3(RBC_BLOCK), 0, s, accept, data,
                     (const ull *)doff, from, roots, proofs, (const ull *)poff, n_items, n);
}
extern "C" void lcbk_merkle_root(hipStream_t s, uint8_t *roots, uint8_t *status, const uint8_t *hashes, const uint64_t *off,
                                 uint8_t *ws, unsigned n_trees) {
    if (!n_trees) return;
    LCB_LAUNCH_GATED(k_merkle_root, dim3(n_trees), dim3(RBC_BLOCK), 0, s, roots, status, hashes, (const ull *)off, ws);
}
