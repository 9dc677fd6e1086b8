// tools/emul/secp_recover_emul.cpp — TEST INFRASTRUCTURE: compiles lachain_amd/csrc/k_secp_recover.hip (and k_secp.hip,
// for the generator's comb table) for the CPU and runs the kernels one lane at a time (no LDS, no barriers, so
// sequential execution is exact).  Lets the CPU suite check the recovery pipeline, the scalar split, the endomorphism
// and the variable-length Keccak against the oracle without a GPU, and counts field products per recovery.  The
// product path never loads this library.
#define SECP_HOST_EMULATION
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
struct emu_dim3 { unsigned x = 0, y = 0, z = 0; };
static emu_dim3 blockIdx, threadIdx, blockDim, gridDim;
static unsigned long long emu_products = 0;
#define SECP_COUNT_PRODUCT() (++emu_products)
#define __device__
#define __host__
#define __forceinline__ inline
#define __noinline__
#define __global__
#define __constant__
#define __launch_bounds__(...)
#include "../../lachain_amd/csrc/k_secp.hip"
#include "../../lachain_amd/csrc/k_secp_recover.hip"

template <class F> static void run(size_t lanes, F f) {
    blockDim.x = 256;
    gridDim.x = (unsigned)((lanes + 255) / 256);
    for (unsigned b = 0; b < gridDim.x; b++)
        for (unsigned t = 0; t < 256; t++) {
            blockIdx.x = b;
            threadIdx.x = t;
            f();
        }
}
static std::vector<secp_aff> g_gtab;
static const secp_aff *gen_table() {
    if (g_gtab.empty()) {
        std::vector<secp_aff> gaff(1);
        std::vector<u32> gok(1);
        g_gtab.resize(33 * 128);
        blockIdx.x = threadIdx.x = 0;
        k_secp_gen(gaff.data(), gok.data());
        std::vector<fe> tmp(2 * 128 * 33);
        run(33, [&] { k_secp_comb_build(gaff.data(), gok.data(), 1, g_gtab.data(), tmp.data(), tmp.data() + 128 * 33); });
    }
    return g_gtab.data();
}

extern "C" {
// u2 (32 B little-endian) -> magnitudes (32 B little-endian each), signs, and the ladder's digits (36 each)
void emu_glv_split(uint8_t *m1, int *neg1, uint8_t *m2, int *neg2, int8_t *e1, int8_t *e2, const uint8_t *k) {
    u32 kk[8], a[8], b[8];
    bool n1, n2;
    memcpy(kk, k, 32);
    glv_split(a, n1, b, n2, kk);
    memcpy(m1, a, 32); memcpy(m2, b, 32);
    *neg1 = n1; *neg2 = n2;
    recode4(e1, a, n1);
    recode4(e2, b, n2);
}
// phi(x, y) = (beta x, y): canonical 32-byte little-endian coordinates
void emu_phi(uint8_t *xo, const uint8_t *x) {
    fe a, r;
    memcpy(&a, x, 32);
    fe_mul(r, a, fe_from(SECP_BETA));
    r = fe_canon(r);
    memcpy(xo, &r, 32);
}
// the whole pipeline; from20 / accept may be null.  Returns the field products spent in the recovery kernel and,
// through products3, in the three kernels (scalars, recovery, finish).
unsigned long long emu_recover(uint8_t *pub33, uint8_t *addr20, uint8_t *ok, uint8_t *accept, const uint8_t *hashes,
                               const uint8_t *sigs, uint32_t sig_len, const uint8_t *from20, uint32_t n, int special,
                               int use_new, int chain_id, unsigned long long *products3) {
    const secp_aff *gt = gen_table();
    std::vector<secp_rjob> jobs(n);
    std::vector<secp_rpoint> pts(n);
    u32 want = special ? 65 : (use_new ? 66 : 65);
    size_t threads = (n + SECP_BATCH - 1) / SECP_BATCH;
    unsigned long long p0 = emu_products;
    run(threads, [&] { k_secp_rec_scalars(hashes, sigs, sig_len, want, chain_id, special, n, jobs.data()); });
    unsigned long long p1 = emu_products;
    run(n, [&] { k_secp_recover(jobs.data(), n, gt, pts.data()); });
    unsigned long long p2 = emu_products;
    run(threads, [&] { k_secp_rec_finish(pts.data(), n, pub33, addr20, ok, from20, accept); });
    unsigned long long p3 = emu_products;
    if (products3) { products3[0] = p1 - p0; products3[1] = p2 - p1; products3[2] = p3 - p2; }
    return p2 - p1;
}
// the test hook's routine switch (secp_debug.hpp) over n items, on the C++ field operations: the layout of
// lcb_debug_secp_op; b may be null for the operations of one operand
void emu_debug_secp_op(int op, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out) {
    if (!b) b = a;
    for (size_t i = 0; i < n; i++)
        secp_debug_op(op, a + SECP_DEBUG_IN * i, b + SECP_DEBUG_IN * i, out + SECP_DEBUG_OUT * i);
}
void emu_keccak256(uint8_t *out32, const uint8_t *data, const uint64_t *off, uint32_t n) {
    run(n, [&] { k_keccak256(data, (const u64 *)off, n, out32); });
}
}
