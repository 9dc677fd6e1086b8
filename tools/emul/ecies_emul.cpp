// tools/emul/ecies_emul.cpp — TEST INFRASTRUCTURE: compiles lachain_amd/csrc/k_ecies.hip (and k_secp.hip, for the
// generator's comb table and d G) for the CPU and runs the kernels one lane at a time.  The only LDS use is the AES
// T-table, which is a plain array here, and the offsets scan has a serial host form, so sequential execution is exact.
// Lets the CPU suite check the ECDH ladder, the one-block SHA-256 and AES-256-GCM against tests/pyref/ecies.py and
// tests/golden/ecies_kats.json without a GPU, and counts field products per ECDH.  The product path never loads this.
//
// Shared library (tests/test_ecies_emul.py):  g++ -O1 -std=c++17 -fPIC -shared -o libecies_emul.so ecies_emul.cpp
// Stand-alone run of the KAT file's cases:    g++ -O1 -std=c++17 -DECIES_EMUL_MAIN -o ecies_emul ecies_emul.cpp
//                                             ./ecies_emul ../../tests/golden/ecies_kats.json
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
#include "../../lachain_amd/csrc/k_ecies.hip"

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
static void fill_te() {
    if (!emu_te[1])
        for (u32 x = 0; x < 256; x++) emu_te[x] = aes_te0_entry(x);
}
// the three ECDH kernels; returns the field products spent in k_ecdh_mul
static unsigned long long ecdh(uint8_t *key32, uint8_t *ok, const uint8_t *pub, const uint64_t *off, uint32_t min_len,
                               const uint8_t *scalars32, const uint32_t *idx, uint32_t n_scalars, uint32_t n) {
    std::vector<ecdh_job> jobs(n);
    std::vector<ecdh_point> pts(n);
    run(n, [&] { k_ecdh_scalars(pub, (const u64 *)off, min_len, scalars32, idx, n_scalars, n, jobs.data()); });
    unsigned long long p0 = emu_products;
    run(n, [&] { k_ecdh_mul(jobs.data(), n, pts.data()); });
    unsigned long long p1 = emu_products;
    run((n + SECP_BATCH - 1) / SECP_BATCH, [&] { k_ecdh_finish(pts.data(), n, key32, ok); });
    return p1 - p0;
}

extern "C" {
unsigned long long emu_ecdh(uint8_t *key32, uint8_t *ok, const uint8_t *pub33, const uint8_t *scalars32,
                            const uint32_t *idx, uint32_t n_scalars, uint32_t n) {
    return ecdh(key32, ok, pub33, nullptr, 0, scalars32, idx, n_scalars, n);
}
void emu_sha256_block(uint8_t *out32, const uint8_t *block64) {
    u32 w[16], h[8];
    for (int k = 0; k < 16; k++)
        w[k] = ((u32)block64[4 * k] << 24) | ((u32)block64[4 * k + 1] << 16) | ((u32)block64[4 * k + 2] << 8) | block64[4 * k + 3];
    sha256_init(h);
    sha256_compress(h, w);
    for (int k = 0; k < 32; k++) out32[k] = (uint8_t)(h[k / 4] >> (8 * (3 - k % 4)));
}
void emu_aes_sbox(uint8_t *out256) {
    fill_te();
    for (u32 x = 0; x < 256; x++) out256[x] = (uint8_t)AES_S(emu_te, x);
}
// out item i at (pt_off[i] - pt_off[0]) + 32 i
void emu_gcm_encrypt(uint8_t *out, const uint8_t *keys32, const uint8_t *nonces16, const uint8_t *pt,
                     const uint64_t *pt_off, uint32_t n) {
    fill_te();
    run(n, [&] { k_gcm_encrypt(keys32, nonces16, pt, (const u64 *)pt_off, n, out, nullptr, nullptr); });
}
// pt_out item i at the sum of the earlier items' plaintext lengths
void emu_gcm_decrypt(uint8_t *pt_out, uint8_t *ok, const uint8_t *keys32, const uint8_t *ct, const uint64_t *ct_off,
                     uint32_t n) {
    fill_te();
    std::vector<u64> oo(n + 1);
    k_gcm_offsets((const u64 *)ct_off, n, 32, oo.data());
    run(n, [&] { k_gcm_decrypt(keys32, ct, (const u64 *)ct_off, oo.data(), n, 0, pt_out, ok, nullptr); });
}
void emu_secp256k1_encrypt(uint8_t *out, uint8_t *ok, const uint8_t *recipient_pub33, const uint8_t *eph_priv32,
                           const uint8_t *nonces16, const uint8_t *pt, const uint64_t *pt_off, uint32_t n) {
    fill_te();
    std::vector<uint8_t> keys(32 * (size_t)n + 1), eph(33 * (size_t)n + 1), pok(n + 1);
    ecdh(keys.data(), ok, recipient_pub33, nullptr, 0, eph_priv32, nullptr, n, n);
    const secp_aff *gt = gen_table();
    run(n, [&] { k_secp_pubkey(eph_priv32, n, gt, eph.data(), pok.data()); });
    run(n, [&] { k_gcm_encrypt(keys.data(), nonces16, pt, (const u64 *)pt_off, n, out, eph.data(), ok); });
}
void emu_secp256k1_decrypt(uint8_t *pt_out, uint8_t *ok, const uint8_t *privs32, const uint32_t *priv_idx,
                           uint32_t n_privs, const uint8_t *ct, const uint64_t *ct_off, uint32_t n) {
    fill_te();
    std::vector<uint8_t> keys(32 * (size_t)n + 1), eok(n + 1);
    std::vector<u64> oo(n + 1);
    ecdh(keys.data(), eok.data(), ct, ct_off, 65, privs32, priv_idx, n_privs, n);
    k_gcm_offsets((const u64 *)ct_off, n, 65, oo.data());
    run(n, [&] { k_gcm_decrypt(keys.data(), ct, (const u64 *)ct_off, oo.data(), n, 33, pt_out, ok, eok.data()); });
}
}

#ifdef ECIES_EMUL_MAIN
// ---------------------------------------------------------------- stand-alone: every case of tests/golden/ecies_kats.json
#include <stdio.h>
#include <map>
#include <string>
typedef std::map<std::string, std::string> obj;
// the flat objects ("name": "hex" or number) of the array called `name`
static std::vector<obj> objects(const std::string &js, const char *name) {
    std::vector<obj> out;
    size_t p = js.find(std::string("\"") + name + "\"");
    if (p == std::string::npos) return out;
    p = js.find('[', p);
    int depth = 0;
    for (; p < js.size(); p++) {
        char c = js[p];
        if (c == '[') depth++;
        else if (c == ']') { if (--depth == 0) break; }
        else if (c == '{') {
            size_t e = js.find('}', p);
            std::string body = js.substr(p + 1, e - p - 1);
            obj o;
            size_t q = 0;
            while ((q = body.find('"', q)) != std::string::npos) {
                size_t q2 = body.find('"', q + 1);
                std::string key = body.substr(q + 1, q2 - q - 1);
                size_t v = body.find(':', q2) + 1;
                while (body[v] == ' ') v++;
                std::string val;
                if (body[v] == '"') { size_t v2 = body.find('"', v + 1); val = body.substr(v + 1, v2 - v - 1); q = v2 + 1; }
                else { size_t v2 = body.find_first_of(",}", v); val = body.substr(v, v2 == std::string::npos ? v2 : v2 - v); q = v2 == std::string::npos ? body.size() : v2; }
                o[key] = val;
            }
            out.push_back(o);
            p = e;
        }
    }
    return out;
}
// exact-size heap copies, so that a sanitizer sees any byte read past an item's end
static uint8_t *unhex(const std::string &h, size_t *len = nullptr) {
    size_t n = h.size() / 2;
    uint8_t *b = (uint8_t *)malloc(n ? n : 1);
    for (size_t i = 0; i < n; i++) b[i] = (uint8_t)strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
    if (len) *len = n;
    return b;
}
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s ecies_kats.json\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::string js;
    char buf[65536];
    size_t r;
    while ((r = fread(buf, 1, sizeof buf, f)) > 0) js.append(buf, r);
    fclose(f);
    int bad = 0, cases = 0;
    for (auto &o : objects(js, "gcm")) {
        size_t plen, clen;
        uint8_t *key = unhex(o["key"]), *nonce = unhex(o["nonce"]), *pt = unhex(o["pt"], &plen), *want = unhex(o["out"], &clen);
        uint64_t off[2] = {0, plen}, coff[2] = {0, clen};
        uint8_t *out = (uint8_t *)malloc(plen + 32), *back = (uint8_t *)malloc(plen ? plen : 1), ok = 0;
        emu_gcm_encrypt(out, key, nonce, pt, off, 1);
        emu_gcm_decrypt(back, &ok, key, want, coff, 1);
        bool good = clen == plen + 32 && !memcmp(out, want, clen) && ok == 1 && !memcmp(back, pt, plen);
        want[clen - 1] ^= 1;
        emu_gcm_decrypt(back, &ok, key, want, coff, 1);
        good = good && ok == 0;
        printf("gcm len %zu: %s\n", plen, good ? "ok" : "MISMATCH");
        bad += !good; cases++;
        free(key); free(nonce); free(pt); free(want); free(out); free(back);
    }
    unsigned long long products = 0, ecdh_ok = 0;
    for (auto &o : objects(js, "ecdh")) {
        uint8_t *pub = unhex(o["pub"]), *d = unhex(o["scalar"]), *want = unhex(o["key"]), key[32], ok = 0;
        unsigned long long p = emu_ecdh(key, &ok, pub, d, nullptr, 1, 1);
        bool good = ok == 1 && !memcmp(key, want, 32);
        if (!good) printf("ecdh %s: MISMATCH\n", o["scalar"].c_str());
        products += p; ecdh_ok++;
        bad += !good; cases++;
        free(pub); free(d); free(want);
    }
    if (ecdh_ok) printf("ecdh: %llu cases, %.1f field products per multiplication\n", ecdh_ok, (double)products / ecdh_ok);
    for (auto &o : objects(js, "envelopes")) {
        size_t plen, elen;
        uint8_t *priv = unhex(o["recipient_priv"]), *pub = unhex(o["recipient_pub"]), *eph = unhex(o["eph_priv"]);
        uint8_t *nonce = unhex(o["nonce"]), *pt = unhex(o["pt"], &plen), *want = unhex(o["envelope"], &elen);
        uint64_t off[2] = {0, plen}, coff[2] = {0, elen};
        uint8_t *out = (uint8_t *)malloc(plen + 65), *back = (uint8_t *)malloc(plen ? plen : 1), ok = 0, ok2 = 0;
        emu_secp256k1_encrypt(out, &ok, pub, eph, nonce, pt, off, 1);
        emu_secp256k1_decrypt(back, &ok2, priv, nullptr, 1, want, coff, 1);
        bool good = elen == plen + 65 && ok == 1 && !memcmp(out, want, elen) && ok2 == 1 && !memcmp(back, pt, plen);
        printf("envelope len %zu: %s\n", plen, good ? "ok" : "MISMATCH");
        bad += !good; cases++;
        free(priv); free(pub); free(eph); free(nonce); free(pt); free(want); free(out); free(back);
    }
    printf("%d cases, %d failed\n", cases, bad);
    return bad || !cases ? 1 : 0;
}
#endif
