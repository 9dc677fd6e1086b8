// tools/emul/txhash_emul.cpp — TEST INFRASTRUCTURE: a stand-alone program that compiles the transaction-hash lane
// (lachain_amd/csrc/txhash_lane.hpp) for the CPU and runs it one item at a time, so the CPU suite checks it against
// tests/pyref/txhash.py without a GPU (tests/test_tx_emul.py builds it with -fsanitize=address,undefined).
//
//   txhash_emul <cases> <results>
// cases:   u32 n | u32 sig_len (0: no signatures) | u32 chain_id | u32 0 | n records of 104 bytes | n + 1 u64 offsets |
//          the invocations back to back | n signatures | n claimed hashes
// results: per item raw hash (32) | full hash (32) | match byte
//
// Every item is run from heap buffers of its own that end with the last aligned 64-bit word holding one of its bytes:
// the invocation at its offset's alignment (offset mod 8) in a buffer of (alignment + length) rounded up to 8 bytes, the
// signature likewise at the alignment it has in the packed array.  The lane's loads are aligned words that hold at
// least one byte of the item, so a load of any other word lands outside the buffer and the sanitizer reports it.
#define RBC_HOST_EMULATION
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#define __constant__
#include "../../lachain_amd/csrc/txhash_lane.hpp"

static std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> d;
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(f);
    return d;
}

// `len` bytes at offset `align` of a fresh buffer of (align + len) rounded up to whole words
static uint8_t *place(const uint8_t *src, size_t len, size_t align, uint8_t **base) {
    size_t size = (align + len + 7) / 8 * 8;
    if (len == 0) size = 0;
    *base = (uint8_t *)malloc(size);                    // malloc aligns to 16
    if (size) memset(*base, 0xa5, size);
    if (len) memcpy(*base + align, src, len);
    return *base + align;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: txhash_emul <cases> <results>\n"); return 2; }
    const std::vector<uint8_t> in = read_file(argv[1]);
    if (in.size() < 16) { fprintf(stderr, "short case file\n"); return 2; }
    uint32_t hdr[4];
    memcpy(hdr, in.data(), 16);
    const size_t n = hdr[0], sig_len = hdr[1];
    const uint32_t chain_id = hdr[2];
    size_t pos = 16;
    const uint8_t *recs = in.data() + pos;
    pos += TX_REC_BYTES * n;
    std::vector<uint64_t> off(n + 1);
    if (in.size() < pos + 8 * (n + 1)) { fprintf(stderr, "short case file\n"); return 2; }
    memcpy(off.data(), in.data() + pos, 8 * (n + 1));
    pos += 8 * (n + 1);
    const uint8_t *inv = in.data() + pos;
    pos += off[n];
    const uint8_t *sigs = in.data() + pos;
    pos += sig_len * n;
    const uint8_t *claimed = in.data() + pos;
    pos += 32 * n;
    if (in.size() != pos) { fprintf(stderr, "case file is %zu bytes, expected %zu\n", in.size(), pos); return 2; }
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    for (size_t i = 0; i < n; i++) {
        uint8_t *b_rec, *b_inv, *b_sig = nullptr, *b_claim;
        uint8_t *rec = place(recs + TX_REC_BYTES * i, TX_REC_BYTES, 0, &b_rec);
        const size_t len = off[i + 1] - off[i], a = off[i] % 8;
        uint8_t *item = place(inv + off[i], len, a, &b_inv);
        uint8_t *sig = sig_len ? place(sigs + sig_len * i, sig_len, (sig_len * i) % 8, &b_sig) : nullptr;
        uint8_t *claim = place(claimed + 32 * i, 32, 0, &b_claim);
        uint8_t *out = (uint8_t *)malloc(65);
        memset(out, 0, 65);
        const u64 one[2] = {0, len};                    // the lane reads off[i], off[i + 1] and inv + off[i]
        tx_lane(0, rec, item, one, sig, (u32)sig_len, claim, chain_id, out, sig ? out + 32 : nullptr,
                sig ? out + 64 : nullptr);
        fwrite(out, 1, 65, fo);
        free(out);
        free(b_rec);
        free(b_inv);
        free(b_sig);
        free(b_claim);
    }
    fclose(fo);
    return 0;
}
