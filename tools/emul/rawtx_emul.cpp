// tools/emul/rawtx_emul.cpp — TEST INFRASTRUCTURE: a stand-alone program that compiles the raw-transaction lane
// (lachain_amd/csrc/rawtx_lane.hpp) for the CPU and runs it one item at a time, so the CPU suite checks it against
// tests/pyref/rawtx.py without a GPU (tests/test_rawtx_emul.py builds it with -fsanitize=address,undefined).
//
//   rawtx_emul <cases> <results>
// cases:   u32 n | u32 sig_len | u32 chain_id | u32 0 | n + 1 u64 offsets | the items back to back
// results: per item status | detail | record (104) | span (2 u64) | signature (sig_len) | raw hash (32) | full hash (32)
//
// Every item is run from a heap buffer of its own that ends with the last aligned 64-bit word holding one of its bytes:
// the item at its offset's alignment (offset mod 8) in a buffer of (alignment + length) rounded up to 8 bytes.  The
// lane reads single bytes inside the item and aligned words that hold at least one of its bytes, so a read of anything
// else lands outside the buffer and the sanitizer reports it.  Each output has an exact-size buffer as well.  The lane
// runs as the kernels run it: first with defer_long (k_rawtx_decode), and again without it when it asks to be listed
// (k_rawtx_long).
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
#include "../../lachain_amd/csrc/rawtx_lane.hpp"

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

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: rawtx_emul <cases> <results>\n"); return 2; }
    const std::vector<uint8_t> in = read_file(argv[1]);
    if (in.size() < 16) { fprintf(stderr, "short case file\n"); return 2; }
    uint32_t hdr[4];
    memcpy(hdr, in.data(), 16);
    const size_t n = hdr[0], sig_len = hdr[1];
    const uint32_t chain_id = hdr[2];
    if (sig_len != 65 && sig_len != 66) { fprintf(stderr, "sig_len must be 65 or 66\n"); return 2; }
    size_t pos = 16;
    std::vector<uint64_t> off(n + 1);
    if (in.size() < pos + 8 * (n + 1)) { fprintf(stderr, "short case file\n"); return 2; }
    memcpy(off.data(), in.data() + pos, 8 * (n + 1));
    pos += 8 * (n + 1);
    const uint8_t *raw = in.data() + pos;
    if (in.size() != pos + off[n]) { fprintf(stderr, "case file is %zu bytes, expected %zu\n", in.size(), pos + (size_t)off[n]); return 2; }
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    for (size_t i = 0; i < n; i++) {
        const size_t len = off[i + 1] - off[i], a = off[i] % 8;
        const size_t size = len ? (a + len + 7) / 8 * 8 : 0;
        uint8_t *base = (uint8_t *)malloc(size);            // malloc aligns to 16
        if (size) memset(base, 0xa5, size);
        if (len) memcpy(base + a, raw + off[i], len);
        uint8_t *status = (uint8_t *)malloc(1), *detail = (uint8_t *)malloc(1), *sig = (uint8_t *)malloc(sig_len);
        uint8_t *rec = (uint8_t *)malloc(TX_REC_BYTES), *raw32 = (uint8_t *)malloc(32), *full32 = (uint8_t *)malloc(32);
        u64 *span = (u64 *)malloc(16);
        *status = *detail = 0xa5;
        memset(sig, 0xa5, sig_len);
        memset(rec, 0xa5, TX_REC_BYTES);
        memset(raw32, 0xa5, 32);
        memset(full32, 0xa5, 32);
        memset(span, 0xa5, 16);
        const u64 one[2] = {0, len};                        // the lane reads off[i], off[i + 1] and raw + off[i]
        if (rawtx_lane(0, base + a, one, off[i], (u32)sig_len, chain_id, true, status, detail, rec, span, sig, raw32, full32))
            rawtx_lane(0, base + a, one, off[i], (u32)sig_len, chain_id, false, status, detail, rec, span, sig, raw32, full32);
        fwrite(status, 1, 1, fo);
        fwrite(detail, 1, 1, fo);
        fwrite(rec, 1, TX_REC_BYTES, fo);
        fwrite(span, 1, 16, fo);
        fwrite(sig, 1, sig_len, fo);
        fwrite(raw32, 1, 32, fo);
        fwrite(full32, 1, 32, fo);
        free(base); free(status); free(detail); free(sig); free(rec); free(raw32); free(full32); free(span);
    }
    fclose(fo);
    return 0;
}
