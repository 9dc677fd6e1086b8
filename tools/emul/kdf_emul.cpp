// tools/emul/kdf_emul.cpp — TEST INFRASTRUCTURE: a stand-alone program that compiles the TPKE keystream lane
// (lachain_amd/csrc/kdf_lane.hpp, the body of k_kdf_xor) for the CPU and runs it one item at a time, so the CPU suite
// checks it against the oracle without a GPU (tests/test_kdf_emul.py builds it with -fsanitize=address,undefined).
//
//   kdf_emul <cases> <results>
// cases: u32 n | u32 data_align | u32 seed_align | u32 out_align, then n + 1 u32 seed offsets | n + 1 u32 data offsets |
//        n ok bytes | the seed material back to back | the data back to back (both offset lists start at 0)
// results: the output bytes, packed as the data
// Item i lies at alignment (data_align + data_off[i]) % 8, its seed at (seed_align + seed_off[i]) % 8 and its output at
// (out_align + data_off[i]) % 8, as in packed arrays whose bases have those alignments; out_align = 8 is in place.
// Every input is run from a heap buffer of its own that starts with the aligned 64-bit word holding its first byte and
// ends with the one holding its last: the lane's loads are aligned words that hold at least one byte of the item, so a
// load of any other word lands outside the buffer and the sanitizer reports it.  The output buffer ends with the item's
// last byte, so a store past it is reported too; the bytes before the item in its first word are guard bytes checked
// here.  In place the output is the data's buffer (out == data) and all of its bytes outside the item are guards.
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
#include "../../lachain_amd/csrc/kdf_lane.hpp"

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
struct Reader {
    const std::vector<uint8_t> &d;
    size_t pos;
    const uint8_t *take(size_t n) {
        if (d.size() < pos + n) { fprintf(stderr, "short case file\n"); exit(2); }
        const uint8_t *p = d.data() + pos;
        pos += n;
        return p;
    }
    std::vector<uint32_t> words(size_t n) {
        std::vector<uint32_t> v(n);
        if (n) memcpy(v.data(), take(4 * n), 4 * n);
        return v;
    }
};

#define GUARD 0xa5
// `len` bytes at offset `align` of a fresh buffer of `size` bytes, guard bytes around them
static uint8_t *place(const uint8_t *src, size_t len, size_t align, size_t size, uint8_t **base) {
    *base = (uint8_t *)malloc(size);                    // malloc aligns to 16
    if (size) memset(*base, GUARD, size);
    if (len && src) memcpy(*base + align, src, len);
    return *base + align;
}
static size_t whole_words(size_t align, size_t len) { return len ? (align + len + 7) / 8 * 8 : 0; }
static bool guards_ok(const uint8_t *base, size_t size, size_t align, size_t len) {
    for (size_t k = 0; k < size; k++)
        if ((k < align || k >= align + len) && base[k] != GUARD) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: kdf_emul <cases> <results>\n"); return 2; }
    const std::vector<uint8_t> in = read_file(argv[1]);
    Reader r = {in, 0};
    uint32_t hdr[4];
    memcpy(hdr, r.take(16), 16);
    const size_t n = hdr[0], data_align = hdr[1] % 8, seed_align = hdr[2] % 8, out_align = hdr[3] % 8;
    const bool in_place = hdr[3] == 8;
    const std::vector<uint32_t> soff = r.words(n + 1), doff = r.words(n + 1);
    const uint8_t *ok = r.take(n);
    const uint8_t *seeds = r.take(soff[n]);
    const uint8_t *data = r.take(doff[n]);
    if (in.size() != r.pos) { fprintf(stderr, "case file is %zu bytes, expected %zu\n", in.size(), r.pos); return 2; }
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    for (size_t i = 0; i < n; i++) {
        if (soff[i + 1] < soff[i] || doff[i + 1] < doff[i]) { fprintf(stderr, "offsets decrease at %zu\n", i); return 2; }
        const size_t slen = soff[i + 1] - soff[i], len = doff[i + 1] - doff[i];
        const size_t sa = (seed_align + soff[i]) % 8, da = (data_align + doff[i]) % 8;
        uint8_t *b_seed, *b_data, *b_out = nullptr;
        const size_t data_size = whole_words(da, len);
        uint8_t *seed = place(seeds + soff[i], slen, sa, whole_words(sa, slen), &b_seed);
        uint8_t *item = place(data + doff[i], len, da, data_size, &b_data);
        const size_t oa = in_place ? da : (out_align + doff[i]) % 8;
        const size_t out_size = len ? oa + len : 0;
        uint8_t *out = in_place ? item : place(nullptr, 0, oa, out_size, &b_out);
        kdf_xor_item(out, seed, slen, item, len, ok[i] != 0);
        if (!guards_ok(in_place ? b_data : b_out, in_place ? data_size : out_size, oa, len)) {
            fprintf(stderr, "item %zu: a byte outside the output range was written\n", i);
            return 1;
        }
        if (len) fwrite(out, 1, len, fo);
        free(b_seed);
        free(b_data);
        free(b_out);
    }
    fclose(fo);
    return 0;
}
