// tools/emul/trie_emul.cpp — TEST INFRASTRUCTURE: a stand-alone program that compiles the state-trie lane
// (lachain_amd/csrc/trie_lane.hpp) for the CPU and runs it one item at a time, so the CPU suite checks it against
// tests/pyref/trie.py without a GPU (tests/test_trie_emul.py builds it with -fsanitize=address,undefined).
//
//   trie_emul <cases> <results>
// cases: u32 mode | u32 n | u32 n_literals | u32 0, then
//   mode 0 (flat nodes, k_trie_flat's lane):  n records of 16 bytes | n + 1 u64 offsets | the items back to back
//           results: 32 bytes per node
//   mode 1 (items, k_trie_items' lane):       n key hashes of 32 bytes | n + 1 u64 value offsets | the values
//           results per item: 51 bytes trie_fragment | the path key (32) | 51 bytes trie_pk_fragment | the leaf hash
//           from the key hash in registers (32) | the common prefix with the item before (1 byte, 255 for the first)
//   mode 2 (rehash, k_trie_level's lane):     records | offsets | items | n + 1 u64 child offsets | the int64 references |
//           n_literals hashes | n u64: the order, children before parents
//           results: 32 bytes per node
// Every item is run from a heap buffer of its own that ends with the last aligned 64-bit word holding one of its
// bytes, at the alignment it has in the packed array: the lane's loads are aligned words that hold at least one byte of
// the item, so a load of any other word lands outside the buffer and the sanitizer reports it.
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
#include "../../lachain_amd/csrc/trie_lane.hpp"

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
    std::vector<uint64_t> words(size_t n) {
        std::vector<uint64_t> v(n);
        if (n) memcpy(v.data(), take(8 * n), 8 * n);
        return v;
    }
};

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
    if (argc != 3) { fprintf(stderr, "usage: trie_emul <cases> <results>\n"); return 2; }
    const std::vector<uint8_t> in = read_file(argv[1]);
    Reader r = {in, 0};
    uint32_t hdr[4];
    memcpy(hdr, r.take(16), 16);
    const uint32_t mode = hdr[0];
    const size_t n = hdr[1], n_lit = hdr[2];
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    if (mode == 0) {
        const uint8_t *recs = r.take(TRIE_NODE_BYTES * n);
        const std::vector<uint64_t> off = r.words(n + 1);
        const uint8_t *data = r.take(off[n]);
        for (size_t i = 0; i < n; i++) {
            uint8_t *b_rec, *b_item;
            uint8_t *rec = place(recs + TRIE_NODE_BYTES * i, TRIE_NODE_BYTES, 0, &b_rec);
            const size_t len = off[i + 1] - off[i];
            uint8_t *item = place(data + off[i], len, off[i] % 8, &b_item);
            const u64 one[2] = {0, len};
            u64 h[4];
            trie_node_hash(h, rec, item, one, 0);
            uint8_t out[33], want[32];
            memset(out, 0, sizeof out);
            trie_node_finish(h, 0, out, nullptr, nullptr);
            memcpy(want, out, 32);
            trie_node_finish(h, 0, nullptr, want, out + 32);      // the comparison path: must accept its own hash
            if (out[32] != 1) { fprintf(stderr, "node %zu: accept path disagrees\n", i); return 1; }
            fwrite(out, 1, 32, fo);
            free(b_rec);
            free(b_item);
        }
    } else if (mode == 1) {
        const uint8_t *khs = r.take(32 * n);
        const std::vector<uint64_t> off = r.words(n + 1);
        const uint8_t *vals = r.take(off[n]);
        u64 prev[4] = {0, 0, 0, 0};
        for (size_t i = 0; i < n; i++) {
            uint8_t *b_kh, *b_val;
            uint8_t *khm = place(khs + 32 * i, 32, (5 * i) % 8, &b_kh);
            const size_t len = off[i + 1] - off[i];
            uint8_t *val = place(vals + off[i], len, off[i] % 8, &b_val);
            u64 kh[4], pk[4], h[4];
            rbc_load_hash(kh, khm);
            uint8_t out[51 + 32 + 51 + 32 + 1];
            for (int f = 0; f < TRIE_FRAGMENTS; f++) out[f] = (uint8_t)trie_fragment(kh, f);
            trie_path_key(pk, kh);
            memcpy(out + 51, pk, 32);
            for (int f = 0; f < TRIE_FRAGMENTS; f++) out[83 + f] = (uint8_t)trie_pk_fragment(pk, f);
            trie_leaf_hash<true>(h, 32, kh, val, len);
            memcpy(out + 134, h, 32);
            out[166] = i ? (uint8_t)trie_pk_lcp(pk, prev) : 255;
            memcpy(prev, pk, 32);
            fwrite(out, 1, sizeof out, fo);
            free(b_kh);
            free(b_val);
        }
    } else if (mode == 2) {
        const uint8_t *recs = r.take(TRIE_NODE_BYTES * n);
        const std::vector<uint64_t> off = r.words(n + 1);
        const uint8_t *data = r.take(off[n]);
        const std::vector<uint64_t> coff = r.words(n + 1);
        const std::vector<uint64_t> refs_raw = r.words(coff[n]);
        uint8_t *b_lit, *b_hash;
        uint8_t *lits = place(r.take(32 * n_lit), 32 * n_lit, 0, &b_lit);
        const std::vector<uint64_t> order = r.words(n);
        uint8_t *hashes = place(std::vector<uint8_t>(32 * n + 1).data(), 32 * n, 0, &b_hash);
        for (size_t t = 0; t < n; t++) {
            const size_t i = (size_t)order[t];
            if (i >= n) { fprintf(stderr, "order out of range\n"); return 2; }
            const u32 *rec = (const u32 *)(recs + TRIE_NODE_BYTES * i);
            u64 h[4];
            if (rec[0] == TRIE_LEAF) {
                uint8_t *b_item;
                const size_t len = off[i + 1] - off[i];
                uint8_t *item = place(data + off[i], len, off[i] % 8, &b_item);
                trie_leaf_hash<false>(h, rec[2], nullptr, item, len);
                free(b_item);
            } else {
                const size_t c = coff[i + 1] - coff[i];
                std::vector<int64_t> mine(c);               // exact size: a reference past the node's own is reported
                for (size_t k = 0; k < c; k++) mine[k] = (int64_t)refs_raw[coff[i] + k];
                trie_children_ref ch = {mine.data(), hashes, lits};
                trie_internal_hash(h, rec[1], (u32)(c < 33 ? c : 33), ch);
            }
            rbc_store_hash(hashes + 32 * i, h);
        }
        fwrite(hashes, 1, 32 * n, fo);
        free(b_lit);
        free(b_hash);
    } else {
        fprintf(stderr, "unknown mode %u\n", mode);
        return 2;
    }
    if (in.size() != r.pos) { fprintf(stderr, "case file is %zu bytes, expected %zu\n", in.size(), r.pos); return 2; }
    fclose(fo);
    return 0;
}
