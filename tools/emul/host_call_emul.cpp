// tools/emul/host_call_emul.cpp — TEST INFRASTRUCTURE: the host-pointer forms' staging scope (lachain_amd/csrc/
// host_call.hpp: HostCall and rebase) on a stand-in HIP runtime whose device memory is the heap at its exact size
// (tools/emul/hip_stub).  Built with -fsanitize=address,undefined by tests/test_host_call_emul.py; exit 0 and a silent
// sanitizer mean every case below held.  The product path never builds this file.
#include <stdio.h>
#include <string>
#include <vector>

#include "../../lachain_amd/csrc/lcb_internal.hpp"

// what host_call.hpp takes from lcb_host.cpp
static std::string g_err;
static int g_err_count = 0;
static bool g_sync_ok = true;
size_t lcb_verify_chunk_now() { return 1; }
void lcb_int::set_err(const char *what, hipError_t) { g_err = what; g_err_count++; }
bool lcb_int::sync_check(lcb_ctx *, const char *what) {
    if (!g_sync_ok) set_err(what);
    return g_sync_ok;
}

using namespace lcb_int;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

static std::vector<uint8_t> pattern(size_t n, uint8_t seed) {
    std::vector<uint8_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (uint8_t)(seed + 7 * i);
    return v;
}
static void release(lcb_ctx &c) {
    for (auto &b : c.stage) b.release();
}

// three inputs and two outputs of the given sizes: five distinct slots in request order, contents round-trip
static void five_slots(lcb_ctx &c, size_t a, size_t b, size_t d, size_t o1, size_t o2) {
    auto va = pattern(a, 1), vb = pattern(b, 2), vd = pattern(d, 3);
    HostCall h(&c, "order");
    const int first = c.stage_next;
    const uint8_t *da = h.in(va.data(), a), *db = h.in(vb.data(), b);
    uint8_t *dd = h.work(vd.data(), d);             // the same copy, writable
    uint8_t *x = h.out<uint8_t>(o1);
    uint32_t *y = h.out<uint32_t>(o2);
    CHECK(h.ok() && c.stage_next == first + 5);
    const void *p[5] = {da, db, dd, x, y};
    for (int i = 0; i < 5; i++) {
        CHECK(p[i] && p[i] == c.stage[first + i].p);
        for (int j = 0; j < i; j++) CHECK(p[i] != p[j]);
    }
    CHECK(c.stage[first + 4].cap >= 4 * o2);
    memset(x, 0x5a, o1);
    for (size_t i = 0; i < o2; i++) y[i] = (uint32_t)(i * 2654435761u);
    std::vector<uint8_t> ra(a), rb(b), rd(d), rx(o1);
    std::vector<uint32_t> ry(o2);
    h.back(ra.data(), da, a);
    h.back(rb.data(), db, b);
    h.back(rd.data(), dd, d);
    h.back(rx.data(), x, o1);
    h.back(ry.data(), y, 4 * o2);
    CHECK(h.finish() == 0);
    CHECK(ra == va && rb == vb && rd == vd);
    CHECK(rx == std::vector<uint8_t>(o1, 0x5a));
    for (size_t i = 0; i < o2; i++) CHECK(ry[i] == (uint32_t)(i * 2654435761u));
}

static void test_order_and_reuse() {
    lcb_ctx c;
    five_slots(c, 100, 33, 7, 64, 5);
    CHECK(c.stage_next == 0);
    size_t cap1[5], cap2[5];
    for (int i = 0; i < 5; i++) cap1[i] = c.stage[i].cap;
    const long allocs1 = hip_emul::allocs;
    five_slots(c, 1000, 330, 70, 640, 50);           // larger: every slot grows
    for (int i = 0; i < 5; i++) { cap2[i] = c.stage[i].cap; CHECK(cap2[i] > cap1[i]); }
    CHECK(hip_emul::allocs == allocs1 + 5);
    five_slots(c, 10, 3, 1, 6, 2);                   // smaller: the same slots, no allocation, none shrinks
    for (int i = 0; i < 5; i++) CHECK(c.stage[i].cap == cap2[i]);
    CHECK(hip_emul::allocs == allocs1 + 5);
    for (int i = 5; i < STAGE_SLOTS; i++) CHECK(!c.stage[i].p);
    release(c);
}

static void test_zero_count() {
    lcb_ctx c;
    {
        HostCall h(&c, "zero");
        const long copies = hip_emul::copies;
        const uint8_t *d = h.in((const uint8_t *)nullptr, 0);
        uint64_t *o = h.out<uint64_t>(0);
        CHECK(h.ok() && d && o && (const void *)d != (const void *)o);
        CHECK(hip_emul::copies == copies);
        CHECK(c.stage[0].cap == 16 && c.stage[1].cap == 16);
        h.back(nullptr, d, 16);                      // a null host pointer and a zero size are skipped
        uint8_t host = 9;
        h.back(&host, d, 0);
        CHECK(hip_emul::copies == copies && host == 9);
        CHECK(h.finish() == 0);
    }
    release(c);
}

// the allocation at `pos` (0..4) of a five-request call fails
static void test_alloc_failure() {
    for (int pos = 0; pos < 5; pos++) {
        lcb_ctx c;
        {
            HostCall h(&c, "alloc");
            auto v = pattern(64, 4);
            const uint8_t *p[5];
            hip_emul::fail_in = pos;
            g_err.clear();
            const int errs = g_err_count;
            for (int i = 0; i < 5; i++) p[i] = i < 3 ? h.in(v.data(), 64) : h.out<uint8_t>(64);
            CHECK(hip_emul::fail_in == -1);
            CHECK(!h.ok() && g_err == "device allocation failed" && g_err_count == errs + 1);
            for (int i = 0; i < 5; i++) CHECK(i < pos ? p[i] != nullptr : p[i] == nullptr);
            CHECK(c.stage_next == pos);
            // later requests, copies and wipes touch nothing
            const long allocs = hip_emul::allocs, copies = hip_emul::copies, fills = hip_emul::fills;
            CHECK(!h.in(v.data(), 64) && !h.out<uint32_t>(3) && !h.lws(64));
            uint8_t host[64];
            memset(host, 0x11, sizeof host);
            h.back(host, p[4], 64);
            if (pos) h.back(host, p[0], 64);         // results of a failed call are not copied back either
            h.wipe(p[4], 64);
            CHECK(hip_emul::allocs == allocs && hip_emul::copies == copies && hip_emul::fills == fills);
            CHECK(host[0] == 0x11 && host[63] == 0x11 && g_err_count == errs + 1);
            if (pos) {                               // a secret already uploaded is still cleared
                h.wipe(p[0], 64);
                CHECK(hip_emul::fills == fills + 1);
                for (int i = 0; i < 64; i++) CHECK(p[0][i] == 0);
            }
            CHECK(h.finish() == -1);
        }
        CHECK(c.stage_next == 0);
        five_slots(c, 64, 64, 64, 64, 16);           // the next call on the context succeeds
        release(c);
    }
}

static void test_exhaustion() {
    lcb_ctx c;
    {
        HostCall h(&c, "exhaust");
        for (int i = 0; i < STAGE_SLOTS; i++) CHECK(h.out<uint8_t>(8));
        CHECK(h.ok() && c.stage_next == STAGE_SLOTS);
        const long allocs = hip_emul::allocs;
        g_err.clear();
        CHECK(!h.out<uint8_t>(8));
        CHECK(!h.ok() && g_err == "host call: out of staging slots");
        CHECK(c.stage_next == STAGE_SLOTS && hip_emul::allocs == allocs);
        CHECK(h.finish() == -1);
    }
    CHECK(c.stage_next == 0);
    release(c);
}

static void test_nesting() {
    lcb_ctx c;
    {
        HostCall outer(&c, "outer");
        auto v = pattern(40, 5);
        const uint8_t *a = outer.in(v.data(), 40);
        uint8_t *b = outer.out<uint8_t>(40);
        memset(b, 0x77, 40);
        CHECK(outer.ok() && c.stage_next == 2);
        {
            HostCall inner(&c, "inner");             // the context's lock is recursive
            auto w = pattern(400, 6);
            const uint8_t *x = inner.in(w.data(), 400);
            uint8_t *y = inner.out<uint8_t>(400);
            CHECK(inner.ok() && x == c.stage[2].p && y == c.stage[3].p && c.stage_next == 4);
            memset(y, 0xee, 400);
            inner.wipe(a, 40);                       // not one of the inner call's slots: left alone
            CHECK(inner.finish() == 0);
        }
        CHECK(c.stage_next == 2 && c.enq_depth == 1);
        for (int i = 0; i < 40; i++) CHECK(a[i] == v[i] && b[i] == 0x77);
        uint8_t *d = outer.out<uint8_t>(8);          // continues where the inner call began
        CHECK(d == c.stage[2].p);
        CHECK(outer.finish() == 0);
    }
    CHECK(c.stage_next == 0 && c.enq_depth == 0);
    release(c);
}

static void test_wipe() {
    lcb_ctx c;
    {
        HostCall h(&c, "wipe");
        auto v = pattern(48, 8);
        const uint8_t *a = h.in(v.data(), 48), *b = h.in(v.data(), 48);
        CHECK(h.ok());
        h.wipe(a, 32);
        for (int i = 0; i < 48; i++) CHECK(a[i] == (i < 32 ? 0 : v[i]) && b[i] == v[i]);
        h.wipe(b, 1000);                             // clamped to the slot's 48 bytes (an overrun would be reported)
        for (int i = 0; i < 48; i++) CHECK(b[i] == 0);
        h.wipe(a + 40, 1000);                        // from inside a slot: to that slot's end
        for (int i = 32; i < 48; i++) CHECK(a[i] == (i < 40 ? v[i] : 0));
        const long fills = hip_emul::fills;
        h.wipe(nullptr, 8);
        h.wipe(a, 0);
        CHECK(hip_emul::fills == fills);
        g_sync_ok = false;                           // a failed synchronisation is the call's result
        CHECK(h.finish() == -1 && g_err == "wipe");
        g_sync_ok = true;
    }
    release(c);
}

static void test_lws() {
    lcb_ctx c;
    {
        HostCall h(&c, "lws");
        uint32_t *w = h.lws(100);
        CHECK(h.ok() && w && w == c.lws.p && c.stage_next == 0);
        hip_emul::fail_in = 0;
        g_err.clear();
        CHECK(!h.lws(1000) && !h.ok() && g_err == "device allocation failed");
    }
    c.lws.release();
}

static void test_rebase() {
    std::vector<uint64_t> rel;
    const uint64_t off[] = {100, 100, 140, 141, 1000};
    CHECK(rebase(rel, off, 4, "unused") && rel == (std::vector<uint64_t>{0, 0, 40, 41, 900}));
    CHECK(rebase(rel, nullptr, 0, "unused") && rel == std::vector<uint64_t>{0});
    const uint64_t one[] = {7};
    CHECK(rebase(rel, one, 0, "unused") && rel == std::vector<uint64_t>{0});
    const uint64_t bad[] = {5, 9, 8, 20};
    g_err.clear();
    CHECK(!rebase(rel, bad, 3, "case: offsets must not decrease") && g_err == "case: offsets must not decrease");
    const uint64_t top[] = {~0ull - 1, ~0ull};
    CHECK(rebase(rel, top, 1, "unused") && rel == (std::vector<uint64_t>{0, 1}));
}

int main() {
    test_order_and_reuse();
    test_zero_count();
    test_alloc_failure();
    test_exhaustion();
    test_nesting();
    test_wipe();
    test_lws();
    test_rebase();
    CHECK(hip_emul::allocs == hip_emul::frees);      // every context released what it held
    printf("host_call_emul: ok\n");
    return 0;
}
