// lachain_amd/csrc/host_call.hpp — the scope of one host-pointer entry point (included from lcb_internal.hpp).
//
// A host-pointer form uploads its arguments, runs the device path the *_dev forms run, copies the results back and
// synchronises.  Every buffer that lives only for that call comes from a HostCall: the slots of lcb_ctx::stage[], handed
// out in request order and anonymous on purpose, so that no other code can come to depend on what one of them held
// (DESIGN.md "Staging slots").  A buffer that device-path code allocates, or that outlives the call, has a named slot of
// its own in lcb_ctx.hpp instead.
#pragma once
#include <vector>

namespace lcb_int {

struct HostCall {
    lcb_ctx *c;
    const char *what;
    Enq q;                    // exclusive use of the context, ordered after its previous work
    hipStream_t s;
    const int first;          // the context's cursor when this call began; put back when it ends, so a host form called
    bool good = true;         // from another one continues behind the outer call's slots
    HostCall(lcb_ctx *c_, const char *what_) : c(c_), what(what_), q(c_, c_->stream), s(c_->stream), first(c_->stage_next) {}
    ~HostCall() { c->stage_next = first; }
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;

    // the next slot with room for `bytes` (0 gives a valid 16-byte slot); null, and the call failed, when there is none
    void *take(size_t bytes) {
        if (!good) return nullptr;
        const bool slot = c->stage_next < STAGE_SLOTS;
        void *d = slot ? c->stage[c->stage_next].get(bytes) : nullptr;
        if (!d) {
            if (slot) fail();
            else set_err("host call: out of staging slots");
            good = false;
            return nullptr;
        }
        c->stage_next++;
        return d;
    }
    // the next slot with a copy of src in it: writable (a workspace the kernels work on in place), or as an input
    template <class T> T *work(const T *src, size_t count) {
        T *d = (T *)take(count * sizeof(T));
        if (d && count) (void)hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, s);
        return d;
    }
    template <class T> const T *in(const T *src, size_t count) { return work(src, count); }
    template <class T> T *out(size_t count) { return (T *)take(count * sizeof(T)); }
    void back(void *host, const void *dev, size_t bytes) {
        if (good && host && dev && bytes) (void)hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s);
    }
    // zero `bytes` at dev, which lies in one of this call's slots, no further than that slot's end (secret-bearing slots;
    // it also runs after a later request has failed)
    void wipe(const void *dev, size_t bytes) {
        for (int k = first; dev && k < c->stage_next; k++) {
            const char *p = (const char *)c->stage[k].p, *d = (const char *)dev;
            if (d < p || d >= p + c->stage[k].cap) continue;
            const size_t room = (size_t)(p + c->stage[k].cap - d);
            if (bytes) (void)hipMemsetAsync((void *)dev, 0, bytes < room ? bytes : room, s);
            return;
        }
    }
    // the context's persistent lanetab.hpp workspace (lcb_ctx::lws), grown to `bytes`
    uint32_t *lws(size_t bytes) {
        void *d = good ? c->lws.get(bytes) : nullptr;
        if (!d) fail();
        return (uint32_t *)d;
    }
    // the call fails as a failed allocation does (also the fault-injection sites' way in)
    void fail() {
        if (good) set_err("device allocation failed");
        good = false;
    }
    bool ok() const { return good; }
    int finish() { return sync_check(c, what) && good ? 0 : -1; }
};

// rel[i] = off[i] - off[0] for i = 0..n, as the staged copy of the bytes from off[0] on sees them (n == 0: {0}, and off
// is not read).  A decreasing pair fails the call with the caller's text.
inline bool rebase(std::vector<uint64_t> &rel, const uint64_t *off, size_t n, const char *err) {
    rel.assign(n + 1, 0);
    for (size_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) { set_err(err); return false; }
    for (size_t i = 1; i <= n; i++) rel[i] = off[i] - off[0];
    return true;
}

}  // namespace lcb_int
