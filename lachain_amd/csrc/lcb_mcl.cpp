// lachain_amd/csrc/lcb_mcl.cpp — the mcl single-element surface of include/lachain_bls.h: every mclBn* function,
// the generators and the G2 sign convention, top to bottom.
//
// The calls that are O(1) field work — Fr arithmetic (fr_host.hpp) and G1 / G2 add, sub, neg, dbl, normalize, compare,
// validity, (de)serialization, GT products (fp_host.hpp) — run on the calling thread, word for word the kernels'
// formulas, because a GPU round trip costs 50-100x the operation.  Every other single-element operation (scalar
// multiplication, hashing to G2, Miller loop, GT power) is a GPU round trip on the calling thread's own staging
// buffers and stream (no process-wide lock: the reference calls mcl from one thread per consensus protocol,
// AbstractProtocol.cs:46-47), and the pairing, multi-scalar products, Lagrange interpolation and polynomial
// evaluation go to batch / cooperative kernels in the thread's host-pointer context (lcb_host.cpp ctx_sync).
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdlib.h>
#include <mutex>
#include <atomic>
#include <vector>
#include <sys/random.h>

#include "launch.h"
#include "bls_constants_host.h"
#include "../../include/lachain_bls.h"
#include "lcb_internal.hpp"
#include "fr_host.hpp"
#include "fp_host.hpp"

using namespace lcb_int;

namespace {

const size_t IO_WORDS = 4096; // 16 KB staging per thread
// the output of a failed void mcl call (mclBnG1_mul, mclBn_pairing, ...): random words with the top limb of the first
// coordinate set to all ones, so it is not a canonical field element (isValid / serialize reject it), and two failed
// calls never compare equal (an equality check between two failed pairings cannot pass)
void fail_out(void *out, size_t bytes) {
    uint8_t *b = (uint8_t *)out;
    size_t got = 0;
    while (got < bytes) {
        ssize_t r = getrandom(b + got, bytes - got, 0);
        if (r <= 0) break;
        got += (size_t)r;
    }
    for (size_t i = got; i < bytes; i++) b[i] = (uint8_t)(0x5a ^ i);
    if (bytes >= 48) memset(b + 44, 0xff, 4);
}

// single-element operations: every calling thread owns its staging (device and pinned host buffers, a stream), so the
// protocol threads (AbstractProtocol.cs:46-47) never queue behind each other's round trips
// A thread's staging and implicit contexts (lcb_host.cpp ThreadCtx) are NOT released when it exits: HIP calls from
// thread-local destructors race the runtime's (and a profiler's) own per-thread teardown (an abort under rocprofv3 in
// round 4).  They are retired to process-wide free lists instead and handed to the next thread that needs one, so their
// number stays bounded by the peak number of calling threads.  Each list and its lock are leaked on purpose (no
// static-destruction order issue); no caller holds both locks.
struct StageRes {
    u32 *dev = nullptr, *host = nullptr;
    hipStream_t s = nullptr;
};
std::mutex &retired_mu() {
    static std::mutex *m = new std::mutex;
    return *m;
}
std::vector<StageRes> &retired_stages() {
    static std::vector<StageRes> *v = new std::vector<StageRes>;
    return *v;
}
struct OpStage : StageRes {
    ~OpStage() {
        if (!(s && dev && host)) return;             // a half-built stage never survives stage_ready
        std::lock_guard<std::mutex> lk(retired_mu());
        retired_stages().push_back(*this);
    }
};
thread_local OpStage t_stage;
bool stage_ready() {
    if (!ready()) return false;
    if (t_stage.s && t_stage.dev && t_stage.host) return true;
    {
        std::lock_guard<std::mutex> lk(retired_mu());
        auto &v = retired_stages();
        // (a pending staging-allocation failure builds a new stage, so the test hook reaches the allocation)
        if (!v.empty() && !t_stage.s && !t_stage.dev && !t_stage.host && !inject_armed(INJ_STAGE_HOST_ALLOC)) {
            static_cast<StageRes &>(t_stage) = v.back();
            v.pop_back();
            return true;
        }
    }
    // all three or none: a partial failure releases what was created, so the next call retries from scratch instead
    // of passing a half-built stage (a set stream with a null host buffer would be written through)
    hipError_t e = t_stage.s ? hipSuccess : hipStreamCreateWithFlags(&t_stage.s, hipStreamNonBlocking);
    if (e == hipSuccess && !t_stage.dev) e = hipMalloc(&t_stage.dev, IO_WORDS * 4);
    if (e == hipSuccess && !t_stage.host) {
        if (injected(INJ_STAGE_HOST_ALLOC)) e = hipErrorOutOfMemory;
        else e = hipHostMalloc(&t_stage.host, IO_WORDS * 4, hipHostMallocDefault);
    }
    if (e != hipSuccess) {
        set_err("single-operation staging", e);
        if (t_stage.host) (void)hipHostFree(t_stage.host);
        if (t_stage.dev) (void)hipFree(t_stage.dev);
        if (t_stage.s) (void)hipStreamDestroy(t_stage.s);
        t_stage.host = nullptr;
        t_stage.dev = nullptr;
        t_stage.s = nullptr;
        return false;
    }
    return true;
}
#define IOH (t_stage.host)

// one round trip on the thread's staging: the first in_bytes of the pinned buffer to the device, `launch` on the
// stage's stream, out_bytes at word out_w back, synchronised; a failed launch reports launch_err, a failed kernel its name
template <class Launch>
bool round_trip(size_t in_bytes, size_t out_w, size_t out_bytes, const char *launch_err, const char *kernel, Launch launch) {
    hipError_t e;
    if (injected(INJ_STAGE_OP)) { set_err("injected failure (single operation)"); return false; }
    if ((e = hipMemcpyAsync(t_stage.dev, t_stage.host, in_bytes, hipMemcpyHostToDevice, t_stage.s)) != hipSuccess) { set_err("H2D", e); return false; }
    launch();
    if ((e = hipGetLastError()) != hipSuccess) { set_err(launch_err, e); return false; }
    if ((e = hipMemcpyAsync(t_stage.host + out_w, t_stage.dev + out_w, out_bytes, hipMemcpyDeviceToHost, t_stage.s)) != hipSuccess) { set_err("D2H", e); return false; }
    if ((e = hipStreamSynchronize(t_stage.s)) != hipSuccess) { set_err(kernel, e); return false; }
    return true;
}
// run one k_op on the thread's staging buffer: copy `in_words` words to the device, launch, copy `out_words` back
bool run_op(int op, size_t in_words, size_t out_words) {
    return round_trip(in_words * 4, 0, out_words * 4, "k_op launch", "k_op",
                      [op] { lcbk_op(dim3(1), t_stage.s, op, t_stage.dev, g_orig_cofactor); });
}
// mclBnG2_hashAndMapTo's round trip: as run_op, on the dedicated one-lane hash kernel (k_ptmul.hip)
bool run_hash(size_t in_words, size_t out_words) {
    return round_trip(in_words * 4, 0, out_words * 4, "k_mcl_g2_hash launch", "k_mcl_g2_hash",
                      [] { lcbk_mcl_g2_hash(t_stage.s, t_stage.dev, g_orig_cofactor); });
}

#define LOCKED_OR(ret)                        \
    if (!stage_ready()) return ret;

} // namespace

extern "C" int mclBn_init(int curve, int compiledTimeVar) {
    if (curve != MCL_BLS12_381 || compiledTimeVar != MCLBN_COMPILED_TIME_VAR) {
        set_err("unsupported curve / compiledTimeVar");
        return -1;
    }
    return ready() ? 0 : -1;
}
extern "C" int mclBn_getOpUnitSize(void) { return 6; }
extern "C" int mclBn_getG1ByteSize(void) { return 48; }
extern "C" int mclBn_getFrByteSize(void) { return 32; }
extern "C" int mclBn_getFpByteSize(void) { return 48; }

// ================================================================== Fr (host arithmetic, fr_host.hpp)
static inline const uint64_t *FRV(const mclBnFr *x) { return (const uint64_t *)x; }
static inline uint64_t *FRW(mclBnFr *x) { return (uint64_t *)x; }
static int fr_set_raw(mclBnFr *y, const u32 raw[8]) {
    uint64_t r[4];
    memcpy(r, raw, 32);
    if (!frh::lt_r(r)) { memset(y, 0, 32); return -1; }
    frh::from_raw(FRW(y), r);
    return 0;
}
static int fr_get_raw(u32 raw[8], const mclBnFr *x) {
    uint64_t r[4];
    frh::to_raw(r, FRV(x));
    memcpy(raw, r, 32);
    return 0;
}
extern "C" int mclBnFr_setInt(mclBnFr *y, mclInt x) {
    u32 raw[8] = {0};
    uint64_t ax = x < 0 ? (uint64_t)(-(x + 1)) + 1 : (uint64_t)x;
    raw[0] = (u32)ax; raw[1] = (u32)(ax >> 32);
    if (fr_set_raw(y, raw)) return -1;
    if (x < 0) mclBnFr_neg(y, y);
    return 0;
}
extern "C" int mclBnFr_setInt32(mclBnFr *y, int x) { return mclBnFr_setInt(y, x); }
extern "C" int mclBnFr_setByCSPRNG(mclBnFr *x) {
    // rejection sampling of a uniform 255-bit value < r
    for (int tries = 0; tries < 64; tries++) {
        u32 raw[8];
        if (getrandom(raw, sizeof raw, 0) != (ssize_t)sizeof raw) return -1;
        raw[7] &= 0x7fffffffu;
        if (fr_set_raw(x, raw) == 0) return 0;
    }
    return -1;
}
extern "C" int mclBnFr_setLittleEndian(mclBnFr *x, const void *buf, mclSize n) {
    // mcl setArrayMask: take at most 32 bytes, mask to 255 bits, and to 254 if still >= r
    u32 raw[8] = {0};
    memcpy(raw, buf, n < 32 ? n : 32);
    raw[7] &= 0x7fffffffu;
    uint64_t r[4];
    memcpy(r, raw, 32);
    if (!frh::lt_r(r)) raw[7] &= 0x3fffffffu;
    return fr_set_raw(x, raw);
}
extern "C" mclSize mclBnFr_serialize(void *buf, mclSize max, const mclBnFr *x) {
    if (max < 32) return 0;
    u32 raw[8];
    fr_get_raw(raw, x);
    memcpy(buf, raw, 32);
    return 32;
}
extern "C" mclSize mclBnFr_deserialize(mclBnFr *x, const void *buf, mclSize n) {
    if (n < 32) return 0;
    u32 raw[8];
    memcpy(raw, buf, 32);
    return fr_set_raw(x, raw) == 0 ? 32 : 0;
}
extern "C" void mclBnFr_clear(mclBnFr *x) { memset(x, 0, sizeof *x); }
extern "C" int mclBnFr_isValid(const mclBnFr *x) { return frh::lt_r(FRV(x)); }
extern "C" int mclBnFr_isEqual(const mclBnFr *x, const mclBnFr *y) { return memcmp(x, y, 32) == 0; }
extern "C" int mclBnFr_isZero(const mclBnFr *x) { return frh::is_zero(FRV(x)); }
extern "C" int mclBnFr_isOne(const mclBnFr *x) { return memcmp(x, frh::ONE, 32) == 0; }
extern "C" void mclBnFr_neg(mclBnFr *y, const mclBnFr *x) { frh::neg(FRW(y), FRV(x)); }
extern "C" void mclBnFr_inv(mclBnFr *y, const mclBnFr *x) { frh::inv(FRW(y), FRV(x)); }
extern "C" void mclBnFr_sqr(mclBnFr *y, const mclBnFr *x) { frh::mul(FRW(y), FRV(x), FRV(x)); }
extern "C" void mclBnFr_add(mclBnFr *z, const mclBnFr *x, const mclBnFr *y) { frh::add(FRW(z), FRV(x), FRV(y)); }
extern "C" void mclBnFr_sub(mclBnFr *z, const mclBnFr *x, const mclBnFr *y) { frh::sub(FRW(z), FRV(x), FRV(y)); }
extern "C" void mclBnFr_mul(mclBnFr *z, const mclBnFr *x, const mclBnFr *y) { frh::mul(FRW(z), FRV(x), FRV(y)); }
extern "C" void mclBnFr_div(mclBnFr *z, const mclBnFr *x, const mclBnFr *y) {
    mclBnFr t;
    mclBnFr_inv(&t, y);
    mclBnFr_mul(z, x, &t);
}

// ================================================================== G1 / G2 (host field work, fp_host.hpp)
// O(1) field work runs on the host like Fr (fp_host.hpp header); G1 / G2 multiplication, the hash to G2 and the
// pairing below stay on the GPU.  Bit-identical to the kernels' results (same formulas, fully reduced residues).
static void g1_op(int op, mclBnG1 *z, const mclBnG1 *x, const mclBnG1 *y, const mclBnFr *k) {
    if (!stage_ready()) { fail_out(z, 144); return; }
    memcpy(IOH + 36, x, 144);
    if (y) memcpy(IOH + 72, y, 144);
    if (k) memcpy(IOH + 108, k, 32);
    if (run_op(op, 116, 36)) memcpy(z, IOH, 144);
    else fail_out(z, 144);
}
std::atomic<int> g_g2_sign_b{0};      // lcb_set_g2_sign_from_b: the G2 wire flag is parity(y.b) instead of parity(y.a)
static inline fph::g1 *G1W(mclBnG1 *x) { return (fph::g1 *)x; }
static inline const fph::g1 *G1R(const mclBnG1 *x) { return (const fph::g1 *)x; }
static inline fph::g2 *G2W(mclBnG2 *x) { return (fph::g2 *)x; }
static inline const fph::g2 *G2R(const mclBnG2 *x) { return (const fph::g2 *)x; }
extern "C" mclSize mclBnG1_serialize(void *buf, mclSize max, const mclBnG1 *x) {
    if (max < 48) return 0;
    fph::g1_compress((uint8_t *)buf, *G1R(x));
    return 48;
}
extern "C" mclSize mclBnG1_deserialize(mclBnG1 *x, const void *buf, mclSize n) {
    if (n < 48) return 0;
    fph::g1a a;
    if (!fph::g1_decompress(a, (const uint8_t *)buf)) return 0;
    fph::jac_from_aff(*G1W(x), a);
    return 48;
}
extern "C" int mclBnG1_isValid(const mclBnG1 *x) { return fph::jac_valid(*G1R(x)); }
extern "C" int mclBnG1_isEqual(const mclBnG1 *x, const mclBnG1 *y) { return fph::jac_eq(*G1R(x), *G1R(y)); }
extern "C" int mclBnG1_isZero(const mclBnG1 *x) {
    static const u32 z[12] = {0};
    return memcmp(&x->z, z, 48) == 0;
}
extern "C" void mclBnG1_clear(mclBnG1 *x) { memset(x, 0, sizeof *x); }
extern "C" void mclBnG1_neg(mclBnG1 *y, const mclBnG1 *x) { fph::jac_neg(*G1W(y), *G1R(x)); }
extern "C" void mclBnG1_dbl(mclBnG1 *y, const mclBnG1 *x) { fph::g1 t; fph::jac_dbl(t, *G1R(x)); *G1W(y) = t; }
extern "C" void mclBnG1_normalize(mclBnG1 *y, const mclBnG1 *x) { fph::jac_normalize(*G1W(y), *G1R(x)); }
extern "C" void mclBnG1_add(mclBnG1 *z, const mclBnG1 *x, const mclBnG1 *y) {
    fph::g1 t;
    fph::jac_add(t, *G1R(x), *G1R(y));
    *G1W(z) = t;
}
extern "C" void mclBnG1_sub(mclBnG1 *z, const mclBnG1 *x, const mclBnG1 *y) {
    fph::g1 ny, t;
    fph::jac_neg(ny, *G1R(y));
    fph::jac_add(t, *G1R(x), ny);
    *G1W(z) = t;
}
// ---- mclBnG1_mul / mclBnG2_mul: the cooperative ladders of k_ptmul.hip (four lanes per ladder, several ladders per
// wave) on the scalar split below, the result assembled here; a base point outside the subgroup (the split is only
// valid on it) takes the exact one-lane ladder of k_op
struct PtJobG1 { u32 x[12], y[12], inf, nwin, pad[2]; uint8_t nib[36]; };
struct PtJobG2 { u32 x[24], y[24], inf, nwin, pad[2]; uint8_t nib[36]; };
static_assert(sizeof(PtJobG1) == 148 && sizeof(PtJobG2) == 244, "k_ptmul.hip PtJob layouts");
typedef unsigned __int128 u128h;
static const uint64_t Z_ABS_H = 0xd201000000010000ull;
// q <- q / u (256-bit), returns q mod u
static uint64_t divmod_u(uint64_t q[4]) {
    u128h rem = 0;
    for (int i = 3; i >= 0; i--) {
        u128h cur = rem << 64 | q[i];
        q[i] = (uint64_t)(cur / Z_ABS_H);
        rem = cur % Z_ABS_H;
    }
    return (uint64_t)rem;
}
// nwin signed 4-bit digits of the little-endian words v (nw 64-bit words), most significant first: each window's
// nibble plus the carry, minus 16 (carry 1) when above 8, so every digit is in [-7, 8] and k_ptmul.hip's table holds
// T[1..8].  A byte is |digit| with bit 7 set for a negative digit.  False if a carry leaves the top window (the
// callers size nwin so that it cannot: 33 windows for < 2^129, 17 for one 64-bit word).
template <class J> static bool put_digits(J &job, const uint64_t *v, int nw, u32 nwin) {
    job.nwin = nwin;
    int carry = 0;
    for (u32 i = 0; i < nwin; i++) {              // i: window index from the least significant
        const u32 bit = 4 * i, word = bit / 64;
        int d = (word < (u32)nw ? (int)((v[word] >> (bit % 64)) & 15) : 0) + carry;
        carry = d > 8;
        if (carry) d -= 16;
        job.nib[nwin - 1 - i] = d < 0 ? (uint8_t)(0x80 | -d) : (uint8_t)d;
    }
    return carry == 0;
}
template <class J, class A> static void put_point(J &job, const A &a) {
    job.inf = a.inf ? 1u : 0u;
    memcpy(job.x, &a.x, sizeof a.x);
    memcpy(job.y, &a.y, sizeof a.y);
}
// run n_jobs ladders (k_ptmul_g1 / _g2) on the thread's staging; outputs the groups' Jacobian results
static bool ptmul_run(int g, const void *jobs, size_t job_bytes, u32 n_jobs, void *out, size_t out_bytes) {
    if (!stage_ready()) return false;
    memcpy(IOH, jobs, job_bytes * n_jobs);
    const size_t out_w = 1024;                    // results at word 1024 of the 16 KB staging
    if (!round_trip(job_bytes * n_jobs, out_w, out_bytes * n_jobs, "k_ptmul launch", "k_ptmul", [=] {
            if (g == 1) lcbk_ptmul_g1(t_stage.s, t_stage.dev, n_jobs, t_stage.dev + out_w);
            else lcbk_ptmul_g2(t_stage.s, t_stage.dev, n_jobs, t_stage.dev + out_w);
        })) return false;
    memcpy(out, IOH + out_w, out_bytes * n_jobs);
    return true;
}
extern "C" void mclBnG1_mul(mclBnG1 *z, const mclBnG1 *x, const mclBnFr *y) {
    uint64_t k[4];
    frh::to_raw(k, FRV(y));                       // canonical scalar < r
    fph::g1a P;
    fph::jac_to_aff(P, *G1R(x));
    if (P.inf || (k[0] | k[1] | k[2] | k[3]) == 0 || !fph::jac_on_curve(*G1R(x))) {
        if (P.inf || (k[0] | k[1] | k[2] | k[3]) == 0) { fph::jac_set_inf(*G1W(z)); return; }
        g1_op(OP_G1_MUL, z, x, nullptr, y);       // not a curve point: mcl's generic ladder semantics
        return;
    }
    // GLV (curve.hpp g1_mul_glv): k = d0 + d1 u + a1 u^2 = (a0 + a1) + a1 lambda, a0 = d0 + d1 u
    uint64_t q[4] = {k[0], k[1], k[2], k[3]};
    const uint64_t d0 = divmod_u(q), d1 = divmod_u(q);   // q = a1 < 2^128
    u128h a0 = (u128h)d1 * Z_ABS_H + d0, a1 = (u128h)q[1] << 64 | q[0];
    u128h s = a0 + a1;
    const uint64_t s_top = s < a0 ? 1 : 0;
    const uint64_t k1[3] = {(uint64_t)s, (uint64_t)(s >> 64), s_top}, k2[2] = {(uint64_t)a1, (uint64_t)(a1 >> 64)};
    const u128h zz = (u128h)Z_ABS_H * Z_ABS_H;
    fph::g1a phiP;
    fph::g1_phi(phiP, P);
    {   // membership on the host: [z^2] P == P + phi(P) = (beta^2 x, -y) (128 doublings of host field code)
        fph::g1 m, PJ;
        fph::jac_from_aff(PJ, P);
        fph::jac_set_inf(m);
        for (int b = 127; b >= 0; b--) {
            fph::jac_dbl(m, m);
            if ((zz >> b) & 1) fph::jac_add(m, m, PJ);
        }
        fph::g1a chk;
        fph::g1_phi(chk, phiP);                   // (beta^2 x, y)
        fph::neg(chk.y, chk.y);
        if (!fph::jac_eq_aff(m, chk)) {           // outside G1: the split does not apply
            g1_op(OP_G1_MUL, z, x, nullptr, y);
            return;
        }
    }
    // four ladders of <= 65 bits: k1 = k1_lo + 2^65 k1_hi over P and [2^65] P, k2 likewise over phi(P) and
    // [2^65] phi(P) = phi([2^65] P) (the doublings on the host): half the serial rounds of two 129-bit ladders
    fph::g1a P65, phiP65;
    {
        fph::g1 t;
        fph::jac_from_aff(t, P);
        for (int i = 0; i < 65; i++) fph::jac_dbl(t, t);
        fph::jac_to_aff(P65, t);
        fph::g1_phi(phiP65, P65);
    }
    if (P65.inf) { g1_op(OP_G1_MUL, z, x, nullptr, y); return; }    // unreachable in G1 (2^65 < r)
    const uint64_t k1lo[2] = {k1[0], k1[1] & 1}, k1hi[2] = {(k1[1] >> 1) | (k1[2] << 63), k1[2] >> 1};
    const uint64_t k2lo[2] = {k2[0], k2[1] & 1}, k2hi[2] = {k2[1] >> 1, 0};
    PtJobG1 jobs[4];
    memset(jobs, 0, sizeof jobs);
    put_point(jobs[0], P);
    put_point(jobs[1], P65);
    put_point(jobs[2], phiP);
    put_point(jobs[3], phiP65);
    if (!put_digits(jobs[0], k1lo, 2, 18) || !put_digits(jobs[1], k1hi, 2, 18) || !put_digits(jobs[2], k2lo, 2, 18) ||
        !put_digits(jobs[3], k2hi, 2, 18)) {
        g1_op(OP_G1_MUL, z, x, nullptr, y);       // unreachable (< 2^66 in 18 signed windows): the exact ladder
        return;
    }
    fph::g1 acc[4];
    if (!ptmul_run(1, jobs, sizeof(PtJobG1), 4, acc, sizeof(fph::g1))) { fail_out(z, 144); return; }
    fph::g1 r;
    fph::jac_add(r, acc[0], acc[1]);
    fph::jac_add(r, r, acc[2]);
    fph::jac_add(r, r, acc[3]);
    *G1W(z) = r;
}
extern "C" void lcb_g1_generator(mclBnG1 *g) { fph::g1_generator(*G1W(g)); }

extern "C" mclSize mclBnG2_serialize(void *buf, mclSize max, const mclBnG2 *x) {
    if (max < 96) return 0;
    fph::g2_compress((uint8_t *)buf, *G2R(x), g_g2_sign_b.load() != 0);
    return 96;
}
extern "C" mclSize mclBnG2_deserialize(mclBnG2 *x, const void *buf, mclSize n) {
    if (n < 96) return 0;
    fph::g2a a;
    if (!fph::g2_decompress(a, (const uint8_t *)buf, g_g2_sign_b.load() != 0)) return 0;
    fph::jac_from_aff(*G2W(x), a);
    return 96;
}
extern "C" int mclBnG2_isValid(const mclBnG2 *x) { return fph::jac_valid(*G2R(x)); }
extern "C" int mclBnG2_isEqual(const mclBnG2 *x, const mclBnG2 *y) { return fph::jac_eq(*G2R(x), *G2R(y)); }
extern "C" int mclBnG2_isZero(const mclBnG2 *x) {
    static const u32 z[24] = {0};
    return memcmp(&x->z, z, 96) == 0;
}
extern "C" void mclBnG2_clear(mclBnG2 *x) { memset(x, 0, sizeof *x); }
extern "C" int mclBnG2_hashAndMapTo(mclBnG2 *x, const void *buf, mclSize n) {
    if (n > (IO_WORDS - 256) * 4) { set_err("message too long"); return -1; }
    LOCKED_OR(-1)
    IOH[250] = (u32)n;
    memcpy(IOH + 256, buf, n);
    if (!run_hash(256 + (n + 3) / 4, 249) || !IOH[248]) return -1;
    memcpy(x, IOH, 288);
    return 0;
}
static void g2_op(int op, mclBnG2 *z, const mclBnG2 *x, const mclBnG2 *y, const mclBnFr *k) {
    if (!stage_ready()) { fail_out(z, 288); return; }
    memcpy(IOH + 72, x, 288);
    if (y) memcpy(IOH + 144, y, 288);
    if (k) memcpy(IOH + 216, k, 32);
    if (run_op(op, 224, 72)) memcpy(z, IOH, 288);
    else fail_out(z, 288);
}
extern "C" void mclBnG2_neg(mclBnG2 *y, const mclBnG2 *x) { fph::jac_neg(*G2W(y), *G2R(x)); }
extern "C" void mclBnG2_dbl(mclBnG2 *y, const mclBnG2 *x) { fph::g2 t; fph::jac_dbl(t, *G2R(x)); *G2W(y) = t; }
extern "C" void mclBnG2_normalize(mclBnG2 *y, const mclBnG2 *x) { fph::jac_normalize(*G2W(y), *G2R(x)); }
extern "C" void mclBnG2_add(mclBnG2 *z, const mclBnG2 *x, const mclBnG2 *y) {
    fph::g2 t;
    fph::jac_add(t, *G2R(x), *G2R(y));
    *G2W(z) = t;
}
extern "C" void mclBnG2_sub(mclBnG2 *z, const mclBnG2 *x, const mclBnG2 *y) {
    fph::g2 ny, t;
    fph::jac_neg(ny, *G2R(y));
    fph::jac_add(t, *G2R(x), ny);
    *G2W(z) = t;
}
extern "C" void mclBnG2_mul(mclBnG2 *z, const mclBnG2 *x, const mclBnFr *y) {
    uint64_t k[4];
    frh::to_raw(k, FRV(y));
    fph::g2a Q;
    fph::jac_to_aff(Q, *G2R(x));
    if (Q.inf || (k[0] | k[1] | k[2] | k[3]) == 0 || !fph::jac_on_curve(*G2R(x))) {
        if (Q.inf || (k[0] | k[1] | k[2] | k[3]) == 0) { fph::jac_set_inf(*G2W(z)); return; }
        g2_op(OP_G2_MUL, z, x, nullptr, y);
        return;
    }
    // GLS (curve.hpp g2_mul_gls): k = d0 + d1 u + d2 u^2 + d3 u^3 over Q, -psi Q, psi^2 Q, -psi^3 Q
    uint64_t q[4] = {k[0], k[1], k[2], k[3]}, d[4];
    d[0] = divmod_u(q);
    d[1] = divmod_u(q);
    d[2] = divmod_u(q);
    d[3] = q[0];                                  // k < r < u^4
    fph::g2a B[4];
    B[0] = Q;
    fph::g2_psi(B[1], Q);
    fph::g2_psi(B[2], B[1]);
    fph::g2_psi(B[3], B[2]);
    fph::g2a psiQ = B[1];
    {   // membership on the host: psi(Q) == -[|z|] Q (64 doublings of host field code)
        fph::g2 m, QJ;
        fph::jac_from_aff(QJ, Q);
        fph::jac_set_inf(m);
        for (int b = 63; b >= 0; b--) {
            fph::jac_dbl(m, m);
            if ((Z_ABS_H >> b) & 1) fph::jac_add(m, m, QJ);
        }
        fph::g2a chk = psiQ;
        fph::neg(chk.y, chk.y);
        if (!fph::jac_eq_aff(m, chk)) {           // outside G2: the split does not apply
            g2_op(OP_G2_MUL, z, x, nullptr, y);
            return;
        }
    }
    // eight ladders of 32 bits: each digit d_i = lo + 2^32 hi over B_i and [2^32] B_i (= +-psi^i([2^32] Q), the
    // doublings on the host): half the serial rounds of four 64-bit ladders
    fph::g2a Q32, C[4];
    {
        fph::g2 t;
        fph::jac_from_aff(t, Q);
        for (int i = 0; i < 32; i++) fph::jac_dbl(t, t);
        fph::jac_to_aff(Q32, t);
    }
    if (Q32.inf) { g2_op(OP_G2_MUL, z, x, nullptr, y); return; }    // unreachable in G2 (2^32 < r)
    C[0] = Q32;
    fph::g2_psi(C[1], Q32);
    fph::g2_psi(C[2], C[1]);
    fph::g2_psi(C[3], C[2]);
    fph::neg(C[1].y, C[1].y);
    fph::neg(C[3].y, C[3].y);
    fph::neg(B[1].y, B[1].y);
    fph::neg(B[3].y, B[3].y);
    PtJobG2 jobs[8];
    memset(jobs, 0, sizeof jobs);
    bool dig_ok = true;
    for (int i = 0; i < 4; i++) {
        const uint64_t lo = d[i] & 0xffffffffull, hi = d[i] >> 32;
        put_point(jobs[2 * i], B[i]);
        put_point(jobs[2 * i + 1], C[i]);
        dig_ok &= put_digits(jobs[2 * i], &lo, 1, 9);
        dig_ok &= put_digits(jobs[2 * i + 1], &hi, 1, 9);
    }
    if (!dig_ok) { g2_op(OP_G2_MUL, z, x, nullptr, y); return; }   // unreachable (32-bit digits): the exact ladder
    fph::g2 acc[8];
    if (!ptmul_run(2, jobs, sizeof(PtJobG2), 8, acc, sizeof(fph::g2))) { fail_out(z, 288); return; }
    fph::g2 r = acc[0];
    for (int i = 1; i < 8; i++) fph::jac_add(r, r, acc[i]);
    *G2W(z) = r;
}
extern "C" void lcb_g2_generator(mclBnG2 *g) { fph::g2_generator(*G2W(g)); }

// ================================================================== GT / pairing
static void pair_op(int op, mclBnGT *z, const mclBnG1 *x, const mclBnG2 *y) {
    if (!stage_ready()) { fail_out(z, 576); return; }
    memcpy(IOH + 144, x, 144);
    memcpy(IOH + 180, y, 288);
    if (run_op(op, 252, 144)) memcpy(z, IOH, 576);
    else fail_out(z, 576);
}
extern "C" void mclBn_millerLoop(mclBnGT *z, const mclBnG1 *x, const mclBnG2 *y) { pair_op(OP_MILLER, z, x, y); }
static void gt_op(int op, mclBnGT *z, const mclBnGT *a, const mclBnGT *b, const mclBnFr *k) {
    if (!stage_ready()) { fail_out(z, 576); return; }
    memcpy(IOH + 252, a, 576);
    if (b) memcpy(IOH + 396, b, 576);
    if (k) memcpy(IOH + 540, k, 32);
    if (run_op(op, 548, 144)) memcpy(z, IOH, 576);
    else fail_out(z, 576);
}
extern "C" void mclBn_millerLoopVec(mclBnGT *z, const mclBnG1 *x, const mclBnG2 *y, mclSize n) {
    mclBnGT acc, t;
    memset(&acc, 0, sizeof acc);
    const uint64_t errs = lcb_error_count();
    for (mclSize i = 0; i < n && lcb_error_count() == errs; i++) {
        mclBn_millerLoop(&t, &x[i], &y[i]);
        if (i == 0) acc = t;
        else mclBnGT_mul(&acc, &acc, &t);
    }
    if (lcb_error_count() != errs) fail_out(&acc, 576);
    *z = acc;
}
// debug-only (not in include/lachain_bls.h): apply tower routine `which` (k_ops.hip OP_DEBUG_FP12) to raw GT words
extern "C" int lcb_debug_fp12(int which, const uint32_t in[144], uint32_t out[144]) {
    LOCKED_OR(-1)
    memcpy(IOH + 252, in, 576);
    IOH[548] = (u32)which;
    if (!run_op(OP_DEBUG_FP12, 549, 144)) return -1;
    memcpy(out, IOH, 576);
    return 0;
}
// test hook: one routine under hash-to-G2, or one device point decoder, on n items, one lane each (k_h2g2_debug;
// h2g2_debug.hpp and include/lachain_bls.h have the layout: 48 words in, 76 words out per item).  Op 12 is no routine of
// that kernel: it runs k_mcl_g2_clear alone, once per item, on the mapped point (x, y, 1) — the second kernel of
// mclBnG2_hashAndMapTo with a chosen point in place of the first kernel's
extern "C" int lcb_debug_h2g2_op(int op, const uint32_t *in, size_t n, uint32_t *out) {
    SYNC_CTX_OR(c, -1)
    if (!n || n > 65536) { set_err("debug h2g2 op: 1..65536 items"); return -1; }
    const int n_ops = lcbk_h2g2_debug_ops();
    if (op < 0 || op > n_ops) { set_err("debug h2g2 op: unknown operation"); return -1; }
    if (!in || !out) { set_err("debug h2g2 op: missing operand"); return -1; }
    const size_t iw = lcbk_h2g2_debug_in_words(), ow = lcbk_h2g2_debug_out_words();
    HostCall h(c, "debug h2g2 op");
    if (op < n_ops) {
        const u32 *din = h.in(in, iw * n);
        u32 *dout = h.out<u32>(ow * n);
        if (!h.ok()) return -1;
        lcbk_h2g2_debug(h.s, op, din, (u32)n, dout);
        if (!launch_ok("debug h2g2 op launch")) return -1;
        h.back(out, dout, 4 * ow * n);
        return h.finish();
    }
    const size_t blk = 256;                           // one io block per item: the point at [0, 72), the flag at 249
    std::vector<u32> io(blk * n, 0u);
    for (size_t i = 0; i < n; i++) {
        memcpy(&io[blk * i], in + iw * i, 48 * 4);
        memcpy(&io[blk * i + 48], LCB_ONE_HOST, 48);
        io[blk * i + 249] = 1u;
    }
    u32 *dio = h.work(io.data(), blk * n);
    if (!h.ok()) return -1;
    for (size_t i = 0; i < n; i++) lcbk_mcl_g2_clear(h.s, dio + blk * i);
    if (!launch_ok("debug h2g2 op launch")) return -1;
    h.back(io.data(), dio, 4 * blk * n);
    if (h.finish()) return -1;
    memset(out, 0, 4 * ow * n);
    for (size_t i = 0; i < n; i++) {
        memcpy(out + ow * i, &io[blk * i], 72 * 4);
        out[ow * i + 72] = 1u;
    }
    return 0;
}
extern "C" void mclBnGT_mul(mclBnGT *z, const mclBnGT *x, const mclBnGT *y) {
    fph::fp12 t;
    fph::mul(t, *(const fph::fp12 *)x, *(const fph::fp12 *)y);
    memcpy(z, &t, 576);
}
extern "C" void mclBnGT_pow(mclBnGT *z, const mclBnGT *x, const mclBnFr *y) { gt_op(OP_GT_POW, z, x, nullptr, y); }
extern "C" int mclBnGT_isEqual(const mclBnGT *x, const mclBnGT *y) { return memcmp(x, y, 576) == 0; }
extern "C" int mclBnGT_isOne(const mclBnGT *x) {
    // Montgomery one of Fp in the first coordinate, zero elsewhere
    const u32 *w = (const u32 *)x;
    if (memcmp(w, LCB_ONE_HOST, 48) != 0) return 0;
    for (int i = 12; i < 144; i++) if (w[i]) return 0;
    return 1;
}
extern "C" int mclBnGT_isZero(const mclBnGT *x) {
    const u32 *w = (const u32 *)x;
    for (int i = 0; i < 144; i++) if (w[i]) return 0;
    return 1;
}
extern "C" void mclBnGT_clear(mclBnGT *x) { memset(x, 0, sizeof *x); }
extern "C" mclSize mclBnGT_serialize(void *buf, mclSize max, const mclBnGT *x) {
    if (max < 576) return 0;
    const fph::fp *a = (const fph::fp *)x;
    uint8_t *b = (uint8_t *)buf;
    for (int i = 0; i < 12; i++) {
        fph::fp r;
        fph::to_raw(r, a[i]);
        memcpy(b + 48 * i, r.v, 48);
    }
    return 576;
}
extern "C" mclSize mclBnGT_deserialize(mclBnGT *x, const void *buf, mclSize n) {
    if (n < 576) return 0;
    fph::fp m[12];
    for (int i = 0; i < 12; i++) {
        fph::fp raw;
        memcpy(raw.v, (const uint8_t *)buf + 48 * i, 48);
        if (!fph::raw_lt_p(raw)) return 0;
        fph::from_raw(m[i], raw);
    }
    memcpy(x, m, 576);
    return 576;
}
extern "C" int lcb_set_g2_sign_from_b(int use_b) {
    // unpinned mcl convention: which coordinate's parity the G2 wire flag carries.  Applies to every
    // later call, host (de)serialization and every kernel that (de)compresses G2 points alike; call it before any
    // batch work, not while one is running.
    if (!ready()) return -1;
    g_g2_sign_b.store(use_b != 0);
    if (lcbk_set_g2_sign_b(use_b != 0)) { set_err("lcb_set_g2_sign_from_b: device configuration failed"); return -1; }
    return 0;
}

// ================================================================== Fr Lagrange / polynomials (host, fr_host.hpp)
extern "C" int mclBn_FrLagrangeInterpolation(mclBnFr *out, const mclBnFr *xVec, const mclBnFr *yVec, mclSize k) {
    // mcl LagrangeInterpolation: sum_i y_i prod_{j != i} x_j / (x_j - x_i); zero or repeated x is an error
    if (k == 0) return -1;
    for (mclSize i = 0; i < k; i++) {
        if (mclBnFr_isZero(&xVec[i])) return -1;
        for (mclSize j = 0; j < i; j++)
            if (mclBnFr_isEqual(&xVec[i], &xVec[j])) return -1;
    }
    if (k == 1) { *out = yVec[0]; return 0; }
    mclBnFr a, acc, t, d;
    memcpy(&a, &xVec[0], 32);
    for (mclSize i = 1; i < k; i++) mclBnFr_mul(&a, &a, &xVec[i]);
    mclBnFr_clear(&acc);
    for (mclSize i = 0; i < k; i++) {
        mclBnFr b = xVec[i];
        for (mclSize j = 0; j < k; j++) {
            if (j == i) continue;
            mclBnFr_sub(&d, &xVec[j], &xVec[i]);
            mclBnFr_mul(&b, &b, &d);
        }
        mclBnFr_div(&t, &a, &b);
        mclBnFr_mul(&t, &t, &yVec[i]);
        mclBnFr_add(&acc, &acc, &t);
    }
    *out = acc;
    return 0;
}
extern "C" int mclBn_FrEvaluatePolynomial(mclBnFr *out, const mclBnFr *c, mclSize n, const mclBnFr *x) {
    if (n == 0) return -1;
    mclBnFr acc = c[n - 1];
    for (mclSize i = n - 1; i-- > 0;) {
        mclBnFr_mul(&acc, &acc, x);
        mclBnFr_add(&acc, &acc, &c[i]);
    }
    *out = acc;
    return 0;
}

// ================================================================== mcl surface on the batch / cooperative kernels
// (k_mcl.hip, k_coop.hip) — each a single synchronous call on the calling thread's own context

#define LCB_PAIR_CACHE 32    // line-set slots per context (2 x 26 KB each)
// mclBn_pairing (GT.Pairing: TPKE/PrivateKey.cs:26, TPKE/PublicKey.cs:91, ThresholdSignature/PublicKey.cs:20) as a
// one-group cooperative check: P and the point at infinity, Q's normalised line set and the set of infinity, then
// the nine-lane final exponentiation.  The lines are normalised (divided by their Fp2 leading coefficient), which
// changes the Miller value by a factor the final exponentiation removes: the GT value is mcl's.
// The line set of one G2 point on the host (pairing.hpp lineset_compute: the same 68 steps and formulas with the host
// field code, which gives the kernels' canonical residues; the normalised lines B' = Bc / A, C' = Cc / A depend only on
// the affine points, so they are the words k_lineset_coop writes).  False when some A_k == 0 (a point outside G2: the
// caller then takes the kernel, whose Miller loop computes such a set's lines on the fly).
static const bool g_pair_host_lines = !(getenv("LCB_PAIR_HOST_LINES") && atoi(getenv("LCB_PAIR_HOST_LINES")) == 0);
static bool lineset_host(uint32_t *dst, const fph::g2a &Q) {
    const int PT = LCB_LS_POINT_WORD, FLAG = PT + 48, NL = 68, NLW = 48;
    memset(dst, 0, LCB_LINESET_BYTES);
    memcpy(dst + PT, &Q.x, 96);
    memcpy(dst + PT + 24, &Q.y, 96);
    dst[FLAG + 1] = Q.inf ? 1u : 0u;
    if (Q.inf) { dst[FLAG] = 1u; return true; }   // every line is the constant 1: B' = C' = 0
    fph::fp twelve, raw12 = fph::zero();
    raw12.v[0] = 12;
    fph::from_raw(twelve, raw12);
    fph::fp2 b3;                                  // 3 b' = 12 (1 + u)
    b3.a = twelve;
    b3.b = twelve;
    fph::fp2 Tx = Q.x, Ty = Q.y, Tz = fph::one2();
    std::vector<fph::fp2> A(NL), B(NL), C(NL);
    int k = 0;
    for (int i = 62; i >= 0; i--) {
        {   // doubling step (ls_dbl_store): A = Y^2 - 3b'Z^2, Bc = -3X^2, Cc = 2YZ; T <- 2T
            fph::fp2 YZ, XY, ZZ, YY, t, u;
            fph::mul(YZ, Ty, Tz);
            fph::mul(XY, Tx, Ty);
            fph::sqr(ZZ, Tz);
            fph::sqr(YY, Ty);
            fph::sqr(t, Tx);
            fph::add(u, t, t);
            fph::add(u, u, t);
            fph::neg(B[k], u);
            fph::add(C[k], YZ, YZ);
            fph::mul(Tz, YY, YZ);
            fph::add(Tz, Tz, Tz);
            fph::mul(ZZ, ZZ, b3);
            fph::sub(A[k], YY, ZZ);
            k++;
            fph::add(t, ZZ, ZZ);
            fph::add(t, t, ZZ);
            fph::mul_fp(XY, XY, fph::INV2);
            fph::sub(u, YY, t);
            fph::mul(Tx, XY, u);
            fph::add(u, YY, t);
            fph::mul_fp(u, u, fph::INV2);
            fph::sqr(Ty, u);
            fph::sqr(t, ZZ);
            fph::add(u, t, t);
            fph::add(u, u, t);
            fph::sub(Ty, Ty, u);
        }
        if ((Z_ABS_H >> i) & 1) {   // addition step (ls_add_store): A = th xQ - la yQ, Bc = -th, Cc = la; T <- T + Q
            fph::fp2 th, la, t, D, E, G;
            fph::mul(t, Q.y, Tz);
            fph::sub(th, Ty, t);
            fph::mul(t, Q.x, Tz);
            fph::sub(la, Tx, t);
            fph::mul(A[k], th, Q.x);
            fph::mul(t, la, Q.y);
            fph::sub(A[k], A[k], t);
            fph::neg(B[k], th);
            C[k] = la;
            k++;
            fph::sqr(D, la);
            fph::mul(E, la, D);
            fph::mul(G, Tx, D);
            fph::sqr(t, th);
            fph::mul(D, Tz, t);
            fph::mul(Tz, Tz, E);
            fph::add(D, E, D);
            fph::sub(D, D, G);
            fph::sub(D, D, G);
            fph::mul(Tx, la, D);
            fph::sub(t, G, D);
            fph::mul(G, th, t);
            fph::mul(t, Ty, E);
            fph::sub(Ty, G, t);
        }
    }
    if (k != NL) return false;
    std::vector<fph::fp2> pre(NL);                // A_0 ... A_k, then one inversion (Montgomery's trick)
    pre[0] = A[0];
    for (int j = 1; j < NL; j++) fph::mul(pre[j], pre[j - 1], A[j]);
    if (fph::is_zero(pre[NL - 1])) return false;
    fph::fp2 inv;
    fph::inv(inv, pre[NL - 1]);
    for (int j = NL - 1; j >= 0; j--) {
        fph::fp2 ai, b, c;
        if (j > 0) fph::mul(ai, inv, pre[j - 1]);
        else ai = inv;
        fph::mul(inv, inv, A[j]);
        fph::mul(b, B[j], ai);
        fph::mul(c, C[j], ai);
        memcpy(dst + j * NLW, &b, 96);
        memcpy(dst + j * NLW + 24, &c, 96);
    }
    dst[FLAG] = 1u;
    return true;
}
extern "C" void mclBn_pairing(mclBnGT *z, const mclBnG1 *x, const mclBnG2 *y) {
    fail_out(z, 576);                  // overwritten on success; a failed call leaves a value no other call produces
    if (injected(INJ_PAIRING_ALLOC)) { set_err("injected failure (pairing)"); return; }
    SYNC_CTX_OR(c, )
    HostCall h(c, "pairing");
    hipStream_t s = h.s;
    const size_t slots = lcbk_fe_slots() > 6 ? (size_t)lcbk_fe_slots() : 6;
    // the group record (P and infinity, then the check's descriptor), staged in one copy
    struct PairIn {
        uint32_t g[2][LCB_G1A_ST_BYTES / 4];
        uint32_t desc[4];
    };
    static_assert(sizeof(PairIn) == 2 * LCB_G1A_ST_BYTES + 16, "PairIn layout");
    uint8_t *gin = h.out<uint8_t>(sizeof(PairIn));
    u32 *park = h.out<u32>(144 * slots);
    uint8_t *fl = h.out<uint8_t>(64);
    if (!h.ok()) return;
    u32 *lines = (u32 *)c->pc_lines.get((size_t)2 * LCB_PAIR_CACHE * LCB_LINESET_BYTES);
    if (!lines) { set_err("device allocation failed"); return; }
    void *gpts = gin, *desc = gin + 2 * LCB_G1A_ST_BYTES;
    if (c->pc_used.empty()) {
        c->pc_keys.assign((size_t)72 * LCB_PAIR_CACHE, 0);
        c->pc_used.assign(LCB_PAIR_CACHE, 0);
    }
    u32 slot = 0;
    bool hit = false;
    for (u32 k = 0; k < LCB_PAIR_CACHE; k++) {
        if (c->pc_used[k] && memcmp(&c->pc_keys[72 * (size_t)k], y, 288) == 0) { slot = k; hit = true; break; }
        if (c->pc_used[k] < c->pc_used[slot]) slot = k;
    }
    c->pc_used[slot] = ++c->pc_tick;
    if (!hit) memcpy(&c->pc_keys[72 * (size_t)slot], y, 288);
    // P and Q to affine on the calling thread (host inversions, tens of us) rather than in a one-lane kernel (~0.5 ms
    // per inversion): the same canonical residues the device's jac_to_aff gives
    PairIn pin;
    memset(&pin, 0, sizeof pin);
    {
        fph::g1 P;
        fph::g1a pa;
        memcpy(&P, x, sizeof P);
        fph::jac_to_aff(pa, P);
        memcpy(&pin.g[0][0], &pa.x, 48);
        memcpy(&pin.g[0][12], &pa.y, 48);
        pin.g[0][24] = pa.inf ? 1u : 0u;
        pin.g[0][25] = 1u;                           // ok
        pin.g[1][24] = 1u;                           // the point at infinity
        pin.g[1][25] = 1u;
        pin.desc[0] = 0u;                            // check 0: points 0 and 1, line-set pair `slot`
        pin.desc[1] = 1u;
        pin.desc[2] = slot;
    }
    hipMemcpyAsync(gin, &pin, sizeof pin, hipMemcpyHostToDevice, s);
    std::vector<uint32_t> hsets;                     // the host line sets (alive until the call's synchronisation)
    bool host_sets = false;
    if (!hit && g_pair_host_lines) {                 // Q's set and the infinity set computed here, one upload
        fph::g2 Q;
        fph::g2a qa, ia;
        memcpy(&Q, y, sizeof Q);
        fph::jac_to_aff(qa, Q);
        memset(&ia, 0, sizeof ia);
        ia.inf = true;
        hsets.assign((size_t)2 * LCB_LINESET_BYTES / 4, 0u);
        if (lineset_host(hsets.data(), qa) && lineset_host(hsets.data() + LCB_LINESET_BYTES / 4, ia)) {
            hipMemcpyAsync(lines + (size_t)2 * slot * (LCB_LINESET_BYTES / 4), hsets.data(), 2 * (size_t)LCB_LINESET_BYTES,
                           hipMemcpyHostToDevice, s);
            host_sets = true;
        }
    }
    if (!hit && !host_sets) {                        // the two sets' points for k_lineset_fill: Q, then infinity
        fph::g2 Q;
        fph::g2a qa;
        memcpy(&Q, y, sizeof Q);
        fph::jac_to_aff(qa, Q);
        uint32_t pt[2][51];                          // x, y (48 words), LCB_LS_FLAG, + 1 (infinity), + 2 (force general)
        memset(pt, 0, sizeof pt);
        memcpy(&pt[0][0], &qa.x, 96);
        memcpy(&pt[0][24], &qa.y, 96);
        pt[0][49] = qa.inf ? 1u : 0u;
        pt[1][49] = 1u;
        for (int k = 0; k < 2; k++)
            hipMemcpyAsync(lines + (size_t)(2 * slot + k) * (LCB_LINESET_BYTES / 4) + LCB_LS_POINT_WORD, pt[k],
                           sizeof pt[k], hipMemcpyHostToDevice, s);
    }
    if (!hit && !host_sets) lcbk_lineset_coop(s, lines + (size_t)2 * slot * (LCB_LINESET_BYTES / 4), 2, nullptr, nullptr);
    lcbk_coop_tpke_miller(s, lines, desc, gpts, 1, park, fl, fl + 32, 1, 1);
    lcbk_coop_final_exp_check(s, park, 1, nullptr);
    u32 r[144];
    h.back(r, park, 576);
    if (!h.finish()) memcpy(z, r, 576);
    else c->pc_used[slot] = 0;                    // the slot's lines may be incomplete
}
// mclBn_finalExp on the nine-lane kernel (park slot 0 of a one-value workspace)
extern "C" void mclBn_finalExp(mclBnGT *y, const mclBnGT *x) {
    mclBnGT xin = *x;                  // y may alias x
    x = &xin;
    fail_out(y, 576);
    SYNC_CTX_OR(c, )
    HostCall h(c, "final exp");
    hipStream_t s = h.s;
    const size_t slots = lcbk_fe_slots() > 6 ? (size_t)lcbk_fe_slots() : 6;
    u32 *park = h.out<u32>(144 * slots);
    if (!h.ok()) return;
    hipMemcpyAsync(park, x, 576, hipMemcpyHostToDevice, s);    // slot 0 of the park workspace
    lcbk_coop_final_exp_check(s, park, 1, nullptr);
    u32 r[144];
    h.back(r, park, 576);
    if (!h.finish()) memcpy(y, r, 576);
}
// sum_i [k_i] x_i (canonical scalars k_i < r, raw words) on the cooperative ladders of mclBnG1_mul: three groups per
// term (GLV halves over P and phi(P), and [z^2] P for the membership the split needs), k_ptmul_g1_multi, the terms
// added on the host.  Returns 1 with *z set, 0 when a term is not on the curve or outside G1 (the caller then takes
// its exact path, so every input keeps that path's value), -1 on a device error.
static const size_t MULVEC_COOP_MAX = 512;
static const bool g_mulvec_coop = !(getenv("LCB_MULVEC_COOP") && atoi(getenv("LCB_MULVEC_COOP")) == 0);
static int g1_mulvec_coop(lcb_ctx *c, mclBnG1 *z, const mclBnG1 *x, const uint64_t (*kraw)[4], size_t n) {
    std::vector<PtJobG1> jobs(3 * n);
    memset(jobs.data(), 0, jobs.size() * sizeof(PtJobG1));
    std::vector<fph::g1a> phis(n);
    std::vector<uint8_t> live(n, 0);
    const u128h zz = (u128h)Z_ABS_H * Z_ABS_H;
    const uint64_t z2[2] = {(uint64_t)zz, (uint64_t)(zz >> 64)}, zero[1] = {0};
    for (size_t i = 0; i < n; i++) {
        PtJobG1 *J = &jobs[3 * i];
        const uint64_t *k = kraw[i];
        fph::g1a P;
        fph::jac_to_aff(P, *G1R(&x[i]));
        if (!P.inf && !fph::jac_on_curve(*G1R(&x[i]))) return 0;
        if (P.inf || (k[0] | k[1] | k[2] | k[3]) == 0) {          // a zero term: three idle ladders
            for (int j = 0; j < 3; j++) { J[j].inf = 1; put_digits(J[j], zero, 1, 33); }
            continue;
        }
        uint64_t q[4] = {k[0], k[1], k[2], k[3]};
        const uint64_t d0 = divmod_u(q), d1 = divmod_u(q);
        const u128h a0 = (u128h)d1 * Z_ABS_H + d0, a1 = (u128h)q[1] << 64 | q[0];
        const u128h sum = a0 + a1;
        const uint64_t k1[3] = {(uint64_t)sum, (uint64_t)(sum >> 64), sum < a0 ? 1ull : 0ull};
        const uint64_t k2[2] = {(uint64_t)a1, (uint64_t)(a1 >> 64)};
        fph::g1_phi(phis[i], P);
        put_point(J[0], P);
        put_point(J[1], phis[i]);
        put_point(J[2], P);
        if (!put_digits(J[0], k1, 3, 33) || !put_digits(J[1], k2, 2, 33) || !put_digits(J[2], z2, 2, 33)) return 0;
        live[i] = 1;
    }
    HostCall h(c, "mulVec");
    const PtJobG1 *dj = h.in(jobs.data(), jobs.size());
    fph::g1 *dout = h.out<fph::g1>(3 * n);
    if (!h.ok()) return -1;
    lcbk_ptmul_g1_multi(h.s, dj, (u32)(3 * n), dout);
    std::vector<fph::g1> acc(3 * n);
    h.back(acc.data(), dout, 3 * n * sizeof(fph::g1));
    if (h.finish()) return -1;
    fph::g1 r;
    fph::jac_set_inf(r);
    for (size_t i = 0; i < n; i++) {
        if (!live[i]) continue;
        fph::g1a chk;
        fph::g1_phi(chk, phis[i]);                // (beta^2 x, y) -> membership: [z^2] P == (beta^2 x, -y)
        fph::neg(chk.y, chk.y);
        if (!fph::jac_eq_aff(acc[3 * i + 2], chk)) return 0;
        fph::g1 t;
        fph::jac_add(t, acc[3 * i], acc[3 * i + 1]);
        fph::jac_add(r, r, t);
    }
    *G1W(z) = r;
    return 1;
}
// the G2 counterpart: sum_i [k_i] x_i on mclBnG2_mul's GLS ladders (five groups per term, k_ptmul_g2_multi); the
// same return convention (0: a term off the curve or outside G2 — the caller's exact path)
static int g2_terms_coop(lcb_ctx *c, mclBnG2 *z, const mclBnG2 *x, const uint64_t (*kraw)[4], size_t n) {
    std::vector<PtJobG2> jobs(5 * n);
    memset(jobs.data(), 0, jobs.size() * sizeof(PtJobG2));
    std::vector<fph::g2a> psis(n);
    std::vector<uint8_t> live(n, 0);
    const uint64_t zero[1] = {0};
    for (size_t i = 0; i < n; i++) {
        PtJobG2 *J = &jobs[5 * i];
        const uint64_t *k = kraw[i];
        fph::g2a Q;
        fph::jac_to_aff(Q, *G2R(&x[i]));
        if (!Q.inf && !fph::jac_on_curve(*G2R(&x[i]))) return 0;
        if (Q.inf || (k[0] | k[1] | k[2] | k[3]) == 0) {
            for (int j = 0; j < 5; j++) { J[j].inf = 1; put_digits(J[j], zero, 1, 17); }
            continue;
        }
        uint64_t q[4] = {k[0], k[1], k[2], k[3]}, d[4];
        d[0] = divmod_u(q);
        d[1] = divmod_u(q);
        d[2] = divmod_u(q);
        d[3] = q[0];
        fph::g2a B[4];
        B[0] = Q;
        fph::g2_psi(B[1], Q);
        fph::g2_psi(B[2], B[1]);
        fph::g2_psi(B[3], B[2]);
        psis[i] = B[1];
        fph::neg(B[1].y, B[1].y);
        fph::neg(B[3].y, B[3].y);
        bool ok = true;
        for (int j = 0; j < 4; j++) {
            put_point(J[j], B[j]);
            ok &= put_digits(J[j], &d[j], 1, 17);
        }
        put_point(J[4], Q);
        ok &= put_digits(J[4], &Z_ABS_H, 1, 17);
        if (!ok) return 0;
        live[i] = 1;
    }
    HostCall h(c, "G2 terms");
    const PtJobG2 *dj = h.in(jobs.data(), jobs.size());
    fph::g2 *dout = h.out<fph::g2>(5 * n);
    if (!h.ok()) return -1;
    lcbk_ptmul_g2_multi(h.s, dj, (u32)(5 * n), dout);
    std::vector<fph::g2> acc(5 * n);
    h.back(acc.data(), dout, 5 * n * sizeof(fph::g2));
    if (h.finish()) return -1;
    fph::g2 r;
    fph::jac_set_inf(r);
    for (size_t i = 0; i < n; i++) {
        if (!live[i]) continue;
        fph::g2a chk = psis[i];                   // membership: psi(Q) == -[|z|] Q
        fph::neg(chk.y, chk.y);
        if (!fph::jac_eq_aff(acc[5 * i + 4], chk)) return 0;
        for (int j = 0; j < 4; j++) fph::jac_add(r, r, acc[5 * i + j]);
    }
    *G2W(z) = r;
    return 1;
}
// Lagrange coefficients lambda_i = prod_{j != i} x_j / (x_j - x_i) as canonical raw words; false on a zero or
// repeated x (the error of k_lagrange_coeffs)
static bool lagrange_lambdas(std::vector<uint64_t> &raw, const mclBnFr *xVec, size_t k) {
    raw.assign(4 * k, 0);
    static const uint64_t one_raw[4] = {1, 0, 0, 0};
    for (size_t i = 0; i < k; i++) {
        const uint64_t *xi = FRV(&xVec[i]);
        if (frh::is_zero(xi)) { set_err("lagrange: zero x"); return false; }
        uint64_t num[4], den[4], t[4];
        frh::from_raw(num, one_raw);
        memcpy(den, num, 32);
        for (size_t j = 0; j < k; j++) {
            if (j == i) continue;
            const uint64_t *xj = FRV(&xVec[j]);
            frh::sub(t, xj, xi);
            if (frh::is_zero(t)) { set_err("lagrange: repeated x"); return false; }
            frh::mul(num, num, xj);
            frh::mul(den, den, t);
        }
        frh::inv(den, den);
        frh::mul(t, num, den);
        frh::to_raw(&raw[4 * i], t);
    }
    return true;
}
// mclBnG1_mulVec: sum_i [y_i] x_i with the canonical scalars (mcl's per-term product, exact for any on-curve x_i):
// up to MULVEC_COOP_MAX terms on the cooperative ladders above; otherwise (or for a term outside G1) one lane per term
// (windowed ladder), then block reductions and a one-lane sum
static bool g1_mulvec(mclBnG1 *z, const mclBnG1 *x, const mclBnFr *y, mclSize n) {
    SYNC_CTX_OR(c, false)
    if (n > 0xffffffffu) { set_err("mulVec: too large"); return false; }
    std::vector<uint64_t> raw(4 * n);
    for (size_t i = 0; i < n; i++) frh::to_raw(&raw[4 * i], FRV(&y[i]));
    if (n <= MULVEC_COOP_MAX && g_mulvec_coop) {
        const int rc = g1_mulvec_coop(c, z, x, (const uint64_t (*)[4])raw.data(), n);
        if (rc != 0) return rc > 0;
    }
    HostCall h(c, "mulVec");
    hipStream_t s = h.s;
    const u32 *pts = h.in((const u32 *)x, 36 * n);
    const uint64_t *sc = h.in(raw.data(), 4 * n);
    uint8_t *terms = h.out<uint8_t>(LCB_G1_JAC_BYTES * n);
    uint8_t *tmp = h.out<uint8_t>(LCB_G1_JAC_BYTES * ((n + 255) / 256));
    uint8_t *dz = h.out<uint8_t>(LCB_G1_JAC_BYTES);
    u32 *ws = h.lws(lcbk_mcl_terms_ws_bytes((u32)n));
    if (!h.ok()) return false;
    lcbk_mcl_g1_terms(s, pts, sc, (u32)n, terms, ws);
    uint8_t *cur = terms;
    size_t cnt = n;
    while (cnt > 256) {
        uint8_t *dst = cur == terms ? tmp : terms;
        lcbk_g1_jac_reduce_block(s, cur, (u32)cnt, 256, dst);
        cnt = (cnt + 255) / 256;
        cur = dst;
    }
    lcbk_mcl_g1_sum(s, cur, (u32)cnt, dz);
    mclBnG1 r;
    h.back(&r, dz, 144);
    if (h.finish()) return false;
    *z = r;
    return true;
}
extern "C" void mclBnG1_mulVec(mclBnG1 *z, const mclBnG1 *x, const mclBnFr *y, mclSize n) {
    if (n == 0) { mclBnG1_clear(z); return; }
    if (!g1_mulvec(z, x, y, n)) fail_out(z, 144);
}
// G1 / G2 Lagrange interpolation of one problem on the batch kernels: mcl records -> wire bytes on the device, the
// k_lagrange.hip coefficient + product kernels, the result decoded back into an mcl record (one round trip)
static int lagrange_points(int g, void *out, const mclBnFr *xVec, const void *yVec, mclSize k) {
    if (k == 0) return -1;
    SYNC_CTX_OR(c, -1)
    if (k > 0xffffffffu) { set_err("lagrange: too large"); return -1; }
    const size_t pb = g == 1 ? 48 : 96, words = g == 1 ? 36 : 72;
    std::vector<uint64_t> xs(4 * k);
    for (size_t i = 0; i < k; i++) frh::to_raw(&xs[4 * i], FRV(&xVec[i]));
    const uint32_t off[2] = {0, (uint32_t)k};
    HostCall h(c, "lagrange");
    hipStream_t s = h.s;
    const uint8_t *dx = (const uint8_t *)h.in(xs.data(), 4 * k);
    const u32 *dyr = h.in((const u32 *)yVec, words * k);
    const uint32_t *doff = h.in(off, 2);
    uint8_t *dy = h.out<uint8_t>(pb * k);
    uint8_t *dst = h.out<uint8_t>(16), *dout = h.out<uint8_t>(pb);
    u32 *rec = h.out<u32>(words);
    uint8_t *dok = h.out<uint8_t>(16);
    if (!h.ok()) return -1;
    lcbk_mcl_to_bytes(s, g, dyr, (u32)k, dy);
    if (lagrange_enqueue(c, g, dout, dst, dx, dy, doff, 1, k, s)) return -1;
    lcbk_mcl_from_bytes(s, g, dout, 1, rec, dok);
    u32 r[72];
    uint8_t st = 0, ok = 0;
    h.back(r, rec, words * 4);
    h.back(&st, dst, 1);
    h.back(&ok, dok, 1);
    if (h.finish() || !st || !ok) return -1;
    memcpy(out, r, words * 4);
    return 0;
}
// G1 Lagrange interpolation of up to 64 points: the coefficients lambda_i = prod_{j != i} x_j / (x_j - x_i) on the host
// (-1 on a zero or repeated x, as k_lagrange_coeffs), the products on the cooperative ladders (g1_mulvec_coop); 1 done,
// 0 for the batch kernels' path (a point outside G1, or more points)
static int g1_lagrange_coop(mclBnG1 *out, const mclBnFr *xVec, const mclBnG1 *yVec, size_t k) {
    if (k > 64 || !g_mulvec_coop) return 0;
    SYNC_CTX_OR(c, -1)
    std::vector<uint64_t> raw;
    if (!lagrange_lambdas(raw, xVec, k)) return -1;
    const int rc = g1_mulvec_coop(c, out, yVec, (const uint64_t (*)[4])raw.data(), k);
    return rc < 0 ? -1 : rc;
}
// the same in G2 (AssembleSignature's interpolation, ThresholdSignature/PublicKeySet.cs:34-42)
static int g2_lagrange_coop(mclBnG2 *out, const mclBnFr *xVec, const mclBnG2 *yVec, size_t k) {
    if (k > 64 || !g_mulvec_coop) return 0;
    SYNC_CTX_OR(c, -1)
    std::vector<uint64_t> raw;
    if (!lagrange_lambdas(raw, xVec, k)) return -1;
    const int rc = g2_terms_coop(c, out, yVec, (const uint64_t (*)[4])raw.data(), k);
    return rc < 0 ? -1 : rc;
}
extern "C" int mclBn_G1LagrangeInterpolation(mclBnG1 *out, const mclBnFr *xVec, const mclBnG1 *yVec, mclSize k) {
    if (k == 1) { *out = yVec[0]; return mclBnFr_isZero(&xVec[0]) ? -1 : 0; }
    if (k == 0) return -1;
    const int rc = g1_lagrange_coop(out, xVec, yVec, k);
    if (rc != 0) return rc > 0 ? 0 : -1;
    return lagrange_points(1, out, xVec, yVec, k);
}
extern "C" int mclBn_G2LagrangeInterpolation(mclBnG2 *out, const mclBnFr *xVec, const mclBnG2 *yVec, mclSize k) {
    if (k == 1) { *out = yVec[0]; return mclBnFr_isZero(&xVec[0]) ? -1 : 0; }
    if (k == 0) return -1;
    const int rc = g2_lagrange_coop(out, xVec, yVec, k);
    if (rc != 0) return rc > 0 ? 0 : -1;
    return lagrange_points(2, out, xVec, yVec, k);
}
// out = a x mod #E(Fp) for G1 (a < #E, x < 2^256): #E(Fp) = p - z = h r (z = -0xd201000000010000), so [k] P depends
// only on k mod #E for every point P of E(Fp), in the subgroup or not
static void ne_mulmod(uint64_t out[6], const uint64_t a[6], const uint64_t x[4]) {
    static const uint64_t NE[6] = {0x8c0000000000aaabull, 0x1eabfffeb1540000ull, 0x6730d2a0f6b0f624ull,
                                   0x64774b84f38512bfull, 0x4b1ba7b6434bacd7ull, 0x1a0111ea397fe69aull};
    typedef unsigned __int128 u128;
    uint64_t prod[10] = {0};
    for (int i = 0; i < 6; i++) {
        uint64_t carry = 0;
        for (int j = 0; j < 4; j++) {
            const u128 t = (u128)a[i] * x[j] + prod[i + j] + carry;
            prod[i + j] = (uint64_t)t;
            carry = (uint64_t)(t >> 64);
        }
        prod[i + 4] = carry;
    }
    uint64_t rem[6] = {0};                       // long division by bits: rem < NE < 2^381, so 2 rem + 1 fits
    for (int b = 639; b >= 0; b--) {
        for (int k = 5; k > 0; k--) rem[k] = (rem[k] << 1) | (rem[k - 1] >> 63);
        rem[0] = (rem[0] << 1) | ((prod[b >> 6] >> (b & 63)) & 1);
        int ge = 1;
        for (int k = 5; k >= 0; k--) {
            if (rem[k] != NE[k]) { ge = rem[k] > NE[k]; break; }
        }
        if (ge) {
            uint64_t br = 0;
            for (int k = 0; k < 6; k++) {
                const u128 t = (u128)rem[k] - NE[k] - br;
                rem[k] = (uint64_t)t;
                br = (uint64_t)(t >> 64) & 1;
            }
        }
    }
    memcpy(out, rem, 48);
}
// G1 EvaluatePolynomial as a sum of independent terms: sum_i [x^i mod #E] c_i (k_mcl_g1_terms_wide, one lane per term,
// then the mulVec sums) — the value of mcl's Horner rule for every on-curve coefficient, with the products side by
// side instead of n - 1 dependent ones
static int eval_poly_g1_terms(lcb_ctx *c, mclBnG1 *out, const mclBnG1 *coef, size_t n, const uint64_t xr[4]) {
    std::vector<uint32_t> sc(12 * n);
    uint64_t e[6] = {1, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < n; i++) {
        if (i) ne_mulmod(e, e, xr);
        memcpy(&sc[12 * i], e, 48);
    }
    HostCall h(c, "evaluate polynomial");
    hipStream_t s = h.s;
    const u32 *pts = h.in((const u32 *)coef, 36 * n);
    const u32 *dsc = h.in(sc.data(), 12 * n);
    uint8_t *terms = h.out<uint8_t>(LCB_G1_JAC_BYTES * n);
    uint8_t *tmp = h.out<uint8_t>(LCB_G1_JAC_BYTES * ((n + 255) / 256));
    uint8_t *dz = h.out<uint8_t>(LCB_G1_JAC_BYTES);
    u32 *ws = h.lws(lcbk_mcl_terms_wide_ws_bytes((u32)n));
    if (!h.ok()) return -1;
    lcbk_mcl_g1_terms_wide(s, pts, dsc, (u32)n, terms, ws);
    uint8_t *cur = terms;
    size_t cnt = n;
    while (cnt > 256) {
        uint8_t *dst = cur == terms ? tmp : terms;
        lcbk_g1_jac_reduce_block(s, cur, (u32)cnt, 256, dst);
        cnt = (cnt + 255) / 256;
        cur = dst;
    }
    lcbk_mcl_g1_sum(s, cur, (u32)cnt, dz);
    mclBnG1 r;
    h.back(&r, dz, 144);
    if (h.finish()) return -1;
    *out = r;
    return 0;
}
// G1 / G2 EvaluatePolynomial: mcl's Horner rule (y = c[n-1]; y = y x + c[i]) — the products are by the integer x, as
// mcl's, so off-subgroup coefficients give mcl's value too.  G1 (n >= 2): the same value as independent terms (above);
// G2 and LCB_EVAL_HORNER=1: the Horner chain in one kernel launch
static int eval_poly(int g, void *out, const void *coef, mclSize n, const mclBnFr *x) {
    if (n == 0) return -1;
    SYNC_CTX_OR(c, -1)
    if (n > 0xffffffffu) { set_err("evaluate polynomial: too large"); return -1; }
    const size_t words = g == 1 ? 36 : 72;
    uint64_t xr[4];
    frh::to_raw(xr, FRV(x));
    static const bool horner = getenv("LCB_EVAL_HORNER") && atoi(getenv("LCB_EVAL_HORNER")) == 1;
    if (g == 1 && n >= 2 && n <= MULVEC_COOP_MAX && !horner && g_mulvec_coop) {
        // coefficients in G1: [x^i mod r] c_i on the cooperative ladders (a coefficient outside G1 returns 0 here
        // and takes the terms below, whose powers are reduced mod #E(Fp) instead)
        std::vector<uint64_t> raw(4 * n);
        uint64_t pw[4], one_raw[4] = {1, 0, 0, 0};
        frh::from_raw(pw, one_raw);
        for (size_t i = 0; i < n; i++) {
            frh::to_raw(&raw[4 * i], pw);
            frh::mul(pw, pw, FRV(x));
        }
        const int rc = g1_mulvec_coop(c, (mclBnG1 *)out, (const mclBnG1 *)coef, (const uint64_t (*)[4])raw.data(), n);
        if (rc != 0) return rc > 0 ? 0 : -1;
    }
    if (g == 1 && n >= 2 && !horner) return eval_poly_g1_terms(c, (mclBnG1 *)out, (const mclBnG1 *)coef, n, xr);
    if (g == 2 && n >= 2 && n <= 64 && !horner && g_mulvec_coop) {   // coefficients in G2: [x^i mod r] c_i, GLS
        std::vector<uint64_t> raw(4 * n);
        uint64_t pw[4], one_raw[4] = {1, 0, 0, 0};
        frh::from_raw(pw, one_raw);
        for (size_t i = 0; i < n; i++) {
            frh::to_raw(&raw[4 * i], pw);
            frh::mul(pw, pw, FRV(x));
        }
        const int rc = g2_terms_coop(c, (mclBnG2 *)out, (const mclBnG2 *)coef, (const uint64_t (*)[4])raw.data(), n);
        if (rc != 0) return rc > 0 ? 0 : -1;
    }
    HostCall h(c, "evaluate polynomial");
    const u32 *dc = h.in((const u32 *)coef, words * n);
    const uint64_t *dx = h.in(xr, 4);
    u32 *dout = h.out<u32>(words);
    if (!h.ok()) return -1;
    lcbk_mcl_horner(h.s, g, dc, (u32)n, dx, dout);
    u32 r[72];
    h.back(r, dout, words * 4);
    if (h.finish()) return -1;
    memcpy(out, r, words * 4);
    return 0;
}
extern "C" int mclBn_G1EvaluatePolynomial(mclBnG1 *out, const mclBnG1 *c, mclSize n, const mclBnFr *x) {
    return eval_poly(1, out, c, n, x);
}
extern "C" int mclBn_G2EvaluatePolynomial(mclBnG2 *out, const mclBnG2 *c, mclSize n, const mclBnFr *x) {
    return eval_poly(2, out, c, n, x);
}
