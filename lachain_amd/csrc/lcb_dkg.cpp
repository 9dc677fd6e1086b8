// lachain_amd/csrc/lcb_dkg.cpp — host side of the trustless DKG's G1 work (include/lachain_bls.h lcb_dkg_*,
// lcb_g1_eval_poly_batch; kernels: k_dkg.hip).
//
// Commitment.Evaluate(x, y) / Evaluate(x) (src/Lachain.Consensus/ThresholdKeygen/Data/Commitment.cs:23-53) for whole
// batches: rows of every distinct (commitment, x) once, then Horner in y per query.  Each entry point is a synchronous
// call on the calling thread's host-pointer context; every buffer is staging of the one call (HostCall).
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "launch.h"
#include "lcb_internal.hpp"
#include "../../include/lachain_bls.h"

using namespace lcb_int;

namespace {
// any decodable point of d_aff (n records) outside G1 (k_g1_subgroup_any; one 4-byte read)
int g1_any_off_subgroup(HostCall &h, const void *d_aff, size_t n, bool *any) {
    hipStream_t s = h.s;
    u32 *d = h.out<u32>(1);
    if (!h.ok()) return -1;
    hipMemsetAsync(d, 0, 4, s);
    if (n) lcbk_g1_subgroup_any(s, d_aff, (u32)n, d);
    u32 any_w = 0;
    if (!launch_ok("subgroup test launch")) return -1;
    if (hipMemcpyAsync(&any_w, d, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        set_err("batched verify: group count");
        return -1;
    }
    *any = any_w != 0;
    return 0;
}
// Commitment.Evaluate(x) rows of n_rows (commitment, x) pairs.  Honest commitments (every coefficient in G1): Horner in
// the small x (k_dkg_rows).  A batch with a coefficient outside G1: the reference's own terms [x^j mod r] C (exact).
int dkg_rows_enqueue(HostCall &h, const uint8_t *d_coeffs, size_t n_comm, size_t n_coef, int degree,
                     const uint32_t *d_comm, const int32_t *d_xs, size_t n_rows, void **rows_out, uint8_t **rows_ok,
                     bool *exact) {
    hipStream_t s = h.s;
    size_t total = n_comm * n_coef, lanes = n_rows * (size_t)(degree + 1);
    if (total > 0xffffffffu || lanes > 0xffffffffu) { set_err("dkg: batch too large"); return -1; }
    void *aff = h.out<uint8_t>(total * LCB_G1A_ST_BYTES);
    void *rows = h.out<uint8_t>(lanes * LCB_G1_JAC_BYTES);
    uint8_t *rok = h.out<uint8_t>(lanes);
    if (!h.ok()) return -1;
    if (total) lcbk_g1_decompress(dim3(nblk(total)), s, d_coeffs, (u32)total, aff);
    if (g1_any_off_subgroup(h, aff, total, exact)) return -1;
    if (lanes && !*exact) {
        lcbk_dkg_rows(dim3(nblk(lanes)), s, aff, (u32)n_coef, (u32)n_comm, (u32)degree, d_comm, d_xs, (u32)n_rows, rows,
                      rok);
    } else if (lanes) {
        const size_t nt = lanes * (size_t)(degree + 1);
        if (nt > 0xffffffffu) { set_err("dkg: batch too large for the exact form"); return -1; }
        void *terms = h.out<uint8_t>(nt * LCB_G1_JAC_BYTES);
        uint8_t *tok = h.out<uint8_t>(nt);
        if (!h.ok()) return -1;
        lcbk_dkg_exact_terms(s, aff, (u32)n_coef, (u32)n_comm, (u32)degree, d_comm, d_xs, (u32)n_rows, terms, tok);
        lcbk_g1_jac_reduce_groups(dim3(nblk(lanes)), s, terms, (u32)nt, (u32)(degree + 1), rows);
        lcbk_and_groups(s, tok, (u32)lanes, (u32)(degree + 1), rok);
    }
    *rows_out = rows;
    *rows_ok = rok;
    return launch_ok("dkg rows launch") ? 0 : -1;
}
bool dkg_shape(size_t n_comm, int degree, size_t *n_coef) {
    if (degree < 0 || degree > 4096) { set_err("dkg: degree out of range"); return false; }
    *n_coef = (size_t)(degree + 1) * (size_t)(degree + 2) / 2;
    (void)n_comm;
    return true;
}
}  // namespace
extern "C" int lcb_dkg_commitment_rows(uint8_t *rows_out, uint8_t *status, const uint8_t *coeffs, size_t n_comm,
                                       int degree, const uint32_t *comm_idx, const int32_t *xs, size_t n_queries) {
    SYNC_CTX_OR(c, -1)
    size_t n_coef;
    if (!dkg_shape(n_comm, degree, &n_coef)) return -1;
    if (!n_queries) return 0;
    HostCall h(c, "dkg rows");
    hipStream_t s = h.s;
    size_t lanes = n_queries * (size_t)(degree + 1);
    const uint8_t *dco = h.in(coeffs, 48 * n_comm * n_coef);
    const uint32_t *dci = h.in(comm_idx, n_queries);
    const int32_t *dx = h.in(xs, n_queries);
    uint8_t *dout = h.out<uint8_t>(48 * lanes);
    if (!h.ok()) return -1;
    void *rows;
    uint8_t *rok;
    bool exact = false;
    if (dkg_rows_enqueue(h, dco, n_comm, n_coef, degree, dci, dx, n_queries, &rows, &rok, &exact)) return -1;
    lcbk_g1_jac_compress(dim3(nblk(lanes)), s, rows, (u32)lanes, dout);
    std::vector<uint8_t> ok(lanes);
    h.back(rows_out, dout, 48 * lanes);
    h.back(ok.data(), rok, lanes);
    if (h.finish()) return -1;
    for (size_t qi = 0; qi < n_queries; qi++) {
        uint8_t st = 1;
        for (int i = 0; i <= degree; i++) st &= ok[qi * (degree + 1) + i];
        status[qi] = st;
    }
    return 0;
}
extern "C" int lcb_dkg_commitment_eval(uint8_t *out, uint8_t *status, const uint8_t *coeffs, size_t n_comm, int degree,
                                       const uint32_t *comm_idx, const int32_t *xs, const int32_t *ys,
                                       size_t n_queries) {
    SYNC_CTX_OR(c, -1)
    size_t n_coef;
    if (!dkg_shape(n_comm, degree, &n_coef)) return -1;
    if (!n_queries) return 0;
    // distinct (commitment, x) pairs -> rows; every query evaluates its row at y
    std::vector<uint32_t> row_comm, row_of(n_queries);
    std::vector<int32_t> row_x;
    {
        std::vector<std::pair<uint64_t, uint32_t>> keys(n_queries);
        for (size_t i = 0; i < n_queries; i++) keys[i] = {((uint64_t)comm_idx[i] << 32) | (uint32_t)xs[i], (uint32_t)i};
        std::sort(keys.begin(), keys.end());
        for (size_t i = 0; i < n_queries; i++) {
            if (i == 0 || keys[i].first != keys[i - 1].first) {
                row_comm.push_back((uint32_t)(keys[i].first >> 32));
                row_x.push_back((int32_t)(uint32_t)keys[i].first);
            }
            row_of[keys[i].second] = (uint32_t)(row_comm.size() - 1);
        }
    }
    HostCall h(c, "dkg eval");
    hipStream_t s = h.s;
    const uint8_t *dco = h.in(coeffs, 48 * n_comm * n_coef);
    const uint32_t *drc = h.in(row_comm.data(), row_comm.size());
    const int32_t *drx = h.in(row_x.data(), row_x.size());
    const uint32_t *drow = h.in(row_of.data(), n_queries);
    const int32_t *dy = h.in(ys, n_queries);
    uint8_t *dout = h.out<uint8_t>(48 * n_queries), *dst = h.out<uint8_t>(n_queries);
    if (!h.ok()) return -1;
    void *rows;
    uint8_t *rok;
    bool exact = false;
    if (dkg_rows_enqueue(h, dco, n_comm, n_coef, degree, drc, drx, row_comm.size(), &rows, &rok, &exact)) return -1;
    if (!exact) {
        lcbk_dkg_horner(dim3(nblk(n_queries)), s, rows, rok, (u32)degree, drow, dy, (u32)n_queries, dout, dst, 0);
        h.back(out, dout, 48 * n_queries);
        h.back(status, dst, n_queries);
        return h.finish();
    }
    // a coefficient outside G1: sum_j [y^j mod r] row_j(x) (Commitment.cs:23-37 as written)
    const size_t D1 = (size_t)degree + 1, nt = n_queries * D1;
    void *terms = h.out<uint8_t>(nt * LCB_G1_JAC_BYTES), *sums = h.out<uint8_t>(n_queries * LCB_G1_JAC_BYTES);
    if (!h.ok()) return -1;
    lcbk_dkg_exact_combine(s, rows, (u32)degree, drow, dy, (u32)n_queries, terms);
    lcbk_g1_jac_reduce_groups(dim3(nblk(n_queries)), s, terms, (u32)nt, (u32)D1, sums);
    lcbk_g1_jac_compress(dim3(nblk(n_queries)), s, sums, (u32)n_queries, dout);
    std::vector<uint8_t> rk(row_comm.size() * D1);
    h.back(out, dout, 48 * n_queries);
    h.back(rk.data(), rok, rk.size());
    if (h.finish()) return -1;
    for (size_t qi = 0; qi < n_queries; qi++) {
        uint8_t st = 1;
        for (size_t j = 0; j < D1; j++) st &= rk[row_of[qi] * D1 + j];
        status[qi] = st;
        if (!st) memset(out + 48 * qi, 0, 48);
    }
    return 0;
}
extern "C" int lcb_g1_eval_poly_batch(uint8_t *out, uint8_t *status, const uint8_t *coeffs, size_t n_coeffs,
                                      const int32_t *xs, size_t n_points) {
    SYNC_CTX_OR(c, -1)
    if (!n_coeffs) { set_err("eval poly: no coefficients"); return -1; }
    if (!n_points) return 0;
    if (n_coeffs > 0xffffffffu || n_points > 0xffffffffu) { set_err("eval poly: batch too large"); return -1; }
    HostCall h(c, "eval poly");
    hipStream_t s = h.s;
    const uint8_t *dco = h.in(coeffs, 48 * n_coeffs);
    const int32_t *dx = h.in(xs, n_points);
    void *aff = h.out<uint8_t>(n_coeffs * LCB_G1A_ST_BYTES), *rows = h.out<uint8_t>(n_coeffs * LCB_G1_JAC_BYTES);
    uint8_t *rok = h.out<uint8_t>(n_coeffs);
    uint32_t *drow = h.out<uint32_t>(n_points);
    uint8_t *dout = h.out<uint8_t>(48 * n_points), *dst = h.out<uint8_t>(n_points);
    if (!h.ok()) return -1;
    hipMemsetAsync(drow, 0, 4 * n_points, s);    // every point evaluates row 0 (the coefficient vector)
    lcbk_g1_decompress(dim3(nblk(n_coeffs)), s, dco, (u32)n_coeffs, aff);
    bool off = false;                            // a coefficient outside G1: negative x multiply by Fr.FromInt(x)
    bool neg = false;
    for (size_t i = 0; i < n_points; i++) neg |= xs[i] < 0;
    if (neg && g1_any_off_subgroup(h, aff, n_coeffs, &off)) return -1;
    lcbk_g1a_to_jac(dim3(nblk(n_coeffs)), s, aff, (u32)n_coeffs, rows, rok);
    lcbk_dkg_horner(dim3(nblk(n_points)), s, rows, rok, (u32)(n_coeffs - 1), drow, dx, (u32)n_points, dout, dst,
                    off ? 1u : 0u);
    h.back(out, dout, 48 * n_points);
    h.back(status, dst, n_points);
    return h.finish();
}
