// lachain_amd/csrc/lcb_dkg.cpp — host side of the trustless DKG's G1 work (include/lachain_bls.h lcb_dkg_*,
// lcb_g1_eval_poly_batch; kernels: k_dkg.hip).
//
// Commitment.Evaluate(x, y) / Evaluate(x) (src/Lachain.Consensus/ThresholdKeygen/Data/Commitment.cs:23-53) for whole
// batches: rows of every distinct (commitment, x) once, then Horner in y per query.  Each entry point is a synchronous
// call on the calling thread's host-pointer context, in its dkg[0..3], dkg[6..8], in[] and out[] workspaces.
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
int g1_any_off_subgroup(lcb_ctx *c, const void *d_aff, size_t n, hipStream_t s, bool *any) {
    u32 *d = (u32 *)c->dkg[8].get(4);
    if (!d) { set_err("device allocation failed"); return -1; }
    hipMemsetAsync(d, 0, 4, s);
    if (n) lcbk_g1_subgroup_any(s, d_aff, (u32)n, d);
    u32 h = 0;
    if (!launch_ok("subgroup test launch")) return -1;
    if (hipMemcpyAsync(&h, d, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        set_err("batched verify: group count");
        return -1;
    }
    *any = h != 0;
    return 0;
}
// Commitment.Evaluate(x) rows of n_rows (commitment, x) pairs.  Honest commitments (every coefficient in G1): Horner in
// the small x (k_dkg_rows).  A batch with a coefficient outside G1: the reference's own terms [x^j mod r] C (exact).
int dkg_rows_enqueue(lcb_ctx *c, const uint8_t *d_coeffs, size_t n_comm, size_t n_coef, int degree,
                     const uint32_t *d_comm, const int32_t *d_xs, size_t n_rows, hipStream_t s, void **rows_out,
                     uint8_t **rows_ok, bool *exact) {
    size_t total = n_comm * n_coef, lanes = n_rows * (size_t)(degree + 1);
    if (total > 0xffffffffu || lanes > 0xffffffffu) { set_err("dkg: batch too large"); return -1; }
    void *aff = c->dkg[0].get(total * LCB_G1A_ST_BYTES);
    void *rows = c->dkg[1].get(lanes * LCB_G1_JAC_BYTES);
    uint8_t *rok = (uint8_t *)c->dkg[2].get(lanes);
    if (!aff || !rows || !rok) { set_err("device allocation failed"); return -1; }
    if (total) lcbk_g1_decompress(dim3(nblk(total)), s, d_coeffs, (u32)total, aff);
    if (g1_any_off_subgroup(c, aff, total, s, exact)) return -1;
    if (lanes && !*exact) {
        lcbk_dkg_rows(dim3(nblk(lanes)), s, aff, (u32)n_coef, (u32)n_comm, (u32)degree, d_comm, d_xs, (u32)n_rows, rows,
                      rok);
    } else if (lanes) {
        const size_t nt = lanes * (size_t)(degree + 1);
        if (nt > 0xffffffffu) { set_err("dkg: batch too large for the exact form"); return -1; }
        void *terms = c->dkg[6].get(nt * LCB_G1_JAC_BYTES);
        uint8_t *tok = (uint8_t *)c->dkg[7].get(nt);
        if (!terms || !tok) { set_err("device allocation failed"); return -1; }
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
    Enq q(c, c->stream);
    hipStream_t s = c->stream;
    size_t lanes = n_queries * (size_t)(degree + 1);
    const uint8_t *dco = up(c->in[0], coeffs, 48 * n_comm * n_coef, s);
    const uint32_t *dci = up(c->in[1], comm_idx, n_queries, s);
    const int32_t *dx = up(c->in[2], xs, n_queries, s);
    uint8_t *dout = (uint8_t *)c->out[0].get(48 * lanes);
    if (!dco || !dci || !dx || !dout) { set_err("device allocation failed"); return -1; }
    void *rows;
    uint8_t *rok;
    bool exact = false;
    if (dkg_rows_enqueue(c, dco, n_comm, n_coef, degree, dci, dx, n_queries, s, &rows, &rok, &exact)) return -1;
    lcbk_g1_jac_compress(dim3(nblk(lanes)), s, rows, (u32)lanes, dout);
    std::vector<uint8_t> ok(lanes);
    hipMemcpyAsync(rows_out, dout, 48 * lanes, hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(ok.data(), rok, lanes, hipMemcpyDeviceToHost, s);
    if (!sync_check(c, "dkg rows")) return -1;
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
    Enq q(c, c->stream);
    hipStream_t s = c->stream;
    const uint8_t *dco = up(c->in[0], coeffs, 48 * n_comm * n_coef, s);
    const uint32_t *drc = up(c->in[1], row_comm.data(), row_comm.size(), s);
    const int32_t *drx = up(c->in[2], row_x.data(), row_x.size(), s);
    const uint32_t *drow = up(c->in[3], row_of.data(), n_queries, s);
    const int32_t *dy = up(c->in[4], ys, n_queries, s);
    uint8_t *dout = (uint8_t *)c->out[0].get(48 * n_queries), *dst = (uint8_t *)c->out[1].get(n_queries);
    if (!dco || !drc || !drx || !drow || !dy || !dout || !dst) { set_err("device allocation failed"); return -1; }
    void *rows;
    uint8_t *rok;
    bool exact = false;
    if (dkg_rows_enqueue(c, dco, n_comm, n_coef, degree, drc, drx, row_comm.size(), s, &rows, &rok, &exact)) return -1;
    if (!exact) {
        lcbk_dkg_horner(dim3(nblk(n_queries)), s, rows, rok, (u32)degree, drow, dy, (u32)n_queries, dout, dst, 0);
        hipMemcpyAsync(out, dout, 48 * n_queries, hipMemcpyDeviceToHost, s);
        hipMemcpyAsync(status, dst, n_queries, hipMemcpyDeviceToHost, s);
        return sync_check(c, "dkg eval") ? 0 : -1;
    }
    // a coefficient outside G1: sum_j [y^j mod r] row_j(x) (Commitment.cs:23-37 as written)
    const size_t D1 = (size_t)degree + 1, nt = n_queries * D1;
    void *terms = c->dkg[6].get(nt * LCB_G1_JAC_BYTES), *sums = c->dkg[3].get(n_queries * LCB_G1_JAC_BYTES);
    if (!terms || !sums) { set_err("device allocation failed"); return -1; }
    lcbk_dkg_exact_combine(s, rows, (u32)degree, drow, dy, (u32)n_queries, terms);
    lcbk_g1_jac_reduce_groups(dim3(nblk(n_queries)), s, terms, (u32)nt, (u32)D1, sums);
    lcbk_g1_jac_compress(dim3(nblk(n_queries)), s, sums, (u32)n_queries, dout);
    std::vector<uint8_t> rk(row_comm.size() * D1);
    hipMemcpyAsync(out, dout, 48 * n_queries, hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(rk.data(), rok, rk.size(), hipMemcpyDeviceToHost, s);
    if (!sync_check(c, "dkg eval")) return -1;
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
    Enq q(c, c->stream);
    hipStream_t s = c->stream;
    const uint8_t *dco = up(c->in[0], coeffs, 48 * n_coeffs, s);
    const int32_t *dx = up(c->in[1], xs, n_points, s);
    void *aff = c->dkg[0].get(n_coeffs * LCB_G1A_ST_BYTES), *rows = c->dkg[1].get(n_coeffs * LCB_G1_JAC_BYTES);
    uint8_t *rok = (uint8_t *)c->dkg[2].get(n_coeffs);
    uint32_t *drow = (uint32_t *)c->dkg[3].get(4 * n_points);
    uint8_t *dout = (uint8_t *)c->out[0].get(48 * n_points), *dst = (uint8_t *)c->out[1].get(n_points);
    if (!dco || !dx || !aff || !rows || !rok || !drow || !dout || !dst) { set_err("device allocation failed"); return -1; }
    hipMemsetAsync(drow, 0, 4 * n_points, s);    // every point evaluates row 0 (the coefficient vector)
    lcbk_g1_decompress(dim3(nblk(n_coeffs)), s, dco, (u32)n_coeffs, aff);
    bool off = false;                            // a coefficient outside G1: negative x multiply by Fr.FromInt(x)
    bool neg = false;
    for (size_t i = 0; i < n_points; i++) neg |= xs[i] < 0;
    if (neg && g1_any_off_subgroup(c, aff, n_coeffs, s, &off)) return -1;
    lcbk_g1a_to_jac(dim3(nblk(n_coeffs)), s, aff, (u32)n_coeffs, rows, rok);
    lcbk_dkg_horner(dim3(nblk(n_points)), s, rows, rok, (u32)(n_coeffs - 1), drow, dx, (u32)n_points, dout, dst,
                    off ? 1u : 0u);
    hipMemcpyAsync(out, dout, 48 * n_points, hipMemcpyDeviceToHost, s);
    hipMemcpyAsync(status, dst, n_points, hipMemcpyDeviceToHost, s);
    return sync_check(c, "eval poly") ? 0 : -1;
}
