// Opt-in bf16 feature storage for the fused training propagation: the chained forward and backward loops of gnx_spmm_train.hip with
// the GATHERED operand stored as bf16 (gnx_spmm_dropped_chained_bf16, gnx_spmm_dropped_back_bf16).
//
// What is bf16: the rows a launch gathers (X) and the rows it hands to the next launch of the loop (the forward's pre-scaled
// iterate, the backward's pre-scaled gradient).  A gathered row is widened exactly to f32 as it arrives.  Every weight (the counter
// RNG, the kept sums, the degree scales: dropped_weight_at of gnx_internal.h, unchanged), every sum, H0, the mix, the running
// gradient sum and both results of a step are f32.  A row that leaves as bf16 is rounded ONCE, after its scale:
// bf(H[i] * D_next[i]) forward, bf(y_beta * acc[r] * D_next[r]) backward (round to nearest even, NaN stays NaN).
//
// Dispatch classes, row orders and summation orders are those of gnx_spmm_train.hip -- one wave per row above 32 lanes, 32/16/8-lane
// groups below, long rows cut into chunks whose f32 partial sums a second kernel adds in chunk order (no float atomics: two calls
// give the same bits) -- with up to 8 bf16 (16 bytes) per lane, so C = 128 runs on 16-lane groups.  Dropped entries (weight exactly
// 0) are not gathered.  The kernels are those of gnx_spmm_drop.h, instantiated here over Bf16RowsT (gnx_spmm_device.h); the f32 kernels'
// U / PIPE variants do not exist for bf16 rows.
#include "gnx_spmm_drop.h"

namespace {

using Bf16Rows = Bf16RowsT<true>;

int launch_bf_drop(gnx_graph *g, const Csr &m, BfArgs &p, hipStream_t s) {
    int rc = bind_csr(g, m, p, s);
    if (rc != GNX_OK) return rc;
    if (m.n_rows == 0) return GNX_OK;
    // the f32 training names with "_bf16" appended, "+long" after the row class when hub rows went through the chunk kernels
    g->last_kernel = launch_drop<Bf16Rows>(p, Bf16Rows::vec(p), s);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

// the checks of both entries that need a handle: square stand-alone graphs, duplicates only with their entry tables
int check_handle(const char *fn, gnx_graph *g) {
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    if (g->blk_col_gid != nullptr) {
        set_error("%s: the handle is a vertex block (gnx_graph_set_block): bf16 training storage covers stand-alone graphs only -- "
                  "use the f32 entry", fn);
        return GNX_ERR_UNSUPPORTED;
    }
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "%s: needs a square stand-alone graph", fn);
    return refuse_duplicates(g, fn);
}

}  // namespace

extern "C" {

int gnx_spmm_dropped_chained_bf16(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                                  const float *d_D_next, const uint16_t *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0,
                                  float beta, float alpha, int act, void *d_out, int out_bf16, int64_t ldo, void *stream) {
    const char *fn = "gnx_spmm_dropped_chained_bf16";
    // the checks that need no handle come first (so that they can be exercised without a device)
    int rc = check_operands(fn, d_X, ldx, C, d_H0, ldh0, d_out, ldo);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1, "%s: out_bf16 must be 0 or 1", fn);
    GNX_CHECK_ARG((act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_NONE || (act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_RELU, "%s: invalid activation %d", fn, act);
    GNX_CHECK_ARG(d_D != nullptr, "%s: NULL degree scales", fn);
    GNX_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout rate %g outside [0, 1)", fn, (double)dropout_p);
    rc = check_handle(fn, g);
    if (rc != GNX_OK) return rc;
    if (!g->a.empty_rows_unreferenced) act &= ~GNX_ACT_SKIP_EMPTY;       // honoured only when nobody gathers the rows it would leave untouched
    BfArgs p{};
    set_values(g, false, p);
    p.Xb = d_X; p.ldx = ldx; p.H0 = d_H0; p.ldh0 = ldh0; p.beta = beta; p.alpha = alpha; p.act = act;
    p.outv = d_out; p.out_bf16 = out_bf16; p.ldo = ldo; p.C = (int)C;
    p.out_scale = d_D_next;
    set_drop_fuse(g, dropout_p, seed, stream_id, d_D, 0, x_prescaled, p);
    return launch_bf_drop(g, g->a, p, (hipStream_t)stream);
}

int gnx_spmm_dropped_back_bf16(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                               const float *d_D_next, const uint16_t *d_X, int64_t ldx, int64_t C, const float *d_S_in, int64_t lds_in,
                               float s_alpha, float s_beta, float *d_S_out, int64_t lds_out, float y_beta, uint16_t *d_Y_out, int64_t ldy,
                               int act, void *stream) {
    const char *fn = "gnx_spmm_dropped_back_bf16";
    int rc = check_operands(fn, d_X, ldx, C, d_S_in, lds_in, d_S_out, lds_out);   // (before the handle, as above)
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_SKIP_EMPTY, "%s: act must be GNX_ACT_NONE or GNX_ACT_SKIP_EMPTY", fn);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || (const void *)d_S_in == (const void *)d_S_out, "%s: GNX_ACT_SKIP_EMPTY needs the sum updated in place", fn);
    GNX_CHECK_ARG(d_D != nullptr && d_S_in != nullptr, "%s: NULL degree scales / running sum", fn);
    GNX_CHECK_ARG(d_Y_out == nullptr || (ldy >= C && (const void *)d_Y_out != (const void *)d_X && (const void *)d_Y_out != (const void *)d_S_out
                                         && (const void *)d_Y_out != (const void *)d_S_in),
                  "%s: the pre-scaled output needs a buffer of its own", fn);
    GNX_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout rate %g outside [0, 1)", fn, (double)dropout_p);
    rc = check_handle(fn, g);
    if (rc != GNX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_transpose(g, s);
    if (rc != GNX_OK) return rc;
    if (!g->t.empty_rows_unreferenced) act = GNX_ACT_NONE;               // honoured only when nobody gathers the rows it would leave untouched
    BfArgs p{};
    set_values(g, true, p);
    p.Xb = d_X; p.ldx = ldx; p.H0 = d_S_in; p.ldh0 = lds_in; p.beta = s_beta; p.alpha = s_alpha; p.act = act;
    p.outv = d_S_out; p.out_bf16 = 0; p.ldo = lds_out; p.C = (int)C;
    p.out2b = d_Y_out; p.ldo2 = ldy; p.beta2 = y_beta; p.out2_scale = d_Y_out ? d_D_next : nullptr;
    set_drop_fuse(g, dropout_p, seed, stream_id, d_D, 1, x_prescaled, p);
    return launch_bf_drop(g, g->t, p, s);
}

}  // extern "C"
