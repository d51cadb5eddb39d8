// The fused training launches over a handle's GATHER ORDER (gnx_spmm_dropped_chained_ord, gnx_spmm_dropped_back_ord): rows, per-row
// entry order, masks, weights and sums stay the caller's; only the matrix that is gathered (and the one the next launch gathers) is
// stored with the vertices in the order the relabelled copy numbers them in -- hub rows share 128-byte lines, a hub's leaves sit in
// consecutive lines -- and is reached through a second column array (gnx_graph::a_gcol / t_gcol, 4 bytes per entry).  Per row the
// same fused multiply-adds on the same values in the same order as gnx_spmm_dropped_chained / gnx_spmm_dropped_back: the same bits.
// The kernels are those of gnx_spmm_drop.h under the F32RowsOrd policy; f32 rows, handles without duplicate entries only.
#include "gnx_spmm_drop.h"

namespace {

int launch_spmm_ord(gnx_graph *g, const Csr &m, OrdArgs &p, hipStream_t s) {
    int rc = bind_csr(g, m, p, s);
    if (rc != GNX_OK) return rc;
    if (m.n_rows == 0) return GNX_OK;
    g->last_kernel = launch_drop<F32RowsOrd>(p, F32RowsOrd::vec(p), s);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

}  // namespace

extern "C" {

int gnx_spmm_dropped_chained_ord(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                                 const float *d_D_next, const float *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0,
                                 float beta, float alpha, int act, float *d_out, int64_t ldo, int order, void *stream) {
    if (order == 0)
        return gnx_spmm_dropped_chained(g, d_D, dropout_p, seed, stream_id, x_prescaled, d_D_next, d_X, ldx, C, d_H0, ldh0, beta, alpha, act,
                                        d_out, ldo, stream);
    int rc = check_common("gnx_spmm_dropped_chained_ord", g, d_X, ldx, C, d_H0, ldh0, d_out, ldo);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG((order & ~(GNX_ORD_X | GNX_ORD_OUT)) == 0, "gnx_spmm_dropped_chained_ord: invalid order flags %d", order);
    GNX_CHECK_ARG((act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_NONE || (act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_RELU,
                  "gnx_spmm_dropped_chained_ord: invalid activation %d", act);
    GNX_CHECK_ARG(d_D != nullptr, "gnx_spmm_dropped_chained_ord: NULL degree scales");
    GNX_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "dropout rate %g outside [0, 1)", (double)dropout_p);
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_train_gather(g, "gnx_spmm_dropped_chained_ord", s);
    if (rc != GNX_OK) return rc;
    if (!g->a.empty_rows_unreferenced) act &= ~GNX_ACT_SKIP_EMPTY;       // as gnx_spmm_dropped_chained
    OrdArgs p{};
    set_values(g, false, p);
    p.X = d_X; p.ldx = ldx; p.H0 = d_H0; p.ldh0 = ldh0; p.beta = beta; p.alpha = alpha; p.act = act;
    p.out = d_out; p.ldo = ldo; p.C = (int)C;
    p.out_scale = d_D_next;
    p.gcol = (order & GNX_ORD_X) ? g->a_gcol : nullptr;
    p.out_rows = (order & GNX_ORD_OUT) ? g->go_rank : nullptr;           // H0 and the scales stay indexed by the caller's row (map_h0 false)
    set_drop_fuse(g, dropout_p, seed, stream_id, d_D, 0, x_prescaled, p);
    return launch_spmm_ord(g, g->a, p, s);
}

int gnx_spmm_dropped_back_ord(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                              const float *d_D_next, const float *d_X, int64_t ldx, int64_t C, const float *d_S_in, int64_t lds_in,
                              float s_alpha, float s_beta, float *d_S_out, int64_t lds_out, float y_beta, float *d_Y_out, int64_t ldy,
                              int act, int order, void *stream) {
    if (order == 0)
        return gnx_spmm_dropped_back(g, d_D, dropout_p, seed, stream_id, x_prescaled, d_D_next, d_X, ldx, C, d_S_in, lds_in, s_alpha, s_beta,
                                     d_S_out, lds_out, y_beta, d_Y_out, ldy, act, stream);
    int rc = check_common("gnx_spmm_dropped_back_ord", g, d_X, ldx, C, d_S_in, lds_in, d_S_out, lds_out);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG((order & ~(GNX_ORD_X | GNX_ORD_OUT)) == 0, "gnx_spmm_dropped_back_ord: invalid order flags %d", order);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_SKIP_EMPTY, "gnx_spmm_dropped_back_ord: act must be GNX_ACT_NONE or GNX_ACT_SKIP_EMPTY");
    GNX_CHECK_ARG(act == GNX_ACT_NONE || (const void *)d_S_in == (const void *)d_S_out,
                  "gnx_spmm_dropped_back_ord: GNX_ACT_SKIP_EMPTY needs the sum updated in place");
    GNX_CHECK_ARG(d_D != nullptr && d_S_in != nullptr, "gnx_spmm_dropped_back_ord: NULL degree scales / running sum");
    GNX_CHECK_ARG(d_Y_out == nullptr || (ldy >= C && (const void *)d_Y_out != (const void *)d_X && (const void *)d_Y_out != (const void *)d_S_out
                                         && (const void *)d_Y_out != (const void *)d_S_in),
                  "gnx_spmm_dropped_back_ord: the pre-scaled output needs a buffer of its own");
    GNX_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "dropout rate %g outside [0, 1)", (double)dropout_p);
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_train_gather(g, "gnx_spmm_dropped_back_ord", s);
    if (rc != GNX_OK) return rc;
    if (!g->t.empty_rows_unreferenced) act = GNX_ACT_NONE;               // as gnx_spmm_dropped_back
    OrdArgs p{};
    set_values(g, true, p);
    p.X = d_X; p.ldx = ldx; p.H0 = d_S_in; p.ldh0 = lds_in; p.beta = s_beta; p.alpha = s_alpha; p.act = act;
    p.out = d_S_out; p.ldo = lds_out; p.C = (int)C;                       // the running sum stays in the caller's order
    p.out2 = d_Y_out; p.ldo2 = ldy; p.beta2 = y_beta; p.out2_scale = d_Y_out ? d_D_next : nullptr;
    p.gcol = (order & GNX_ORD_X) ? g->t_gcol : nullptr;
    p.out2_rows = (d_Y_out && (order & GNX_ORD_OUT)) ? g->go_rank : nullptr;
    set_drop_fuse(g, dropout_p, seed, stream_id, d_D, 1, x_prescaled, p);
    return launch_spmm_ord(g, g->t, p, s);
}

}  // extern "C"
