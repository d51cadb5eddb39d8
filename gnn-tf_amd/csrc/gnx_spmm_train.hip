// Training-mode propagation on gfx950: the dropped + re-normalised adjacency values of one iteration (layered.py:47-50, gnn.py:37-42)
// are produced INSIDE the SpMM kernels from the counter RNG, so a training iteration reads every stored entry's column and raw
// value, gathers only the kept entries' rows, and writes no value array.  Entries: gnx_spmm_dropped, gnx_spmm_dropped_chained (forward
// loop), gnx_spmm_dropped_back (backward loop, over the transposed structure).  The kernels and their launchers are written once over the
// row-storage policy in gnx_spmm_drop.h; this unit instantiates them for f32 rows, gnx_spmm_train_bf16.hip for bf16 rows.
#include "gnx_spmm_drop.h"

namespace gnx {

// per-entry dropout of duplicated COO entries needs the tables gnx_graph_enable_entry_dropout builds
int refuse_duplicates(const gnx_graph *g, const char *fn) {
    if (!g->has_dups || g->entry_drop) return GNX_OK;
    set_error("%s: the graph holds duplicate COO entries: call gnx_graph_enable_entry_dropout on the handle first (or use "
              "gnx_graph_normalize + gnx_spmm)", fn);
    return GNX_ERR_UNSUPPORTED;
}

// what a fused launch over handle g reads as its per-slot values (after ensure_transpose when `transposed`), and the entry tables
// of a handle with duplicates
void set_values(const gnx_graph *g, bool transposed, SpmmArgs &p) {
    if (!g->has_dups) {
        p.vals = transposed ? g->t_raw : g->raw_vals;
        return;
    }
    p.vals = transposed ? g->t_ed_vals : g->ed_vals;
    p.fuse.mult = transposed ? g->t_ed_mult : g->ed_mult;
    p.fuse.e_vals = g->e_vals;
    p.fuse.slot_ptr = g->slot_ptr;
    p.fuse.perm = transposed ? g->t_perm : nullptr;
}

// the counter-RNG part of a fused launch over a stand-alone handle or a vertex block: keep threshold, kept-value scale, stream, block keys
void set_drop_fuse(const gnx_graph *g, float dropout_p, uint64_t seed, uint64_t stream_id, const float *d_D, int transposed,
                   int x_prescaled, SpmmArgs &p) {
    p.fuse.D = d_D; p.fuse.seed = seed; p.fuse.stream = stream_id; p.fuse.offset = g->stream_offset;
    p.fuse.thr = (uint32_t)((double)dropout_p * 16777216.0);
    p.fuse.scale = 1.0f / (1.0f - dropout_p);
    p.fuse.transposed = transposed;
    p.fuse.col_prescaled = x_prescaled ? 1 : 0;
    p.fuse.row0_key = g->blk_row0_global; p.fuse.row0_D = g->blk_row0_buf; p.fuse.gid = g->blk_col_gid;
}

const char *launch_spmm_dropped(const SpmmArgs &p, int vec, hipStream_t s) { return launch_drop<F32Rows>(p, vec, s); }

}  // namespace gnx

extern "C" {

int gnx_spmm_dropped(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int transposed,
                     const float *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0, float beta, float alpha, int act,
                     float *d_out, int64_t ldo, void *stream) {
    int rc = check_common("gnx_spmm_dropped", g, d_X, ldx, C, d_H0, ldh0, d_out, ldo);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "gnx_spmm_dropped: invalid activation %d", act);
    GNX_CHECK_ARG(d_D != nullptr, "gnx_spmm_dropped: NULL degree scales");
    GNX_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "dropout rate %g outside [0, 1)", (double)dropout_p);
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols || g->blk_col_gid != nullptr, "gnx_spmm_dropped: needs a square graph or a vertex block (gnx_graph_set_block)");
    rc = refuse_duplicates(g, "gnx_spmm_dropped");
    if (rc != GNX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (transposed) {
        rc = ensure_transpose(g, s);
        if (rc != GNX_OK) return rc;
    }
    SpmmArgs p{};
    set_values(g, transposed, p);
    p.X = d_X; p.ldx = ldx; p.H0 = d_H0; p.ldh0 = ldh0; p.beta = beta; p.alpha = alpha; p.act = act;
    p.out = d_out; p.ldo = ldo; p.C = (int)C;
    set_drop_fuse(g, dropout_p, seed, stream_id, d_D, transposed ? 1 : 0, 0, p);
    return launch_spmm(g, transposed ? g->t : g->a, p, s);
}

int gnx_spmm_dropped_chained(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                             const float *d_D_next, const float *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0, float beta,
                             float alpha, int act, float *d_out, int64_t ldo, void *stream) {
    int rc = check_common("gnx_spmm_dropped_chained", g, d_X, ldx, C, d_H0, ldh0, d_out, ldo);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG((act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_NONE || (act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_RELU,
                  "gnx_spmm_dropped_chained: invalid activation %d", act);
    if (!g->a.empty_rows_unreferenced) act &= ~GNX_ACT_SKIP_EMPTY;       // honoured only when nobody gathers the rows it would leave untouched
    GNX_CHECK_ARG(d_D != nullptr, "gnx_spmm_dropped_chained: NULL degree scales");
    GNX_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "dropout rate %g outside [0, 1)", (double)dropout_p);
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols || g->blk_col_gid != nullptr, "gnx_spmm_dropped_chained: needs a square graph or a vertex block");
    rc = refuse_duplicates(g, "gnx_spmm_dropped_chained");
    if (rc != GNX_OK) return rc;
    SpmmArgs p{};
    set_values(g, false, p);
    p.X = d_X; p.ldx = ldx; p.H0 = d_H0; p.ldh0 = ldh0; p.beta = beta; p.alpha = alpha; p.act = act;
    p.out = d_out; p.ldo = ldo; p.C = (int)C;
    p.out_scale = d_D_next ? d_D_next + g->blk_row0_buf : nullptr;
    set_drop_fuse(g, dropout_p, seed, stream_id, d_D, 0, x_prescaled, p);
    return launch_spmm(g, g->a, p, (hipStream_t)stream);
}

int gnx_spmm_dropped_back(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                          const float *d_D_next, const float *d_X, int64_t ldx, int64_t C, const float *d_S_in, int64_t lds_in,
                          float s_alpha, float s_beta, float *d_S_out, int64_t lds_out, float y_beta, float *d_Y_out, int64_t ldy,
                          int act, void *stream) {
    int rc = check_common("gnx_spmm_dropped_back", g, d_X, ldx, C, d_S_in, lds_in, d_S_out, lds_out);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_SKIP_EMPTY, "gnx_spmm_dropped_back: act must be GNX_ACT_NONE or GNX_ACT_SKIP_EMPTY");
    GNX_CHECK_ARG(act == GNX_ACT_NONE || (const void *)d_S_in == (const void *)d_S_out,
                  "gnx_spmm_dropped_back: GNX_ACT_SKIP_EMPTY needs the sum updated in place");
    GNX_CHECK_ARG(d_D != nullptr && d_S_in != nullptr, "gnx_spmm_dropped_back: NULL degree scales / running sum");
    GNX_CHECK_ARG(d_Y_out == nullptr || (ldy >= C && (const void *)d_Y_out != (const void *)d_X && (const void *)d_Y_out != (const void *)d_S_out
                                         && (const void *)d_Y_out != (const void *)d_S_in),
                  "gnx_spmm_dropped_back: the pre-scaled output needs a buffer of its own");
    GNX_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "dropout rate %g outside [0, 1)", (double)dropout_p);
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols && g->blk_col_gid == nullptr, "gnx_spmm_dropped_back: needs a square stand-alone graph");
    rc = refuse_duplicates(g, "gnx_spmm_dropped_back");
    if (rc != GNX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_transpose(g, s);
    if (rc != GNX_OK) return rc;
    if (!g->t.empty_rows_unreferenced) act = GNX_ACT_NONE;               // honoured only when nobody gathers the rows it would leave untouched
    SpmmArgs p{};
    set_values(g, true, p);
    p.X = d_X; p.ldx = ldx; p.H0 = d_S_in; p.ldh0 = lds_in; p.beta = s_beta; p.alpha = s_alpha; p.act = act;
    p.out = d_S_out; p.ldo = lds_out; p.C = (int)C;
    p.out2 = d_Y_out; p.ldo2 = ldy; p.beta2 = y_beta; p.out2_scale = d_Y_out ? d_D_next : nullptr;
    set_drop_fuse(g, dropout_p, seed, stream_id, d_D, 1, x_prescaled, p);   // (stand-alone handle: the block keys are 0 / null)
    return launch_spmm(g, g->t, p, s);
}

}  // extern "C"
