// Training-mode propagation on gfx950: the dropped + re-normalised adjacency values of one iteration (layered.py:47-50, gnn.py:37-42)
// are produced INSIDE the SpMM kernels from the counter RNG, so a training iteration reads every stored entry's column and raw
// value, gathers only the kept entries' rows, and writes no value array.  Entries: gnx_spmm_dropped, gnx_spmm_dropped_chained (forward
// loop), gnx_spmm_dropped_back (backward loop, over the transposed structure).  The kernels, their launchers and the two loop entries are
// written once over the row-storage policy in gnx_spmm_drop.h; this unit instantiates them for f32 rows, gnx_spmm_train_bf16.hip for bf16
// rows, gnx_spmm_train_ord.hip for f32 rows in the handle's gather order.
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
    p.fuse.thr = drop_threshold(dropout_p);
    p.fuse.scale = drop_scale(dropout_p);
    p.fuse.transposed = transposed;
    p.fuse.col_prescaled = x_prescaled ? 1 : 0;
    p.fuse.row0_key = g->blk_row0_global; p.fuse.row0_D = g->blk_row0_buf; p.fuse.gid = g->blk_col_gid;
}

const char *launch_spmm_dropped(const SpmmArgs &p, int vec, hipStream_t s) { return launch_drop<F32Rows>(p, vec, s); }

// the long rows of a fused-dropout launch whose short rows another translation unit's kernel took (the fused layer units): the chunk kernels of
// launch_drop over the same DropFuse + the reduce
void launch_long_rows_dropped(const SpmmArgs &p, hipStream_t s) {
    with_vec<F32Rows>(F32Rows::vec(p), [&](auto V) {
        if (p.fuse.mult) launch_long_drop<F32Rows, V(), true>(p, s);
        else launch_long_drop<F32Rows, V(), false>(p, s);
    });
}

}  // namespace gnx

extern "C" {

int gnx_spmm_dropped(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int transposed,
                     const float *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0, float beta, float alpha, int act,
                     float *d_out, int64_t ldo, void *stream) {
    int rc = check_dropped_forward<F32Rows>("gnx_spmm_dropped", g, d_X, ldx, C, d_H0, ldh0, d_out, ldo, act, 0, d_D, dropout_p);
    if (rc != GNX_OK) return rc;
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
    set_operands<F32Rows>(p, d_X, ldx, d_H0, ldh0, beta, alpha, act, d_out, 0, ldo, C);
    set_drop_fuse(g, dropout_p, seed, stream_id, d_D, transposed ? 1 : 0, 0, p);
    return launch_spmm(g, transposed ? g->t : g->a, p, s);
}

int gnx_spmm_dropped_chained(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                             const float *d_D_next, const float *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0, float beta,
                             float alpha, int act, float *d_out, int64_t ldo, void *stream) {
    const char *fn = "gnx_spmm_dropped_chained";
    const auto admit = [fn](gnx_graph *g, hipStream_t) -> int {
        GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols || g->blk_col_gid != nullptr, "%s: needs a square graph or a vertex block", fn);
        return refuse_duplicates(g, fn);
    };
    return spmm_dropped_chained<F32Rows>(fn, admit, g, d_D, dropout_p, seed, stream_id, x_prescaled, d_D_next, d_X, ldx, C, d_H0, ldh0, beta,
                                         alpha, act, d_out, 0, ldo, 0, stream);
}

int gnx_spmm_dropped_back(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                          const float *d_D_next, const float *d_X, int64_t ldx, int64_t C, const float *d_S_in, int64_t lds_in,
                          float s_alpha, float s_beta, float *d_S_out, int64_t lds_out, float y_beta, float *d_Y_out, int64_t ldy,
                          int act, void *stream) {
    const char *fn = "gnx_spmm_dropped_back";
    const auto admit = [fn](gnx_graph *g, hipStream_t) -> int {
        GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols && g->blk_col_gid == nullptr, "%s: needs a square stand-alone graph", fn);
        return refuse_duplicates(g, fn);
    };
    return spmm_dropped_back<F32Rows>(fn, admit, g, d_D, dropout_p, seed, stream_id, x_prescaled, d_D_next, d_X, ldx, C, d_S_in, lds_in, s_alpha,
                                      s_beta, d_S_out, lds_out, y_beta, d_Y_out, ldy, act, 0, stream);
}

}  // extern "C"
