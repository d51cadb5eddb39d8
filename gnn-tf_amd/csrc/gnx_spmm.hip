// The hot path on gfx950: CSR SpMM with the residual mix fused into its epilogue.
//
//   out[i,:] = act( beta * ( sum_j A[i,j] X[j,:] + diag[i] X[i,:] ) + alpha * H0[i,:] )
//
// replaces tf.sparse.sparse_dense_matmul + the three element-wise ops behind it in the
// reference (gnntf/core/gnn/architectures/filter.py:19-22; gcn.py:88).
//
// The kernel is HBM-bound (2 flop per 4 gathered bytes), so the design is about memory
// parallelism and cache behaviour, not MFMA:
//   * wide features (more than 32 lanes of VEC columns, e.g. C = 256): one 64-lane wave per row, each
//     lane owning VEC contiguous columns, so every neighbour row is ONE coalesced wave-instruction
//     (C = 256: 64 x float4 = the whole 1 KiB row).  The row's (col, val) pairs are fetched 64 at a
//     time with one coalesced load and broadcast from registers with v_readlane, and U = 8 neighbour
//     rows are kept in flight per wave before the first FMA;
//   * narrow features: G = 8..32 lanes per row, 64/G rows per wave, rows taken in a degree-binned
//     order (Csr::row_order) so that the rows sharing a wave have similar lengths; for G <= 8 the next
//     (col, val) batch is prefetched behind the gathers;
//   * power-law rows: a row with more than p.long_row entries is cut into p.long_chunk-entry chunks summed
//     by separate waves into a partial slab (wide: lanes across columns; narrow: sub-groups of lanes
//     across the chunk's entries + a fixed xor tree), then added in chunk order by a second kernel
//     (fixed order: results are bitwise reproducible, no float atomics).  Chunks are processed in
//     column-window order (Csr::chunk_order) so the hub rows they share stay in L2 / Infinity Cache.
//
// Every dispatch class is written once, over how a feature row is stored (the row-storage policy of gnx_spmm_device.h), in
// gnx_spmm_eval.h; this unit instantiates them for f32 rows and holds the f32 entry points, gnx_spmm_bf16.hip does the same for bf16.
#include "gnx_spmm_eval.h"

namespace {

// ---- small helpers --------------------------------------------------------------------------------
__global__ void k_gather_vals(const float *__restrict__ vals, const int32_t *__restrict__ perm, int64_t n,
                              float *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = vals[perm[k]];
}

// out[r, :] = X[idx[r], :] for int32 row ids, any width (the relabelled K loop permutes H0 once per call)
__global__ __launch_bounds__(256) void k_gather_rows32(const float *__restrict__ X, int64_t ldx, const int32_t *__restrict__ idx, int64_t n_idx,
                                                        int C, float *__restrict__ out, int64_t ldo) {
    // grid-stride: a launch may not hold more than 2^32 work-items, and n_idx * C can (80M rows x 128 columns)
    const int64_t total = n_idx * C, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / C;
        const int c = (int)(e % C);
        out[r * ldo + c] = X[(int64_t)idx[r] * ldx + c];
    }
}

}  // namespace

namespace gnx {

#ifdef GNX_TUNING
int tune_override = -1;   // set through gnx_debug_set_tune (tuning builds only: make TUNING=1)
#endif

int launch_spmm(gnx_graph *g, const Csr &m, SpmmArgs &p, hipStream_t s) {
    // eval launches of 4 values per lane over the handle's own matrix gather through its hinted columns, where it keeps any
    const int32_t *hint_cols = nullptr;
    if (p.fuse.D == nullptr && F32Rows::vec(p) == 4) {
        const int rc = gather_hints_for(g, m, p.C, s, &hint_cols);
        if (rc != GNX_OK) return rc;
    }
    return launch_bound(g, m, p, s, [&](SpmmArgs &q) {
#ifdef GNX_TUNING   // kernel-variant switches exist only in tuning builds (tools/tune_spmm.py); the product library has none
        static const int tune = [] { const char *e = getenv("GNX_TUNE"); return e ? atoi(e) : 0; }();
        q.tune = tune_override >= 0 ? tune_override : tune;
        if (q.tune & 16384) q.ldx = 0;         // (every gather reads row 0 -- what a launch costs without its gather misses; wrong results)
#endif
        // (tried for C = 128: one wave per row with float2 lanes instead of 32-lane groups of float4 -- 10.9 vs 8.2 ms)
        // a training iteration (q.fuse.D) goes to the kernels of gnx_spmm_train.hip
        if (hint_cols != nullptr) {
            q.colidx = hint_cols;
            g->last_hint_hot = g->hint_hot;
            return launch_eval<F32Rows, true>(q, s);
        }
        return q.fuse.D != nullptr ? launch_spmm_dropped(q, F32Rows::vec(q), s) : launch_eval<F32Rows>(q, s);
    });
}

// the long rows of a launch whose short rows another translation unit's kernel took (the fused layer units): partial sums + reduce
void launch_long_rows(const SpmmArgs &p, hipStream_t s) {
    with_vec<F32Rows>(F32Rows::vec(p), [&](auto V) { launch_long<F32Rows, V()>(p, s); });
}

}  // namespace gnx

extern "C" {

#ifdef GNX_TUNING
// tuning builds only (make TUNING=1), not part of include/gnx.h: lets tools/tune_spmm.py flip kernel variants inside one process
int gnx_debug_set_tune(int t) { tune_override = t; return 0; }
#endif

int gnx_spmm(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_X, int64_t ldx, int64_t C,
             const float *d_H0, int64_t ldh0, float beta, float alpha, int act, float *d_out, int64_t ldo, void *stream) {
    int rc = check_common("gnx_spmm", g, d_X, ldx, C, d_H0, ldh0, d_out, ldo);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG((act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_NONE || (act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_RELU, "gnx_spmm: invalid activation %d", act);
    GNX_CHECK_ARG(d_diag == nullptr || g->a.n_rows == g->a.n_cols, "gnx_spmm: diag needs a square graph");
    SpmmArgs p{};
    p.vals = d_vals ? d_vals : g->raw_vals;
    p.diag = d_diag;
    set_operands<F32Rows>(p, d_X, ldx, d_H0, ldh0, beta, alpha, act, d_out, 0, ldo, C);
    return launch_spmm(g, g->a, p, (hipStream_t)stream);
}

int gnx_spmm_t(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_X, int64_t ldx, int64_t C,
               const float *d_H0, int64_t ldh0, float beta, float alpha, int act, float *d_out, int64_t ldo, void *stream) {
    int rc = check_common("gnx_spmm_t", g, d_X, ldx, C, d_H0, ldh0, d_out, ldo);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "gnx_spmm_t: invalid activation %d", act);
    GNX_CHECK_ARG(d_diag == nullptr || g->a.n_rows == g->a.n_cols, "gnx_spmm_t: diag needs a square graph");
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_transpose(g, s);
    if (rc != GNX_OK) return rc;
    const float *src = d_vals ? d_vals : g->raw_vals;
    if (g->a.nnz > 0)
        hipLaunchKernelGGL(k_gather_vals, dim3(blocks_for(g->a.nnz, 256)), dim3(256), 0, s, src, g->t_perm, g->a.nnz, g->t_vals);
    SpmmArgs p{};
    p.vals = g->t_vals;
    p.diag = d_diag;
    set_operands<F32Rows>(p, d_X, ldx, d_H0, ldh0, beta, alpha, act, d_out, 0, ldo, C);
    return launch_spmm(g, g->t, p, s);
}

int gnx_spmm_scatter(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_X, int64_t ldx, int64_t C,
                     const float *d_H0, int64_t ldh0, float beta, float alpha, int act, const int32_t *d_out_rows,
                     float *d_out, int64_t ldo, void *stream) {
    int rc = check_common("gnx_spmm_scatter", g, d_X, ldx, C, d_H0, ldh0, d_out, ldo);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "gnx_spmm_scatter: invalid activation %d", act);
    GNX_CHECK_ARG(d_diag == nullptr || g->a.n_rows == g->a.n_cols, "gnx_spmm_scatter: diag needs a square graph");
    SpmmArgs p{};
    p.vals = d_vals ? d_vals : g->raw_vals;
    p.diag = d_diag; p.out_rows = d_out_rows;
    set_operands<F32Rows>(p, d_X, ldx, d_H0, ldh0, beta, alpha, act, d_out, 0, ldo, C);
    return launch_spmm(g, g->a, p, (hipStream_t)stream);
}

int gnx_spmm_rows(gnx_graph_t g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0,
                  float beta, float alpha, int act, const int32_t *d_rows, float *d_out, int64_t ldo, void *stream) {
    int rc = check_common("gnx_spmm_rows", g, d_X, ldx, C, d_H0, ldh0, d_out, ldo);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG((act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_NONE || (act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_RELU, "gnx_spmm_rows: invalid activation %d", act);
    GNX_CHECK_ARG(d_rows != nullptr || g->a.n_rows == 0, "gnx_spmm_rows: NULL row map");
    SpmmArgs p{};
    p.vals = d_vals ? d_vals : g->raw_vals;
    p.out_rows = d_rows; p.map_h0 = true;
    set_operands<F32Rows>(p, d_X, ldx, d_H0, ldh0, beta, alpha, act, d_out, 0, ldo, C);
    return launch_spmm(g, g->a, p, (hipStream_t)stream);
}

int gnx_graph_permute_values_t(gnx_graph_t g, const float *d_vals, float *d_vals_t_out, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_permute_values_t: NULL handle");
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_transpose(g, s);
    if (rc != GNX_OK) return rc;
    if (g->a.nnz == 0) return GNX_OK;
    GNX_CHECK_ARG(d_vals_t_out != nullptr, "gnx_graph_permute_values_t: NULL output");
    hipLaunchKernelGGL(k_gather_vals, dim3(blocks_for(g->a.nnz, 256)), dim3(256), 0, s, d_vals ? d_vals : g->raw_vals, g->t_perm,
                       g->a.nnz, d_vals_t_out);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_spmm_tv(gnx_graph_t g, const float *d_vals_t, const float *d_diag, const float *d_X, int64_t ldx, int64_t C,
                const float *d_H0, int64_t ldh0, float beta, float alpha, int act, float *d_out, int64_t ldo, void *stream) {
    int rc = check_common("gnx_spmm_tv", g, d_X, ldx, C, d_H0, ldh0, d_out, ldo);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "gnx_spmm_tv: invalid activation %d", act);
    GNX_CHECK_ARG(d_diag == nullptr || g->a.n_rows == g->a.n_cols, "gnx_spmm_tv: diag needs a square graph");
    GNX_CHECK_ARG(g->a.nnz == 0 || d_vals_t != nullptr, "gnx_spmm_tv: NULL values");
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_transpose(g, s);
    if (rc != GNX_OK) return rc;
    SpmmArgs p{};
    p.vals = d_vals_t;
    p.diag = d_diag;
    set_operands<F32Rows>(p, d_X, ldx, d_H0, ldh0, beta, alpha, act, d_out, 0, ldo, C);
    return launch_spmm(g, g->t, p, s);
}

int gnx_ppr_step(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_H, const float *d_H0, float a,
                 int64_t C, int act, float *d_out, void *stream) {
    GNX_CHECK_ARG(d_H0 != nullptr, "gnx_ppr_step: NULL H0");
    return gnx_spmm(g, d_vals, d_diag, d_H, C, C, d_H0, C, (float)(1.0 - (double)a), a, act, d_out, C, stream);
}

int gnx_appnp_propagate(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_H0, float a, int K,
                        int64_t C, float *d_out, float *d_work, void *stream) {
    return gnx_appnp_propagate_act(g, d_vals, d_diag, d_H0, a, K, C, GNX_ACT_NONE, d_out, d_work, stream);
}

int gnx_appnp_propagate_act(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_H0, float a, int K,
                            int64_t C, int act, float *d_out, float *d_work, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_appnp_propagate: NULL handle");
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "gnx_appnp_propagate: invalid activation %d", act);
    GNX_CHECK_ARG(K >= 0, "gnx_appnp_propagate: negative iteration count");
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "gnx_appnp_propagate: needs a square graph");
    GNX_CHECK_ARG(d_H0 && d_out && (K < 2 || d_work), "gnx_appnp_propagate: NULL buffer");
    GNX_CHECK_ARG(d_out != d_H0 && d_work != d_H0 && d_out != d_work, "gnx_appnp_propagate: H0, out and work must be distinct");
    g->last_pend = false;
    if (K == 0) {
        GNX_HIP(hipMemcpyAsync(d_out, d_H0, (size_t)g->a.n_rows * C * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return GNX_OK;
    }
    const int64_t n = g->a.n_rows;
    hipStream_t s = (hipStream_t)stream;
    // Narrow features on a large graph: every gather moves a whole 128-byte line for a 16..64-byte row, so what counts is how
    // often a line is found in cache.  The K iterations then run on the degree-relabelled copy of the matrix (hub rows adjacent:
    // four to eight of the rows that receive most gathers share a line): H0 is permuted once on the way in, the LAST iteration
    // scatters its rows straight back into the caller's order.  -16..-21 % per iteration at C = 16 / 8 (RMAT 10M / 100M); the
    // sums run over a row's columns in the relabelled order, so results agree with the plain path to float32 rounding.
    if (C <= RELABEL_MAX_C && n >= (1 << 20) && g->a.nnz >= n && d_diag == nullptr && g->a.order_window == 0) {
        int rc = ensure_relabel(g, s);
        if (rc != GNX_OK) return rc;
        rc = ensure_relabel_features(g, (size_t)n * C * sizeof(float), s);
        if (rc != GNX_OK) return rc;
        hipLaunchKernelGGL(k_gather_vals, dim3(blocks_for(g->a.nnz, 256)), dim3(256), 0, s, d_vals ? d_vals : g->raw_vals, g->r_perm, g->a.nnz,
                           g->r_vals);
        GNX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_gather_rows32, dim3((unsigned)std::min<int64_t>(blocks_for(n * C, 256), 1 << 22)), dim3(256), 0, s, d_H0, C,
                           g->go_order, n, (int)C, g->r_feat, C);
        GNX_HIP(hipGetLastError());
        const float *src = g->r_feat;
        for (int k = 0; k < K; ++k) {
            const bool last = k == K - 1;
            float *dst = last ? d_out : (((K - 2 - k) % 2 == 0) ? d_work : d_out);
            SpmmArgs p{};
            p.vals = g->r_vals;
            // rows without entries: written by the last iteration (it scatters every row); in between only if somebody gathers them
            // (with a relu such a row is relu(a * H0) after every iteration: just as constant)
            const int act_k = (!last && (k >= 2 || g->r.empty_rows_unreferenced)) ? (act | GNX_ACT_SKIP_EMPTY) : act;
            set_operands<F32Rows>(p, src, C, g->r_feat, C, (float)(1.0 - (double)a), a, act_k, dst, 0, C, C);
            p.out_rows = last ? g->go_order : nullptr;              // relabelled row i is the caller's row go_order[i]
            rc = launch_spmm(g, g->r, p, s);
            if (rc != GNX_OK) return rc;
            src = dst;
        }
        return GNX_OK;
    }
    // A row without entries is act(a * H0) after every iteration and nobody's sum depends on when it was written: such rows are
    // computed the first time each of the two buffers is a destination (k = 0, 1) and left alone afterwards (GNX_ACT_SKIP_EMPTY)
    // -- on the R-MAT workloads 60 % of the rows, 7-10 % of an iteration's bytes.  Same arithmetic, same bits.
    // Pendant rows (gnx_graph_set_pendant_elision): an elidable row's iterates between H0 and the result have one reader, its
    // neighbour, which forms them itself (gnx_spmm_eval.h, PEND): the row is computed by the last iteration only, and no buffer
    // receives it, or is read at it, before.  Where the launches take hints, at 4 values per lane on 16 or 32 lanes.
    const int32_t *pend_cols = nullptr;
    if (K >= 2 && d_diag == nullptr && C <= 128) {
        SpmmArgs probe{};
        set_operands<F32Rows>(probe, d_H0, C, d_H0, C, 0.f, 0.f, act, d_out, 0, C, C);
        const int32_t *hint_cols = nullptr;
        if (F32Rows::vec(probe) == 4 && aligned(d_work, 16)) {
            int rc = gather_hints_for(g, g->a, C, s, &hint_cols);
            if (rc == GNX_OK && hint_cols != nullptr) rc = pendant_plan_for(g, C, s, &pend_cols);
            if (rc != GNX_OK) return rc;
        }
    }
    if (pend_cols != nullptr) {
        const float *vals = d_vals ? d_vals : g->raw_vals.get();
        int rc = pendant_weights(g, vals, s);
        if (rc != GNX_OK) return rc;
        const float *src = d_H0;
        for (int k = 0; k < K; ++k) {
            float *dst = ((K - 1 - k) % 2 == 0) ? d_out : d_work;
            const bool settled = k >= 2 || (g->a.empty_rows_unreferenced && dst == d_work);     // (as below)
            PendArgs p{};
            p.vals = vals;
            set_operands<F32Rows>(p, src, C, d_H0, C, (float)(1.0 - (double)a), a, settled ? (act | GNX_ACT_SKIP_EMPTY) : act, dst, 0, C, C);
            p.P = k == 1 ? d_H0 : dst;      // iterate k - 1 of every row: H0 itself, or what iteration k - 2 left in this destination
            p.ldp = C;
            p.pend_raw = k == 0;
            p.pend_w = g->pend_w; p.pend_slot_mark = g->pend_slot_mark; p.pend_row_mark = g->pend_row_mark;
            if (k < K - 1) { p.skip_beg = g->pend_slot0; p.skip_end = g->pend_slot0 + g->n_pend; }
            rc = launch_bound(g, g->a, p, s, [&](PendArgs &q) {
                q.colidx = pend_cols;
                g->last_hint_hot = g->hint_hot;
                return launch_eval_pend(q, s);
            });
            if (rc != GNX_OK) return rc;
            src = dst;
        }
        g->last_pend = true;
        return GNX_OK;
    }
    const float *src = d_H0;
    for (int k = 0; k < K; ++k) {
        float *dst = ((K - 1 - k) % 2 == 0) ? d_out : d_work;
        // ... and when no entry points at such a row (g->a.empty_rows_unreferenced: every symmetric pattern) nobody ever gathers it: the
        // work buffer never needs it, the result buffer gets it the first time it is a destination
        const bool settled = k >= 2 || (g->a.empty_rows_unreferenced && dst == d_work);
        const int act_k = (settled && d_diag == nullptr) ? (act | GNX_ACT_SKIP_EMPTY) : act;
        int rc = gnx_spmm(g, d_vals, d_diag, src, C, C, d_H0, C, (float)(1.0 - (double)a), a, act_k, dst, C, stream);
        if (rc != GNX_OK) return rc;
        src = dst;
    }
    return GNX_OK;
}

}  // extern "C"
