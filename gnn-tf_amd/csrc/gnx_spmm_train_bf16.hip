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

// the checks of both entries that need a handle (behind the handle-free ones): square stand-alone graphs, duplicates only with their
// entry tables
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

// (the reported names are the f32 training names with "_bf16" appended, "+long" after the row class when hub rows went through the
// chunk kernels)
int gnx_spmm_dropped_chained_bf16(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                                  const float *d_D_next, const uint16_t *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0,
                                  float beta, float alpha, int act, void *d_out, int out_bf16, int64_t ldo, void *stream) {
    const char *fn = "gnx_spmm_dropped_chained_bf16";
    const auto admit = [fn](gnx_graph *g, hipStream_t) { return check_handle(fn, g); };
    return spmm_dropped_chained<Bf16Rows>(fn, admit, g, d_D, dropout_p, seed, stream_id, x_prescaled, d_D_next, d_X, ldx, C, d_H0, ldh0, beta,
                                          alpha, act, d_out, out_bf16, ldo, 0, stream);
}

int gnx_spmm_dropped_back_bf16(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                               const float *d_D_next, const uint16_t *d_X, int64_t ldx, int64_t C, const float *d_S_in, int64_t lds_in,
                               float s_alpha, float s_beta, float *d_S_out, int64_t lds_out, float y_beta, uint16_t *d_Y_out, int64_t ldy,
                               int act, void *stream) {
    const char *fn = "gnx_spmm_dropped_back_bf16";
    const auto admit = [fn](gnx_graph *g, hipStream_t) { return check_handle(fn, g); };
    return spmm_dropped_back<Bf16Rows>(fn, admit, g, d_D, dropout_p, seed, stream_id, x_prescaled, d_D_next, d_X, ldx, C, d_S_in, lds_in,
                                       s_alpha, s_beta, d_S_out, lds_out, y_beta, d_Y_out, ldy, act, 0, stream);
}

}  // extern "C"
