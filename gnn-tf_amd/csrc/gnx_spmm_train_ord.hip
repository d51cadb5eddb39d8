// The fused training launches over a handle's GATHER ORDER (gnx_spmm_dropped_chained_ord, gnx_spmm_dropped_back_ord): rows, per-row
// entry order, masks, weights and sums stay the caller's; only the matrix that is gathered (and the one the next launch gathers) is
// stored with the vertices in the order the relabelled copy numbers them in -- hub rows share 128-byte lines, a hub's leaves sit in
// consecutive lines -- and is reached through a second column array (gnx_graph::a_gcol / t_gcol, 4 bytes per entry).  Per row the
// same fused multiply-adds on the same values in the same order as gnx_spmm_dropped_chained / gnx_spmm_dropped_back: the same bits.
// The kernels are those of gnx_spmm_drop.h under the F32RowsOrd policy; f32 rows, handles without duplicate entries only.
#include "gnx_spmm_drop.h"

extern "C" {

int gnx_spmm_dropped_chained_ord(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                                 const float *d_D_next, const float *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0,
                                 float beta, float alpha, int act, float *d_out, int64_t ldo, int order, void *stream) {
    if (order == 0)
        return gnx_spmm_dropped_chained(g, d_D, dropout_p, seed, stream_id, x_prescaled, d_D_next, d_X, ldx, C, d_H0, ldh0, beta, alpha, act,
                                        d_out, ldo, stream);
    const char *fn = "gnx_spmm_dropped_chained_ord";
    const auto admit = [fn](gnx_graph *g, hipStream_t s) { return ensure_train_gather(g, fn, s); };
    return spmm_dropped_chained<F32RowsOrd>(fn, admit, g, d_D, dropout_p, seed, stream_id, x_prescaled, d_D_next, d_X, ldx, C, d_H0, ldh0, beta,
                                            alpha, act, d_out, 0, ldo, order, stream);
}

int gnx_spmm_dropped_back_ord(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                              const float *d_D_next, const float *d_X, int64_t ldx, int64_t C, const float *d_S_in, int64_t lds_in,
                              float s_alpha, float s_beta, float *d_S_out, int64_t lds_out, float y_beta, float *d_Y_out, int64_t ldy,
                              int act, int order, void *stream) {
    if (order == 0)
        return gnx_spmm_dropped_back(g, d_D, dropout_p, seed, stream_id, x_prescaled, d_D_next, d_X, ldx, C, d_S_in, lds_in, s_alpha, s_beta,
                                     d_S_out, lds_out, y_beta, d_Y_out, ldy, act, stream);
    const char *fn = "gnx_spmm_dropped_back_ord";
    const auto admit = [fn](gnx_graph *g, hipStream_t s) { return ensure_train_gather(g, fn, s); };
    return spmm_dropped_back<F32RowsOrd>(fn, admit, g, d_D, dropout_p, seed, stream_id, x_prescaled, d_D_next, d_X, ldx, C, d_S_in, lds_in,
                                         s_alpha, s_beta, d_S_out, lds_out, y_beta, d_Y_out, ldy, act, order, stream);
}

}  // extern "C"
