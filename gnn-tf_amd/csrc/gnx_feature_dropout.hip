// Feature dropout as a pass of its own (the counter RNG of the edge dropout: drop_values, gnx_layer_device.h) and the backward's gate.
//   k_feature_dropout  the mask over whole rows or the rows listed: gnx_feature_dropout, and launch_feature_dropout (gnx_internal.h) for
//                      the layers' rows that go through memory -- hub rows, the other widths, the generic composition
//   the gate           k_feature_dropout_back, .._back_bf16: gnx_feature_dropout_back, gnx_feature_dropout_back_bf16 through
//                      feature_dropout_back<R>; launch_row_pass picks their vector width and grid
#include "gnx_layer_device.h"

namespace {

// out[r, :] = drop(X[r, :]) for the rows listed (null: rows 0 .. n), r the row id the mask is keyed by; out may be X (each lane reads the
// values it overwrites).  VEC = 4: 16-byte accesses (C, both row strides and both bases allow them)
template <int VEC>
__global__ __launch_bounds__(256) void k_feature_dropout(const float *X, int64_t ldx, const int32_t *__restrict__ rows, int64_t n, int64_t C,
                                                        const DropFuse fd, float *out, int64_t ldo) {
    const int64_t per_row = C / VEC, total = n * per_row, stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t stream = drop_stream(fd);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / per_row, r = rows ? (int64_t)rows[i] : i, c = (e % per_row) * VEC;
        float x[VEC];
        vload<VEC>(x, X + r * ldx + c);
        drop_values<VEC>(fd, stream, r, c, x);
        vstore<VEC>(out + r * ldo + c, x);
    }
}

// The backward's gate in one pass: G = kept ? g * scale : +0, and with RELU also +0 where y <= 0 (y = the DROPPED forward output, so
// y > 0 implies kept: the hash is taken only where y lets the value through, the same bits either way).  G may be g.
template <int VEC, bool RELU>
__global__ __launch_bounds__(256) void k_feature_dropout_back(const float *g, int64_t ldg, const float *__restrict__ y, int64_t ldy, int64_t n,
                                                             int64_t C, const DropFuse fd, float *G, int64_t ldG) {
    const int64_t per_row = C / VEC, total = n * per_row, stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t stream = drop_stream(fd);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / per_row, c = (e % per_row) * VEC;
        float x[VEC];
        vload<VEC>(x, g + r * ldg + c);
        if constexpr (RELU) {
            float out[VEC];
            vload<VEC>(out, y + r * ldy + c);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (out[v] <= 0.f) x[v] = 0.f;
                else x[v] = (fd.thr == 0 || hash_u24(fd.seed, stream, (uint64_t)r, (uint64_t)(c + v), 0) >= fd.thr) ? x[v] * fd.scale : 0.f;
            }
        } else {
            drop_values<VEC>(fd, stream, r, c, x);
        }
        vstore<VEC>(G + r * ldG + c, x);
    }
}

// k_feature_dropout_back over the STORED bf16 forward output y (gnx_feature_dropout_back_bf16), the gated gradient written twice: G
// in f32 (what gnx_dense_wgrad and the row's own product of the backward read) and Gb = bf(G) (what the backward gathers).  The gate is
// on the stored value: a positive f32 output that rounded to bf16 zero was stored as zero and passes nothing.
template <int VEC, bool RELU>
__global__ __launch_bounds__(256) void k_feature_dropout_back_bf16(const float *g, int64_t ldg, const uint16_t *__restrict__ y, int64_t ldy,
                                                                  int64_t n, int64_t C, const DropFuse fd, float *G, int64_t ldG,
                                                                  uint16_t *__restrict__ Gb, int64_t ldGb) {
    const int64_t per_row = C / VEC, total = n * per_row, stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t stream = drop_stream(fd);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / per_row, c = (e % per_row) * VEC;
        float x[VEC];
        vload<VEC>(x, g + r * ldg + c);
        if constexpr (RELU) {
            float out[VEC];
            bload<VEC>(out, y + r * ldy + c);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (out[v] <= 0.f) x[v] = 0.f;
                else x[v] = (fd.thr == 0 || hash_u24(fd.seed, stream, (uint64_t)r, (uint64_t)(c + v), 0) >= fd.thr) ? x[v] * fd.scale : 0.f;
            }
        } else {
            drop_values<VEC>(fd, stream, r, c, x);
        }
        vstore<VEC>(G + r * ldG + c, x);
        bstore<VEC>(Gb + r * ldGb + c, x);
    }
}

// gnx_feature_dropout_back (F32Rows: no Gb) and gnx_feature_dropout_back_bf16: one host path
template <typename R>
int feature_dropout_back(const char *fn, gnx_graph *g, const float *d_g, int64_t ldg, const typename R::Elem *d_y, int64_t ldy, int64_t n_rows,
                         int64_t C, double dropout_p, uint64_t seed, uint64_t stream_id, int act, float *d_G, int64_t ldG, uint16_t *d_Gb,
                         int64_t ldGb, void *stream) {
    constexpr bool BF = R::BF16 != 0;
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "%s: invalid activation %d", fn, act);
    GNX_CHECK_ARG(n_rows >= 0 && C >= 1, "%s: negative row count or C < 1", fn);
    GNX_CHECK_ARG(d_g != nullptr && d_G != nullptr && ldg >= C && ldG >= C && (!BF || (d_Gb != nullptr && ldGb >= C)),
                  "%s: NULL g / G%s or a row stride below C", fn, BF ? " / Gb" : "");
    GNX_CHECK_ARG(d_G != d_g || ldG == ldg, "%s: in place needs ldG == ldg", fn);
    GNX_CHECK_ARG(!BF || ((const void *)d_Gb != (const void *)d_g && (const void *)d_Gb != (const void *)d_G), "%s: Gb must not alias g / G", fn);
    const bool relu = act == GNX_ACT_RELU;
    const void *written = BF ? (const void *)d_Gb : (const void *)d_G;      // the result in y's format
    GNX_CHECK_ARG(!relu || (d_y != nullptr && ldy >= C && (const void *)d_y != written), "%s: relu needs y (not %s itself) with ldy >= C", fn,
                  BF ? "Gb" : "G");
    DropFuse fd{};
    int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    if (n_rows == 0) return GNX_OK;
    hipStream_t s = (hipStream_t)stream;
    const RowsAt y_rows = relu ? RowsAt{d_y, 4 * sizeof(typename R::Elem), ldy} : RowsAt{nullptr, 1, 0};      // y is read with relu only
    const RowsAt gb_rows = BF ? RowsAt{d_Gb, 8, ldGb} : RowsAt{nullptr, 1, 0};                                 // Gb exists for bf16 only
    auto gate = [&](auto V, auto RELU, unsigned grid) {
        if constexpr (BF) GNX_LAUNCH((k_feature_dropout_back_bf16<V(), RELU()>), grid, d_g, ldg, d_y, ldy, n_rows, C, fd, d_G, ldG, d_Gb, ldGb);
        else GNX_LAUNCH((k_feature_dropout_back<V(), RELU()>), grid, d_g, ldg, d_y, ldy, n_rows, C, fd, d_G, ldG);
    };
    launch_row_pass(n_rows, C, {{d_g, 16, ldg}, {d_G, 16, ldG}, gb_rows, y_rows}, [&](auto V, unsigned grid) {
        if (relu) gate(V, std::true_type{}, grid);
        else      gate(V, std::false_type{}, grid);
    });
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

}  // namespace

void gnx::launch_feature_dropout(const float *X, int64_t ldx, const int32_t *rows, int64_t n, int64_t C, const DropFuse &fd, float *out, int64_t ldo,
                            hipStream_t s) {
    if (n == 0 || C == 0) return;
    launch_row_pass(n, C, {{X, 16, ldx}, {out, 16, ldo}},
                    [&](auto V, unsigned grid) { GNX_LAUNCH(k_feature_dropout<V()>, grid, X, ldx, rows, n, C, fd, out, ldo); });
}

extern "C" {

int gnx_feature_dropout(gnx_graph_t g, const float *d_X, int64_t ldx, int64_t n_rows, int64_t C, const int32_t *d_rows, double dropout_p,
                        uint64_t seed, uint64_t stream_id, float *d_out, int64_t ldo, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_feature_dropout: NULL handle");
    GNX_CHECK_ARG(n_rows >= 0 && C >= 1, "gnx_feature_dropout: negative row count or C < 1");
    GNX_CHECK_ARG(d_X != nullptr && d_out != nullptr && ldx >= C && ldo >= C, "gnx_feature_dropout: NULL X / out or a row stride below C");
    GNX_CHECK_ARG(d_out != d_X || ldo == ldx, "gnx_feature_dropout: in place needs ldo == ldx");
    DropFuse fd{};
    int rc = make_feat_drop("gnx_feature_dropout", g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    if (dropout_p == 0.0 && d_out == d_X) return GNX_OK;
    launch_feature_dropout(d_X, ldx, d_rows, n_rows, C, fd, d_out, ldo, (hipStream_t)stream);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_feature_dropout_back(gnx_graph_t g, const float *d_g, int64_t ldg, const float *d_y, int64_t ldy, int64_t n_rows, int64_t C,
                             double dropout_p, uint64_t seed, uint64_t stream_id, int act, float *d_G, int64_t ldG, void *stream) {
    return feature_dropout_back<F32Rows>("gnx_feature_dropout_back", g, d_g, ldg, d_y, ldy, n_rows, C, dropout_p, seed, stream_id, act, d_G, ldG,
                                         nullptr, 0, stream);
}

int gnx_feature_dropout_back_bf16(gnx_graph_t g, const float *d_g, int64_t ldg, const uint16_t *d_y, int64_t ldy, int64_t n_rows, int64_t C,
                                  double dropout_p, uint64_t seed, uint64_t stream_id, int act, float *d_G, int64_t ldG, uint16_t *d_Gb,
                                  int64_t ldGb, void *stream) {
    return feature_dropout_back<Bf16Rows>("gnx_feature_dropout_back_bf16", g, d_g, ldg, d_y, ldy, n_rows, C, dropout_p, seed, stream_id, act, d_G,
                                          ldG, d_Gb, ldGb, stream);
}

}  // extern "C"
