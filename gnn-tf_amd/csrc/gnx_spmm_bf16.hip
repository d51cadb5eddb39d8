// Opt-in bf16 feature storage for eval-mode propagation: the SpMM of gnx_spmm.hip with the GATHERED operand stored as bf16.
//
//   out[i,:] = act( beta * ( sum_j A[i,j] X~[j,:] + diag[i] X~[i,:] ) + alpha * H0[i,:] )
//
// X~ is bf16, widened exactly to f32 (a 16-bit shift) as it arrives; the sums, H0 and the epilogue are f32, and the result is
// rounded once (round to nearest even, NaN stays NaN: the plain cast, v_cvt_pk_bf16_f32) when the caller asks for a bf16 result.
// The propagation is bound by the random gathers of neighbour rows (profiles/NOTES.md): halving a gathered row halves the lines
// it moves (C = 128: 512 -> 256 bytes; C = 40 padded to 64: one 128-byte line instead of 160 bytes over two).
//
// The dispatch classes, their row orders and their summation orders are those of gnx_spmm.hip -- one wave per row for rows wider
// than 32 lanes, 32/16/8-lane groups below, long rows cut into chunks whose f32 partial sums a second kernel adds in chunk order
// (no float atomics: two calls give the same bits) -- with up to 8 bf16 (16 bytes) per lane: C = 128 runs on 16-lane groups.
// The kernels are those of gnx_spmm_eval.h, instantiated here over Bf16RowsT (gnx_spmm_device.h); the f32 tuning switches do not exist
// for bf16 rows.
// gnx_spmm_rows_bf16 (the interior / boundary handles of a vertex block): SpmmArgs::out_rows / map_h0 send result row r to
// out[rows[r]] and mix H0[rows[r]] in every row class; with a null map a row is its own destination, as before.
#include "gnx_spmm_eval.h"

namespace {

using Bf16Rows = Bf16RowsT<false>;

// f32 -> bf16, any leading dimensions; VEC = 4 when every row start is 16-byte (src) / 8-byte (dst) aligned
template <int VEC>
__global__ __launch_bounds__(256) void k_cast_bf16(const float *__restrict__ src, int64_t lds, int64_t n_rows, int64_t C,
                                                  uint16_t *__restrict__ dst, int64_t ldd) {
    const int64_t per_row = C / VEC, total = n_rows * per_row, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / per_row, c = (e % per_row) * VEC;
        float x[VEC];
        vload<VEC>(x, src + r * lds + c);
        bstore<VEC>(dst + r * ldd + c, x);
    }
}

int launch_bf_eval(gnx_graph *g, const Csr &m, BfArgs &p, hipStream_t s) {
    // "+long" in the name when hub rows went through the chunk kernels
    return launch_bound(g, m, p, s, [&](BfArgs &q) { return launch_eval<Bf16Rows>(q, s); });
}

int cast_bf16(const float *src, int64_t n_rows, int64_t C, int64_t lds, uint16_t *dst, int64_t ldd, hipStream_t s) {
    if (n_rows == 0) return GNX_OK;
    const bool v4 = C % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && aligned(src, 16) && aligned(dst, 8);
    const int64_t items = n_rows * (v4 ? C / 4 : C);
    const unsigned grid = (unsigned)std::min<int64_t>(blocks_for(items, 256), 1 << 20);
    if (v4) hipLaunchKernelGGL(k_cast_bf16<4>, dim3(grid), dim3(256), 0, s, src, lds, n_rows, C, dst, ldd);
    else    hipLaunchKernelGGL(k_cast_bf16<1>, dim3(grid), dim3(256), 0, s, src, lds, n_rows, C, dst, ldd);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

// the arguments of an f32 launch with its rows gathered from bf16 Xb and finished as f32 into `out`
BfArgs bf_rows_of(const SpmmArgs &p, const uint16_t *Xb, float *out) {
    BfArgs q{};
    static_cast<SpmmArgs &>(q) = p;
    q.X = nullptr; q.out = nullptr;
    q.Xb = Xb; q.outv = out; q.out_bf16 = 0;
    return q;
}

}  // namespace

namespace gnx {

// launch_eval<Bf16Rows> with the hub chunks on the lane groups of the f32 launch (at most 4 columns per lane): the group width deals a
// chunk's entries to sub-groups, i.e. it IS the long rows' summation order.  The short rows keep 8 columns per lane wherever they have a
// launch of their own (their entries are added in ascending order whatever the lane width).
int launch_spmm_bf16_f32_order(gnx_graph *g, const Csr &m, const SpmmArgs &p, const uint16_t *Xb, float *out, hipStream_t s) {
    BfArgs bound = bf_rows_of(p, Xb, out);
    return launch_bound(g, m, bound, s, [&](BfArgs &q) {
        const int vec = Bf16Rows::vec(q);
        return with_vec<F32Rows>(std::min(vec, 4), [&](auto V4) {
            RowClass rows = launch_rows_and_chunks<Bf16Rows, V4()>(q, s);
            if (rows != ROWS_NONE) return kernel_name<Bf16Rows>(rows, MODE_EVAL, HUBS_CHUNKS);
            rows = with_vec<Bf16Rows>(vec, [&](auto V) { return launch_rows<Bf16Rows, V()>(q, s); });
            if (q.n_long > 0) launch_long<Bf16Rows, V4()>(q, s);
            return kernel_name<Bf16Rows>(rows, MODE_EVAL, q.n_long > 0 ? HUBS_LONG : HUBS_NONE);
        });
    });
}

void launch_long_rows_bf16(const SpmmArgs &p, const uint16_t *Xb, float *out, hipStream_t s) {
    const BfArgs q = bf_rows_of(p, Xb, out);
    with_vec<F32Rows>(std::min(Bf16Rows::vec(q), 4), [&](auto V) { launch_long<Bf16Rows, V()>(q, s); });
}

}  // namespace gnx

extern "C" {

int gnx_cast_bf16(const float *d_src, int64_t n_rows, int64_t C, int64_t lds, uint16_t *d_dst, int64_t ldd, void *stream) {
    GNX_CHECK_ARG(n_rows >= 0, "gnx_cast_bf16: negative row count");
    GNX_CHECK_ARG(C >= 1 && C <= (1 << 20), "gnx_cast_bf16: feature width %lld not in [1, 2^20]", (long long)C);
    GNX_CHECK_ARG(lds >= C && ldd >= C, "gnx_cast_bf16: leading dimension smaller than C");
    GNX_CHECK_ARG(n_rows == 0 || (d_src != nullptr && d_dst != nullptr), "gnx_cast_bf16: NULL buffer");
    GNX_CHECK_ARG(n_rows == 0 || (const void *)d_src != (const void *)d_dst, "gnx_cast_bf16: dst must not alias src");
    return cast_bf16(d_src, n_rows, C, lds, d_dst, ldd, (hipStream_t)stream);
}

int gnx_spmm_bf16(gnx_graph_t g, const float *d_vals, const float *d_diag, const uint16_t *d_X, int64_t ldx, int64_t C,
                  const float *d_H0, int64_t ldh0, float beta, float alpha, int act, void *d_out, int out_bf16, int64_t ldo,
                  void *stream) {
    int rc = check_common("gnx_spmm_bf16", g, d_X, ldx, C, d_H0, ldh0, d_out, ldo);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1, "gnx_spmm_bf16: out_bf16 must be 0 or 1");
    GNX_CHECK_ARG((act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_NONE || (act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_RELU, "gnx_spmm_bf16: invalid activation %d", act);
    GNX_CHECK_ARG(d_diag == nullptr || g->a.n_rows == g->a.n_cols, "gnx_spmm_bf16: diag needs a square graph");
    BfArgs p{};
    p.vals = d_vals ? d_vals : g->raw_vals;
    p.diag = d_diag;
    set_operands<Bf16Rows>(p, d_X, ldx, d_H0, ldh0, beta, alpha, act, d_out, out_bf16, ldo, C);
    return launch_bf_eval(g, g->a, p, (hipStream_t)stream);
}

int gnx_spmm_rows_bf16(gnx_graph_t g, const float *d_vals, const uint16_t *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0,
                       float beta, float alpha, int act, const int32_t *d_rows, void *d_out, int out_bf16, int64_t ldo, void *stream) {
    int rc = check_common("gnx_spmm_rows_bf16", g, d_X, ldx, C, d_H0, ldh0, d_out, ldo);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1, "gnx_spmm_rows_bf16: out_bf16 must be 0 or 1");
    GNX_CHECK_ARG((act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_NONE || (act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_RELU, "gnx_spmm_rows_bf16: invalid activation %d", act);
    GNX_CHECK_ARG(d_rows != nullptr || g->a.n_rows == 0, "gnx_spmm_rows_bf16: NULL row map");
    BfArgs p{};
    p.vals = d_vals ? d_vals : g->raw_vals;
    p.out_rows = d_rows; p.map_h0 = true;
    set_operands<Bf16Rows>(p, d_X, ldx, d_H0, ldh0, beta, alpha, act, d_out, out_bf16, ldo, C);
    return launch_bf_eval(g, g->a, p, (hipStream_t)stream);
}

int gnx_appnp_propagate_bf16(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_H0, float a, int K, int64_t C,
                             int act, float *d_out, uint16_t *d_work, void *stream) {
    // the checks that need no handle come first (so that they can be exercised without a device)
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "gnx_appnp_propagate_bf16: invalid activation %d", act);
    GNX_CHECK_ARG(K >= 0, "gnx_appnp_propagate_bf16: negative iteration count");
    GNX_CHECK_ARG(C >= 1 && C <= (1 << 20), "gnx_appnp_propagate_bf16: feature width %lld not in [1, 2^20]", (long long)C);
    GNX_CHECK_ARG(d_H0 && d_out && (K < 1 || d_work), "gnx_appnp_propagate_bf16: NULL buffer");
    GNX_CHECK_ARG((const void *)d_out != (const void *)d_H0 && (const void *)d_work != (const void *)d_H0 && (const void *)d_out != (const void *)d_work,
                  "gnx_appnp_propagate_bf16: H0, out and work must be distinct");
    GNX_CHECK_ARG(g != nullptr, "gnx_appnp_propagate_bf16: NULL handle");
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "gnx_appnp_propagate_bf16: needs a square graph");
    const int64_t n = g->a.n_rows;
    hipStream_t s = (hipStream_t)stream;
    if (K == 0) {
        GNX_HIP(hipMemcpyAsync(d_out, d_H0, (size_t)n * C * sizeof(float), hipMemcpyDeviceToDevice, s));
        return GNX_OK;
    }
    // H~_0 = bf(H0) into the first half of d_work; iteration k < K-1 writes bf(H_{k+1}) into the other half, the last one f32 H_K
    uint16_t *buf[2] = {d_work, d_work + n * C};
    int rc = cast_bf16(d_H0, n, C, C, buf[0], C, s);
    if (rc != GNX_OK) return rc;
    for (int k = 0; k < K; ++k) {
        const bool last = k == K - 1;
        // rows without entries are act(a * H0) after every iteration: buf[1] has them after k = 0, buf[0] after k = 1 (it held
        // bf(H0) before); when nobody gathers them (empty_rows_unreferenced) the work buffers never need them at all.  The
        // last iteration writes every row of d_out.
        const bool settled = !last && (k >= 2 || g->a.empty_rows_unreferenced);
        BfArgs p{};
        p.vals = d_vals ? d_vals : g->raw_vals;
        p.diag = d_diag;
        set_operands<Bf16Rows>(p, buf[k % 2], C, d_H0, C, (float)(1.0 - (double)a), a, (settled && d_diag == nullptr) ? (act | GNX_ACT_SKIP_EMPTY) : act,
                               last ? (void *)d_out : (void *)buf[(k + 1) % 2], last ? 0 : 1, C, C);
        rc = launch_bf_eval(g, g->a, p, s);
        if (rc != GNX_OK) return rc;
    }
    return GNX_OK;
}

}  // extern "C"
