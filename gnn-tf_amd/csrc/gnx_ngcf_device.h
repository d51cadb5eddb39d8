// What the three NGCF units share (gnx_ngcf.hip: the one-launch layer at C_in <= 64, its row passes and its backward; gnx_ngcf_wide.hip
// and gnx_ngcf_wide_back.hip: the row-local launches at C_in = 128): the pieces of a finished value, so that a row is finished by the same
// code whichever kernel made its pre-activations, the argument checks of the two forward entries (ngcf_admit), and the host path of the
// two backward entries (NgcfBackCall).  The width-128 row frame is gnx_ngcf_wide_device.h.  Internal linkage, as in gnx_layer_device.h.
#pragma once
#include "gnx_layer_device.h"

namespace {

//   ngcf_act        act(v): the identity, the relu of tile_times_Ms, or tf.nn.leaky_relu's v > 0 ? v : 0.2f v
//   ngcf_mask_sq    x <- drop(x) for columns c .. c + VEC - 1 of a row, then ss <- fmaf(x[v], x[v], ss) over the columns below C_out in
//                   ascending order: a lane's share of the row's sum of squares, one fmaf chain
//   ngcf_row_sum    the lanes of a row (GL consecutive lanes, GL a power of two) add their shares through xor-shuffles, strides 1, 2, ..
//                   GL / 2: every lane ends with the same bits, and lanes that hold +0 beyond a narrower row leave them unchanged
//   ngcf_rnorm      r = 1 / sqrt(max(ss, 1e-12f)) -- IEEE sqrt and divide, correctly rounded each -- and whether the clamp acted
__device__ __forceinline__ float ngcf_act(float v, int act) {
    if (act == GNX_ACT_RELU) return fmaxf(v, 0.f);
    if (act == GNX_ACT_LEAKY) return v > 0.f ? v : 0.2f * v;
    return v;
}

template <int VEC, bool DROP>
__device__ __forceinline__ float ngcf_mask_sq(const DropFuse &f, uint64_t stream, int64_t row, int64_t c, int64_t C_out, float (&x)[VEC], float ss) {
    if constexpr (DROP) drop_values<VEC>(f, stream, row, c, x);
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        if (c + v < C_out) ss = fmaf(x[v], x[v], ss);
    return ss;
}

template <int GL>
__device__ __forceinline__ float ngcf_row_sum(float ss) {
#pragma unroll
    for (int m = 1; m < GL; m <<= 1) ss += __shfl_xor(ss, m);
    return ss;
}

__device__ __forceinline__ float ngcf_rnorm(float ss, bool &clamped) {
    clamped = !(ss >= 1e-12f);
    return 1.0f / sqrtf(fmaxf(ss, 1e-12f));
}

}  // namespace

namespace gnx {

struct NgcfOut { float *out; int64_t ldo; float *agg; uint32_t *gate; float *rnorm; float *work; int64_t work_floats; };

// What gnx_ngcf_step and gnx_step_wide_ngcf check before they size their scratch: the activation, the widths, pointers and strides, a
// square graph, and that out, d_agg, d_gate, d_rnorm and d_work are buffers of their own.  Nothing is launched.
inline int ngcf_admit(const char *fn, gnx_graph *g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C_in, const float *d_W1, int64_t ldw1,
                      const float *d_W2, int64_t ldw2, int64_t C_out, const float *d_b1, const float *d_b2, int act, int normalize, const NgcfOut &o) {
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU || act == GNX_ACT_LEAKY, "%s: invalid activation %d", fn, act);
    GNX_CHECK_ARG(normalize == 0 || normalize == 1, "%s: normalize must be 0 or 1", fn);
    GNX_CHECK_ARG(C_in >= 1 && C_in <= (1 << 20) && C_out >= 1 && C_out <= (1 << 20), "%s: widths %lld -> %lld not in [1, 2^20]", fn,
                  (long long)C_in, (long long)C_out);
    GNX_CHECK_ARG(d_X != nullptr && d_W1 != nullptr && d_W2 != nullptr && o.out != nullptr, "%s: NULL X / W1 / W2 / out", fn);
    GNX_CHECK_ARG(ldx >= C_in, "%s: ldx %lld < C_in %lld", fn, (long long)ldx, (long long)C_in);
    GNX_CHECK_ARG(ldw1 >= C_out && ldw2 >= C_out, "%s: ldw1 %lld or ldw2 %lld < C_out %lld", fn, (long long)ldw1, (long long)ldw2, (long long)C_out);
    GNX_CHECK_ARG(o.ldo >= C_out, "%s: ldo %lld < C_out %lld", fn, (long long)o.ldo, (long long)C_out);
    GNX_CHECK_ARG(o.rnorm == nullptr || normalize, "%s: d_rnorm without normalize", fn);
    GNX_CHECK_ARG(o.work_floats >= 0 && (o.work != nullptr || o.work_floats == 0), "%s: work_floats %lld without d_work, or negative", fn,
                  (long long)o.work_floats);
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "%s: needs a square graph", fn);
    auto input = [&](const void *b) {
        return b == d_X || b == d_W1 || b == d_W2 || (d_b1 && b == d_b1) || (d_b2 && b == d_b2) || (d_vals && b == d_vals);
    };
    const void *gate = o.gate, *rnorm = o.rnorm;
    GNX_CHECK_ARG(!input(o.out), "%s: out must not alias an input (X / W1 / W2 / the biases / the values)", fn);
    GNX_CHECK_ARG(o.agg == nullptr || (!input(o.agg) && o.agg != o.out), "%s: d_agg must be a buffer of its own", fn);
    GNX_CHECK_ARG(gate == nullptr || (!input(gate) && gate != o.out && gate != o.agg), "%s: d_gate must be a buffer of its own", fn);
    GNX_CHECK_ARG(rnorm == nullptr || (!input(rnorm) && rnorm != o.out && rnorm != o.agg && rnorm != gate), "%s: d_rnorm must be a buffer of its own", fn);
    GNX_CHECK_ARG(o.work == nullptr || (!input(o.work) && o.work != o.out && o.work != o.agg && o.work != gate && o.work != rnorm),
                  "%s: d_work must be a buffer of its own", fn);
    return GNX_OK;
}

// ---- the backward entries (gnx_step_back_ngcf, gnx_step_back_wide_ngcf: one parameter list) ---------------------------------------------
// Their host path around the launches, once.  An entry calls front, refuses the widths it has no launch for, calls args and own, refuses in
// its own words what aligned16 does not admit (its "square stand-alone graph" line stays where it is), sizes its slabs, then prelude, its launches, finish.
struct NgcfBackCall {
    gnx_graph *g; const float *d_g; int64_t ldg; const float *d_y; int64_t ldy; const float *d_rnorm; const uint32_t *d_gate; int64_t C_out;
    int act; float *d_G1, *d_G2; int64_t ldG; double dropout_p; uint64_t seed, stream_id;      // (so far: what gnx_ngcf_back_gate takes)
    const float *d_vals_t, *d_X; int64_t ldx; const float *d_agg; int64_t C_in; const float *d_W1; int64_t ldw1; const float *d_W2; int64_t ldw2;
    float *d_P, *d_db1, *d_db2, *d_dA, *d_R, *d_dX; int64_t lddx; float *d_work; int64_t work_floats; void *stream;

    bool products() const { return d_dX != nullptr; }      // dX asked for: both products, dA, R and the transposed SpMM

    // the handle, the activation, the dropout rate and the range of the widths
    int front(const char *fn) const {
        GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
        GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU || act == GNX_ACT_LEAKY, "%s: invalid activation %d", fn, act);
        GNX_CHECK_ARG(dropout_p >= 0.0 && dropout_p < 1.0, "%s: dropout rate %g outside [0, 1)", fn, dropout_p);
        GNX_CHECK_ARG(C_in >= 1 && C_in <= (1 << 20) && C_out >= 1 && C_out <= (1 << 20), "%s: widths %lld -> %lld not in [1, 2^20]", fn,
                      (long long)C_in, (long long)C_out);
        return GNX_OK;
    }
    // what the gate pass reads and writes (gnx_ngcf_back_gate's checks too): the gradient, y with the reciprocal norms, the gate words, G1, G2
    int grads(const char *fn) const {
        GNX_CHECK_ARG(d_g != nullptr && d_G1 != nullptr && d_G2 != nullptr && ldg >= C_out && ldG >= C_out, "%s: NULL g / G1 / G2 or a row stride below C_out", fn);
        GNX_CHECK_ARG(d_rnorm == nullptr || (d_y != nullptr && ldy >= C_out), "%s: d_rnorm needs y (the normalised forward output) with ldy >= C_out", fn);
        GNX_CHECK_ARG(act == GNX_ACT_NONE || d_gate != nullptr, "%s: relu / leaky_relu need d_gate", fn);
        return GNX_OK;
    }
    // pointers, strides and the scratch: the handle is not looked at
    int args(const char *fn) const {
        const int rc = grads(fn);
        if (rc != GNX_OK) return rc;
        GNX_CHECK_ARG(d_X != nullptr && d_agg != nullptr && ldx >= C_in, "%s: NULL X / agg, or ldx %lld < C_in %lld", fn, (long long)ldx, (long long)C_in);
        GNX_CHECK_ARG(!products() || (d_W1 != nullptr && d_W2 != nullptr && d_dA != nullptr && d_R != nullptr), "%s: dX needs W1, W2, d_dA and d_R", fn);
        GNX_CHECK_ARG(!products() || (ldw1 >= C_out && ldw2 >= C_out), "%s: ldw1 %lld or ldw2 %lld < C_out %lld", fn, (long long)ldw1, (long long)ldw2,
                      (long long)C_out);
        GNX_CHECK_ARG(!products() || lddx >= C_in, "%s: lddx %lld < C_in %lld", fn, (long long)lddx, (long long)C_in);
        GNX_CHECK_ARG(work_floats >= 0 && (d_work != nullptr || work_floats == 0), "%s: work_floats %lld without d_work, or negative", fn,
                      (long long)work_floats);
        return GNX_OK;
    }
    // buffers of their own: no output is an input or another output (d_dA and d_R are looked at only where they are written)
    int own(const char *fn) const {
        const void *in[] = {d_vals_t, d_g, d_y, d_rnorm, d_gate, d_X, d_agg, d_W1, d_W2};
        const void *out[] = {d_G1, d_G2, d_P, d_db1, d_db2, products() ? d_dA : nullptr, products() ? d_R : nullptr, d_dX, d_work};
        const char *names[] = {"d_G1", "d_G2", "d_P", "d_db1", "d_db2", "d_dA", "d_R", "d_dX", "d_work"};
        for (size_t i = 0; i < sizeof(out) / sizeof(out[0]); ++i) {
            if (out[i] == nullptr) continue;
            bool own = true;
            for (const void *b : in) own = own && out[i] != b;
            for (size_t j = 0; j < i; ++j) own = own && out[i] != out[j];
            GNX_CHECK_ARG(own, "%s: %s must be a buffer of its own", fn, names[i]);
        }
        return GNX_OK;
    }
    // whole 16-byte accesses of X, A, G1, G2, P, dA and R
    bool aligned16() const {
        return ldx % 4 == 0 && ldG % 4 == 0 && aligned(d_X, 16) && aligned(d_agg, 16) && aligned(d_G1, 16) && aligned(d_G2, 16) && aligned(d_P, 16) &&
               (!products() || (aligned(d_dA, 16) && aligned(d_R, 16)));
    }
    // Before the first launch: the mask of the call, then -- for dX -- the transposed structure and the hub rows' slab (under capture a
    // part that would have to be built refuses the whole call).  A graph without rows is finished here, db1 / db2 zeroed: the entry returns.
    int prelude(const char *fn, DropFuse &fd) const {
        hipStream_t s = (hipStream_t)stream;
        int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
        if (rc == GNX_OK && products()) rc = ensure_transpose(g, s);
        if (rc == GNX_OK && products()) rc = reserve_partial(g, g->t, C_in, s);
        if (rc != GNX_OK || g->a.n_rows != 0) return rc;
        if (d_db1) GNX_HIP(hipMemsetAsync(d_db1, 0, (size_t)C_out * sizeof(float), s));
        if (d_db2) GNX_HIP(hipMemsetAsync(d_db2, 0, (size_t)C_out * sizeof(float), s));
        return GNX_OK;
    }
    // dX = A_hat^T dA + R where it is asked for -- the transposed SpMM over dA with R mixed in -- then the name the handle reports
    int finish(const char *name) const {
        const float *vals_t = d_vals_t ? d_vals_t : g->t_raw.get();
        const int rc = products() ? gnx_spmm_tv(g, vals_t, nullptr, d_dA, C_in, C_in, d_R, C_in, 1.f, 1.f, GNX_ACT_NONE, d_dX, lddx, stream) : GNX_OK;
        if (rc == GNX_OK) g->last_kernel = name;
        return rc;
    }
};

}  // namespace gnx
