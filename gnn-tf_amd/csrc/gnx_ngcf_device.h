// What the two NGCF units share (gnx_ngcf.hip: the one-launch layer at C_in <= 64, its row passes and its backward; gnx_ngcf_wide.hip:
// the SpMM and one row-local launch at C_in = 128): the pieces of a finished value, so that a row is finished by the same code whichever
// kernel made its pre-activations, and the argument checks of the two forward entries.  Internal linkage, as in gnx_layer_device.h.
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

}  // namespace gnx
