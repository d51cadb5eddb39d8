// The epilogue the two spectral-preserving layers share (gnx_gcnii.hip: gnx_gcnii_step_spectral; gnx_gcn.hip: gnx_step_spectral_gcn):
//   out = 2 drop(act(P') - bias),  one gate bit per element, P' > 0
// spectral_finish is shared by contract, as what stands in gnx_layer_device.h is: the store loops of k_spmm_gcnii and k_spmm_gcn and the
// row pass behind the dense kernel (k_spectral_tail, a kernel of gnx_gcnii.hip; gnx::launch_spectral_tail of gnx_internal.h launches it
// for both units) run this code, so a row has the same bits whichever path made it.  No kernel stands here.
#pragma once
#include "gnx_layer_device.h"

namespace {

// x[v] = act(P') of columns c .. c + VEC - 1 of row `row`  ->  2 drop(x[v] - bias[v]): the ONE place the finished value is formed, for
// the store loop of the fused launch and for the row pass behind the dense kernel (k_spectral_tail), so that a row has the same bits
// whichever path made it.  Returns the gate bits of the VEC columns, bit v = (x[v] > 0): with the relu act(P') > 0 iff P' > 0, so the
// gate is that of the pre-activation itself and never a guess from the finished value (relu(P') - bias rounds to -bias for a tiny P').
template <int VEC, bool DROP>
__device__ __forceinline__ uint32_t spectral_finish(const DropFuse &f, uint64_t stream, int64_t row, int64_t c, const float (&bias)[VEC],
                                                    float (&x)[VEC]) {
    uint32_t bits = 0;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        bits |= (x[v] > 0.f ? 1u : 0u) << v;
        x[v] -= bias[v];
    }
    if constexpr (DROP) drop_values<VEC>(f, stream, row, c, x);
#pragma unroll
    for (int v = 0; v < VEC; ++v) x[v] *= 2.f;
    return bits;
}

}  // namespace
