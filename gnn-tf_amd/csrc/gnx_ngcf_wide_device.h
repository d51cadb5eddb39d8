// What the two width-128 NGCF units share (gnx_ngcf_wide.hip: k_ngcf_rows; gnx_ngcf_wide_back.hip: k_ngcf_rows_back) of one launch shape
// -- a block of eight waves per CU, persistent over 16-row tiles, two weight images in LDS: its constants, the 4 x 4 lane exchange before
// a vector store, the launch, and a runtime count of 16-column blocks as a template argument.  Internal linkage, as in gnx_layer_device.h.
// The two-product MFMA loop stays written out in both kernels (over ngcf_image_at), and k_ngcf_rows keeps ngcf_exchange's loop inline: a
// force-inlined function is unrolled on its own before it is inlined, and with either piece called all sixteen k_ngcf_rows come out
// different, thirteen with more VGPRs (profiles/NOTES.md, "NGCF units, written once").  A fix to one copy goes into the other.
#pragma once
#include "gnx_dense_device.h"
#include "gnx_layer_device.h"

namespace {

constexpr int WIDE_C = 128;       // C_in of the launch
constexpr int WIDE_NT = 8;        // its blocks of 16 columns
constexpr int WIDE_WPB = 8;       // waves per block: one block per CU, two waves per SIMD

// The lane's place in the two LDS weight images, made opaque once per tile: read as a loop invariant, the images of the narrow
// instantiations are hoisted out of the tile loop into registers -- up to 160 of them -- and the forward's instantiations of 32 to 80
// columns spill (profiles/NOTES.md, "NGCF layer at width 128").
__device__ __forceinline__ int ngcf_image_at(int lane) {
    int at = lane;
    asm volatile("" : "+v"(at));
    return at;
}

// The four lanes 4 q .. 4 q + 3 of a row exchange a 4 x 4 block (k_ngcf_rows' store): v[i] is the lane's value -- column 16 (4 h + i) +
// cc of its row -- of result block 4 h + i; afterwards w[e] is column 64 h + 16 j + 4 q + e, (j, q) = (cc & 3, cc >> 2).
__device__ __forceinline__ void ngcf_exchange(const float (&v)[4], int j, float (&w)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {      // lane j ^ s sends its value of block j
        const int i = j ^ s;
        const float t = i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3];
        const float got = s ? __shfl_xor(t, s) : t;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = e == i ? got : w[e];
    }
}

// the launch of a row kernel over n rows: the dynamic-LDS limit once per device and instantiation, a block per CU
template <auto Kernel, typename Args>
int launch_ngcf_rows_kernel(const Args &a, size_t lds_bytes, int64_t n, hipStream_t s) {
    const int cus = persistent_launch<Kernel>();
    if (cus < 0) return cus;
    const int64_t blocks = std::min<int64_t>(cus, blocks_for(blocks_for(n, 16), WIDE_WPB));
    hipLaunchKernelGGL(Kernel, dim3((unsigned)blocks), dim3(64 * WIDE_WPB), lds_bytes, s, a);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

// f(IntC<n_tiles>) for the LO .. 8 blocks of 16 columns of the second width (C_out <= C_in = 128; LO = 0: the launch without products)
template <int LO, typename F>
int with_wide_tiles(int n_tiles, F &&f) {
    if constexpr (LO <= WIDE_NT) return n_tiles == LO ? f(IntC<LO>{}) : with_wide_tiles<LO + 1>(n_tiles, f);
    else return GNX_ERR_INVALID;      // (not reached: the entries admit C_out <= 128)
}

}  // namespace
