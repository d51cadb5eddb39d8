// bf16 rows on the device, shared by the bf16 translation units (gnx_spmm_bf16.hip: eval-mode propagation; gnx_spmm_train_bf16.hip:
// the fused training loops): one load of up to 8 bf16 (16 bytes) widened exactly to f32, the rounding store, and f32 rows at up to
// 8 values per lane.  Internal linkage, forceinline templates: every translation unit gets its own copies.
#pragma once
#include "gnx_spmm_device.h"

namespace {

template <int VEC> struct BfRaw;
template <> struct BfRaw<1> { using type = uint16_t; };
template <> struct BfRaw<2> { using type = uint32_t; };
template <> struct BfRaw<4> { using type = uint2; };
template <> struct BfRaw<8> { using type = uint4; };

// VEC bf16 values (2 * VEC bytes, one load) widened to f32: exact, a bf16 is the upper half of an f32
template <int VEC>
__device__ __forceinline__ void bload(float (&x)[VEC], const uint16_t *__restrict__ p) {
    if constexpr (VEC == 1) {
        x[0] = __uint_as_float((uint32_t)*p << 16);
    } else {
        using T = typename BfRaw<VEC>::type;
        const T v = *reinterpret_cast<const T *>(p);
        uint32_t w[VEC / 2];
        __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
        for (int i = 0; i < VEC / 2; ++i) {
            x[2 * i] = __uint_as_float(w[i] << 16);
            x[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
        }
    }
}

__device__ __forceinline__ uint16_t to_bf16(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }   // RNE, NaN-preserving

template <int VEC>
__device__ __forceinline__ void bstore(uint16_t *__restrict__ p, const float (&x)[VEC]) {
    uint16_t h[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) h[v] = to_bf16(x[v]);
    using T = typename BfRaw<VEC>::type;
    T t;
    __builtin_memcpy(&t, h, sizeof(T));
    *reinterpret_cast<T *>(p) = t;
}

// f32 rows at up to 8 values per lane (two 16-byte accesses at 8)
template <int VEC>
__device__ __forceinline__ void fload(float (&x)[VEC], const float *__restrict__ p) {
    if constexpr (VEC == 8) {
        vload<4>(*reinterpret_cast<float(*)[4]>(&x[0]), p);
        vload<4>(*reinterpret_cast<float(*)[4]>(&x[4]), p + 4);
    } else {
        vload<VEC>(x, p);
    }
}
template <int VEC>
__device__ __forceinline__ void fstore(float *__restrict__ p, const float (&x)[VEC]) {
    if constexpr (VEC == 8) {
        vstore<4>(p, *reinterpret_cast<const float(*)[4]>(&x[0]));
        vstore<4>(p + 4, *reinterpret_cast<const float(*)[4]>(&x[4]));
    } else {
        vstore<VEC>(p, x);
    }
}

}  // namespace
