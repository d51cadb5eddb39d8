// Device-side pieces every SpMM translation unit shares: vector loads / stores, the row-storage policy (F32Rows / Bf16RowsT: how a
// gathered feature row and a finished row are stored), the wave-wide accumulate, the fused epilogue of filter.py:20-22, the slot and
// chunk prologues, the XCD block map, the long rows' second pass, and the launch plumbing.  The dispatch classes themselves are written
// once over the policy in gnx_spmm_eval.h (eval) and gnx_spmm_drop.h (training) and instantiated by gnx_spmm.hip / gnx_spmm_train.hip
// for f32 rows and by gnx_spmm_bf16.hip / gnx_spmm_train_bf16.hip for bf16 rows.  Internal linkage throughout: every translation unit
// gets its own copies (all of it is templates / forceinline device code / small host helpers).
#pragma once
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

#include "gnx_internal.h"

using namespace gnx;

namespace {

template <int VEC> struct VecT;
template <> struct VecT<1> { using type = float; };
template <> struct VecT<2> { using type = float2; };
template <> struct VecT<4> { using type = float4; };

// (VEC = 8, the f32 side of bf16 rows at 8 values per lane: two 16-byte accesses)
template <int VEC>
__device__ __forceinline__ void vload(float (&x)[VEC], const float *__restrict__ p) {
    if constexpr (VEC == 8) {
        vload<4>(*reinterpret_cast<float(*)[4]>(&x[0]), p);
        vload<4>(*reinterpret_cast<float(*)[4]>(&x[4]), p + 4);
    } else {
        using T = typename VecT<VEC>::type;
        const T v = *reinterpret_cast<const T *>(p);
        __builtin_memcpy(x, &v, sizeof(T));
    }
}
template <int VEC>
__device__ __forceinline__ void vstore(float *__restrict__ p, const float (&x)[VEC]) {
    if constexpr (VEC == 8) {
        vstore<4>(p, *reinterpret_cast<const float(*)[4]>(&x[0]));
        vstore<4>(p + 4, *reinterpret_cast<const float(*)[4]>(&x[4]));
    } else {
        using T = typename VecT<VEC>::type;
        T v;
        __builtin_memcpy(&v, x, sizeof(T));
        *reinterpret_cast<T *>(p) = v;
    }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int VEC> struct NatT;
template <> struct NatT<1> { using type = float; };
template <> struct NatT<2> { using type = f32x2; };
template <> struct NatT<4> { using type = f32x4; };

// ---- hinted gathers (gnx_graph_set_gather_hints; f32 rows, 16 bytes per lane) ----------------------------------------------------
// A hinted column (gnx_graph::hint_cols) carries in bit 31 whether the gathered row is COLD: not one of the handle's hot rows, the
// ones with the most entries, which are gathered again and again.  A cold row is loaded non-temporally: gfx950's caches then replace
// it first, and the hot rows stay (tools/gather_policy_probe.hip: hit rate of a 2 MiB hot table beside cold gathers 41 % -> 99 %,
// the cold gathers themselves 8 % faster; what that is worth in these kernels, and for which hot sets: gnx_internal.h, HINT_HOT_BYTES).
// Source-level selection between a plain and a non-temporal load does not survive the compiler (it merges the two into one plain
// load, or speculates both), so one asm statement holds both forms.  hipcc counts nothing inside asm: a batch of gathers is followed by ONE gather_wait over the batch's registers, and nothing reads them before.
// The statements carry no "memory" clobber on purpose: the gathered matrix is only read by its launch, and the index loads of the
// compiler must stay free to move ahead of the gathers (behind one, their wait would drain it).
constexpr int HINT_NONE = -1;            // hinted column of an entry that does not exist (ragged batch): neither form loads
__device__ __forceinline__ int hint_col(int j) { return j & 0x7fffffff; }

// per lane: the lanes of one wave may hold rows of either kind (two 32-lane groups), so the choice is by exec mask, restored at the
// end; a form that no lane takes is branched over (an instruction without lanes still takes its turn in the address unit)
__device__ __forceinline__ void gather16_hinted(f32x4 &x, const float *q, int j) {
    uint64_t keep;
    asm volatile("s_mov_b64 %[keep], exec\n\t"
                 "v_cmp_gt_i32_e32 vcc, -1, %[j]\n\t"              // cold: bit 31 set, and not HINT_NONE
                 "s_and_b64 exec, %[keep], vcc\n\t"
                 "s_cbranch_scc0 .Lgnx_nocold%=\n\t"
                 "global_load_dwordx4 %[x], %[q], off nt\n"
                 ".Lgnx_nocold%=:\n\t"
                 "s_mov_b64 exec, %[keep]\n\t"
                 "v_cmp_lt_i32_e32 vcc, -1, %[j]\n\t"              // hot: bit 31 clear
                 "s_and_b64 exec, %[keep], vcc\n\t"
                 "s_cbranch_scc0 .Lgnx_nohot%=\n\t"
                 "global_load_dwordx4 %[x], %[q], off\n"
                 ".Lgnx_nohot%=:\n\t"
                 "s_mov_b64 exec, %[keep]"
                 : [x] "+v"(x), [keep] "=&s"(keep)
                 : [q] "v"(q), [j] "v"(j)
                 : "vcc", "scc");
}

// the column is wave-uniform (v_readlane): a scalar branch picks the form
__device__ __forceinline__ void gather16_hinted_uniform(f32x4 &x, const float *q, int j) {
    asm volatile("s_bitcmp1_b32 %[j], 31\n\t"
                 "s_cbranch_scc1 .Lgnx_cold%=\n\t"
                 "global_load_dwordx4 %[x], %[q], off\n\t"
                 "s_branch .Lgnx_done%=\n"
                 ".Lgnx_cold%=:\n\t"
                 "global_load_dwordx4 %[x], %[q], off nt\n"
                 ".Lgnx_done%=:"
                 : [x] "+v"(x)
                 : [q] "v"(q), [j] "s"(j)
                 : "scc");
}

// every hinted gather of a batch has landed; the batch's registers are operands so that nothing reads them ahead of the wait
template <int U>
__device__ __forceinline__ void gather_wait(f32x4 (&x)[U]) {
    static_assert(U == 4 || U == 8, "batches of 4 or 8 gathers");
    if constexpr (U == 4) asm volatile("s_waitcnt vmcnt(0)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]));
    else asm volatile("s_waitcnt vmcnt(0)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]));
}

// ---- bf16 rows: one load of up to 8 bf16 (16 bytes) widened exactly to f32, and the rounding store ----
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

inline bool aligned(const void *p, size_t a) { return p == nullptr || ((uintptr_t)p % a) == 0; }

// widest per-lane vector every row start allows (the policies' vec()): up to max_vec values per lane, X / out / out2 holding
// elements of x_size / out_size / out2_size bytes, H0 f32; an access is at most 16 bytes
[[maybe_unused]] int pick_vec(const SpmmArgs &p, int max_vec, const void *X, size_t x_size, const void *out, size_t out_size, const void *out2,
             size_t out2_size) {
    for (int vec = max_vec; vec > 1; vec >>= 1) {
        if (p.C % vec == 0 && p.ldx % vec == 0 && p.ldo % vec == 0 && (p.H0 == nullptr || p.ldh0 % vec == 0) &&
            (out2 == nullptr || p.ldo2 % vec == 0) && aligned(X, std::min<size_t>(x_size * vec, 16)) &&
            aligned(out, std::min<size_t>(out_size * vec, 16)) && aligned(p.H0, std::min<size_t>(4 * vec, 16)) &&
            aligned(out2, std::min<size_t>(out2_size * vec, 16)))
            return vec;
    }
    return 1;
}

// ---- how a launch stores its feature rows: the policy every dispatch class is templated on -------------------------------------
// Args = the argument struct of its kernels; MAX_VEC = the widest per-lane vector (16 bytes of a gathered row); X / load = the
// gathered operand and VEC of its columns as float[VEC]; store / store2 = VEC finished columns of the main and of the second result
// (`at` = element offset of the row, c = first column); diag / out_rows / out_scale / has_out2 = the optional pieces of the epilogue,
// runtime-null pointers where an entry point of that storage can set them and a constant null where none can; EXPERIMENTS = the
// kernels carry the A/B switches of the tuning build (SpmmArgs::tune, the PIPE / U variants), which exist for f32 rows only.
// BF16 / NAMES_LONG only pick the reported name (kernel_name).  GATHER_ORDER = the kernels read OrdArgs::gcol / out2_rows (F32RowsOrd
// below); where it is false those loads do not exist in the kernel.  Host side: Out / Out2 = how an entry point types the main and the
// second result, bind_X / bind_out / bind_out2 = where Args keeps the typed buffers (set_operands fills the rest around them).
struct F32Rows {
    using Args = SpmmArgs;
    using Elem = float;
    using Out = float;
    using Out2 = float;
    static constexpr int MAX_VEC = 4;
    static constexpr bool EXPERIMENTS = true;
    static constexpr int BF16 = 0;
    static constexpr bool NAMES_LONG = false;    // the reported name does not say whether hub rows went through the chunk kernels
    static constexpr bool GATHER_ORDER = false;
    __device__ static const float *X(const Args &p) { return p.X; }
    template <int VEC>
    __device__ static void load(float (&x)[VEC], const float *__restrict__ q) { vload<VEC>(x, q); }
    __device__ static const float *diag(const Args &p) { return p.diag; }
    __device__ static const int32_t *out_rows(const Args &p) { return p.out_rows; }
    __device__ static bool has_out2(const Args &p) { return p.out2 != nullptr; }
    __device__ static const float *out_scale(const Args &p) { return p.out_scale; }
    template <int VEC>
    __device__ static void store(const Args &p, int64_t at, int c, const float (&o)[VEC]) { vstore<VEC>(p.out + at + c, o); }
    template <int VEC>
    __device__ static void store2(const Args &p, int64_t at, int c, const float (&o)[VEC]) { vstore<VEC>(p.out2 + at + c, o); }
    // (the second result's row starts are not looked at: every caller so far keeps it laid out like the first)
    static int vec(const Args &p) { return pick_vec(p, MAX_VEC, p.X, 4, p.out, 4, nullptr, 0); }
    static void bind_X(Args &p, const float *X) { p.X = X; }
    static void bind_out(Args &p, float *out, int /* out_bf16: f32 rows have no such choice */) { p.out = out; }
    static void bind_out2(Args &p, float *out2) { p.out2 = out2; }
};

// f32 rows of a training launch whose gathered operand and / or results live in the handle's gather order (gnx_spmm_dropped_chained_ord,
// gnx_spmm_dropped_back_ord): the lane that owns an entry loads its gather column (OrdArgs::gcol) beside its column -- the draw, the
// mask and D[col] keep the column, the gather address takes the gather column -- and the second result goes through out2_rows as
// the first goes through out_rows.  Per row the same fused multiply-adds on the same values in the same order as F32Rows.
// (the two arrays live in an argument struct of their own, behind SpmmArgs, as the bf16 buffers do: inside SpmmArgs they would move
// the bf16 kernels' arguments, and those kernels would no longer be the ones measured so far)
struct OrdArgs : SpmmArgs {
    const int32_t *gcol;        // per entry the row of X to gather (gnx_graph::a_gcol / t_gcol: X is stored in gather order); null = colidx
    const int32_t *out2_rows;   // destination row of every row of the second result; null = the row itself
};

struct F32RowsOrd : F32Rows {
    using Args = OrdArgs;
    static constexpr bool EXPERIMENTS = false;
    static constexpr bool NAMES_LONG = true;
    static constexpr bool GATHER_ORDER = true;
};

// f32 rows of a K-loop launch that elides the handle's pendant rows (gnx_graph_set_pendant_elision; gnx_internal.h, PendantPart):
// the sub-wave hinted kernels of 4 values per lane only.  SpmmArgs::colidx holds the handle's pend_cols.  An entry whose column is
// elidable gathers that column's H0 row instead of its iterate -- nobody wrote one -- and forms the iterate from it, from pend_w and
// from the gathering row's own values of two iterations ago, P[row] (pendant_iterate).  (An argument struct of its own, behind
// SpmmArgs, as for OrdArgs: no other kernel takes a new argument.)
struct PendArgs : SpmmArgs {
    const float *P;                  // [n, ldp] the gathering rows' iterate of two iterations ago: H0, or the destination buffer as the launch finds it
    int64_t ldp;
    const float *pend_w;             // [n] per elidable row the value of its one entry
    const uint8_t *pend_slot_mark;   // [n] per row slot: the row stores an entry whose column is elidable
    const uint8_t *pend_row_mark;    // [n] the same per row (the chunk kernels)
    int pend_raw;                    // the first iteration: the gathered operand IS H0, an elidable column's H0 row is its iterate
    int64_t skip_beg, skip_end;      // row slots this launch leaves out: the elidable rows, in every iteration but the last
};

struct F32RowsPend : F32Rows {
    using Args = PendArgs;
    static constexpr bool EXPERIMENTS = false;
};
template <typename R> constexpr bool IS_PEND = std::is_same_v<typename R::Args, PendArgs>;

__device__ __forceinline__ bool pend_col(int j) { return (j & PEND_COL_BIT) != 0 && j != HINT_NONE; }

// One value of iterate k+1 of an elidable row i, as its neighbour h forms it: x = H0[i], prev = iterate k of h, w = pend_w[i].  The
// very operations the row's own launch ran on it: a batch of four entries of which three do not exist -- fmaf(0, 0, t) turns -0
// into +0 -- and the epilogue of epilogue_store for a row with H0 and nothing optional.
__device__ __forceinline__ float pendant_iterate(float w, float prev, float x, float beta, float alpha, int act) {
    float t = fmaf(w, prev, 0.f);
#pragma unroll
    for (int u = 1; u < 4; ++u) t = fmaf(0.f, 0.f, t);
    float o = fmaf(t, beta, x * alpha);
    if (act == GNX_ACT_RELU) o = fmaxf(o, 0.f);
    return o;
}

struct BfArgs : SpmmArgs {     // SpmmArgs::X / ::out / ::out2 stay null: the typed buffers are here
    const uint16_t *Xb;        // bf16 [rows, ldx]: the gathered operand
    void *outv;                // f32 or bf16 [n_rows, ldo]
    int out_bf16;
    uint16_t *out2b;           // bf16 [n_rows, ldo2] or null (gnx_spmm_dropped_back_bf16: the operand of the next call)
};

// X is bf16, widened exactly as it arrives; sums, H0, the partial slab and the epilogue stay f32; a row that leaves as bf16 is
// rounded once (round to nearest even, NaN stays NaN: the plain cast, v_cvt_pk_bf16_f32).  TRAIN says which entry points launch:
// the training ones set the second result and the next iteration's scale and never a diagonal or a row map, the eval ones the
// reverse.  What a side cannot set is compiled out of its kernels: as runtime tests these pointers cost the eval group kernels 6
// VGPRs (a wave per SIMD at 8 values per lane on 16/32-lane groups) and the training kernels up to 22 SGPRs (profiles/NOTES.md).
template <bool TRAIN>
struct Bf16RowsT {
    using Args = BfArgs;
    using Elem = uint16_t;
    using Out = void;
    using Out2 = uint16_t;
    static constexpr int MAX_VEC = 8;
    static constexpr bool EXPERIMENTS = false;
    static constexpr int BF16 = 1;
    static constexpr bool NAMES_LONG = true;
    static constexpr bool GATHER_ORDER = false;
    __device__ static const uint16_t *X(const Args &p) { return p.Xb; }
    template <int VEC>
    __device__ static void load(float (&x)[VEC], const uint16_t *__restrict__ q) { bload<VEC>(x, q); }
    __device__ static const float *diag(const Args &p) { return TRAIN ? nullptr : p.diag; }
    __device__ static const int32_t *out_rows(const Args &p) { return TRAIN ? nullptr : p.out_rows; }
    __device__ static bool has_out2(const Args &p) { return TRAIN && p.out2b != nullptr; }
    __device__ static const float *out_scale(const Args &p) { return TRAIN ? p.out_scale : nullptr; }
    template <int VEC>
    __device__ static void store(const Args &p, int64_t at, int c, const float (&o)[VEC]) {
        if (p.out_bf16) bstore<VEC>(static_cast<uint16_t *>(p.outv) + at + c, o);
        else vstore<VEC>(static_cast<float *>(p.outv) + at + c, o);
    }
    template <int VEC>
    __device__ static void store2(const Args &p, int64_t at, int c, const float (&o)[VEC]) { bstore<VEC>(p.out2b + at + c, o); }
    static int vec(const Args &p) { return pick_vec(p, MAX_VEC, p.Xb, 2, p.outv, p.out_bf16 ? 2 : 4, p.out2b, 2); }
    static void bind_X(Args &p, const uint16_t *X) { p.Xb = X; }
    static void bind_out(Args &p, void *out, int out_bf16) { p.outv = out; p.out_bf16 = out_bf16; }
    static void bind_out2(Args &p, uint16_t *out2) { p.out2b = out2; }
};

__device__ __forceinline__ int readlane_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float readlane_f(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// per entry the row of X a training kernel gathers: the handle's gather columns under a GATHER_ORDER policy whose launch stores X
// in gather order, the column itself otherwise (wave-uniform, chosen once per kernel)
template <typename R>
__device__ __forceinline__ const int32_t *gather_cols(const typename R::Args &p) {
    if constexpr (R::GATHER_ORDER) return p.gcol ? p.gcol : p.colidx;
    else return nullptr;
}

// Sum of w_e * X[col_e, c .. c+VEC) over entries [beg, end) of one row; the whole wave works
// on the same entries (beg/end wave-uniform), lane `lane` owns columns c .. c+VEC.  ENTRIES (with FUSE): the handle holds duplicate
// entries and the weight of a slot is its kept sum (dropped_weight_entries).  GCOL (with FUSE): the gathered row of an entry is
// gcol[entry] instead of its column (gather_cols).  HINT (eval, f32 rows of 4 values per lane): `colidx` holds the handle's hinted
// columns and the gathers go through gather16_hinted_uniform; the same entries in the same order into the same fused multiply-adds.
// (nt_index: no caller sets it any more -- the tuning switch that did measured +-0 % and is gone -- but taking the parameter out
// changes the instruction schedule of the training kernels, which are kept as measured)
template <typename R, int VEC, int U, bool FUSE = false, bool ENTRIES = false, bool GCOL = false, bool HINT = false>
__device__ __forceinline__ void wave_accumulate(const int32_t *__restrict__ colidx, const float *__restrict__ vals,
                                                const typename R::Elem *__restrict__ X, int64_t ldx, int64_t beg, int64_t end,
                                                int c, int lane, float (&acc)[VEC], bool nt_index = false,
                                                const DropFuse *fuse = nullptr, int64_t row = 0,
                                                const int32_t *__restrict__ gcol = nullptr) {
    for (int64_t base = beg; base < end; base += 64) {
        const int n = (int)((end - base) < 64 ? (end - base) : 64);
        int mycol = 0;
        [[maybe_unused]] int mygcol = 0;
        float myval = 0.f;
        if (lane < n) {
            if (nt_index) {
                mycol = __builtin_nontemporal_load(colidx + base + lane);
                myval = __builtin_nontemporal_load(vals + base + lane);
            } else {
                mycol = colidx[base + lane];
                myval = vals[base + lane];
            }
            if constexpr (GCOL) mygcol = gcol[base + lane];
            if (FUSE) myval = dropped_weight_at<ENTRIES>(*fuse, myval, base + lane, row, mycol);   // one entry per lane: 64 weights per wave instruction
        }
        int i = 0;
        if (FUSE) {
            // a dropped entry has weight exactly 0: its row is not gathered at all (fmaf(0, x, acc) == acc for finite x), so a
            // training iteration moves only the kept rows -- half of them at p = 0.5; kept entries stay in ascending order
            uint64_t keep = __ballot(myval != 0.f);
            while (keep) {
                float x[U][VEC];
                int idx[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    idx[u] = keep ? (int)__builtin_ctzll(keep) : -1;
                    if (keep) keep &= keep - 1;
                    if (idx[u] >= 0) {
                        int j;
                        if constexpr (GCOL) j = readlane_i(mygcol, idx[u]);
                        else j = readlane_i(mycol, idx[u]);
                        R::template load<VEC>(x[u], X + (int64_t)j * ldx + c);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (idx[u] >= 0) {
                        const float w = readlane_f(myval, idx[u]);
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, x[u][v], acc[v]);
                    }
                }
            }
            continue;
        }
        if constexpr (HINT) {
            static_assert(VEC == 4 && !FUSE && std::is_same_v<typename R::Elem, float>, "hinted gathers: f32 rows, 16 bytes per lane, eval");
            for (; i + U <= n; i += U) {
                f32x4 x[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int j = readlane_i(mycol, i + u);
                    x[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                    gather16_hinted_uniform(x[u], X + (int64_t)hint_col(j) * ldx + c, j);
                }
                gather_wait<U>(x);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float w = readlane_f(myval, i + u);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, x[u][v], acc[v]);
                }
            }
            if (i < n) {  // 1 .. U-1 entries left (wave-uniform branches)
                f32x4 x[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    x[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (u < U - 1 && i + u < n) {
                        const int j = readlane_i(mycol, i + u);
                        gather16_hinted_uniform(x[u], X + (int64_t)hint_col(j) * ldx + c, j);
                    }
                }
                gather_wait<U>(x);
#pragma unroll
                for (int u = 0; u < U - 1; ++u) {
                    if (i + u < n) {
                        const float w = readlane_f(myval, i + u);
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, x[u][v], acc[v]);
                    }
                }
            }
            continue;
        }
        for (; i + U <= n; i += U) {
            float x[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = readlane_i(mycol, i + u);
                R::template load<VEC>(x[u], X + (int64_t)j * ldx + c);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float w = readlane_f(myval, i + u);
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, x[u][v], acc[v]);
            }
        }
        if (i < n) {  // 1 .. U-1 entries left: issue all loads, then all FMAs (wave-uniform branches)
            float x[U][VEC];
#pragma unroll
            for (int u = 0; u < U - 1; ++u) {
                if (i + u < n) {
                    const int j = readlane_i(mycol, i + u);
                    R::template load<VEC>(x[u], X + (int64_t)j * ldx + c);
                }
            }
#pragma unroll
            for (int u = 0; u < U - 1; ++u) {
                if (i + u < n) {
                    const float w = readlane_f(myval, i + u);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, x[u][v], acc[v]);
                }
            }
        }
    }
}

// filter.py:20-22: out = act(acc*beta + h0*alpha), with the add_eye diagonal folded in first.
// (every optional piece hangs on a wave-uniform null test of the policy's pointer: diag, the second result, the row map, the next
// iteration's scale)
template <typename R, int VEC>
__device__ __forceinline__ void epilogue_store(const typename R::Args &p, int64_t row, int c, bool active, float (&acc)[VEC]) {
    if (!active) return;
    if (R::diag(p)) {
        const float d = R::diag(p)[row];
        float xr[VEC];
        R::template load<VEC>(xr, R::X(p) + row * p.ldx + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = fmaf(d, xr[v], acc[v]);
    }
    if (R::has_out2(p)) {                          // second result of the same sums (see SpmmArgs::out2)
        const float f2 = p.out2_scale ? p.out2_scale[row] : 1.f;
        float o2[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) o2[v] = (acc[v] * p.beta2) * f2;
        int64_t row2 = row;
        if constexpr (R::GATHER_ORDER) {
            if (p.out2_rows) row2 = (int64_t)p.out2_rows[row];
        }
        R::template store2<VEC>(p, row2 * p.ldo2, c, o2);
    }
    float o[VEC];
    const int64_t orow = R::out_rows(p) ? (int64_t)R::out_rows(p)[row] : row;
    if (p.H0) {
        const int64_t hrow = p.map_h0 ? orow : row;   // gnx_spmm_rows: H0 is indexed like the output
        float h0[VEC];
        vload<VEC>(h0, p.H0 + hrow * p.ldh0 + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] = fmaf(acc[v], p.beta, h0[v] * p.alpha);   // spelled out: every kernel variant rounds alike
    } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] = acc[v] * p.beta;
    }
    if (p.act == GNX_ACT_RELU) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] = fmaxf(o[v], 0.f);
    }
    if (R::out_scale(p)) {
        const float os = R::out_scale(p)[row];
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] *= os;
    }
    R::template store<VEC>(p, orow * p.ldo, c, o);
}

// Which block of row slots this workgroup takes.  Default: its own index.  With a locality order (SpmmArgs::xcd_rows > 0) the index
// is remapped so that the workgroups the dispatcher places on one XCD (observed: round-robin, blockIdx % 8 -- a speed assumption,
// never a correctness one: the map is a bijection of the padded grid whatever the placement) take whole CHUNKS of xcd_chunk
// consecutive blocks, chunk j * 8 + x going to group x: an XCD then works on one contiguous stretch of the numbering at a time and
// its L2 holds THAT neighbourhood of H, instead of every L2 holding a slice of everything in flight (cdna_hip_programming.md T1).
// A chunk is one WINDOW's worth of slots: inside a window the rows are sorted by length, so any finer chunk hands the same XCDs the
// heavy part of every window (measured: chunks of a quarter window 2 x slower on orders with heavy heads), and contiguous eighths
// of the whole order hold unequal work (profiles/NOTES.md round 5).  The launcher pads the grid to a multiple of 8 chunks; padded
// blocks map past the last slot and leave.
__device__ __forceinline__ int64_t xcd_block(const SpmmArgs &p) {
    const uint32_t b = blockIdx.x;
    if (p.xcd_rows <= 0) return (int64_t)b;
    const uint32_t x = b & 7u, i = b >> 3, ch = p.xcd_chunk;
    return ((int64_t)(i / ch) * 8 + x) * ch + i % ch;
}

// Row slot (below p.n_rows) -> (row, beg, end) of a row kernel.  WAVE (one wave per row, wave-uniform slot): the rows in ascending
// order (their H0 / out rows stream), or the ascending list of the rows that have entries; `degree_order` is the f32 eval kernel's
// experiment.  Otherwise (G lanes per row): degree-binned slots, so that the rows of one wave have similar lengths, with slot_beg /
// slot_cnt read in slot order (coalesced, independent of the row_order load).
// The kernel itself tests slot < p.n_rows before the call and leaves afterwards on a long row and, under GNX_ACT_SKIP_EMPTY, on a row
// without entries.  Those three exits are not in here on purpose: with them inside (a bool result and reference outputs) the
// compiler merges the exit branches and moves kernarg loads, and the f32 kernels no longer match the ones measured so far.
struct RowSpan { int64_t row, beg, end; };
template <bool WAVE>
__device__ __forceinline__ RowSpan slot_row(const SpmmArgs &p, int64_t slot, bool degree_order = false) {
    if (WAVE) {
        const int64_t row = p.row_list ? (int64_t)__builtin_amdgcn_readfirstlane(p.row_list[slot])
                                       : (degree_order ? (int64_t)__builtin_amdgcn_readfirstlane(p.row_order[slot]) : slot);
        return {row, p.rowptr[row], p.rowptr[row + 1]};
    }
    const int64_t row = p.row_order ? (int64_t)p.row_order[slot] : slot;
    if (p.slot_beg) { const int64_t beg = p.slot_beg[slot]; return {row, beg, beg + p.slot_cnt[slot]}; }
    return {row, p.rowptr[row], p.rowptr[row + 1]};
}

// Chunk slot (below p.n_chunks) -> (chunk, row, beg, end) of a long-row kernel: chunks in column-window order (Csr::chunk_order),
// chunk k of a long row = its entries [k * long_chunk, (k + 1) * long_chunk).
struct ChunkSpan { int64_t chunk, row, beg, end; };
__device__ __forceinline__ ChunkSpan slot_chunk(const SpmmArgs &p, int64_t cslot) {
    const int64_t chunk = p.chunk_order ? (int64_t)p.chunk_order[cslot] : cslot;
    const int32_t li = p.chunk_long[chunk];
    const int64_t row = p.long_rows[li];
    const int64_t beg = p.rowptr[row] + (chunk - p.long_chunk_ptr[li]) * p.long_chunk;
    const int64_t rend = p.rowptr[row + 1];
    return {chunk, row, beg, beg + p.long_chunk < rend ? beg + p.long_chunk : rend};
}

// ---- long rows, second pass: the chunks' partial sums added in chunk order + the epilogue (shared by the eval and training paths) ----
template <typename R, int VEC>
__global__ __launch_bounds__(256) void k_spmm_long_reduce(const typename R::Args p) {
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t li = (int64_t)blockIdx.x * 4 + wib;
    if (li >= p.n_long) return;
    const int64_t row = p.long_rows[li];
    const int64_t cb = p.long_chunk_ptr[li], ce = p.long_chunk_ptr[li + 1];
    for (int c0 = 0; c0 < p.C; c0 += 64 * VEC) {
        const int c = c0 + lane * VEC;
        const bool active = c < p.C;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        if (active) {
            for (int64_t k = cb; k < ce; ++k) {  // chunk order
                float x[VEC];
                vload<VEC>(x, p.partial + k * (int64_t)p.C + c);
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] += x[v];
            }
        }
        epilogue_store<R, VEC>(p, row, c, active, acc);
    }
}

#define GNX_LAUNCH(kern, grid, ...) hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, __VA_ARGS__)

// One launch holds at most 2^32 work-items (the dispatch packet's grid size is 32 bits).  A wave per row reaches that at 67M rows,
// 32 lanes per row at 134M -- sizes a 288 GB card holds -- so the row kernels are dealt in pieces of at most 2^31 work-items
// (SpmmArgs::slot0 = first row slot of the piece; one piece for everything smaller).
template <typename Args, typename Kern>
void launch_row_pieces(Kern kern, const Args &p, int rows_per_block, int threads, hipStream_t s) {
    const int64_t per_launch = (((int64_t)1 << 31) / threads) * rows_per_block;
    for (int64_t r0 = 0; r0 < p.n_rows; r0 += per_launch) {
        Args q = p;
        q.slot0 = r0;
        const int64_t rows = p.n_rows - r0 < per_launch ? p.n_rows - r0 : per_launch;
        q.n_rows = r0 + rows;    // a piece ends where the next begins (padded blocks of the XCD map must not run on)
        unsigned grid = blocks_for(rows, rows_per_block);
        if (q.xcd_rows > 0 && rows < 64 * q.xcd_rows) q.xcd_rows = 0;   // a few windows only: they would not fill 8 XCDs evenly
        if (q.xcd_rows > 0) {     // xcd_block: whole chunks, the grid padded to 8 of them
            q.xcd_chunk = (uint32_t)((q.xcd_rows + rows_per_block - 1) / rows_per_block);
            const unsigned span = 8u * q.xcd_chunk;
            grid = (grid + span - 1) / span * span;
        }
        hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), 0, s, q);
    }
}
#define GNX_ROW_PIECES(kern, rows_per_block, threads) launch_row_pieces(kern, p, rows_per_block, threads, s)

// A structure's arrays and long-row plan into the launch arguments, GNX_ACT_SKIP_EMPTY moved from p.act into p.skip_empty, and the
// partial slab of its long rows (grown outside a capture only: GNX_ERR_UNSUPPORTED naming gnx_graph_reserve otherwise).
[[maybe_unused]] int bind_csr(gnx_graph *g, const Csr &m, SpmmArgs &p, hipStream_t s) {
    p.rowptr = m.rowptr; p.colidx = m.colidx; p.n_rows = m.n_rows; p.n_nonempty = m.n_nonempty; p.nonempty_rows = m.nonempty_rows; p.row_list = nullptr;
    p.slot_beg = m.slot_beg; p.slot_cnt = m.slot_cnt;
    p.long_rows = m.long_rows; p.long_chunk_ptr = m.long_chunk_ptr; p.chunk_long = m.chunk_long;
    p.row_order = m.row_order;
    p.xcd_rows = m.order_window;
    p.chunk_order = m.chunk_order;
    p.tune = 0;
    p.n_long = m.n_long; p.n_chunks = m.n_chunks; p.long_row = m.long_row; p.long_chunk = m.long_chunk;
    p.partial = nullptr;
    p.skip_empty = (p.act & GNX_ACT_SKIP_EMPTY) != 0 && p.diag == nullptr;
    p.act &= ~GNX_ACT_SKIP_EMPTY;
    if (m.n_rows > 0 && m.n_long > 0) {
        int rc = ensure_partial(g, (size_t)m.n_chunks * (size_t)p.C * sizeof(float), s);
        if (rc != GNX_OK) return rc;
        p.partial = g->partial;
    }
    return GNX_OK;
}

// The tail of every SpMM entry: p bound to structure m, nothing launched on a structure without rows, `pick(p)` launches and returns
// the name gnx_graph_last_kernel reports.
template <typename Args, typename Pick>
int launch_bound(gnx_graph *g, const Csr &m, Args &p, hipStream_t s, Pick pick) {
    int rc = bind_csr(g, m, p, s);
    if (rc != GNX_OK) return rc;
    if (m.n_rows == 0) return GNX_OK;
    g->last_hint_hot = 0;          // (set again by a launch that gathers through the hinted columns: launch_spmm)
    g->last_kernel = pick(p);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

// GNX_ACT_SKIP_EMPTY in the row launchers: the sub-wave kernels walk the rows through row_order, whose trailing slots are exactly the
// rows without entries -- those slots are not launched at all (on the R-MAT workloads 60 % of the rows: no wave, no row-pointer
// read); the one-wave-per-row kernels keep the rows in ascending order and walk the ascending list of the rows that have entries.
[[maybe_unused]] void trim_empty_rows(SpmmArgs &p, int lanes) {
    if (!p.skip_empty || p.n_nonempty >= p.n_rows) return;
    if (lanes <= 32 && p.row_order != nullptr) p.n_rows = p.n_nonempty;
    else if (lanes > 32 && p.nonempty_rows != nullptr) { p.row_list = p.nonempty_rows; p.n_rows = p.n_nonempty; }
}

// ---- dispatch: the per-lane vector and the lanes per row as template arguments, and the names gnx_graph_last_kernel reports ------
template <int N> using IntC = std::integral_constant<int, N>;

// f(IntC<VEC>) for the width pick_vec chose
template <typename R, typename F>
auto with_vec(int vec, F &&f) {
    if constexpr (R::MAX_VEC == 8) {
        if (vec == 8) return f(IntC<8>{});
    }
    if (vec == 4) return f(IntC<4>{});
    if (vec == 2) return f(IntC<2>{});
    return f(IntC<1>{});
}

enum RowClass { ROWS_NONE, ROWS_WAVE, ROWS_G32, ROWS_G16, ROWS_G8, ROWS_G4 };

// The class ladder below one wave per row: f(IntC<G>) for the G lanes a row of `lanes` per-lane vectors runs on (256 / G rows per
// block).  Rows of up to 4 lanes run on 8-lane groups as well (the lanes beyond the row's width share the index fetch / the draws)
// unless G4: in the chunk kernels the group width is also how a chunk's entries are dealt to sub-groups, i.e. the long rows'
// summation order, which the eval and the training kernels of the same width share bit for bit.
template <bool G4, typename F>
RowClass with_group(int lanes, F &&f) {
    if (lanes > 16) { f(IntC<32>{}); return ROWS_G32; }
    if (lanes > 8)  { f(IntC<16>{}); return ROWS_G16; }
    if constexpr (G4) {
        if (lanes <= 4) { f(IntC<4>{}); return ROWS_G4; }
    }
    f(IntC<8>{});
    return ROWS_G8;
}

// "spmm_" class ["+long" | "+chunks"] ["_drop" ["_entries"]] ["_bf16" | "_ord"]: every name reported so far, byte for byte, from one scheme.
// (A launch that gathers through the handle's hinted columns reports the name of its class unchanged -- clients and tests compare
// these names -- and gnx_graph_gather_hints says how many hot rows the last launch ran with.)
// (The table spells out the whole product; most of its combinations -- "spmm_wave+chunks", "spmm_group4_drop" -- cannot be reported.)
enum NameHubs { HUBS_NONE, HUBS_LONG, HUBS_CHUNKS };      // hub rows: none (or not named), separate chunk launches, chunks in the row launch
enum NameMode { MODE_EVAL, MODE_DROP, MODE_DROP_ENTRIES };
#define GNX_NAMES6(mid, tail) {"spmm_none" mid tail, "spmm_wave" mid tail, "spmm_group32" mid tail, "spmm_group16" mid tail, "spmm_group8" mid tail, "spmm_group4" mid tail}
#define GNX_NAMES3(tail) {GNX_NAMES6("", tail), GNX_NAMES6("+long", tail), GNX_NAMES6("+chunks", tail)}
#define GNX_NAMES(tail) {GNX_NAMES3(tail), GNX_NAMES3("_drop" tail), GNX_NAMES3("_drop_entries" tail)}
[[maybe_unused]] const char *const kKernelNames[3][3][3][6] = {GNX_NAMES(""), GNX_NAMES("_bf16"), GNX_NAMES("_ord")};
#undef GNX_NAMES
#undef GNX_NAMES3
#undef GNX_NAMES6

template <typename R>
const char *kernel_name(RowClass rows, NameMode mode, NameHubs hubs) {
    if (hubs == HUBS_LONG && !R::NAMES_LONG) hubs = HUBS_NONE;
    return kKernelNames[R::GATHER_ORDER ? 2 : R::BF16][mode][hubs][rows];
}

// the operands of one launch into its arguments: the gathered rows, the mix and the main result (`out_bf16` where the policy has the choice)
template <typename R>
void set_operands(typename R::Args &p, const typename R::Elem *X, int64_t ldx, const float *H0, int64_t ldh0, float beta, float alpha, int act,
                  typename R::Out *out, int out_bf16, int64_t ldo, int64_t C) {
    R::bind_X(p, X); p.ldx = ldx; p.H0 = H0; p.ldh0 = ldh0; p.beta = beta; p.alpha = alpha; p.act = act;
    R::bind_out(p, out, out_bf16); p.ldo = ldo; p.C = (int)C;
}

// the operand checks every SpMM entry starts with (the bf16 training entries make them BEFORE they look at the handle, so that they
// can be exercised without a device)
[[maybe_unused]] int check_operands(const char *fn, const void *X, int64_t ldx, int64_t C, const float *H0, int64_t ldh0, const void *out,
                                    int64_t ldo) {
    GNX_CHECK_ARG(C >= 1 && C <= (1 << 20), "%s: feature width %lld not in [1, 2^20]", fn, (long long)C);
    GNX_CHECK_ARG(X != nullptr && out != nullptr, "%s: NULL X/out", fn);
    GNX_CHECK_ARG(ldx >= C && ldo >= C && (H0 == nullptr || ldh0 >= C || ldh0 == 0), "%s: leading dimension smaller than C", fn);
    GNX_CHECK_ARG(X != out, "%s: out must not alias X", fn);
    return GNX_OK;
}

[[maybe_unused]] int check_common(const char *fn, gnx_graph *g, const void *X, int64_t ldx, int64_t C, const float *H0, int64_t ldh0,
                                  const void *out, int64_t ldo) {
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    return check_operands(fn, X, ldx, C, H0, ldh0, out, ldo);
}

}  // namespace
