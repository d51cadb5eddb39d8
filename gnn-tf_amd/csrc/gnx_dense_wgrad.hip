// The weight gradient of the dense transform (gnx_dense.hip) on gfx950 matrix cores.
//
//   gnx_dense_wgrad  dW[F, O] = X^T . G      what tf.GradientTape derives for gnntf/core/nn/layers.py:136
//   gnx_dense_wgrad_drop  dW = drop_in(X)^T . G   the same behind gnx_dense_drop: the DROP form of both kernels makes the input mask again
//
// k_wgrad_acc (accumulators stationary: tall inputs, widths multiples of 4) or k_wgrad_mfma (every other shape) leaves one partial dW
// per row slab in the caller's scratch; k_sum_slabs adds them in slab order, as it does for gnx_gcnii_wgrad (gnx_gcnii.hip).
#include "gnx_dense_device.h"
#include "gnx_layer_device.h"

namespace {

// The input mask of the DROP instantiations (gnx_dense_wgrad_drop: dW = drop_in(X)^T . G, the mask of gnx_dense_drop made again from its
// triple -- drop_values, gnx_layer_device.h); the instantiations without DROP take an empty struct in its place.
template <bool DROP> struct WgradMask {};
template <> struct WgradMask<true> { DropFuse din; };

// ---- dW[F, O] = X^T . G, a reduction over the N rows, in panels ---------------------------------------------------------------
// M = F, N = O, K = rows.  grid.x = row slabs, grid.y = panels of 256 features, grid.z = panels of 16 NT outputs.  A block
// stages 32-row tiles of X (its 256 features) and G (its outputs) in LDS with coalesced 16-byte loads; wave w owns features
// [64 w, 64 w + 64) of the panel as 4 x NT accumulator tiles: A[m = feature][k = row] and B[k = row][n = output] fragments are
// read from LDS (row stride = 16 mod 32 banks, so the two k-groups of a half-wave hit disjoint banks).  Every slab writes its
// partial dW; a second kernel adds the slabs in order (fixed order: reproducible, no float atomics).
// DROP: the tile of X is masked between its global load and its LDS store.
template <int NT, bool DROP = false>
__global__ __launch_bounds__(256) void k_wgrad_mfma(const float *__restrict__ X, int64_t ldx, const float *__restrict__ G, int64_t ldg,
                                                     int64_t n, int F, int O, int64_t rows_per_slab, bool aligned,
                                                     float *__restrict__ partial, const WgradMask<DROP> mask) {
    constexpr int R = 32, XS = 256 + 16, GS = 16 * NT + 16;
    __shared__ float Xs[R * XS];
    __shared__ float Gs[R * GS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int f0 = blockIdx.y * 256, o0 = blockIdx.z * 16 * NT;
    const int64_t r_beg = (int64_t)blockIdx.x * rows_per_slab;
    const int64_t r_end = r_beg + rows_per_slab < n ? r_beg + rows_per_slab : n;
    [[maybe_unused]] uint64_t in_stream = 0;
    if constexpr (DROP) in_stream = drop_stream(mask.din);
    f32x4 acc[4][NT];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[ft][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t r0 = r_beg; r0 < r_end; r0 += R) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < R * 64; idx += 256) {                 // X tile: 32 rows x 256 features
            const int rr = idx / 64, cc = (idx % 64) * 4;
            const int64_t row = r0 + rr;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row < r_end) {
                const float *__restrict__ src = X + row * ldx + f0 + cc;
                if (aligned && f0 + cc + 3 < F) v = *reinterpret_cast<const f32x4 *>(src);
                else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) if (f0 + cc + t < F) v[t] = src[t];
                }
                if constexpr (DROP) {
                    if (f0 + cc < F) {                                          // (columns past F hold zeros)
                        float x[4] = {v[0], v[1], v[2], v[3]};
                        drop_values<4>(mask.din, in_stream, row, f0 + cc, x);
                        v = f32x4{x[0], x[1], x[2], x[3]};
                    }
                }
            }
            *reinterpret_cast<f32x4 *>(Xs + rr * XS + cc) = v;
        }
        for (int idx = threadIdx.x; idx < R * 4 * NT; idx += 256) {             // G tile: 32 rows x 16 NT outputs
            const int rr = idx / (4 * NT), cc = (idx % (4 * NT)) * 4;
            const int64_t row = r0 + rr;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row < r_end) {
                const float *__restrict__ src = G + row * ldg + o0 + cc;
                if (aligned && o0 + cc + 3 < O) v = *reinterpret_cast<const f32x4 *>(src);
                else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) if (o0 + cc + t < O) v[t] = src[t];
                }
            }
            *reinterpret_cast<f32x4 *>(Gs + rr * GS + cc) = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < R / 4; ++kk) {
            const float *__restrict__ xrow = Xs + (4 * kk + g) * XS + 64 * wave + c;
            const float *__restrict__ grow = Gs + (4 * kk + g) * GS + c;
            float b[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = grow[16 * nt];
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) {
                const float a = xrow[16 * ft];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[ft][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[nt], acc[ft][nt], 0, 0, 0);
            }
        }
    }
    float *__restrict__ out = partial + (int64_t)blockIdx.x * F * O;
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int o = o0 + 16 * nt + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = f0 + 64 * wave + 16 * ft + 4 * g + r;
                if (f < F && o < O) out[(int64_t)f * O + o] = acc[ft][nt][r];
            }
        }
}

// ---- the same gradient with the ACCUMULATORS stationary: every wave keeps a whole F x O partial in its registers --------------------
// For F x O <= 16384 (256 x 64, 128 x 128, 64 x 64, ...: the layers of the path) one wave's 512 registers hold the complete result,
// (F / 16) x (O / 16) accumulator tiles (wider layers: one panel of at most 128 outputs x 16384 / 128 features per wave, every slab of
// rows walked once per panel; widths that are not 32 / 64 / 128 / 256 are padded inside the LDS image only).  A wave then needs
// nobody: it owns a slab of rows, streams X[rows, :] and G[rows, :] through a
// private LDS ring by LDS-DMA (whole lines, no VGPR staging, RING - 1 stages in flight behind a counted s_waitcnt vmcnt), and per 4 rows
// reads F / 16 + O / 16 single-word fragments for (F / 16) (O / 16) MFMAs -- no barrier anywhere, nothing recomputed, and shapes narrower
// than k_wgrad_mfma's 256-feature panel waste nothing.  The LDS image is lane-linear (an LDS-DMA cannot scatter), so the 16-byte pieces
// of ODD rows are swapped in groups of four (piece ^ 4) on the source address: a half-wave's fragment read -- 2 rows x 16 consecutive
// words -- then covers all 32 banks once.  G is the MFMA's A operand: a lane ends up with four consecutive outputs of one feature row
// (16-byte stores of the partial).  The partials of the waves are added in wave order by k_sum_slabs (fixed order: reproducible).
template <int MT, int NT> struct WgradAcc {
    static constexpr int F = 16 * MT, O = 16 * NT, R = 8;                 // rows per stage
    static constexpr int XI = R * F / 256, GI = R * O / 256, NI = XI + GI; // LDS-DMA instructions per stage
    static constexpr int STAGE = R * (F + O);                             // floats
    static constexpr int RING_FIT = (36 << 10) / (STAGE * 4);
    static constexpr int RING = RING_FIT > 8 ? 8 : (RING_FIT < 2 ? 2 : RING_FIT);
    static_assert(NI * (RING - 1) <= 63, "vmcnt is a 6-bit counter");
    static_assert(MT * NT <= 64, "the accumulators must fit the register file");
};

// DROP: the single-word X fragments are masked as they are read from the ring (each element of X is read by one lane, once per panel).
template <int MT, int NT, bool DROP = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_wgrad_acc(const float *__restrict__ X, uint32_t x_pitch, int f_all, const float *__restrict__ G, uint32_t g_pitch, int o_all, uint32_t n,
                 uint32_t rows_per_wave, uint32_t f_panels, uint32_t panels, float *__restrict__ partial, const WgradMask<DROP> mask) {
    using Cfg = WgradAcc<MT, NT>;
    // F x O: the PANEL this wave accumulates (padded to whole 16-column tiles of a power-of-two count).  Columns past the real widths
    // stage a piece that exists (piece 0 of the row) and feed only accumulator cells that are never stored.
    // Block -> (row slabs, panel): the panels of one group of slabs are 8 blocks apart, i.e. dispatched together AND on the same XCD
    // (blocks go round the 8 XCDs), so the rows of G that every panel reads again come out of that XCD's L2.
    constexpr int F = Cfg::F, O = Cfg::O, R = Cfg::R, RING = Cfg::RING, STAGE = Cfg::STAGE;
    const uint32_t bgroup = blockIdx.x / (8 * panels), brem = blockIdx.x % (8 * panels);
    const uint32_t slab_block = bgroup * 8 + brem % 8;
    const int f0 = (int)((brem / 8) % f_panels) * F, o0 = (int)((brem / 8) / f_panels) * O;       // panels = feature panels x output panels
    const uint32_t f_pieces = (uint32_t)((f_all - f0 < F ? f_all - f0 : F) / 4), o_pieces = (uint32_t)((o_all - o0 < O ? o_all - o0 : O) / 4);
    X += f0;
    G += o0;
    extern __shared__ float lds[];                                // [4 waves][RING][STAGE: R rows of X | R rows of G]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 15, g = lane >> 4;
    const uint32_t wid = slab_block * 4 + wave;
    const uint32_t r_beg = wid * rows_per_wave;
    if (r_beg >= n) return;                                       // (whole waves; there is no barrier in this kernel)
    const uint32_t r_end = r_beg + rows_per_wave < n ? r_beg + rows_per_wave : n;
    const uint32_t n_stages = (r_end - r_beg + R - 1) / R;
    float *__restrict__ ring = lds + wave * (RING * STAGE);
    const char *__restrict__ Xb = reinterpret_cast<const char *>(X);
    const char *__restrict__ Gb = reinterpret_cast<const char *>(G);

    // staging: instruction i of the X part fills slots 64 i .. 64 i + 63 of the stage's X image (slot = 16-byte piece, F / 4 per row)
    uint32_t pf = 0, pf_slot = 0;
    auto issue_next = [&]() {
        const uint32_t row0 = r_beg + (pf < n_stages ? pf : n_stages - 1) * R;      // past the slab: the last stage again, which nobody reads
        float *dst = ring + pf_slot * STAGE;
        // `count` instructions fill the image of R rows of `width` floats at `to`; columns past the real width (`pieces`) stage piece 0
        auto part = [&](int count, int width, const char *__restrict__ base, uint32_t pitch, uint32_t pieces, float *to) {
#pragma unroll
            for (int i = 0; i < count; ++i) {
                const uint32_t q = 64 * i + lane, r = q / (width / 4);
                uint32_t piece = (q % (width / 4)) ^ (4 * (r & 1));
                piece = piece < pieces ? piece : 0;
                uint32_t row = row0 + r;
                row = row < n ? row : n - 1;                      // rows past the end read a valid row; their fragments are zeroed
                __builtin_amdgcn_global_load_lds(reinterpret_cast<const float *>(base + (uint64_t)row * pitch + 16 * piece), to + i * 256, 16, 0, 0);
            }
        };
        part(Cfg::XI, F, Xb, x_pitch, f_pieces, dst);
        part(Cfg::GI, O, Gb, g_pitch, o_pieces, dst + R * F);
        ++pf;
        pf_slot = pf_slot + 1 == RING ? 0 : pf_slot + 1;
    };
    // fragments of k step s (rows 4 s + g): word 16 t + c of the row sits in piece group t ^ (g & 1)
    const int flip = g & 1;
    const int x_lane = g * F + c, g_lane = g * O + c;
    [[maybe_unused]] uint64_t in_stream = 0;
    if constexpr (DROP) in_stream = drop_stream(mask.din);
    f32x4 acc[MT][NT];
#pragma unroll
    for (int ft = 0; ft < MT; ++ft)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[ft][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // `row0` (DROP): the first row of the stage in `slot`
    auto multiply = [&](auto masked, uint32_t slot, uint32_t valid_rows, [[maybe_unused]] uint32_t row0) {
        const float *__restrict__ Xs = ring + slot * STAGE + x_lane;
        const float *__restrict__ Gs = ring + slot * STAGE + R * F + g_lane;
#pragma unroll
        for (int s = 0; s < R / 4; ++s) {
            float a[MT], b[NT];
#pragma unroll
            for (int ft = 0; ft < MT; ++ft) a[ft] = Xs[4 * s * F + 16 * (ft ^ flip)];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = Gs[4 * s * O + 16 * (nt ^ flip)];
            if constexpr (DROP) {                                 // a[ft] = X[row0 + 4 s + g][f0 + 16 ft + c]; the row's round of the hash is shared
#pragma unroll
                for (int ft = 0; ft < MT; ++ft) {
                    float x[1] = {a[ft]};
                    drop_values<1>(mask.din, in_stream, (int64_t)(row0 + 4 * s + g), f0 + 16 * ft + c, x);
                    a[ft] = x[0];
                }
            }
            if constexpr (decltype(masked)::value) {
                if ((uint32_t)(4 * s + g) >= valid_rows) {        // 0 x 0: a row past the slab adds nothing, whatever the row that was read holds
#pragma unroll
                    for (int ft = 0; ft < MT; ++ft) a[ft] = 0.f;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) b[nt] = 0.f;
                }
            }
#pragma unroll
            for (int ft = 0; ft < MT; ++ft)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[ft][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[nt], a[ft], acc[ft][nt], 0, 0, 0);
        }
    };
#pragma unroll
    for (int s0 = 0; s0 < RING - 1; ++s0) issue_next();
    uint32_t slot = 0;
    for (uint32_t st = 0; st + 1 < n_stages; ++st) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // the fragments of the stage whose slot is restaged next have been read
        issue_next();
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(Cfg::NI * (RING - 1)) : "memory");    // all but the youngest RING - 1 stages: stage st has landed
        multiply(std::false_type{}, slot, R, r_beg + st * R);
        slot = slot + 1 == RING ? 0 : slot + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // (also: nothing of this wave may still be writing LDS when it retires)
    multiply(std::true_type{}, slot, r_end - (r_beg + (n_stages - 1) * R), r_beg + (n_stages - 1) * R);
    // D layout with G as the A operand: lane (c, g), register r -> feature 16 ft + c, output 16 nt + 4 g + r
    float *__restrict__ out = partial + (uint64_t)wid * ((uint32_t)f_all * (uint32_t)o_all) + (uint32_t)f0 * (uint32_t)o_all + o0;
#pragma unroll
    for (int ft = 0; ft < MT; ++ft)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            if (f0 + 16 * ft + c < f_all && o0 + 16 * nt + 4 * g < o_all)
                *reinterpret_cast<f32x4 *>(out + (16 * ft + c) * o_all + 16 * nt + 4 * g) = acc[ft][nt];
}

template <int MT, int NT, bool DROP>
int launch_wgrad_acc(const float *X, int64_t ldx, int64_t F, const float *G, int64_t ldg, int64_t O, int64_t n, float *work, int64_t max_slabs,
                     int64_t *n_slabs, const WgradMask<DROP> &mask, hipStream_t s) {
    using Cfg = WgradAcc<MT, NT>;
    const size_t lds_bytes = (size_t)4 * Cfg::RING * Cfg::STAGE * sizeof(float);
    const int cus = persistent_launch<k_wgrad_acc<MT, NT, DROP>>();
    if (cus < 0) return cus;
    const int64_t f_panels = (F + Cfg::F - 1) / Cfg::F, panels = f_panels * ((O + Cfg::O - 1) / Cfg::O);
    int64_t waves = std::min<int64_t>(std::max<int64_t>((int64_t)cus * 4 / panels, 64), max_slabs);        // row slabs; every slab is walked once per panel
    int64_t rows_per_wave = (n + waves - 1) / waves;
    rows_per_wave = std::max<int64_t>((rows_per_wave + Cfg::R - 1) / Cfg::R * Cfg::R, 8 * Cfg::R);
    waves = (n + rows_per_wave - 1) / rows_per_wave;
    const int64_t slab_blocks = (waves + 3) / 4, grid = (slab_blocks + 7) / 8 * 8 * panels;
    hipLaunchKernelGGL((k_wgrad_acc<MT, NT, DROP>), dim3((unsigned)grid), dim3(256), lds_bytes, s, X, (uint32_t)(ldx * 4), (int)F, G, (uint32_t)(ldg * 4), (int)O,
                       (uint32_t)n, (uint32_t)rows_per_wave, (uint32_t)f_panels, (uint32_t)panels, work, mask);
    *n_slabs = waves;
    return GNX_OK;
}

// Whole aligned rows, F and O multiples of 4: the result is cut into panels of FP features x OP outputs, FP x OP <= 16384, each of which
// one wave holds (OP = 32 / 64 / 128 >= O where that exists; FP = 16384 / OP, at most 256, narrower for narrow inputs); widths that
// are not a power of two are padded inside the LDS image.  GNX_OK: launched; < 0: not taken, the panel kernel runs.
template <bool DROP>
int wgrad_acc_dispatch(const float *X, int64_t ldx, const float *G, int64_t ldg, int64_t n, int64_t F, int64_t O, bool aligned, float *work,
                       int64_t max_slabs, int64_t *n_slabs, const WgradMask<DROP> &mask, hipStream_t s) {
    if (!aligned || n < 16 * 1024 || n >= (1ll << 31) || ldx >= (1ll << 30) || ldg >= (1ll << 30) || F % 4 || O % 4 || F * O >= (1ll << 31) || max_slabs < 64)
        return -1;
    const int op = O <= 32 ? 32 : O <= 64 ? 64 : 128;
    int fp = std::min(16384 / op, 256);
    while (fp > 32 && fp / 2 >= F) fp /= 2;                                   // a narrow input does not need the widest panel
    const int64_t panels = ((F + fp - 1) / fp) * ((O + op - 1) / op);
    if (panels > 64) return -1;                                                // (very wide layers: every slab would be walked too often)
#define GNX_WGRAD_ACC(MT_, NT_) if (fp == 16 * MT_ && op == 16 * NT_) return launch_wgrad_acc<MT_, NT_, DROP>(X, ldx, F, G, ldg, O, n, work, max_slabs, n_slabs, mask, s)
    GNX_WGRAD_ACC(2, 2); GNX_WGRAD_ACC(2, 4); GNX_WGRAD_ACC(2, 8);
    GNX_WGRAD_ACC(4, 2); GNX_WGRAD_ACC(4, 4); GNX_WGRAD_ACC(4, 8);
    GNX_WGRAD_ACC(8, 2); GNX_WGRAD_ACC(8, 4); GNX_WGRAD_ACC(8, 8);
    GNX_WGRAD_ACC(16, 2); GNX_WGRAD_ACC(16, 4);
#undef GNX_WGRAD_ACC
    return -1;
}

// slabs [group * per, min(group * per + per, n_slabs)) added in index order into out[group]; blockIdx.y = group.  One group of all the
// slabs is the whole sum; smaller groups are the first level of a two-level sum (fixed association: reproducible)
__global__ void k_sum_slabs(const float *__restrict__ partial, int64_t n_slabs, int64_t per, int64_t elems, float *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= elems) return;
    const int64_t s0 = (int64_t)blockIdx.y * per, s1 = s0 + per < n_slabs ? s0 + per : n_slabs;
    float acc = 0.f;
    for (int64_t s = s0; s < s1; ++s) acc += partial[s * elems + e];
    out[(int64_t)blockIdx.y * elems + e] = acc;
}

}  // namespace

namespace gnx {

// the [elems] partials of n_slabs row slabs added in slab order into out: the last pass of gnx_dense_wgrad and of gnx_gcnii_wgrad
void sum_slabs(const float *partial, int64_t n_slabs, int64_t elems, float *out, hipStream_t s) {
    hipLaunchKernelGGL(k_sum_slabs, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, partial, n_slabs, n_slabs, elems, out);
}

}  // namespace gnx

namespace {

// what gnx_dense_wgrad and gnx_dense_wgrad_drop check before anything is read or launched
int check_wgrad_args(const char *fn, const float *d_X, int64_t ldx, const float *d_G, int64_t ldg, int64_t n, int64_t F, int64_t O, float *d_dW,
                     float *d_work, int64_t work_floats) {
    GNX_CHECK_ARG(n >= 0 && F >= 1 && O >= 1 && F <= (1 << 20) && O <= (1 << 20), "%s: bad sizes", fn);
    GNX_CHECK_ARG(ldx >= F && ldg >= O, "%s: leading dimension smaller than the row", fn);
    GNX_CHECK_ARG(d_dW != nullptr, "%s: NULL output", fn);
    if (n == 0) return GNX_OK;
    GNX_CHECK_ARG(d_X && d_G, "%s: NULL input", fn);
    GNX_CHECK_ARG(d_work != nullptr && work_floats / (F * O) >= 1, "%s: the scratch must hold at least F * O floats", fn);
    return GNX_OK;
}

// gnx_dense_wgrad and gnx_dense_wgrad_drop (DROP: X under `mask`) behind their checks: one host path -- the same slabs, wave -> slab
// assignment and summation order
template <bool DROP>
int dense_wgrad(const float *d_X, int64_t ldx, const float *d_G, int64_t ldg, int64_t n, int64_t F, int64_t O, float *d_dW,
                float *d_work, int64_t work_floats, const WgradMask<DROP> &mask, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        GNX_HIP(hipMemsetAsync(d_dW, 0, (size_t)F * O * sizeof(float), s));
        return GNX_OK;
    }
    // row slabs: as many as the scratch holds (each slab leaves an F x O partial), at least 256 rows each, at most 2048 slabs
    const int64_t fo = F * O;
    int64_t max_slabs = work_floats / fo;
    if (max_slabs > 2048) max_slabs = 2048;
    int64_t rows_per_slab = (n + max_slabs - 1) / max_slabs;
    if (rows_per_slab < 256) rows_per_slab = 256;
    rows_per_slab = (rows_per_slab + 31) / 32 * 32;
    const int64_t n_slabs = (n + rows_per_slab - 1) / rows_per_slab;
    const bool al = ldx % 4 == 0 && ldg % 4 == 0 && aligned(d_X, 16) && aligned(d_G, 16);
    int64_t waves = 0;                                // k_wgrad_acc's slabs  (tuning builds: GNX_WGRAD_ACC=0 keeps the panel kernel)
    if (tuning_switch("GNX_WGRAD_ACC") && aligned(d_work, 16) &&
        wgrad_acc_dispatch<DROP>(d_X, ldx, d_G, ldg, n, F, O, al, d_work, max_slabs, &waves, mask, s) == GNX_OK) {
        // the waves' partials, added in wave order: in groups of 32 first when the scratch has room for the group sums (a sum over a
        // thousand slabs of a few thousand elements is otherwise a launch of a few blocks walking a long chain each)
        const int64_t per = 32, groups = (waves + per - 1) / per;
        if (waves > 64 && work_floats >= (waves + groups) * fo) {
            float *tmp = d_work + waves * fo;
            hipLaunchKernelGGL(k_sum_slabs, dim3((unsigned)((fo + 255) / 256), (unsigned)groups), dim3(256), 0, s, d_work, waves, per, fo, tmp);
            sum_slabs(tmp, groups, fo, d_dW, s);
        } else {
            sum_slabs(d_work, waves, fo, d_dW, s);
        }
    } else {
        const int nt_all = (int)((O + 15) / 16);
        const int NTsel = nt_all >= 4 ? 4 : (nt_all >= 2 ? 2 : 1);
        dim3 grid((unsigned)n_slabs, (unsigned)((F + 255) / 256), (unsigned)((nt_all + NTsel - 1) / NTsel));
        if (NTsel == 4)      hipLaunchKernelGGL((k_wgrad_mfma<4, DROP>), grid, dim3(256), 0, s, d_X, ldx, d_G, ldg, n, (int)F, (int)O, rows_per_slab, al, d_work, mask);
        else if (NTsel == 2) hipLaunchKernelGGL((k_wgrad_mfma<2, DROP>), grid, dim3(256), 0, s, d_X, ldx, d_G, ldg, n, (int)F, (int)O, rows_per_slab, al, d_work, mask);
        else                 hipLaunchKernelGGL((k_wgrad_mfma<1, DROP>), grid, dim3(256), 0, s, d_X, ldx, d_G, ldg, n, (int)F, (int)O, rows_per_slab, al, d_work, mask);
        sum_slabs(d_work, n_slabs, fo, d_dW, s);
    }
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

}  // namespace

extern "C" {

int gnx_dense_wgrad(const float *d_X, int64_t ldx, const float *d_G, int64_t ldg, int64_t n, int64_t F, int64_t O, float *d_dW,
                    float *d_work, int64_t work_floats, void *stream) {
    const int rc = check_wgrad_args("gnx_dense_wgrad", d_X, ldx, d_G, ldg, n, F, O, d_dW, d_work, work_floats);
    if (rc != GNX_OK) return rc;
    return dense_wgrad<false>(d_X, ldx, d_G, ldg, n, F, O, d_dW, d_work, work_floats, WgradMask<false>{}, stream);
}

int gnx_dense_wgrad_drop(gnx_graph_t g, const float *d_X, int64_t ldx, const float *d_G, int64_t ldg, int64_t n, int64_t F, int64_t O,
                         double in_p, uint64_t in_seed, uint64_t in_stream, float *d_dW, float *d_work, int64_t work_floats, void *stream) {
    // (the handle is read -- for its dropout counter -- only once every other argument has passed)
    GNX_CHECK_ARG(g != nullptr, "gnx_dense_wgrad_drop: NULL handle");
    GNX_CHECK_ARG(in_p >= 0.0 && in_p < 1.0, "gnx_dense_wgrad_drop: dropout rate %g outside [0, 1)", in_p);
    int rc = check_wgrad_args("gnx_dense_wgrad_drop", d_X, ldx, d_G, ldg, n, F, O, d_dW, d_work, work_floats);
    if (rc != GNX_OK) return rc;
    WgradMask<true> mask{};
    rc = make_feat_drop("gnx_dense_wgrad_drop", g, in_p, in_seed, in_stream, mask.din);
    if (rc != GNX_OK) return rc;
    if (mask.din.thr == 0)                           // no mask: the plain gradient, nothing hashed
        return dense_wgrad<false>(d_X, ldx, d_G, ldg, n, F, O, d_dW, d_work, work_floats, WgradMask<false>{}, stream);
    return dense_wgrad<true>(d_X, ldx, d_G, ldg, n, F, O, d_dW, d_work, work_floats, mask, stream);
}

}  // extern "C"
