// The NGCF layer (gcn.py:116-135) at C_in = 128 on gfx950: the SpMM of gnx_spmm.hip, then ONE row-local launch (gnx_step_wide_ngcf).
//   k_ngcf_rows        everything of the layer behind the gather: both transforms on the matrix cores with the rows' X and A = A_hat . X
//                      held as MFMA operand fragments in registers, the gate words, the activations' sum, the mask and the row norm
//   gnx_step_wide_ngcf gnx_spmm into d_agg (or d_work), then k_ngcf_rows over all n rows
// Why two launches and not k_spmm_ngcf at a fourth width: profiles/NOTES.md, "NGCF layer at width 128" (eight waves per CU cannot keep
// the gathers in flight beside 128 KiB of weights; the wide SpMM alone already runs at the random-gather rate).
// The constants of the launch shape it shares with k_ngcf_rows_back, the launch and the dispatch of the block count stand in
// gnx_ngcf_wide_device.h (which also says why the kernel keeps its own text); the pieces of a finished value and the entry's checks in
// gnx_ngcf_device.h.
#include "gnx_ngcf_device.h"
#include "gnx_ngcf_wide_device.h"

namespace {

constexpr int WIDE_KK = WIDE_C / 4;      // the MFMA steps of four k

struct NgcfRows {
    const float *X; int64_t ldx; const float *A; int64_t n;       // A [n, 128] contiguous
    const float *W1; int64_t ldw1; const float *W2; int64_t ldw2; int C_out;
    const float *b1, *b2; int act;
    float *out; int64_t ldo; uint32_t *gate; float *rnorm; bool normalize, vec_out;
    DropFuse feat;
};

// Word w of one product's gate bits for row 4 g + r of the tile: a wave ballot of (d[nt][r] > 0) holds bit 16 g' + cc for row 4 g' + r,
// column 16 nt + cc; the word takes the 16 bits of the lane's g from the blocks nt = 2 w and 2 w + 1.  Every lane of the wave calls it.
template <int NTO>
__device__ __forceinline__ uint32_t ngcf_rows_word(const f32x4 (&d)[NTO], int w, int r, int g) {
    const unsigned long long lo = __ballot(d[2 * w][r] > 0.f);
    unsigned long long hi = 0ull;
    if (2 * w + 1 < NTO) hi = __ballot(d[2 * w + 1 < NTO ? 2 * w + 1 : 0][r] > 0.f);
    return (uint32_t)((lo >> (16 * g)) & 0xffffull) | ((uint32_t)((hi >> (16 * g)) & 0xffffull) << 16);
}

// One block of eight waves per CU, persistent: block b takes the tiles 8 b + w, 8 (b + gridDim.x) + w, .. (tile t: rows 16 t .. 16 t + 15)
// with its wave w.  Which wave finishes a row changes no bit of it: nothing below depends on the tile but the row ids.
//   weights      W1 and W2 [128, C_out] once per block into LDS, f32, in the order the B operand is read: float (kk NTO + nt) 64 + lane
//                is W[4 kk + (lane >> 4), 16 nt + (lane & 15)], zero from column C_out on -- a wave's read of one (kk, nt) is 256
//                contiguous bytes, no padding and no bank conflict: 16 NTO KiB, 128 KiB at C_out > 112
//   operands     lane (cc, g) = (lane & 15, lane >> 4) loads X[row cc, 4 kk + g] and A[row cc, 4 kk + g], kk = 0 .. 31: the A operand
//                of v_mfma_f32_16x16x4_f32 as the instruction wants it, 32 + 32 registers; rows past n are zeros.  X * A is one multiply
//                per element in that layout
//   products     d2 += A . W2 and d1 += (X * A) . W1, kk ascending (k ascending), NTO accumulators of four registers each: lane (cc, g),
//                register r of d[nt] is row 4 g + r, column 16 nt + cc.  + bias as the accumulator leaves
//   gate         bit (P > 0) of the biased pre-activation: a wave ballot per (nt, r) holds the 16 bits of four rows; a row's word is cut
//                from two of them.  The padded columns hold 0 + 0 and set no bit
//   finish       act(P1) + act(P2), the mask (keyed by row and column), then per row the sum of squares over the columns below C_out:
//                a lane's fmaf chain over its columns 16 nt + cc, nt ascending, then the row's 16 lanes through xor-shuffles at strides
//                1, 2, 4, 8 (ngcf_row_sum); r = 1 / sqrt(max(., 1e-12f)) (ngcf_rnorm), rnorm[row] negated where the clamp acted, x r
//   store        vec_out: the four lanes 4 q .. 4 q + 3 of a row exchange a 4 x 4 block (three xor-shuffles), after which lane 4 q + j
//                holds the columns 64 h + 16 j + 4 q .. + 3 and stores them whole; a piece that crosses C_out, and every piece without
//                vec_out, leaves as single values from where it stands.  Nothing is written from column C_out on
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; the table of all sixteen instantiations in profiles/NOTES.md, "NGCF
// layer at width 128"): 128 output columns 173 VGPRs (190 with the mask), 16 columns 95 (111); no AGPRs; scratch 0 bytes per lane in every
// instantiation; LDS 16 NTO KiB per block, dynamic, 128 KiB at NTO = 8: one block of eight waves per CU, two waves per SIMD.
template <int NTO, bool DROP>
__global__ __launch_bounds__(64 * WIDE_WPB) void k_ngcf_rows(const NgcfRows a) {
    static_assert(NTO >= 1 && NTO <= WIDE_C / 16, "C_out <= C_in = 128");
    constexpr int IMG = WIDE_KK * NTO * 64;
    extern __shared__ float lds[];
    float *W1s = lds, *W2s = lds + IMG;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cc = lane & 15, g = lane >> 4;
    for (int idx = threadIdx.x; idx < IMG; idx += 64 * WIDE_WPB) {
        const int l = idx & 63, q = idx >> 6, nt = q % NTO, kk = q / NTO;
        const int k = 4 * kk + (l >> 4), col = 16 * nt + (l & 15);
        W1s[idx] = col < a.C_out ? a.W1[(int64_t)k * a.ldw1 + col] : 0.f;
        W2s[idx] = col < a.C_out ? a.W2[(int64_t)k * a.ldw2 + col] : 0.f;
    }
    __syncthreads();
    float bv1[NTO], bv2[NTO];
#pragma unroll
    for (int nt = 0; nt < NTO; ++nt) {
        const bool has = 16 * nt + cc < a.C_out;
        bv1[nt] = a.b1 != nullptr && has ? a.b1[16 * nt + cc] : 0.f;
        bv2[nt] = a.b2 != nullptr && has ? a.b2[16 * nt + cc] : 0.f;
    }
    const int words = (a.C_out + 31) >> 5;
    uint64_t stream = 0;
    if constexpr (DROP) stream = drop_stream(a.feat);
    const int64_t n_tiles = (a.n + 15) / 16;
    for (int64_t tile = (int64_t)blockIdx.x * WIDE_WPB + wave; tile < n_tiles; tile += (int64_t)gridDim.x * WIDE_WPB) {
        // the operand fragments
        float xa[WIDE_KK], aa[WIDE_KK];
        const int64_t arow = tile * 16 + cc;
        if (arow < a.n) {
            const float *__restrict__ xp = a.X + arow * a.ldx + g;
            const float *__restrict__ ap = a.A + arow * WIDE_C + g;
#pragma unroll
            for (int kk = 0; kk < WIDE_KK; ++kk) { xa[kk] = xp[4 * kk]; aa[kk] = ap[4 * kk]; }
        } else {
#pragma unroll
            for (int kk = 0; kk < WIDE_KK; ++kk) { xa[kk] = 0.f; aa[kk] = 0.f; }
        }
        // both products
        f32x4 d1[NTO], d2[NTO];
#pragma unroll
        for (int nt = 0; nt < NTO; ++nt) { d1[nt] = f32x4{0.f, 0.f, 0.f, 0.f}; d2[nt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        const int at = ngcf_image_at(lane);
#pragma unroll
        for (int kk = 0; kk < WIDE_KK; ++kk) {
            const float av = aa[kk], mv = xa[kk] * aa[kk];
            const float *w1 = W1s + kk * NTO * 64 + at, *w2 = W2s + kk * NTO * 64 + at;
#pragma unroll
            for (int nt = 0; nt < NTO; ++nt) {
                d2[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w2[64 * nt], d2[nt], 0, 0, 0);
                d1[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(mv, w1[64 * nt], d1[nt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int nt = 0; nt < NTO; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { d1[nt][r] += bv1[nt]; d2[nt][r] += bv2[nt]; }
        // the rows this lane finishes
        int64_t orow[4];
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { orow[r] = tile * 16 + 4 * g + r; ok[r] = orow[r] < a.n; }
        if (a.gate != nullptr) {      // (uniform)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int w = 0; w < (NTO + 1) / 2; ++w) {
                    const uint32_t word[2] = {ngcf_rows_word<NTO>(d1, w, r, g), ngcf_rows_word<NTO>(d2, w, r, g)};
                    if (cc == 0 && ok[r]) {
                        a.gate[orow[r] * (2 * words) + w] = word[0];
                        a.gate[orow[r] * (2 * words) + words + w] = word[1];
                    }
                }
        }
        // act(P1) + act(P2), the mask, the row's sum of squares
        float ss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int nt = 0; nt < NTO; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float t[1] = {ngcf_act(d1[nt][r], a.act) + ngcf_act(d2[nt][r], a.act)};
                ss[r] = ngcf_mask_sq<1, DROP>(a.feat, stream, orow[r], 16 * nt + cc, a.C_out, t, ss[r]);
                d1[nt][r] = t[0];
            }
        if (a.normalize) {            // (uniform: every lane of the wave takes part in the shuffles)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bool clamped;
                const float rn = ngcf_rnorm(ngcf_row_sum<16>(ss[r]), clamped);
#pragma unroll
                for (int nt = 0; nt < NTO; ++nt) d1[nt][r] *= rn;
                if (a.rnorm != nullptr && cc == 0 && ok[r]) a.rnorm[orow[r]] = clamped ? -rn : rn;
            }
        }
        // the rows leave
        if (a.vec_out) {              // (uniform)
            const int j = cc & 3, q = cc >> 2;
#pragma unroll
            for (int h = 0; h < (NTO + 3) / 4; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v[4], w[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = 4 * h + i < NTO ? d1[4 * h + i < NTO ? 4 * h + i : 0][r] : 0.f;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {      // lane j ^ s sends its value of block j: afterwards w[i] is column 4 q + i of block j
                        const int i = j ^ s;
                        const float t = i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3];
                        const float got = s ? __shfl_xor(t, s) : t;
#pragma unroll
                        for (int e = 0; e < 4; ++e) w[e] = e == i ? got : w[e];
                    }
                    const int col = 64 * h + 16 * j + 4 * q;
                    if (!ok[r] || col >= a.C_out) continue;
                    float *__restrict__ dst = a.out + orow[r] * a.ldo + col;
                    if (col + 4 <= a.C_out) vstore<4>(dst, w);
                    else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (col + e < a.C_out) dst[e] = w[e];
                    }
                }
        } else {
#pragma unroll
            for (int nt = 0; nt < NTO; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (ok[r] && 16 * nt + cc < a.C_out) a.out[orow[r] * a.ldo + 16 * nt + cc] = d1[nt][r];
        }
    }
}

// what gnx_graph_last_kernel reports for gnx_step_wide_ngcf: [mask][norm]
const char *const kNgcfWide[2][2] = {{"spmm+k_ngcf_rows<128>", "spmm+k_ngcf_rows<128>_norm"},
                                     {"spmm+k_ngcf_rows<128>_drop", "spmm+k_ngcf_rows<128>_drop_norm"}};

}  // namespace

extern "C" {

int gnx_step_wide_ngcf(gnx_graph_t g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C_in, const float *d_W1, int64_t ldw1,
                       const float *d_W2, int64_t ldw2, int64_t C_out, const float *d_b1, const float *d_b2, int act, double dropout_p,
                       uint64_t seed, uint64_t stream_id, int normalize, float *d_out, int64_t ldo, float *d_agg, uint32_t *d_gate, float *d_rnorm,
                       float *d_work, int64_t work_floats, void *stream) {
    const char *fn = "gnx_step_wide_ngcf";
    // (the handle is not looked at before the widths and the alignment are admitted: make_feat_drop reads it)
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(dropout_p >= 0.0 && dropout_p < 1.0, "%s: dropout rate %g outside [0, 1)", fn, dropout_p);
    GNX_CHECK_ARG(C_in >= 1 && C_in <= (1 << 20) && C_out >= 1 && C_out <= (1 << 20), "%s: widths %lld -> %lld not in [1, 2^20]", fn,
                  (long long)C_in, (long long)C_out);
    if (C_in != WIDE_C || C_out > C_in) {
        set_error("%s: widths %lld -> %lld are not supported (the row-local launch takes C_in = 128 and C_out <= 128; keep gnx_ngcf_step elsewhere)",
                  fn, (long long)C_in, (long long)C_out);
        return GNX_ERR_UNSUPPORTED;
    }
    if (ldx % 4 != 0 || !aligned(d_X, 16) || !aligned(d_agg, 16) || !aligned(d_work, 16)) {
        set_error("%s: misaligned rows (ldx %lld must be a multiple of 4 and X / d_agg / d_work 16-byte aligned; keep gnx_ngcf_step elsewhere)", fn,
                  (long long)ldx);
        return GNX_ERR_UNSUPPORTED;
    }
    DropFuse fd{};
    int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    const NgcfOut o{d_out, ldo, d_agg, d_gate, d_rnorm, d_work, work_floats};
    rc = ngcf_admit(fn, g, d_vals, d_X, ldx, C_in, d_W1, ldw1, d_W2, ldw2, C_out, d_b1, d_b2, act, normalize, o);
    if (rc != GNX_OK) return rc;
    const int64_t n = g->a.n_rows;
    const int64_t need = d_agg == nullptr ? roundup4(n * C_in) : 0;
    GNX_CHECK_ARG(work_floats >= need, "%s: needs d_work of %lld floats, has %lld (roundup4(n * C_in): the aggregated rows without d_agg)", fn,
                  (long long)need, (long long)work_floats);
    if (n == 0) return GNX_OK;
    float *T = d_agg ? d_agg : d_work;
    rc = gnx_spmm(g, d_vals, nullptr, d_X, ldx, C_in, nullptr, 0, 1.f, 0.f, GNX_ACT_NONE, T, C_in, stream);
    if (rc != GNX_OK) return rc;
    const bool drop = dropout_p != 0.0;      // p == 0 hashes nothing
    const NgcfRows a{d_X, ldx, T, n, d_W1, ldw1, d_W2, ldw2, (int)C_out, d_b1, d_b2, act, d_out, ldo,
                     act == GNX_ACT_NONE ? nullptr : d_gate,      // (the identity has nothing to gate)
                     d_rnorm, normalize != 0, ldo % 4 == 0 && aligned(d_out, 16), fd};
    rc = with_wide_tiles<1>((int)blocks_for(C_out, 16), [&](auto NTO) {      // (both weight images as dynamic LDS)
        constexpr size_t lds_bytes = (size_t)2 * WIDE_KK * NTO() * 64 * sizeof(float);
        return drop ? launch_ngcf_rows_kernel<k_ngcf_rows<NTO(), true>>(a, lds_bytes, n, (hipStream_t)stream)
                    : launch_ngcf_rows_kernel<k_ngcf_rows<NTO(), false>>(a, lds_bytes, n, (hipStream_t)stream);
    });
    if (rc != GNX_OK) return rc;
    g->last_kernel = kNgcfWide[drop ? 1 : 0][normalize];
    return GNX_OK;
}

}  // extern "C"
