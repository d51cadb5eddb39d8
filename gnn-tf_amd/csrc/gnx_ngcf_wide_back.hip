// The backward of the NGCF layer at C_in = 128 around its two weight gradients (gnx_step_back_wide_ngcf): the gate pass of gnx_ngcf.hip,
// ONE row-local launch, the transposed SpMM of gnx_spmm.hip.
//   k_ngcf_rows_back          Q1 = G1 . W1^T and Q2 = G2 . W2^T on the matrix cores with the rows' G1 and G2 held as MFMA operand fragments
//                             in registers, then dA = Q1 * X + Q2, R = Q1 * A and P = X * A as the accumulators leave
//   k_ngcf_wide_colsums, k_ngcf_wide_slabsum   db1 / db2: the column sums of G1 / G2 in slabs of rows, the slabs added in index order
//   gnx_step_back_wide_ngcf   gnx_ngcf_back_gate, the two sums, k_ngcf_rows_back over all n rows, gnx_spmm_tv over dA with R mixed in
// The launch shape is k_ngcf_rows' (gnx_ngcf_wide.hip): a block of eight waves per CU, persistent over 16-row tiles, both weight
// matrices in LDS; what the two units share of it stands in gnx_ngcf_wide_device.h, and the entry's host path, which is
// gnx_step_back_ngcf's, in gnx_ngcf_device.h.  Measured against the composed backward in profiles/NOTES.md, "NGCF backward at width 128".
#include "gnx_ngcf_device.h"
#include "gnx_ngcf_wide_device.h"

namespace {

struct NgcfRowsBack {
    const float *G1, *G2; int64_t ldG; int C_out, pad;              // pad = roundup4(C_out): the columns of G1 / G2 that exist
    const float *X; int64_t ldx; const float *A; int64_t n;        // A [n, 128] contiguous
    const float *W1; int64_t ldw1; const float *W2; int64_t ldw2;
    float *P, *dA, *R;                                              // [n, 128] contiguous each; P may be null
};

// One block of eight waves per CU, persistent: block b takes the tiles 8 b + w, 8 (b + gridDim.x) + w, .. (tile t: rows 16 t .. 16 t + 15)
// with its wave w.  Which wave finishes a row changes no bit of it: nothing below depends on the tile but the row ids.  No gather.
//   weights      W1^T and W2^T once per block into LDS, f32, read from W1 / W2 [128, C_out] as stored, in the order the B operand is
//                read: float (kk 8 + nt) 64 + lane is W[16 nt + (lane & 15), 4 kk + (lane >> 4)], zero where 4 kk + (lane >> 4) >= C_out;
//                kk < 4 NTK, nt < 8 -- a wave's read of one (kk, nt) is 256 contiguous bytes, no padding: 16 NTK KiB, 128 KiB at
//                C_out > 112.  (The fill reads a row of W along k, whole cache lines, and scatters into the image.)
//   operands     lane (cc, g) = (lane & 15, lane >> 4) loads G1[row cc, 4 kk + g] and G2[row cc, 4 kk + g], kk < 4 NTK: the A operand of
//                v_mfma_f32_16x16x4_f32, 4 NTK + 4 NTK registers.  A step of four columns from pad = roundup4(C_out) on is not loaded but
//                set to zero (the branch is uniform: pad is a multiple of four); rows past n are zeros
//   products     d2 += G2 . W2^T and d1 += G1 . W1^T in one k loop, kk ascending (the output columns ascending), 8 + 8 accumulators
//                of four registers each: lane (cc, g), register r of d[nt] is row 4 g + r, column 16 nt + cc
//   walk         elementwise, so its bits do not depend on where a value stands: Q1 and Q2 go through the 4 x 4 exchange first
//                (ngcf_exchange), after which lane 4 q + j holds the columns 64 h + 16 j + 4 q .. + 3 of row 4 g + r of both, loads X
//                and A there whole, and stores dA = fmaf(Q1, X, Q2), R = Q1 * A and -- where P is given -- P = X * A as whole 16 bytes
// NTK = 0 is the launch without products (dX not asked for): no LDS, no MFMA, P = X * A alone.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; the table in profiles/NOTES.md, "NGCF backward at width 128"): no
// scratch and fewer than 256 registers in every instantiation; LDS 16 NTK KiB per block, dynamic.
template <int NTK>
__global__ __launch_bounds__(64 * WIDE_WPB) void k_ngcf_rows_back(const NgcfRowsBack a) {
    static_assert(NTK >= 0 && NTK <= WIDE_C / 16, "C_out <= C_in = 128");
    constexpr int KK = 4 * NTK, CK = 16 * NTK, IMG = KK * WIDE_NT * 64;
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cc = lane & 15, g = lane >> 4, j = cc & 3, q = cc >> 2;
    if constexpr (NTK > 0) {
        float *W1s = lds, *W2s = lds + IMG;
        for (int idx = threadIdx.x; idx < WIDE_C * CK; idx += 64 * WIDE_WPB) {
            const int k = idx % CK, c = idx / CK;
            const int at = ((k >> 2) * WIDE_NT + (c >> 4)) * 64 + (k & 3) * 16 + (c & 15);
            W1s[at] = k < a.C_out ? a.W1[(int64_t)c * a.ldw1 + k] : 0.f;
            W2s[at] = k < a.C_out ? a.W2[(int64_t)c * a.ldw2 + k] : 0.f;
        }
        __syncthreads();
    }
    const int64_t n_tiles = (a.n + 15) / 16;
    for (int64_t tile = (int64_t)blockIdx.x * WIDE_WPB + wave; tile < n_tiles; tile += (int64_t)gridDim.x * WIDE_WPB) {
        f32x4 d1[WIDE_NT], d2[WIDE_NT];
        if constexpr (NTK > 0) {
            // the operand fragments
            float g1[KK], g2[KK];
            const int64_t arow = tile * 16 + cc;
            if (arow < a.n) {
                const float *__restrict__ p1 = a.G1 + arow * a.ldG + g;
                const float *__restrict__ p2 = a.G2 + arow * a.ldG + g;
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const bool has = 4 * kk < a.pad;      // (uniform)
                    g1[kk] = has ? p1[4 * kk] : 0.f;
                    g2[kk] = has ? p2[4 * kk] : 0.f;
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) { g1[kk] = 0.f; g2[kk] = 0.f; }
            }
            // both products
#pragma unroll
            for (int nt = 0; nt < WIDE_NT; ++nt) { d1[nt] = f32x4{0.f, 0.f, 0.f, 0.f}; d2[nt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            const int at = ngcf_image_at(lane);
            const float *W1s = lds, *W2s = lds + IMG;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const float *w1 = W1s + kk * WIDE_NT * 64 + at, *w2 = W2s + kk * WIDE_NT * 64 + at;
#pragma unroll
                for (int nt = 0; nt < WIDE_NT; ++nt) {
                    d2[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(g2[kk], w2[64 * nt], d2[nt], 0, 0, 0);
                    d1[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(g1[kk], w1[64 * nt], d1[nt], 0, 0, 0);
                }
            }
        }
        // the walk
#pragma unroll
        for (int h = 0; h < WIDE_NT / 4; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float q1[4] = {0.f, 0.f, 0.f, 0.f}, q2[4] = {0.f, 0.f, 0.f, 0.f};
                if constexpr (NTK > 0) {      // (every lane of the wave takes part in the shuffles)
                    const float v1[4] = {d1[4 * h][r], d1[4 * h + 1][r], d1[4 * h + 2][r], d1[4 * h + 3][r]};
                    const float v2[4] = {d2[4 * h][r], d2[4 * h + 1][r], d2[4 * h + 2][r], d2[4 * h + 3][r]};
                    ngcf_exchange(v1, j, q1);
                    ngcf_exchange(v2, j, q2);
                }
                const int64_t row = tile * 16 + 4 * g + r;
                if (row >= a.n) continue;
                const int col = 64 * h + 16 * j + 4 * q;
                float x[4], av[4], o[4];
                vload<4>(x, a.X + row * a.ldx + col);
                vload<4>(av, a.A + row * WIDE_C + col);
                if constexpr (NTK > 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = fmaf(q1[e], x[e], q2[e]);
                    vstore<4>(a.dA + row * WIDE_C + col, o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = q1[e] * av[e];
                    vstore<4>(a.R + row * WIDE_C + col, o);
                }
                if (a.P != nullptr) {      // (uniform)
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = x[e] * av[e];
                    vstore<4>(a.P + row * WIDE_C + col, o);
                }
            }
    }
}

// db1 / db2 without float atomics, in an order that follows from (n, C_out) alone.  Block s takes the rows s per .. min((s + 1) per, n)
// - 1: with cg = pad / 4 float4 columns and RL = 256 / cg row lanes, thread (rl, c4) adds the float4 c4 of the rows s per + rl,
// + RL, .. of G1 and of G2 in ascending order; then thread e < 2 C_out adds the RL shares of its column in ascending rl: slab s of
// `work` is db1's share (C_out floats), then db2's.
__global__ __launch_bounds__(256) void k_ngcf_wide_colsums(const float *__restrict__ G1, const float *__restrict__ G2, int64_t ldG, int64_t n,
                                                          int64_t per, int C_out, int pad, float *__restrict__ work) {
    __shared__ float part[2][256][4];
    const int cg = pad >> 2, RL = 256 / cg;
    const int t = threadIdx.x, c4 = t % cg, rl = t / cg;
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = r0 + per < n ? r0 + per : n;
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    if (rl < RL) {
#pragma unroll 4
        for (int64_t r = r0 + rl; r < r1; r += RL) {
            float u[4], v[4];
            vload<4>(u, G1 + r * ldG + 4 * c4);
            vload<4>(v, G2 + r * ldG + 4 * c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { s1[e] += u[e]; s2[e] += v[e]; }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { part[0][t][e] = s1[e]; part[1][t][e] = s2[e]; }
    __syncthreads();
    if (t < 2 * C_out) {
        const int which = t / C_out, col = t % C_out;
        float acc = 0.f;
        for (int k = 0; k < RL; ++k) acc += part[which][k * cg + (col >> 2)][col & 3];
        work[(int64_t)blockIdx.x * (2 * C_out) + t] = acc;
    }
}

// one block: thread e < 2 C_out adds its value of the slabs in index order; db1 is the first C_out sums, db2 the second (either may be null)
__global__ __launch_bounds__(256) void k_ngcf_wide_slabsum(const float *__restrict__ work, int64_t n_slabs, int C_out, float *__restrict__ db1,
                                                          float *__restrict__ db2) {
    const int e = threadIdx.x;
    if (e >= 2 * C_out) return;
    float acc = 0.f;
#pragma unroll 16
    for (int64_t s = 0; s < n_slabs; ++s) acc += work[s * (2 * C_out) + e];
    float *out = e < C_out ? db1 : db2;
    if (out != nullptr) out[e < C_out ? e : e - C_out] = acc;
}

// what gnx_graph_last_kernel reports for gnx_step_back_wide_ngcf: [mask][dX ran]
const char *const kNgcfWideBack[2][2] = {{"k_ngcf_rows_back<128>", "k_ngcf_rows_back<128>+spmm_tv"},
                                         {"k_ngcf_rows_back<128>_drop", "k_ngcf_rows_back<128>_drop+spmm_tv"}};

// the slabs of the column sums: a function of n alone
int64_t ngcf_wide_slabs(int64_t n) { return std::max<int64_t>(1, std::min<int64_t>(1024, blocks_for(n, 512))); }

}  // namespace

extern "C" {

// Everything is checked before the first launch; the widths and alignments without the launch are refused.
int gnx_step_back_wide_ngcf(gnx_graph_t g, const float *d_vals_t, const float *d_g, int64_t ldg, const float *d_y, int64_t ldy,
                            const float *d_rnorm, const uint32_t *d_gate, int64_t C_out, int act, double dropout_p, uint64_t seed,
                            uint64_t stream_id, const float *d_X, int64_t ldx, const float *d_agg, int64_t C_in, const float *d_W1,
                            int64_t ldw1, const float *d_W2, int64_t ldw2, float *d_G1, float *d_G2, int64_t ldG, float *d_P, float *d_db1,
                            float *d_db2, float *d_dA, float *d_R, float *d_dX, int64_t lddx, float *d_work, int64_t work_floats,
                            void *stream) {
    const char *fn = "gnx_step_back_wide_ngcf";
    const NgcfBackCall c{g, d_g, ldg, d_y, ldy, d_rnorm, d_gate, C_out, act, d_G1, d_G2, ldG, dropout_p, seed, stream_id, d_vals_t, d_X, ldx, d_agg,
                         C_in, d_W1, ldw1, d_W2, ldw2, d_P, d_db1, d_db2, d_dA, d_R, d_dX, lddx, d_work, work_floats, stream};
    int rc = c.front(fn);
    if (rc != GNX_OK) return rc;
    if (C_in != WIDE_C || C_out > C_in) {
        set_error("%s: widths %lld -> %lld are not supported (the row-local launch takes C_in = 128 and C_out <= 128; keep the composed backward "
                  "elsewhere)", fn, (long long)C_in, (long long)C_out);
        return GNX_ERR_UNSUPPORTED;
    }
    rc = c.args(fn);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols && g->blk_col_gid == nullptr, "%s: needs a square stand-alone graph", fn);
    rc = c.own(fn);
    if (rc != GNX_OK) return rc;
    const bool products = c.products();
    const int64_t pad = roundup4(C_out);
    if (!c.aligned16() || ldG < pad) {
        set_error("%s: misaligned rows (ldx %lld and ldG %lld must be multiples of 4, ldG >= roundup4(C_out) = %lld, and X / d_agg / G1 / G2 / P / "
                  "dA / R 16-byte aligned; keep the composed backward elsewhere)", fn, (long long)ldx, (long long)ldG, (long long)pad);
        return GNX_ERR_UNSUPPORTED;
    }
    const int64_t n = g->a.n_rows;
    const bool sums = d_db1 != nullptr || d_db2 != nullptr;
    const int64_t slabs = ngcf_wide_slabs(n);
    GNX_CHECK_ARG(!sums || work_floats >= slabs * 2 * C_out,
                  "%s: needs d_work of %lld floats, has %lld (s = max(1, min(1024, ceil(n / 512))) = %lld slabs of 2 * C_out floats)", fn,
                  (long long)(slabs * 2 * C_out), (long long)work_floats, (long long)slabs);
    DropFuse fd{};      // (the gate pass makes its own: the prelude checks the rate under this entry's name)
    rc = c.prelude(fn, fd);
    if (rc != GNX_OK || n == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    // step A: the gate pass, its own kernel (every argument it checks was checked above, under this entry's name)
    rc = gnx_ngcf_back_gate(g, d_g, ldg, d_y, ldy, d_rnorm, d_gate, n, C_out, act, dropout_p, seed, stream_id, d_G1, d_G2, ldG, stream);
    if (rc != GNX_OK) return rc;
    if (sums) {
        const int64_t per = blocks_for(n, (int)slabs), blocks = blocks_for(n, (int)per);      // blocks <= slabs
        hipLaunchKernelGGL(k_ngcf_wide_colsums, dim3((unsigned)blocks), dim3(256), 0, s, d_G1, d_G2, ldG, n, per, (int)C_out, (int)pad, d_work);
        hipLaunchKernelGGL(k_ngcf_wide_slabsum, dim3(1), dim3(256), 0, s, d_work, blocks, (int)C_out, d_db1, d_db2);
        GNX_HIP(hipGetLastError());
    }
    // step B: the row-local launch (without dX: P alone, where it is asked for)
    if (products || d_P != nullptr) {
        const NgcfRowsBack a{d_G1, d_G2, ldG, (int)C_out, (int)pad, d_X, ldx, d_agg, n, d_W1, ldw1, d_W2, ldw2, d_P, products ? d_dA : nullptr,
                             products ? d_R : nullptr};
        rc = with_wide_tiles<0>(products ? (int)blocks_for(C_out, 16) : 0, [&](auto NTK) {      // (0: P alone; both weight images as dynamic LDS)
            return launch_ngcf_rows_kernel<k_ngcf_rows_back<NTK()>>(a, (size_t)2 * 4 * NTK() * WIDE_NT * 64 * sizeof(float), n, s);
        });
        if (rc != GNX_OK) return rc;
    }
    // step C
    return c.finish(kNgcfWideBack[dropout_p != 0.0 ? 1 : 0][products]);
}

}  // extern "C"
