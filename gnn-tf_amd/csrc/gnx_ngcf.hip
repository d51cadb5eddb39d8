// The NGCF layer (gcn.py:116-135) on gfx950: one kernel on the 16-row tile frame of gnx_layer_device.h, the row passes around it, and its
// host path over the launch plumbing of that header.
//   k_spmm_ngcf        the NGCF layer in one launch: k_spmm_gcn's fill, two matrices in LDS, the message product kept in the accumulators
//                      while the tile is multiplied by the rows' own X, the mask and the row norm in the store loop (k_ngcf_product and
//                      k_ngcf_tail: the same layer as row passes around the dense kernel; k_ngcf_back_gate: the backward's first pass)
//   k_ngcf_back        the backward around the transposed SpMM in one launch (gnx_step_back_ngcf): the gate, G1 . W1^T and G2 . W2^T
//                      through one tile per wave, dA, R and P from the walk, the bias sums as slabs (k_ngcf_back_sums adds them)
//   ngcf_forward       gnx_ngcf_step (gnx_ngcf_back_gate and gnx_step_back_ngcf are entries of their own; the backward's checks, prelude
//                      and transposed SpMM are NgcfBackCall's in gnx_ngcf_device.h, which gnx_step_back_wide_ngcf goes through too)
#include "gnx_ngcf_device.h"

namespace {

// ---- NGCF layer: SpMM + both transforms + the activations' sum + mask + row norm, one launch (gnx_ngcf_step) ------------------------------
//   A = sum_j Ahat[i,j] X[j,:]   P1 = (X[i,:] * A) . W1 + b1   P2 = A . W2 + b2   out = l2_normalize(drop(act(P1) + act(P2)))  (gcn.py:116-135)
// The pieces of the finished value that the fused launch and the row pass behind the dense kernel (k_ngcf_tail) share -- ngcf_act,
// ngcf_mask_sq, ngcf_row_sum, ngcf_rnorm -- stand in gnx_ngcf_device.h, beside the checks of the forward entries: the row-local launch
// of gnx_ngcf_wide.hip finishes its rows with them too.

// d <- tile . Ms + bias, KEPT IN THE ACCUMULATOR REGISTERS: tile_times_Ms (BIAS, NTN) without the activation and without the way back
// through the tile -- a sibling, not more template parameters of tile_times_Ms, so that its instantiations stay the ones measured.  On
// return (behind a wave barrier) every lane has read its part of the tile, which may be written again.  Lane (cc, g), register r of d[nt]
// holds row 4 g + r, column 16 nt + cc.
template <int NT, int NTN>
__device__ __forceinline__ void tile_times_Ms_kept(const float *T, const float *__restrict__ Ms, int lane, const float *__restrict__ bias,
                                                   int n_bias, f32x4 (&d)[NTN]) {
    constexpr int C = 16 * NT, STRIDE = Tile<NT>::STRIDE;
    static_assert(NTN >= 1 && NTN <= NT, "the result tile overwrites the gathered one");
    const int cc = lane & 15, g = lane >> 4;
#pragma unroll
    for (int nt = 0; nt < NTN; ++nt) d[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int kk = 0; kk < C / 4; ++kk) {
        const float a = T[cc * STRIDE + 4 * kk + g];
        const float *__restrict__ mrow = Ms + (4 * kk + g) * STRIDE + cc;
#pragma unroll
        for (int nt = 0; nt < NTN; ++nt) d[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, mrow[16 * nt], d[nt], 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int nt = 0; nt < NTN; ++nt) {
        const float bv = 16 * nt + cc < n_bias ? bias[16 * nt + cc] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) d[nt][r] += bv;
    }
}

// The gate words of one product, then its activation, on the accumulator registers: bit (16 nt + cc) & 31 of word (16 nt + cc) >> 5 of
// row 4 g + r = (d[nt][r] > 0), the biased pre-activation itself.  The 16 lanes that hold a row OR their bits through xor-shuffles and
// lane cc == 0 stores the word at gate[row, which * words + w] (trow[r]: the slot's row id, -1 for a dead slot, which stores nothing).
// The padded columns hold 0 + 0 and set no bit.  gate == nullptr (uniform): no shuffles, the activation alone.
template <int NTN>
__device__ __forceinline__ void ngcf_gate_act(f32x4 (&d)[NTN], int act, uint32_t *__restrict__ gate, const int (&trow)[4], int words, int which,
                                              int cc) {
    constexpr int WMAX = (NTN + 1) / 2;
    if (gate != nullptr) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int w = 0; w < WMAX; ++w) {
                uint32_t word = 0;
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    if (2 * w + h < NTN) word |= (d[2 * w + h][r] > 0.f ? 1u : 0u) << (16 * h + cc);
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) word |= (uint32_t)__shfl_xor((int)word, m);
                if (cc == 0 && trow[r] >= 0 && w < words) gate[(int64_t)trow[r] * (2 * words) + which * words + w] = word;
            }
    }
#pragma unroll
    for (int nt = 0; nt < NTN; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) d[nt][r] = ngcf_act(d[nt][r], act);
}

// The frame at C_in = 16 NTI with gathered_row as the row's body -- the fill of k_spmm_gcn: same entry order and fmaf chain, `agg` from the
// lanes that made the rows -- and BOTH matrices in LDS, W1 and W2 [C_in, C_out], their columns from C_out to 16 NTO zero-filled there and
// nowhere else.  Each slot's row id (-1: dead) rides in the slot's first padding column of the tile, as in k_spmm_gcn_back: the lanes
// that hold a row in the accumulators are not the ones that filled it.  One tile per wave:
//   message      d2 = tile . W2 + b2 (tile_times_Ms_kept), its gate words and activation on the registers, where it STAYS
//   interaction  each lane multiplies its own four columns of the tile in place by X[row, c .. c + 3] (a dead slot keeps zeros), then
//                d1 = tile . W1 + b1, gate words, activation; d1 + d2 -- one f32 add per element -- goes back through the tile
//   store loop   drop (DROP: `feat`, keyed by row and column), then with `normalize` the row's sum of squares over the columns below
//                C_out (ngcf_mask_sq, ngcf_row_sum over the row's 4 NTI lanes), r = 1 / sqrt(max(., 1e-12f)) -- to rnorm[row] when given,
//                NEGATED where the clamp acted, which is how the backward knows -- and the row leaves as x r; stores as in k_spmm_gcn
// f32 rows only.  LDS at C_in = 64: 2 x 17 408 B + 8 x 4 352 B = 68 KiB, two blocks of eight waves per CU (profiles/NOTES.md).
template <typename R, int NTI, int NTO, int U, int WPB, bool DROP = false>
__global__ __launch_bounds__(64 * WPB) void k_spmm_ngcf(const typename R::Args p, const float *__restrict__ W1, int64_t ldw1,
                                                        const float *__restrict__ W2, int64_t ldw2, int C_out, const float *__restrict__ b1,
                                                        const float *__restrict__ b2, int act, float *__restrict__ agg,
                                                        uint32_t *__restrict__ gate, float *__restrict__ rnorm, bool normalize, bool vec_out,
                                                        const DropFuse feat) {
    static_assert(!R::BF16, "the NGCF layer exists over f32 rows");
    static_assert(NTO >= 1 && NTO <= NTI, "C_out <= C_in: the result tile overwrites the gathered one");
    using TL = Tile<NTI>;
    constexpr int C = TL::C, CO = 16 * NTO, G = TL::G, RPP = TL::RPP, PASSES = TL::PASSES, STRIDE = TL::STRIDE;
    __shared__ float W1s[C * STRIDE];
    __shared__ float W2s[C * STRIDE];
    __shared__ float Ts[WPB][16 * STRIDE];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int idx = threadIdx.x; idx < C * CO; idx += 64 * WPB) {
        const int k = idx / CO, n = idx % CO;
        W1s[k * STRIDE + n] = n < C_out ? W1[(int64_t)k * ldw1 + n] : 0.f;
        W2s[k * STRIDE + n] = n < C_out ? W2[(int64_t)k * ldw2 + n] : 0.f;
    }
    __syncthreads();
    const int64_t tile = (int64_t)blockIdx.x * WPB + wave;
    if (tile * 16 >= p.n_rows) return;
    float *T = Ts[wave];
    const int sub = lane % G, c = sub * 4;
    int64_t rows[PASSES];
    bool live[PASSES];
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int rr = ps * RPP + lane / G;
        const int64_t slot = tile * 16 + rr;
        int64_t row = -1;
        int64_t beg = 0, end = 0;
        if (slot < p.n_rows) {
            row = slot_row(p, slot);
            beg = p.rowptr[row]; end = p.rowptr[row + 1];
        }
        live[ps] = row >= 0 && end - beg <= p.long_row;
        rows[ps] = row;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (live[ps]) {
            gathered_row<R, U>(p, row, beg, end, c, acc);
            if (agg) vstore<4>(agg + row * (int64_t)C + c, acc);
        }
        vstore<4>(T + rr * STRIDE + c, acc);
        if (sub == 0) T[rr * STRIDE + C] = __int_as_float(live[ps] ? (int)row : -1);
    }
    __builtin_amdgcn_wave_barrier();
    const int cc = lane & 15, g4 = (lane >> 4) * 4, words = (C_out + 31) >> 5;
    int trow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) trow[r] = __float_as_int(T[(g4 + r) * STRIDE + C]);
    f32x4 d2[NTO];
    tile_times_Ms_kept<NTI, NTO>(T, W2s, lane, b2, b2 ? C_out : 0, d2);
    ngcf_gate_act<NTO>(d2, act, gate, trow, words, 1, cc);
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        if (!live[ps]) continue;
        const int rr = ps * RPP + lane / G;
        float t[4], x[4];
        vload<4>(t, T + rr * STRIDE + c);
        vload<4>(x, p.X + rows[ps] * p.ldx + c);
#pragma unroll
        for (int v = 0; v < 4; ++v) t[v] *= x[v];
        vstore<4>(T + rr * STRIDE + c, t);
    }
    __builtin_amdgcn_wave_barrier();
    f32x4 d1[NTO];
    tile_times_Ms_kept<NTI, NTO>(T, W1s, lane, b1, b1 ? C_out : 0, d1);
    ngcf_gate_act<NTO>(d1, act, gate, trow, words, 0, cc);
#pragma unroll
    for (int nt = 0; nt < NTO; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) T[(g4 + r) * STRIDE + 16 * nt + cc] = d1[nt][r] + d2[nt][r];
    __builtin_amdgcn_wave_barrier();
    // (every lane of the wave takes part in the shuffles of the row sum; a row's lanes are live or not together)
    const bool has = c < C_out, whole = vec_out && c + 4 <= C_out;
    uint64_t stream = 0;
    if constexpr (DROP) stream = drop_stream(feat);
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int rr = ps * RPP + lane / G;
        const bool mine = live[ps] && has;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        float ss = 0.f;
        if (mine) {
            vload<4>(o, T + rr * STRIDE + c);
            ss = ngcf_mask_sq<4, DROP>(feat, stream, rows[ps], c, C_out, o, 0.f);
        }
        if (normalize) {
            bool clamped;
            const float r = ngcf_rnorm(ngcf_row_sum<G>(ss), clamped);
#pragma unroll
            for (int v = 0; v < 4; ++v) o[v] *= r;
            if (rnorm != nullptr && live[ps] && sub == 0) rnorm[rows[ps]] = clamped ? -r : r;
        }
        if (!mine) continue;
        float *__restrict__ dst = p.out + rows[ps] * p.ldo + c;
        if (whole) vstore<4>(dst, o);
        else {
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (c + v < C_out) dst[v] = o[v];
        }
    }
}

// ---- the NGCF layer's row passes (hub rows of gnx_ngcf_step; every row of its composed form; the backward's gate) -------------------------
// Pm[i, :] = X[r, :] * T[r, :] for r = rows[i] (null: row i): the interaction's operand of the rows that go through memory, compact
// ([n, C] contiguous, row i), one f32 multiply per element as in the fused launch.  T is [., C] contiguous at the row ids.
template <int VEC>
__global__ __launch_bounds__(256) void k_ngcf_product(const float *__restrict__ X, int64_t ldx, const float *__restrict__ T,
                                                     const int32_t *__restrict__ rows, int64_t n, int64_t C, float *__restrict__ Pm) {
    const int64_t per_row = C / VEC, total = n * per_row, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / per_row, r = rows ? (int64_t)rows[i] : i, c = (e % per_row) * VEC;
        float x[VEC], t[VEC];
        vload<VEC>(x, X + r * ldx + c);
        vload<VEC>(t, T + r * C + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) t[v] *= x[v];
        vstore<VEC>(Pm + i * C + c, t);
    }
}

void launch_ngcf_product(const float *X, int64_t ldx, const float *T, const int32_t *rows, int64_t n, int64_t C, float *Pm, hipStream_t s) {
    if (n == 0) return;
    launch_row_pass(n, C, {{X, 16, ldx}, {T, 16, C}, {Pm, 16, C}},
                    [&](auto V, unsigned grid) { GNX_LAUNCH(k_ngcf_product<V()>, grid, X, ldx, T, rows, n, C, Pm); });
}

// The store loop of k_spmm_ngcf as a row pass behind the dense kernel: P1[i, :] (compact, row stride ldp) and out[r, :], r = rows[i]
// (null: row i), hold the biased pre-activations P1 and P2; out[r, :] leaves as l2_normalize(drop(act(P1) + act(P2))) in place, with
// the row's gate words and rnorm[r] beside it -- ngcf_act, ngcf_mask_sq, ngcf_row_sum, ngcf_rnorm: the store loop's own code.  16 lanes
// per row, lane `sub` the columns 4 sub .. 4 sub + 3 of every panel of 64 (any width and row stride; at C_out <= 64 the sum of squares
// has the order of the fused launch: a lane's fmaf chain, then the xor-shuffles); 8 lanes OR the bits of a 32-column word.
template <bool DROP>
__global__ __launch_bounds__(256) void k_ngcf_tail(const float *__restrict__ P1, int64_t ldp, float *out, int64_t ldo,
                                                  const int32_t *__restrict__ rows, int64_t n, int64_t C_out, int act, const DropFuse fd,
                                                  uint32_t *__restrict__ gate, float *__restrict__ rnorm, bool normalize) {
    const int sub = threadIdx.x & 15;
    const int64_t words = (C_out + 31) >> 5, stride = (int64_t)gridDim.x * 16;
    uint64_t stream = 0;
    if constexpr (DROP) stream = drop_stream(fd);
    for (int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); i < n; i += stride) {
        const int64_t r = rows ? (int64_t)rows[i] : i;
        const float *__restrict__ p1 = P1 + i * ldp;
        float *o = out + r * ldo;
        float ss = 0.f;
        for (int64_t c0 = 0; c0 < C_out; c0 += 64) {
            const int64_t c = c0 + 4 * sub;
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            uint32_t w1 = 0, w2 = 0;
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (c + v < C_out) {
                    const float a = p1[c + v], b = o[c + v];
                    w1 |= (a > 0.f ? 1u : 0u) << v;
                    w2 |= (b > 0.f ? 1u : 0u) << v;
                    x[v] = ngcf_act(a, act) + ngcf_act(b, act);
                }
            ss = ngcf_mask_sq<4, DROP>(fd, stream, r, c, C_out, x, ss);
            if (gate != nullptr) {
                w1 <<= (c & 31); w2 <<= (c & 31);
#pragma unroll
                for (int m = 1; m < 8; m <<= 1) {
                    w1 |= (uint32_t)__shfl_xor((int)w1, m);
                    w2 |= (uint32_t)__shfl_xor((int)w2, m);
                }
                if ((sub & 7) == 0 && c < C_out) {
                    gate[r * (2 * words) + (c >> 5)] = w1;
                    gate[r * (2 * words) + words + (c >> 5)] = w2;
                }
            }
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (c + v < C_out) o[c + v] = x[v];
        }
        if (!normalize) continue;
        bool clamped;
        const float rn = ngcf_rnorm(ngcf_row_sum<16>(ss), clamped);
        if (rnorm != nullptr && sub == 0) rnorm[r] = clamped ? -rn : rn;
        for (int64_t c = 4 * sub; c < C_out; c += 64)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (c + v < C_out) o[c + v] *= rn;      // (the lane's own values: it reads what it wrote)
    }
}

void launch_ngcf_tail(const float *P1, int64_t ldp, float *out, int64_t ldo, const int32_t *rows, int64_t n, int64_t C_out, int act,
                      const DropFuse *fd, uint32_t *gate, float *rnorm, bool normalize, hipStream_t s) {
    if (n == 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks_for(n, 16), 1 << 20);
    if (fd) GNX_LAUNCH(k_ngcf_tail<true>, grid, P1, ldp, out, ldo, rows, n, C_out, act, *fd, gate, rnorm, normalize);
    else    GNX_LAUNCH(k_ngcf_tail<false>, grid, P1, ldp, out, ldo, rows, n, C_out, act, DropFuse{}, gate, rnorm, normalize);
}

// The backward's first pass (gnx_ngcf_back_gate): from the upstream gradient g of out = y, back through the norm, the mask and the two
// activations, 16 lanes per row as in k_ngcf_tail.  rnorm[r] > 0: the row was normalised with r and g_s = r (g - y (y . g)), y . g a
// lane's fmaf chain over its columns in ascending order, then the xor-shuffles; rnorm[r] < 0: the clamp acted, y = |r| x and
// g_s = |r| g; rnorm == null: g_s = g.  g_u = kept ? g_s * scale : +0 (the forward's mask, made again), G1 = bit1 ? g_u : g_u * slope
// and G2 likewise (gate == null: every bit counts as set); the columns C_out .. pad - 1 of G1 / G2 are written as zeros.
// THE ROW BODY HAS A TWIN: ngcf_gate_row below (k_ngcf_back) repeats it statement for statement and must keep its bits -- change both
// (tests/test_gpu_ngcf_back.py compares G1 / G2 of the two bit for bit).
__global__ __launch_bounds__(256) void k_ngcf_back_gate(const float *__restrict__ g, int64_t ldg, const float *__restrict__ y, int64_t ldy,
                                                       const float *__restrict__ rnorm, const uint32_t *__restrict__ gate, int64_t n,
                                                       int64_t C_out, int64_t pad, float slope, const DropFuse fd, float *__restrict__ G1,
                                                       float *__restrict__ G2, int64_t ldG) {
    const int sub = threadIdx.x & 15;
    const int64_t words = (C_out + 31) >> 5, stride = (int64_t)gridDim.x * 16;
    const uint64_t stream = drop_stream(fd);
    for (int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); r < n; r += stride) {
        const float rn = rnorm ? rnorm[r] : 1.f;
        const bool project = rnorm != nullptr && rn > 0.f;
        float dot = 0.f;
        if (project) {
            for (int64_t c = 4 * sub; c < C_out; c += 64)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (c + v < C_out) dot = fmaf(y[r * ldy + c + v], g[r * ldg + c + v], dot);
            dot = ngcf_row_sum<16>(dot);
        }
        const float scale = fabsf(rn);
        for (int64_t c = 4 * sub; c < pad; c += 64)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t cv = c + v;
                if (cv >= pad) continue;
                float g1 = 0.f, g2 = 0.f;
                if (cv < C_out) {
                    float x[1] = {g[r * ldg + cv]};
                    if (project) x[0] = scale * (x[0] - y[r * ldy + cv] * dot);
                    else if (rnorm != nullptr) x[0] = scale * x[0];
                    drop_values<1>(fd, stream, r, cv, x);
                    bool bit1 = true, bit2 = true;
                    if (gate != nullptr) {
                        bit1 = (gate[r * (2 * words) + (cv >> 5)] >> (cv & 31)) & 1u;
                        bit2 = (gate[r * (2 * words) + words + (cv >> 5)] >> (cv & 31)) & 1u;
                    }
                    g1 = bit1 ? x[0] : x[0] * slope;
                    g2 = bit2 ? x[0] : x[0] * slope;
                }
                G1[r * ldG + cv] = g1;
                G2[r * ldG + cv] = g2;
            }
    }
}

// ---- the NGCF layer's backward around the transposed SpMM, one launch (gnx_step_back_ngcf) ------------------------------------------------
//   G1, G2 = the gate pass      Q1 = G1 . W1^T      Q2 = G2 . W2^T      dA = Q1 * X + Q2      R = Q1 * A      P = X * A      db = sum_rows G
// Row-local, no gather: the 16-row tile frame over the rows as numbered.  ngcf_gate_row is the row body of k_ngcf_back_gate, statement
// for statement -- the gate pass itself keeps its own text: every way of calling one function from both kernels changed its instructions
// (profiles/NOTES.md, "Fused NGCF backward"), as with the tile frame's fill and walk -- so G1 / G2 have the gate pass's bits; the tests
// compare them bit for bit.
struct NgcfBack {
    const float *g; int64_t ldg; const float *y; int64_t ldy; const float *rnorm; const uint32_t *gate;      // the gate pass's operands
    int64_t n; int C_out, pad; float slope; DropFuse fd;
    const float *X; int64_t ldx; const float *A;                                                               // A [n, C_in] contiguous
    const float *W1; int64_t ldw1; const float *W2; int64_t ldw2;
    float *G1, *G2; int64_t ldG;
    float *P, *dA, *R;                   // [n, C_in] contiguous each; P may be null; dA == null: no products at all (R is null too)
    float *work;                         // the bias slabs, 2 C_out floats per block, or null
    int64_t tiles_per_block;
};

// G1 / G2 of the columns 4 sub .. 4 sub + 3 of row r (zeros from C_out on), 16 lanes per row: the arithmetic of k_ngcf_back_gate
template <bool DROP>
__device__ __forceinline__ void ngcf_gate_row(const NgcfBack &a, int64_t r, int sub, uint64_t stream, float (&g1)[4], float (&g2)[4]) {
    const int64_t C_out = a.C_out, words = (C_out + 31) >> 5, c = 4 * sub;
    const float *__restrict__ g = a.g, *__restrict__ y = a.y;
    const uint32_t *__restrict__ gate = a.gate;
    const float rn = a.rnorm ? a.rnorm[r] : 1.f;
    const bool project = a.rnorm != nullptr && rn > 0.f;
    float dot = 0.f;
    if (project) {
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (c + v < C_out) dot = fmaf(y[r * a.ldy + c + v], g[r * a.ldg + c + v], dot);
        dot = ngcf_row_sum<16>(dot);
    }
    const float scale = fabsf(rn);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int64_t cv = c + v;
        g1[v] = 0.f; g2[v] = 0.f;
        if (cv < C_out) {
            float x[1] = {g[r * a.ldg + cv]};
            if (project) x[0] = scale * (x[0] - y[r * a.ldy + cv] * dot);
            else if (a.rnorm != nullptr) x[0] = scale * x[0];
            if constexpr (DROP) drop_values<1>(a.fd, stream, r, cv, x);      // (without a mask the gate pass multiplies by a scale of 1)
            bool bit1 = true, bit2 = true;
            if (gate != nullptr) {
                bit1 = (gate[r * (2 * words) + (cv >> 5)] >> (cv & 31)) & 1u;
                bit2 = (gate[r * (2 * words) + words + (cv >> 5)] >> (cv & 31)) & 1u;
            }
            g1[v] = bit1 ? x[0] : x[0] * a.slope;
            g2[v] = bit2 ? x[0] : x[0] * a.slope;
        }
    }
}

// Block b takes the tiles b tiles_per_block .. (b + 1) tiles_per_block - 1 (tile t: rows 16 t .. 16 t + 15), wave w every WPB-th of
// them from the w-th on: which rows a block and a wave take follows from (n, the grid) alone.  Both matrices sit TRANSPOSED in LDS --
// W^T [16 NTK, C_in], read from W as stored, the rows from C_out on zero -- and a wave holds ONE tile, which both products pass through:
//   gate      four passes of four rows, 16 lanes per row (ngcf_gate_row): G1 / G2 to memory as whole float4 rows up to pad =
//             roundup4(C_out); a lane keeps its 16 + 16 values in registers and adds them to its column sums
//   message   G2 into the first 16 NTK columns of the tile, tile <- tile . W2^T on the matrix cores (tile_times_Ms with the k extent
//             16 NTK, k ascending): Q2, which each lane of the walk takes into registers -- a float4 of its row per pass
//   interaction  G1 into the tile from the registers, tile <- tile . W1^T: Q1
//   walk      a float4 of the lane's row per pass: dA = fmaf(Q1, X, Q2), R = Q1 * A, P = X * A
//   sums      a lane's sums over its rows in ascending order, then the block's 4 WPB row lanes of a column in (wave, lane) order through
//             LDS into slab b of `work` (db1, then db2); k_ngcf_back_sums adds the slabs in index order.  No float atomics.
// WPB = 4, three waves per SIMD asked of the compiler (121 .. 165 VGPRs, no scratch): LDS at C_in = 64 is 2 x 17 408 B + 4 x 4 352 B =
// 51 KiB, three blocks of four waves per CU by LDS and by registers alike (profiles/NOTES.md, "Fused NGCF backward").  The one
// instantiation that would spill under that bound -- 64 -> up to 16 columns with the mask -- is asked for two.
constexpr int ngcf_back_waves(int NTI, int NTK, bool DROP) { return NTI == 4 && NTK == 1 && DROP ? 2 : 3; }

template <int NTI, int NTK, int WPB, bool DROP>
__global__ __launch_bounds__(64 * WPB, ngcf_back_waves(NTI, NTK, DROP)) void k_ngcf_back(const NgcfBack a) {
    static_assert(NTK >= 1 && NTK <= NTI, "C_out <= C_in: the products overwrite the gradient tile");
    using TL = Tile<NTI>;
    constexpr int C = TL::C, CK = 16 * NTK, G = TL::G, RPP = TL::RPP, PASSES = TL::PASSES, STRIDE = TL::STRIDE;
    constexpr int TS = WPB * (16 * STRIDE > 512 ? 16 * STRIDE : 512);      // the tiles, and at the end eight column sums per thread
    __shared__ float W1t[CK * STRIDE];
    __shared__ float W2t[CK * STRIDE];
    __shared__ float Ts[TS];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const bool products = a.dA != nullptr;
    if (products) {
        for (int idx = threadIdx.x; idx < C * CK; idx += 64 * WPB) {
            const int c = idx / CK, k = idx % CK;
            W1t[k * STRIDE + c] = k < a.C_out ? a.W1[(int64_t)c * a.ldw1 + k] : 0.f;
            W2t[k * STRIDE + c] = k < a.C_out ? a.W2[(int64_t)c * a.ldw2 + k] : 0.f;
        }
    }
    __syncthreads();
    float *T = Ts + wave * (16 * STRIDE);
    const int64_t n_tiles = (a.n + 15) / 16;
    const int64_t first = (int64_t)blockIdx.x * a.tiles_per_block;
    const int64_t last = first + a.tiles_per_block < n_tiles ? first + a.tiles_per_block : n_tiles;
    const int gsub = lane & 15, grow = lane >> 4;          // the gate's lanes: 16 per row, four rows per pass
    const int sub = lane % G, c = sub * 4;                 // the walk's lanes: G per row
    uint64_t stream = 0;
    if constexpr (DROP) stream = drop_stream(a.fd);
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t tile = first + wave; tile < last; tile += WPB) {
        float g1[4][4], q2[PASSES][4];
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const int rr = 4 * ps + grow;
            const int64_t r = tile * 16 + rr;
            float g2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int v = 0; v < 4; ++v) g1[ps][v] = 0.f;
            if (r < a.n) {                                  // (the 16 lanes of a row together: the shuffles of y . g stay inside them)
                ngcf_gate_row<DROP>(a, r, gsub, stream, g1[ps], g2);
                if (4 * gsub < a.pad) {
                    vstore<4>(a.G1 + r * a.ldG + 4 * gsub, g1[ps]);
                    vstore<4>(a.G2 + r * a.ldG + 4 * gsub, g2);
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) { s1[v] += g1[ps][v]; s2[v] += g2[v]; }
            }
            if (4 * gsub < CK) vstore<4>(T + rr * STRIDE + 4 * gsub, g2);
        }
        if (products) {
            __builtin_amdgcn_wave_barrier();
            tile_times_Ms<NTI, false, NTI, NTK>(T, W2t, lane, GNX_ACT_NONE);
#pragma unroll
            for (int ps = 0; ps < PASSES; ++ps) vload<4>(q2[ps], T + (ps * RPP + lane / G) * STRIDE + c);
            __builtin_amdgcn_wave_barrier();                // (every lane has its Q2 before G1 takes the tile)
#pragma unroll
            for (int ps = 0; ps < 4; ++ps)
                if (4 * gsub < CK) vstore<4>(T + (4 * ps + grow) * STRIDE + 4 * gsub, g1[ps]);
            __builtin_amdgcn_wave_barrier();
            tile_times_Ms<NTI, false, NTI, NTK>(T, W1t, lane, GNX_ACT_NONE);
        }
        if (products || a.P != nullptr) {
#pragma unroll
            for (int ps = 0; ps < PASSES; ++ps) {
                const int rr = ps * RPP + lane / G;
                const int64_t r = tile * 16 + rr;
                if (r >= a.n) continue;
                float x[4], t[4];
                vload<4>(x, a.X + r * a.ldx + c);
                vload<4>(t, a.A + r * C + c);
                if (a.P != nullptr) {
                    float p[4];
#pragma unroll
                    for (int v = 0; v < 4; ++v) p[v] = x[v] * t[v];
                    vstore<4>(a.P + r * C + c, p);
                }
                if (products) {
                    float q1[4], d[4];
                    vload<4>(q1, T + rr * STRIDE + c);
#pragma unroll
                    for (int v = 0; v < 4; ++v) { d[v] = fmaf(q1[v], x[v], q2[ps][v]); q1[v] *= t[v]; }
                    vstore<4>(a.dA + r * C + c, d);
                    vstore<4>(a.R + r * C + c, q1);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();                    // (the walk has read the tile before the next gate writes it)
    }
    if (a.work == nullptr) return;                          // (uniform)
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        Ts[threadIdx.x * 8 + v] = s1[v];
        Ts[threadIdx.x * 8 + 4 + v] = s2[v];
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * a.C_out) {
        const int which = threadIdx.x / a.C_out, col = threadIdx.x % a.C_out;
        float acc = 0.f;
        for (int k = 0; k < 4 * WPB; ++k) acc += Ts[(k * 16 + (col >> 2)) * 8 + 4 * which + (col & 3)];
        a.work[(int64_t)blockIdx.x * (2 * a.C_out) + threadIdx.x] = acc;
    }
}

// Block q adds the slabs q per .. min((q + 1) per, n_slabs) - 1 in index order.  `group` given (the first level of a two-level sum:
// fixed association, reproducible): the sum is slab q of `group`; else (one block) db1 = its first C_out columns, db2 the second
// (either may be null).
__global__ __launch_bounds__(128) void k_ngcf_back_sums(const float *__restrict__ work, int64_t n_slabs, int64_t per, int C_out,
                                                       float *__restrict__ group, float *__restrict__ db1, float *__restrict__ db2) {
    const int e = threadIdx.x;
    if (e >= 2 * C_out) return;
    const int64_t s0 = (int64_t)blockIdx.x * per, s1 = s0 + per < n_slabs ? s0 + per : n_slabs;
    float acc = 0.f;
#pragma unroll 8
    for (int64_t s = s0; s < s1; ++s) acc += work[s * (2 * C_out) + e];
    if (group != nullptr) { group[(int64_t)blockIdx.x * (2 * C_out) + e] = acc; return; }
    float *out = e < C_out ? db1 : db2;
    if (out != nullptr) out[e < C_out ? e : e - C_out] = acc;
}

// what gnx_graph_last_kernel reports for gnx_step_back_ngcf: [C_in = 16, 32, 64][mask][dX ran]
#define GNX_NGCF_BACK_NAMES(c) {{"k_ngcf_back<" c ">", "k_ngcf_back<" c ">+spmm_tv"}, {"k_ngcf_back<" c ">_drop", "k_ngcf_back<" c ">_drop+spmm_tv"}}
const char *const kNgcfBack[3][2][2] = {GNX_NGCF_BACK_NAMES("16"), GNX_NGCF_BACK_NAMES("32"), GNX_NGCF_BACK_NAMES("64")};
#undef GNX_NGCF_BACK_NAMES

// ---- the NGCF layer's host path (gnx_ngcf_step) -------------------------------------------------------------------------------------------
// what gnx_graph_last_kernel reports: [C_in = 16, 32, 64][mask][norm][hub rows ran]; the composed form [mask][norm]
#define GNX_NGCF_NAMES(c) {{GNX_TILE_NAMES("k_spmm_ngcf", c, ""), GNX_TILE_NAMES("k_spmm_ngcf", c, "_norm")}, {GNX_TILE_NAMES("k_spmm_ngcf", c, "_drop"), GNX_TILE_NAMES("k_spmm_ngcf", c, "_drop_norm")}}
const char *const kNgcfFused[3][2][2][2] = {GNX_NGCF_NAMES("16"), GNX_NGCF_NAMES("32"), GNX_NGCF_NAMES("64")};
const char *const kNgcfComposed[2][2] = {{"spmm+dense_mfma_ngcf", "spmm+dense_mfma_ngcf_norm"}, {"spmm+dense_mfma_ngcf_drop", "spmm+dense_mfma_ngcf_drop_norm"}};
#undef GNX_NGCF_NAMES

// out = l2_normalize(drop(act((X * (A . X)) . W1 + b1) + act((A . X) . W2 + b2))).  The fused launch takes C_in = 16, 32 or 64 with
// C_out <= C_in over 16-byte aligned rows; its hub rows, and every row of everything else, are composed inside this call: the
// aggregated rows at T (d_agg, else the first roundup4(n C_in) floats of d_work), the product pass into compact rows, the dense kernel
// twice without activation (P1 compact, P2 into out), then k_ngcf_tail.  Nothing is launched before the last check has passed.
int ngcf_forward(const char *fn, gnx_graph *g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C_in, const float *d_W1, int64_t ldw1,
                 const float *d_W2, int64_t ldw2, int64_t C_out, const float *d_b1, const float *d_b2, int act, const DropFuse *fd, int normalize,
                 const NgcfOut &o, void *stream) {
    const int admitted = ngcf_admit(fn, g, d_vals, d_X, ldx, C_in, d_W1, ldw1, d_W2, ldw2, C_out, d_b1, d_b2, act, normalize, o);
    if (admitted != GNX_OK) return admitted;
    const Csr &m = g->a;
    const int64_t n = m.n_rows;
    const bool fusable = fused_width(C_in) && C_out <= C_in && ldx % 4 == 0 && aligned(d_X, 16) && aligned(o.agg, 16) && aligned(o.work, 16);
    // the rows that are composed: k of them -- the hub rows of the fused launch, else all -- need roundup4(k C_in) + k C_out floats of
    // d_work behind the [n, C_in] share that holds their aggregated rows where d_agg does not
    const int64_t k = fusable ? m.n_long : n;
    const int64_t share = (o.agg == nullptr && k > 0) ? roundup4(n * C_in) : 0;
    const int64_t need = k > 0 ? share + roundup4(k * C_in) + k * C_out : 0;
    GNX_CHECK_ARG(o.work_floats >= need,
                  "%s: needs d_work of %lld floats, has %lld (%s: %lld rows are composed in memory -- %s roundup4(rows * C_in) + rows * C_out)", fn,
                  (long long)need, (long long)o.work_floats,
                  !fused_width(C_in) ? "C_in is not 16, 32 or 64" : C_out > C_in ? "C_out > C_in" : !fusable ? "misaligned rows" : "the graph has hub rows",
                  (long long)k, o.agg ? "" : "roundup4(n * C_in) without d_agg, then");
    hipStream_t s = (hipStream_t)stream;
    uint32_t *gate_words = act == GNX_ACT_NONE ? nullptr : o.gate;      // (the identity has nothing to gate)
    float *T = o.agg ? o.agg : o.work;
    float *Pm = o.work ? o.work + share : nullptr, *P1 = Pm ? Pm + roundup4(k * C_in) : nullptr;
    // aggregated rows at T (the k listed; null: rows 0 .. k) -> their product with X, both transforms, and the store loop as a row pass
    auto transform_rows = [&](const int32_t *rows, int64_t cnt) -> int {
        launch_ngcf_product(d_X, ldx, T, rows, cnt, C_in, Pm, s);
        int err = dense_rows(Pm, C_in, cnt, C_in, d_W1, ldw1, C_out, d_b1, GNX_ACT_NONE, nullptr, nullptr, P1, C_out, s);
        if (err != GNX_OK) return err;
        err = dense_rows(T, C_in, cnt, C_in, d_W2, ldw2, C_out, d_b2, GNX_ACT_NONE, rows, rows, o.out, o.ldo, s);
        if (err != GNX_OK) return err;
        launch_ngcf_tail(P1, C_out, o.out, o.ldo, rows, cnt, C_out, act, fd, gate_words, o.rnorm, normalize != 0, s);
        GNX_HIP(hipGetLastError());
        return GNX_OK;
    };
    if (!fusable) {
        if (n == 0) return GNX_OK;
        const int rc = gnx_spmm(g, d_vals, nullptr, d_X, ldx, C_in, nullptr, 0, 1.f, 0.f, GNX_ACT_NONE, T, C_in, stream);
        if (rc != GNX_OK) return rc;
        g->last_kernel = kNgcfComposed[fd ? 1 : 0][normalize];
        return transform_rows(nullptr, n);
    }
    if (n == 0) return GNX_OK;
    int rc = reserve_partial(g, m, C_in, s);
    if (rc != GNX_OK) return rc;
    SpmmArgs p{};
    bind_values(g, nullptr, false, d_vals, p);
    set_operands<F32Rows>(p, d_X, ldx, nullptr, 0, 1.f, 0.f, GNX_ACT_NONE, o.out, 0, o.ldo, C_in);
    bind_fused(m, p);
    const bool vec_out = o.ldo % 4 == 0 && aligned(o.out, 16);
    const DropFuse feat = fd ? *fd : DropFuse{};
    with_tile_width(C_in, n, [&](auto NTI, dim3 grid) {
        with_out_tiles((int)blocks_for(C_out, 16), [&](auto NTO) {      // (C_out <= C_in: no NTO above NTI)
            with_flags([&](auto DROP) {
                if constexpr (NTO() <= NTI())
                    hipLaunchKernelGGL((k_spmm_ngcf<F32Rows, NTI(), NTO(), 4, 8, DROP()>), grid, dim3(512), 0, s, p, d_W1, ldw1, d_W2, ldw2, (int)C_out,
                                       d_b1, d_b2, act, o.agg, gate_words, o.rnorm, normalize != 0, vec_out, feat);
            }, fd != nullptr);
        });
    });
    g->last_kernel = kNgcfFused[C_in == 16 ? 0 : C_in == 32 ? 1 : 2][fd ? 1 : 0][normalize][m.n_long > 0];
    // hub rows: chunked partial sums -> aggregated rows at their row ids of T -> composed, those rows alone
    p.ldo = C_in;
    return hub_rows_tail<F32Rows>(g, m, p, d_X, T, false, s, transform_rows);
}

}  // namespace

extern "C" {

int gnx_ngcf_step(gnx_graph_t g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C_in, const float *d_W1, int64_t ldw1,
                  const float *d_W2, int64_t ldw2, int64_t C_out, const float *d_b1, const float *d_b2, int act, double dropout_p, uint64_t seed,
                  uint64_t stream_id, int normalize, float *d_out, int64_t ldo, float *d_agg, uint32_t *d_gate, float *d_rnorm, float *d_work,
                  int64_t work_floats, void *stream) {
    const char *fn = "gnx_ngcf_step";
    DropFuse fd{};
    const int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    return ngcf_forward(fn, g, d_vals, d_X, ldx, C_in, d_W1, ldw1, d_W2, ldw2, C_out, d_b1, d_b2, act, dropout_p != 0.0 ? &fd : nullptr, normalize,
                        NgcfOut{d_out, ldo, d_agg, d_gate, d_rnorm, d_work, work_floats}, stream);
}

int gnx_ngcf_back_gate(gnx_graph_t g, const float *d_g, int64_t ldg, const float *d_y, int64_t ldy, const float *d_rnorm, const uint32_t *d_gate,
                       int64_t n_rows, int64_t C_out, int act, double dropout_p, uint64_t seed, uint64_t stream_id, float *d_G1, float *d_G2,
                       int64_t ldG, void *stream) {
    const char *fn = "gnx_ngcf_back_gate";
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU || act == GNX_ACT_LEAKY, "%s: invalid activation %d", fn, act);
    GNX_CHECK_ARG(n_rows >= 0 && C_out >= 1 && C_out <= (1 << 20), "%s: negative row count or C_out not in [1, 2^20]", fn);
    int rc = NgcfBackCall{g, d_g, ldg, d_y, ldy, d_rnorm, d_gate, C_out, act, d_G1, d_G2, ldG}.grads(fn);
    if (rc != GNX_OK) return rc;
    const void *gate = d_gate;
    GNX_CHECK_ARG(d_G1 != d_G2 && d_G1 != d_g && d_G2 != d_g && d_G1 != d_y && d_G2 != d_y && d_G1 != d_rnorm && d_G2 != d_rnorm &&
                  (const void *)d_G1 != gate && (const void *)d_G2 != gate, "%s: G1 and G2 must be buffers of their own", fn);
    DropFuse fd{};
    rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    if (n_rows == 0) return GNX_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t pad = std::min<int64_t>(ldG, roundup4(C_out));
    const float slope = act == GNX_ACT_LEAKY ? 0.2f : act == GNX_ACT_RELU ? 0.f : 1.f;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks_for(n_rows, 16), 1 << 20);
    GNX_LAUNCH(k_ngcf_back_gate, grid, d_g, ldg, d_y, ldy, d_rnorm, act == GNX_ACT_NONE ? nullptr : d_gate, n_rows, C_out, pad, slope, fd, d_G1, d_G2, ldG);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

// The backward of gnx_ngcf_step around the two weight gradients: k_ngcf_back, the slab sum, and -- for dX -- the transposed SpMM over dA
// with R mixed in.  Everything is checked before the first launch; the widths and alignments without the launch are refused.
int gnx_step_back_ngcf(gnx_graph_t g, const float *d_vals_t, const float *d_g, int64_t ldg, const float *d_y, int64_t ldy, const float *d_rnorm,
                       const uint32_t *d_gate, int64_t C_out, int act, double dropout_p, uint64_t seed, uint64_t stream_id, const float *d_X,
                       int64_t ldx, const float *d_agg, int64_t C_in, const float *d_W1, int64_t ldw1, const float *d_W2, int64_t ldw2,
                       float *d_G1, float *d_G2, int64_t ldG, float *d_P, float *d_db1, float *d_db2, float *d_dA, float *d_R, float *d_dX,
                       int64_t lddx, float *d_work, int64_t work_floats, void *stream) {
    const char *fn = "gnx_step_back_ngcf";
    const NgcfBackCall c{g, d_g, ldg, d_y, ldy, d_rnorm, d_gate, C_out, act, d_G1, d_G2, ldG, dropout_p, seed, stream_id, d_vals_t, d_X, ldx, d_agg,
                         C_in, d_W1, ldw1, d_W2, ldw2, d_P, d_db1, d_db2, d_dA, d_R, d_dX, lddx, d_work, work_floats, stream};
    int rc = c.front(fn);
    if (rc != GNX_OK) return rc;
    if (!fused_width(C_in)) return refuse_unfused(fn, C_in);
    if (C_out > C_in) {
        set_error("%s: C_out %lld > C_in %lld is not supported (the fused backward takes C_out <= C_in; keep the composed backward elsewhere)", fn,
                  (long long)C_out, (long long)C_in);
        return GNX_ERR_UNSUPPORTED;
    }
    rc = c.args(fn);
    if (rc == GNX_OK) rc = c.own(fn);
    if (rc != GNX_OK) return rc;
    if (!c.aligned16()) return refuse_unfused(fn, C_in);
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols && g->blk_col_gid == nullptr, "%s: needs a square stand-alone graph", fn);
    const bool products = c.products();
    const int64_t n = g->a.n_rows, n_tiles = blocks_for(n, 16);
    const bool sums = d_db1 != nullptr || d_db2 != nullptr;
    constexpr int WPB = 4;
    // the bias slabs: one per block, at most 8192 -- ten rounds of the 768 blocks a device of 256 CUs holds at once, so that the last,
    // partly filled round is a small share of the launch -- and one per group of 64 of them behind those (the two-level sum): a function
    // of n alone; a block takes whole rounds of its four waves
    const int64_t slabs = std::max<int64_t>(1, std::min<int64_t>(8192, blocks_for(n_tiles, WPB))), group_slabs = blocks_for(slabs, 64);
    GNX_CHECK_ARG(!sums || work_floats >= (slabs + group_slabs) * 2 * C_out,
                  "%s: needs d_work of %lld floats, has %lld (s = max(1, min(8192, ceil(ceil(n / 16) / 4))) = %lld slabs and ceil(s / 64) = %lld "
                  "group sums of 2 * C_out floats)", fn, (long long)((slabs + group_slabs) * 2 * C_out), (long long)work_floats, (long long)slabs,
                  (long long)group_slabs);
    DropFuse fd{};
    rc = c.prelude(fn, fd);
    if (rc != GNX_OK || n == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool drop = dropout_p != 0.0;      // p == 0 hashes nothing
    const int64_t tiles_per_block = (blocks_for(n_tiles, (int)slabs) + WPB - 1) / WPB * WPB;
    const int64_t blocks = (n_tiles + tiles_per_block - 1) / tiles_per_block;      // <= slabs
    NgcfBack a{d_g, ldg, d_y, ldy, d_rnorm, act == GNX_ACT_NONE ? nullptr : d_gate, n, (int)C_out, (int)roundup4(C_out),
               act == GNX_ACT_LEAKY ? 0.2f : act == GNX_ACT_RELU ? 0.f : 1.f, fd, d_X, ldx, d_agg, d_W1, ldw1, d_W2, ldw2, d_G1, d_G2, ldG, d_P,
               products ? d_dA : nullptr, products ? d_R : nullptr, sums ? d_work : nullptr, tiles_per_block};
    with_tile_width(C_in, n, [&](auto NTI, dim3) {
        with_out_tiles((int)blocks_for(C_out, 16), [&](auto NTK) {      // (C_out <= C_in: no NTK above NTI)
            with_flags([&](auto DROP) {
                if constexpr (NTK() <= NTI())
                    hipLaunchKernelGGL((k_ngcf_back<NTI(), NTK(), WPB, DROP()>), dim3((unsigned)blocks), dim3(64 * WPB), 0, s, a);
            }, drop);
        });
    });
    if (sums) {      // the blocks' slabs in groups of 64, then the groups: index order at both levels
        float *groups = d_work + slabs * 2 * C_out;
        const int64_t n_groups = blocks_for(blocks, 64);
        hipLaunchKernelGGL(k_ngcf_back_sums, dim3((unsigned)n_groups), dim3(128), 0, s, d_work, blocks, (int64_t)64, (int)C_out, groups, nullptr, nullptr);
        hipLaunchKernelGGL(k_ngcf_back_sums, dim3(1), dim3(128), 0, s, groups, n_groups, n_groups, (int)C_out, nullptr, d_db1, d_db2);
    }
    GNX_HIP(hipGetLastError());
    return c.finish(kNgcfBack[C_in == 16 ? 0 : C_in == 32 ? 1 : 2][drop][products]);
}

}  // extern "C"
