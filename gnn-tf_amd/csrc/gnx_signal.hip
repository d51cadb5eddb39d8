// Node signals at width 1 (gfx950): one scalar per node.  The projection f = sigmoid(X . w), the width-1 SpMV with its three
// epilogues (the PPR mix, the smoothness quotient's forward, its backward), the fixed-order global sums and the uniform draw of
// FastReg's projection vector.  What PPRSweep and FastReg (experimental_filter.py:7-43 of the reference) sit on.
//
// The gather.  The SpMM kernels give a row to a lane group whose lanes split the COLUMNS; at one column one lane of the group would
// gather alone.  Here the lanes of a group split the row's ENTRIES: lane `sub` of G takes entries beg + sub, beg + sub + G, ... (index
// and value loads coalesced across the group), runs its own fmaf chain in entry order, and the G sums are added in a fixed xor tree.
// Rows longer than the structure's long_row are the plan's hub rows: one wave per chunk (lanes at stride 64, the same tree) leaves a
// chunk sum in the handle's slab, and the row's group adds its chunk sums in chunk order.  No float atomics: a result is a function of
// the structure and the operands alone.  A row without entries gives +0.
//
// The sums.  A block takes SIG_SLAB_ROWS consecutive slots of the structure's row order -- boundaries that depend on n alone -- and
// leaves its two partial sums as one slab; k_signal_sum adds slabs in index order (thread-strided, then a fixed tree), level by level,
// and its last launch writes {num, den, num / den}.
#include "gnx_internal.h"

#include <algorithm>

namespace gnx {
namespace {

constexpr int SIG_THREADS = 256;
constexpr int SIG_SLAB_ROWS = 256;      // rows per block = rows per slab of the global sums
// slabs one block of k_signal_sum adds.  Small on purpose: a level between costs a launch of a few microseconds, and with 64 slabs of 256
// rows it exists from 2^14 rows on, so structures of test size run it (the sums of 10^7 rows take three launches)
constexpr int SIG_SUM_SPAN = 64;
// lanes per short row: 8.  Measured against 4 (profiles/NOTES.md, "Width-1 node signals")
#ifndef GNX_SIGNAL_GROUP
#define GNX_SIGNAL_GROUP 8
#endif

enum { EPI_MIX = 0, EPI_SMOOTH = 1, EPI_BACK = 2 };

struct SignalArgs {
    // the structure walked and its plan
    const int64_t *rowptr;
    const int32_t *colidx;
    const float *vals;
    const int32_t *row_order;
    const int32_t *long_rows;
    const int64_t *long_chunk_ptr;
    const int32_t *chunk_long;
    float *partial;             // [n_chunks] chunk sums of the hub rows
    int64_t n_rows, n_long, n_chunks;
    int long_row, long_chunk;
    const float *x;             // the gathered signal
    float *out;                 // MIX: the result; SMOOTH: d = f - p; BACK: gz
    // MIX
    const float *h0;            // null: the constant 1
    float beta, alpha;
    // SMOOTH / BACK
    const float *f, *colsum;
    float *slabs;               // SMOOTH: [2 * blocks] partial sums of d^2 and of D f^2
    const float *d, *sums, *upstream;   // BACK
};

template <int W>
__device__ __forceinline__ float xor_tree(float v) {
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, W);
    return v;
}

// one wave per chunk of a hub row
__global__ __launch_bounds__(SIG_THREADS) void k_signal_chunks(const SignalArgs p) {
    const int64_t c = (int64_t)blockIdx.x * (SIG_THREADS / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    float acc = 0.f;
    if (c < p.n_chunks) {
        const int32_t li = p.chunk_long[c];
        const int64_t row = p.long_rows[li];
        const int64_t beg = p.rowptr[row] + (c - p.long_chunk_ptr[li]) * p.long_chunk;
        const int64_t end = min(beg + (int64_t)p.long_chunk, p.rowptr[row + 1]);
        for (int64_t e = beg + lane; e < end; e += 64) acc = fmaf(p.vals[e], p.x[p.colidx[e]], acc);
    }
    acc = xor_tree<64>(acc);
    if (c < p.n_chunks && lane == 0) p.partial[c] = acc;
}

// two sums of a block in a fixed tree; the result in thread 0
__device__ __forceinline__ void block_pair_sum(float &a, float &b) {
    __shared__ float sa[SIG_THREADS], sb[SIG_THREADS];
    const int t = threadIdx.x;
    sa[t] = a; sb[t] = b;
    __syncthreads();
#pragma unroll
    for (int s = SIG_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) { sa[t] += sa[t + s]; sb[t] += sb[t + s]; }
        __syncthreads();
    }
    a = sa[0]; b = sb[0];
}

template <int G, int EPI>
__global__ __launch_bounds__(SIG_THREADS) void k_signal_rows(const SignalArgs p) {
    constexpr int ROWS = SIG_THREADS / G;           // rows of one pass of the block
    const int sub = threadIdx.x % G, grp = threadIdx.x / G;
    const int64_t slot0 = (int64_t)blockIdx.x * SIG_SLAB_ROWS;
    float s_num = 0.f, s_den = 0.f;
    for (int pass = 0; pass < SIG_SLAB_ROWS / ROWS; ++pass) {
        const int64_t slot = slot0 + pass * ROWS + grp;
        const bool live = slot < p.n_rows;
        int64_t row = 0;
        float acc = 0.f;
        if (live) {
            row = p.row_order ? (int64_t)p.row_order[slot] : slot;
            const int64_t beg = p.rowptr[row], end = p.rowptr[row + 1];
            if (end - beg > p.long_row) {
                if (sub == 0) {     // a hub row: its chunk sums in chunk order (long_rows is ascending)
                    int64_t lo = 0, hi = p.n_long - 1;
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        if (p.long_rows[mid] < row) lo = mid + 1; else hi = mid;
                    }
                    const int64_t c1 = p.long_chunk_ptr[lo + 1];
                    for (int64_t c = p.long_chunk_ptr[lo]; c < c1; ++c) acc += p.partial[c];
                }
            } else {
                for (int64_t e = beg + sub; e < end; e += G) acc = fmaf(p.vals[e], p.x[p.colidx[e]], acc);
            }
        }
        acc = xor_tree<G>(acc);     // (outside every branch: all lanes of the wave take part; the other lanes of a hub row add zeros)
        if (live && sub == 0) {
            if constexpr (EPI == EPI_MIX) {
                const float mix = p.alpha * (p.h0 ? p.h0[row] : 1.f);      // rounded on its own, so that NULL is bit for bit a vector of ones
                p.out[row] = fmaf(p.beta, acc, mix);
            } else if constexpr (EPI == EPI_SMOOTH) {
                const float f = p.f[row];
                const float d = f - acc;
                p.out[row] = d;
                s_num = fmaf(d, d, s_num);
                s_den = fmaf(p.colsum[row] * f, f, s_den);
            } else {
                const float f = p.f[row], d = p.d[row];
                const float den = p.sums[1], lam = p.sums[2], u = p.upstream[0];
                const float inner = (d - acc) - lam * p.colsum[row] * f;
                p.out[row] = u * (2.f / den) * inner * f * (1.f - f);
            }
        }
    }
    if constexpr (EPI == EPI_SMOOTH) {
        block_pair_sum(s_num, s_den);
        if (threadIdx.x == 0) {
            p.slabs[2 * (int64_t)blockIdx.x] = s_num;
            p.slabs[2 * (int64_t)blockIdx.x + 1] = s_den;
        }
    }
}

// out pair b = the pairs [b * SIG_SUM_SPAN, (b + 1) * SIG_SUM_SPAN) of `in`, added in index order per thread and then in a fixed tree;
// final: one block, out = {num, den, num / den} (plain IEEE division)
__global__ __launch_bounds__(SIG_THREADS) void k_signal_sum(const float *__restrict__ in, int64_t n_in, float *__restrict__ out, int final) {
    const int64_t beg = (int64_t)blockIdx.x * SIG_SUM_SPAN, end = min(beg + (int64_t)SIG_SUM_SPAN, n_in);
    float a = 0.f, b = 0.f;
    for (int64_t i = beg + threadIdx.x; i < end; i += SIG_THREADS) { a += in[2 * i]; b += in[2 * i + 1]; }
    block_pair_sum(a, b);
    if (threadIdx.x == 0) {
        if (final) { out[0] = a; out[1] = b; out[2] = a / b; }
        else { out[2 * (int64_t)blockIdx.x] = a; out[2 * (int64_t)blockIdx.x + 1] = b; }
    }
}

__global__ __launch_bounds__(SIG_THREADS) void k_signal_fill(float *out, int64_t n, float v) {
    const int64_t i = (int64_t)blockIdx.x * SIG_THREADS + threadIdx.x;
    if (i < n) out[i] = v;
}

// out[i] = bound * u_i, u_i uniform on the 2^24 multiples of 2^-23 in [-1, 1), from the counter RNG of the edge dropout
__global__ __launch_bounds__(SIG_THREADS) void k_signal_uniform(float *out, int64_t n, float bound, uint64_t seed, uint64_t stream,
                                                                const uint64_t *offset) {
    const int64_t i = (int64_t)blockIdx.x * SIG_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = hash_u24(seed, stream + (offset ? *offset : 0), (uint64_t)i, 0, 0);
    out[i] = bound * ((float)((int32_t)h - (1 << 23)) * (1.f / 8388608.f));
}

// f_i = act(sum_c X[i, c] w[c]): G lanes per row, each takes its columns (VEC: its float4s, then the row's last C % 4 values one per
// lane) in ascending order, then the xor tree
template <int G, bool VEC>
__global__ __launch_bounds__(SIG_THREADS) void k_signal_project(const float *__restrict__ X, int64_t ldx, int64_t n, int C,
                                                                const float *__restrict__ w, int act, float *__restrict__ out) {
    const int sub = threadIdx.x % G;
    const int64_t row = (int64_t)blockIdx.x * (SIG_THREADS / G) + threadIdx.x / G;
    float acc = 0.f;
    if (row < n) {
        const float *x = X + row * ldx;
        if constexpr (VEC) {
            const int C4 = C / 4;
            for (int j = sub; j < C4; j += G) {
                const float4 v = *reinterpret_cast<const float4 *>(x + 4 * j);
                acc = fmaf(v.x, w[4 * j], acc);
                acc = fmaf(v.y, w[4 * j + 1], acc);
                acc = fmaf(v.z, w[4 * j + 2], acc);
                acc = fmaf(v.w, w[4 * j + 3], acc);
            }
            for (int c = 4 * C4 + sub; c < C; c += G) acc = fmaf(x[c], w[c], acc);
        } else {
            for (int c = sub; c < C; c += G) acc = fmaf(x[c], w[c], acc);
        }
    }
    acc = xor_tree<G>(acc);
    if (row < n && sub == 0) out[row] = act ? 1.f / (1.f + expf(-acc)) : acc;
}

template <int G>
void launch_project(bool vec, const float *X, int64_t ldx, int64_t n, int C, const float *w, int act, float *out, hipStream_t s) {
    const dim3 grid(blocks_for(n, SIG_THREADS / G)), threads(SIG_THREADS);
    if (vec) hipLaunchKernelGGL((k_signal_project<G, true>), grid, threads, 0, s, X, ldx, n, C, w, act, out);
    else hipLaunchKernelGGL((k_signal_project<G, false>), grid, threads, 0, s, X, ldx, n, C, w, act, out);
}

template <int EPI>
void launch_rows_epi(const SignalArgs &p, hipStream_t s) {
    const dim3 grid(blocks_for(p.n_rows, SIG_SLAB_ROWS)), threads(SIG_THREADS);
#ifdef GNX_TUNING   // tuning builds: GNX_SIGNAL_LANES=4 in the environment runs the other candidate (tools/signal_bench.py --only groups)
    const char *e = getenv("GNX_SIGNAL_LANES");
    if (e && atoi(e) == 4) {
        hipLaunchKernelGGL((k_signal_rows<4, EPI>), grid, threads, 0, s, p);
        return;
    }
#endif
    hipLaunchKernelGGL((k_signal_rows<GNX_SIGNAL_GROUP, EPI>), grid, threads, 0, s, p);
}

// the structure's part of the arguments; sizes the hub rows' slab
int bind_structure(gnx_graph *g, const Csr &m, const float *vals, SignalArgs &p, hipStream_t s) {
    p.rowptr = m.rowptr; p.colidx = m.colidx; p.vals = vals;
    p.row_order = m.row_order;
    p.long_rows = m.long_rows; p.long_chunk_ptr = m.long_chunk_ptr; p.chunk_long = m.chunk_long;
    p.n_rows = m.n_rows; p.n_long = m.n_long; p.n_chunks = m.n_chunks;
    p.long_row = m.long_row; p.long_chunk = m.long_chunk;
    if (m.n_chunks > 0) {
        const int rc = ensure_partial(g, (size_t)m.n_chunks * sizeof(float), s);
        if (rc != GNX_OK) return rc;
    }
    p.partial = g->partial;
    return GNX_OK;
}

template <int EPI>
int launch_signal(gnx_graph *g, SignalArgs &p, const char *name, const char *name_long, hipStream_t s) {
    if (p.n_rows == 0) return GNX_OK;
    if (p.n_chunks > 0) hipLaunchKernelGGL(k_signal_chunks, dim3(blocks_for(p.n_chunks, SIG_THREADS / 64)), dim3(SIG_THREADS), 0, s, p);
    launch_rows_epi<EPI>(p, s);
    GNX_HIP(hipGetLastError());
    g->last_kernel = p.n_chunks > 0 ? name_long : name;
    return GNX_OK;
}

int64_t slab_count(int64_t n) { return (n + SIG_SLAB_ROWS - 1) / SIG_SLAB_ROWS; }

#define SIG_STR2(x) #x
#define SIG_STR(x) SIG_STR2(x)
#define SIG_NAME(what) "signal_" what "_group" SIG_STR(GNX_SIGNAL_GROUP)

}  // namespace
}  // namespace gnx

using namespace gnx;

extern "C" {

int gnx_signal_project(const float *d_X, int64_t ldx, int64_t n, int64_t C, const float *d_w, int act, float *d_out, void *stream) {
    GNX_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "gnx_signal_project: row count %lld outside [0, 2^31)", (long long)n);
    GNX_CHECK_ARG(C >= 1 && C < ((int64_t)1 << 24), "gnx_signal_project: width %lld outside [1, 2^24)", (long long)C);
    GNX_CHECK_ARG(ldx >= C, "gnx_signal_project: ldx %lld < C %lld", (long long)ldx, (long long)C);
    GNX_CHECK_ARG(act == 0 || act == 1, "gnx_signal_project: act %d is neither 0 (the dot product) nor 1 (sigmoid)", act);
    if (n == 0) return GNX_OK;
    GNX_CHECK_ARG(d_X && d_w && d_out, "gnx_signal_project: NULL buffer");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = C >= 4 && ldx % 4 == 0 && ((uintptr_t)d_X % 16) == 0;
    const int64_t per_lane = vec ? 16 : 4;      // values a lane should find before a second lane pays
    if (C >= 4 * per_lane) launch_project<16>(vec, d_X, ldx, n, (int)C, d_w, act, d_out, s);
    else if (C >= per_lane) launch_project<4>(vec, d_X, ldx, n, (int)C, d_w, act, d_out, s);
    else launch_project<1>(vec, d_X, ldx, n, (int)C, d_w, act, d_out, s);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_signal_spmv(gnx_graph_t g, const float *d_vals, int transposed, const float *d_x, const float *d_h0, float beta, float alpha,
                    float *d_out, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_signal_spmv: NULL handle");
    GNX_CHECK_ARG(d_x != nullptr || g->a.nnz == 0, "gnx_signal_spmv: NULL signal");
    GNX_CHECK_ARG(d_out != nullptr || (transposed ? g->a.n_cols : g->a.n_rows) == 0, "gnx_signal_spmv: NULL output");
    GNX_CHECK_ARG(d_out == nullptr || d_out != d_x, "gnx_signal_spmv: the output must not be the gathered signal");
    hipStream_t s = (hipStream_t)stream;
    if (transposed) {
        const int rc = ensure_transpose(g, s);
        if (rc != GNX_OK) return rc;
    }
    SignalArgs p{};
    const float *vals = d_vals ? d_vals : transposed ? g->t_raw.get() : g->raw_vals.get();
    const int rc = bind_structure(g, transposed ? g->t : g->a, vals, p, s);
    if (rc != GNX_OK) return rc;
    p.x = d_x; p.h0 = d_h0; p.beta = beta; p.alpha = alpha; p.out = d_out;
    return launch_signal<EPI_MIX>(g, p, SIG_NAME("spmv"), SIG_NAME("spmv") "+long", s);
}

int gnx_signal_ppr(gnx_graph_t g, const float *d_vals, const float *d_h0, float a, int K, float *d_out, float *d_work, void *stream) {
    GNX_CHECK_ARG(K >= 0, "gnx_signal_ppr: negative iteration count");
    GNX_CHECK_ARG(g != nullptr, "gnx_signal_ppr: NULL handle");
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "gnx_signal_ppr: needs a square graph");
    const int64_t n = g->a.n_rows;
    if (n == 0) return GNX_OK;
    // the work buffer: from two iterations on, and for one iteration over the constant signal (which has to stand somewhere)
    GNX_CHECK_ARG(d_out != nullptr && (d_work != nullptr || (K < 2 && (d_h0 != nullptr || K < 1))), "gnx_signal_ppr: NULL buffer");
    GNX_CHECK_ARG((d_h0 == nullptr || (d_out != d_h0 && d_work != d_h0)) && d_out != d_work, "gnx_signal_ppr: h0, out and work must be distinct");
    hipStream_t s = (hipStream_t)stream;
    const float beta = (float)(1.0 - (double)a);
    // iteration k writes dst(k); the constant signal 1 (h0 == NULL) starts in the buffer iteration 0 does not write
    auto dst = [&](int k) { return ((K - 1 - k) % 2 == 0) ? d_out : d_work; };
    const float *src = d_h0;
    if (d_h0 == nullptr) {
        float *ones = K == 0 ? d_out : (dst(0) == d_out ? d_work : d_out);
        hipLaunchKernelGGL(k_signal_fill, dim3(blocks_for(n, SIG_THREADS)), dim3(SIG_THREADS), 0, s, ones, n, 1.f);
        GNX_HIP(hipGetLastError());
        src = ones;
    } else if (K == 0) {
        GNX_HIP(hipMemcpyAsync(d_out, d_h0, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    for (int k = 0; k < K; ++k) {
        const int rc = gnx_signal_spmv(g, d_vals, 0, src, d_h0, beta, a, dst(k), stream);
        if (rc != GNX_OK) return rc;
        src = dst(k);
    }
    return GNX_OK;
}

int gnx_signal_smoothness(gnx_graph_t g, const float *d_vals, const float *d_f, const float *d_colsum, float *d_diff_out,
                          float *d_sums_out, float *d_work, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_signal_smoothness: NULL handle");
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "gnx_signal_smoothness: needs a square graph");
    GNX_CHECK_ARG(d_sums_out != nullptr && d_work != nullptr, "gnx_signal_smoothness: NULL buffer");
    const int64_t n = g->a.n_rows;
    GNX_CHECK_ARG(n == 0 || (d_f && d_colsum && d_diff_out), "gnx_signal_smoothness: NULL buffer");
    GNX_CHECK_ARG(n == 0 || d_diff_out != d_f, "gnx_signal_smoothness: the differences must not overwrite the signal");
    hipStream_t s = (hipStream_t)stream;
    SignalArgs p{};
    const int rc = bind_structure(g, g->a, d_vals ? d_vals : g->raw_vals.get(), p, s);
    if (rc != GNX_OK) return rc;
    p.x = d_f; p.f = d_f; p.colsum = d_colsum; p.out = d_diff_out; p.slabs = d_work;
    const int rc2 = launch_signal<EPI_SMOOTH>(g, p, SIG_NAME("smooth"), SIG_NAME("smooth") "+long", s);
    if (rc2 != GNX_OK) return rc2;
    float *cur = d_work;
    int64_t n_cur = slab_count(n);
    while (n_cur > SIG_SUM_SPAN) {      // levels between: each leaves its pairs behind the level it read
        const int64_t n_next = (n_cur + SIG_SUM_SPAN - 1) / SIG_SUM_SPAN;
        float *next = cur + 2 * n_cur;
        hipLaunchKernelGGL(k_signal_sum, dim3((unsigned)n_next), dim3(SIG_THREADS), 0, s, cur, n_cur, next, 0);
        cur = next; n_cur = n_next;
    }
    hipLaunchKernelGGL(k_signal_sum, dim3(1), dim3(SIG_THREADS), 0, s, cur, n_cur, d_sums_out, 1);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_signal_smoothness_back(gnx_graph_t g, const float *d_vals_t, const float *d_f, const float *d_diff, const float *d_colsum,
                               const float *d_sums, const float *d_upstream, float *d_gz_out, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_signal_smoothness_back: NULL handle");
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "gnx_signal_smoothness_back: needs a square graph");
    const int64_t n = g->a.n_rows;
    if (n == 0) return GNX_OK;
    GNX_CHECK_ARG(d_f && d_diff && d_colsum && d_sums && d_upstream && d_gz_out, "gnx_signal_smoothness_back: NULL buffer");
    GNX_CHECK_ARG(d_gz_out != d_diff && d_gz_out != d_f, "gnx_signal_smoothness_back: the gradient must not overwrite an operand");
    hipStream_t s = (hipStream_t)stream;
    const int rc = ensure_transpose(g, s);
    if (rc != GNX_OK) return rc;
    SignalArgs p{};
    const int rc2 = bind_structure(g, g->t, d_vals_t ? d_vals_t : g->t_raw.get(), p, s);
    if (rc2 != GNX_OK) return rc2;
    p.x = d_diff; p.d = d_diff; p.f = d_f; p.colsum = d_colsum; p.sums = d_sums; p.upstream = d_upstream; p.out = d_gz_out;
    return launch_signal<EPI_BACK>(g, p, SIG_NAME("back"), SIG_NAME("back") "+long", s);
}

int gnx_signal_uniform(gnx_graph_t g, int64_t n, float bound, uint64_t seed, uint64_t stream_id, float *d_out, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_signal_uniform: NULL handle");
    GNX_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "gnx_signal_uniform: count %lld outside [0, 2^31)", (long long)n);
    if (n == 0) return GNX_OK;
    GNX_CHECK_ARG(d_out != nullptr, "gnx_signal_uniform: NULL output");
    hipLaunchKernelGGL(k_signal_uniform, dim3(blocks_for(n, SIG_THREADS)), dim3(SIG_THREADS), 0, (hipStream_t)stream, d_out, n, bound, seed,
                       stream_id, g->stream_offset);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

}  // extern "C"
