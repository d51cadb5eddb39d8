// Normalisation of the adjacency on gfx950: GNN.get_adjacency of the reference
// (gnntf/core/gnn/gnn.py:36-50) and the edge dropout in front of it
// (gnntf/core/nn/layered.py:47-50).  All of this is HBM-bound integer/float streaming over
// nnz-sized arrays; no LDS tiling is needed, only coalesced slot-parallel passes.
#include "gnx_internal.h"
#include <type_traits>
#include <utility>

using namespace gnx;

namespace {

struct Drop {
    uint64_t seed, stream;
    const uint64_t *offset;    // optional device counter added to the stream id (graph-captured training steps)
    uint32_t thr;    // keep iff hash >= thr
    float scale;     // 1/(1-p)
    const float *e_vals;       // entry values (null when no duplicates)
    const int64_t *slot_ptr;   // entry range per slot (null when no duplicates)
    int64_t row0;              // vertex block (gnx_graph_set_block): global id of row 0, else 0
    const int32_t *gid;        // vertex block: global id of every column, else null
};

// the (row, col) the dropout draw of an entry is keyed by: global ids when the handle is a vertex block
__device__ __forceinline__ uint64_t key_row(const Drop &d, int64_t row) { return (uint64_t)(row + d.row0); }
__device__ __forceinline__ uint64_t key_col(const Drop &d, int64_t col) { return d.gid ? (uint64_t)d.gid[col] : (uint64_t)col; }

__device__ __forceinline__ uint64_t stream_of(const Drop &d) { return d.stream + (d.offset ? *d.offset : 0); }

// value of coalesced slot k after per-entry dropout (layered.py:50: kept * 1/(1-p), dropped -> 0)
template <bool DROPOUT>
__device__ __forceinline__ float slot_value(const float *__restrict__ raw, const Drop &d, int64_t k, int32_t row, int32_t col) {
    if (!DROPOUT) return raw[k];
    if (d.slot_ptr == nullptr)
        return hash_u24(d.seed, stream_of(d), key_row(d, row), key_col(d, col), 0) >= d.thr ? raw[k] * d.scale : 0.f;
    float acc = 0.f;
    const int64_t b = d.slot_ptr[k], e = d.slot_ptr[k + 1];
    const uint64_t kr = key_row(d, row), kc = key_col(d, col);
    for (int64_t i = b; i < e; ++i)
        if (hash_u24(d.seed, stream_of(d), kr, kc, (uint64_t)(i - b)) >= d.thr) acc = kept_term(acc, d.e_vals[i], d.scale);   // (gnx_internal.h: slot_kept_sum rounds alike)
    return acc;
}

// the same for position p of the transposed structure; without duplicates the raw value is read from
// the transposed-order copy (a streaming read instead of a gather through t_perm)
template <bool DROPOUT>
__device__ __forceinline__ float t_value(const float *__restrict__ raw, const float *__restrict__ t_raw,
                                         const int32_t *__restrict__ t_perm, const Drop &d, int64_t p, int32_t row, int32_t col) {
    if (d.slot_ptr != nullptr) return slot_value<DROPOUT>(raw, d, t_perm[p], row, col);
    const float v = t_raw[p];
    if (!DROPOUT) return v;
    return hash_u24(d.seed, stream_of(d), key_row(d, row), key_col(d, col), 0) >= d.thr ? v * d.scale : 0.f;
}

// ---- column sums over the transposed structure ---------------------------------------------------------------------------------
// Two walks, each written once.  k_colsum_short: 8 lanes per column, lane `sub` adds the positions b + sub, b + sub + 8, ... of its
// column in that order from 0.f, then the xor tree 4, 2, 1.  k_colsum_long: one 256-thread block per column of more than long_row
// entries (the short walk leaves those alone), thread i adds the positions b + i, b + i + 256, ..., then an LDS tree from 128 down
// to 1.  What ONE position contributes is the walk's Term: add(acc, ns, p, c) adds position p of a column into acc[NS], one sum per
// dropout stream of the batch (out[s * n_cols + j], s < ns <= NS; a batch holds at least one stream); c = column(j) is what the
// term wants to know of column j, made once per column (the dropout key of a vertex block's column is a gather, and the compiler
// does not move it out of the walk on its own).  The lane mapping, the order of additions and the reduction trees do not depend on
// the term, so every stream's sums are bit for bit the single-stream sums, whichever term made them.  A term that is LISTED may be
// launched over the list of the columns that have entries.

// one stream: the slot's value after dropout (gnx_graph_colsum; a handle with duplicates but without entry tables walks its entry lists)
template <bool DROPOUT>
struct SlotTerm {
    static constexpr int MAX_NS = 1;
    static constexpr bool LISTED = false;
    const int32_t *t_colidx, *t_perm;
    const float *raw, *t_raw;
    Drop d;
    template <int NS>
    __device__ __forceinline__ void add(float (&acc)[NS], int, int64_t p, int32_t j) const {
        acc[0] += t_value<DROPOUT>(raw, t_raw, t_perm, d, p, t_colidx[p], j);
    }
    __device__ __forceinline__ int32_t column(int64_t j) const { return (int32_t)j; }
};

// one stream of a handle without duplicates (gnx_graph_colsum_streams with one stream): SlotTerm<true>'s sum without its entry-list
// branch and the t_perm it would gather through, the column's key made once (profiles/NOTES.md, "The column sums written once":
// 5 to 8 % of the config-4 graph's one-stream sums)
struct StreamTerm {
    static constexpr int MAX_NS = 1;
    static constexpr bool LISTED = false;
    const int32_t *t_colidx;
    const float *t_raw;
    Drop d;
    template <int NS>
    __device__ __forceinline__ void add(float (&acc)[NS], int, int64_t p, uint64_t kc) const {
        const float v = t_raw[p] * d.scale;
        acc[0] += hash_u24(d.seed, stream_of(d), key_row(d, t_colidx[p]), kc, 0) >= d.thr ? v : 0.f;
    }
    __device__ __forceinline__ uint64_t column(int64_t j) const { return key_col(d, j); }
};

// The sums of up to 16 streams in TWO passes (training steps: K streams at once, gnx_graph_colsum_streams; no duplicate entries).  With
// the hashes inside the column walk, the loop's trip count differs from lane to lane (8 lanes per column, columns of every length in
// one wave): most of the VALU time goes to lanes that have run out of entries (measured round 4: 5.5 ms for 8 streams over 10^8
// entries, hash-bound).  Pass 1 hashes with EVERY lane busy -- one lane per transposed position, all streams of the batch, the keep
// bits packed into one 16-bit word per entry; pass 2 is the column walk over MaskTerm, a 2-byte read where the hashes were.
__global__ __launch_bounds__(256) void k_keep_masks(const int32_t *__restrict__ t_rowidx /* column of A */, const int32_t *__restrict__ t_colidx /* row of A */,
                                                    int64_t nnz, Drop d, int ns, uint16_t *__restrict__ mask) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const uint64_t row = key_row(d, t_colidx[p]), kc = key_col(d, t_rowidx[p]);
    const uint64_t stream = stream_of(d);
    uint32_t bits = 0;
#pragma unroll 2
    for (int s = 0; s < ns; ++s) bits |= (hash_u24(d.seed, stream + s, row, kc, 0) >= d.thr ? 1u : 0u) << s;
    mask[p] = (uint16_t)bits;
}

struct MaskTerm {
    static constexpr int MAX_NS = 16;
    static constexpr bool LISTED = true;
    const float *t_raw;
    const uint16_t *mask;    // k_keep_masks
    float scale;
    template <int NS>
    __device__ __forceinline__ void add(float (&acc)[NS], int, int64_t p, int) const {
        const float v = t_raw[p] * scale;
        const uint32_t m = mask[p];
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s] += ((m >> s) & 1u) ? v : 0.f;
    }
    __device__ __forceinline__ int column(int64_t) const { return 0; }
};

// up to 16 streams on a handle with duplicate entries (gnx_graph_enable_entry_dropout): each position's kept slot sum made per stream
// from the entry tables in transposed order (slot_kept_sum: a uniform slot reads its multiplicity and value, a general one walks its
// entries through t_perm), the structure read once for all of them
struct EntryTerm {
    static constexpr int MAX_NS = 16;
    static constexpr bool LISTED = false;
    const int32_t *t_colidx, *t_perm;
    const uint8_t *t_mult;
    const float *t_uval;
    Drop d;
    template <int NS>
    __device__ __forceinline__ void add(float (&acc)[NS], int ns, int64_t p, uint64_t kc) const {
        const uint64_t row = key_row(d, t_colidx[p]), stream = stream_of(d);
        const uint32_t m = t_mult[p];
        const float uval = t_uval[p];
        const int64_t slot = m == ENTRY_GENERAL ? (int64_t)t_perm[p] : 0;
#pragma unroll
        for (int s = 0; s < NS; ++s)
            if (NS == 1 || s < ns) acc[s] += slot_kept_sum(hash_key(d.seed, stream + s, row, kc), d.thr, d.scale, m, uval, d.e_vals, d.slot_ptr, slot);
    }
    __device__ __forceinline__ uint64_t column(int64_t j) const { return key_col(d, j); }
};

// ``list`` / ``n_slots`` (a LISTED term): the columns WITH entries in ascending order (the transposed structure's nonempty_rows; the
// sums of the others are zeroed by the caller and their lanes never launched), or null / n_cols.  Compiled in for such a term only:
// the columns of an R-MAT graph hold ten entries on average, and the look-up showed in the time of the one-stream sums.
template <int NS, class Term>
__global__ void k_colsum_short(const int64_t *__restrict__ t_rowptr, Term term, int ns, int64_t n_cols, int long_row,
                               const int32_t *__restrict__ list, int64_t n_slots, float *__restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t j = gid >> 3;
    if constexpr (Term::LISTED) j = j < n_slots ? (list ? (int64_t)list[j] : j) : n_cols;
    const int sub = (int)(gid & 7);
    float acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.f;
    bool is_long = false;
    if (j < n_cols) {
        const int64_t b = t_rowptr[j], e = t_rowptr[j + 1];
        is_long = (e - b) > long_row;
        if (!is_long) {
            const auto c = term.column(j);
            for (int64_t p = b + sub; p < e; p += 8) term.add(acc, ns, p, c);
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float a = acc[s];
        a += __shfl_xor(a, 4);
        a += __shfl_xor(a, 2);
        a += __shfl_xor(a, 1);
        if (j < n_cols && sub == 0 && !is_long && (NS == 1 || s < ns)) out[(int64_t)s * n_cols + j] = a;
    }
}

template <int NS, class Term>
__global__ __launch_bounds__(256) void k_colsum_long(const int64_t *__restrict__ t_rowptr, Term term, int ns,
                                                     const int32_t *__restrict__ long_rows, int64_t n_cols, float *__restrict__ out) {
    __shared__ float red[256];
    const int32_t j = long_rows[blockIdx.x];
    const int64_t b = t_rowptr[j], e = t_rowptr[j + 1];
    float acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.f;
    const auto c = term.column(j);
    for (int64_t p = b + threadIdx.x; p < e; p += 256) term.add(acc, ns, p, c);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (NS == 1 || s < ns) {                                     // (block-uniform)
            if (s > 0) __syncthreads();                              // red[] of stream s - 1 has been read
            red[threadIdx.x] = acc[s];
            __syncthreads();
            for (int w = 128; w > 0; w >>= 1) {
                if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
                __syncthreads();
            }
            if (threadIdx.x == 0) out[(int64_t)s * n_cols + j] = red[0];
        }
    }
}

// gnx_graph_enable_entry_dropout: per coalesced slot its multiplicity and, when all its entries are the same float, that value
__global__ void k_entry_tables(const float *__restrict__ e_vals, const int64_t *__restrict__ slot_ptr, int64_t nslots,
                               uint8_t *__restrict__ mult, float *__restrict__ uval) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nslots) return;
    const int64_t b = slot_ptr[k], e = slot_ptr[k + 1];
    const uint32_t bits = __float_as_uint(e_vals[b]);
    bool uniform = e - b < (int64_t)ENTRY_GENERAL;
    for (int64_t i = b + 1; uniform && i < e; ++i) uniform = __float_as_uint(e_vals[i]) == bits;
    mult[k] = uniform ? (uint8_t)(e - b) : (uint8_t)ENTRY_GENERAL;
    uval[k] = uniform ? __uint_as_float(bits) : 0.f;
}

__global__ void k_permute_entry_tables(const int32_t *__restrict__ perm, int64_t n, const uint8_t *__restrict__ mult,
                                       const float *__restrict__ uval, uint8_t *__restrict__ t_mult, float *__restrict__ t_uval) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int32_t k = perm[p];
    t_mult[p] = mult[k];
    t_uval[p] = uval[k];
}

// gnn.py:41 / :44 with optional "+I before" folded in as +1 on every column sum
__global__ void k_degree_scale(float *__restrict__ d, int64_t n, int normalized, float eye) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    float x = d[j] + eye;
    if (normalized == GNX_NORM_SYMMETRIC) x = sqrtf(x);
    d[j] = (x != 0.f) ? 1.0f / x : 0.f;   // tf.math.divide_no_nan(1., x)
}

// gnn.py:42 / :45: v_ij <- (rs[i] * v_ij) * cs[j], written in slot order or, TRANSPOSED, in the order of the transposed structure:
// position k then holds entry (row = t_colidx[k], col = t_rowidx[k]) of A, which the caller passes as rowidx / colidx
template <bool DROPOUT, bool TRANSPOSED>
__global__ void k_scale_values(const int32_t *__restrict__ rowidx, const int32_t *__restrict__ colidx,
                               const int32_t *__restrict__ t_perm, const float *__restrict__ raw,
                               const float *__restrict__ t_raw, Drop d, const float *__restrict__ rs,
                               const float *__restrict__ cs, int64_t nnz, float *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz) return;
    const int32_t r = rowidx[k], c = colidx[k];
    float v = TRANSPOSED ? t_value<DROPOUT>(raw, t_raw, t_perm, d, k, r, c) : slot_value<DROPOUT>(raw, d, k, r, c);
    if (rs) v = rs[r] * v;
    if (cs) v = v * cs[c];
    out[k] = v;
}

// diagonal weight of the identity added by add_eye (gnn.py:39,49)
__global__ void k_diag(const float *__restrict__ deg, int64_t n, int mode /*0: ones, 1: deg^2, 2: deg*/, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = mode == 0 ? 1.0f : (mode == 1 ? deg[i] * 1.0f * deg[i] : deg[i]);
}

int make_drop(gnx_graph *g, float p, uint64_t seed, uint64_t stream_id, Drop &d) {
    GNX_CHECK_ARG(p >= 0.f && p < 1.f, "dropout rate %g outside [0, 1)", (double)p);
    d.seed = seed; d.stream = stream_id; d.offset = g->stream_offset;
    d.thr = drop_threshold(p);
    d.scale = drop_scale(p);
    d.e_vals = g->has_dups ? g->e_vals : nullptr;
    d.slot_ptr = g->has_dups ? g->slot_ptr : nullptr;
    d.row0 = g->blk_row0_global; d.gid = g->blk_col_gid;
    return GNX_OK;
}

int ensure_deg(gnx_graph *g) {
    if (g->deg) return GNX_OK;
    GNX_HIP(g->deg.alloc(g->a.n_cols));
    return GNX_OK;
}

template <int N> using IntC = std::integral_constant<int, N>;

// f(IntC<NS>) for the accumulators per lane a batch of ns streams takes (one for a term that only ever sums one stream)
template <class Term, typename F>
void with_streams(int ns, F &&f) {
    if constexpr (Term::MAX_NS > 1) {
        if (ns > 8) return f(IntC<16>{});
        if (ns > 4) return f(IntC<8>{});
        if (ns > 2) return f(IntC<4>{});
        if (ns > 1) return f(IntC<2>{});
    }
    return f(IntC<1>{});
}

// f(std::true_type) with dropout, f(std::false_type) without
template <typename F>
void with_dropout(float p, F &&f) {
    if (p > 0.f) f(std::true_type{});
    else f(std::false_type{});
}

// the column sums of one batch of ns streams over the transposed structure t (t.n_rows > 0) into out[s * t.n_rows + j]: the short walk
// and, where the plan has long columns, the long one.  ``trim`` (a LISTED term): only the columns that have entries are launched
// (ascending: the stores stay in order); the caller has zeroed the sums of the others
template <class Term>
void launch_colsums(const Csr &t, const Term &term, int ns, bool trim, float *out, hipStream_t s) {
    const int64_t n_slots = trim ? t.n_nonempty : t.n_rows;
    with_streams<Term>(ns, [&](auto NS) {
        hipLaunchKernelGGL((k_colsum_short<NS(), Term>), dim3(blocks_for(n_slots * 8)), dim3(256), 0, s, t.rowptr, term, ns, t.n_rows,
                           t.long_row, trim ? t.nonempty_rows : nullptr, n_slots, out);
        if (t.n_long > 0)
            hipLaunchKernelGGL((k_colsum_long<NS(), Term>), dim3((unsigned)t.n_long), dim3(256), 0, s, t.rowptr, term, ns, t.long_rows,
                               t.n_rows, out);
    });
}

template <bool DROPOUT>
SlotTerm<DROPOUT> slot_term(const gnx_graph *g, const Drop &d) { return {g->t.colidx, g->t_perm, g->raw_vals, g->t_raw, d}; }

}  // namespace

extern "C" {

int gnx_graph_set_dropout_counter(gnx_graph_t g, const uint64_t *d_counter) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_set_dropout_counter: NULL handle");
    g->stream_offset = d_counter;
    return GNX_OK;
}

int gnx_graph_set_block(gnx_graph_t g, int64_t row0_global, int64_t row0_buf, const int32_t *d_col_gid, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_set_block: NULL handle");
    if (d_col_gid == nullptr) {                              // back to a stand-alone graph
        g->blk_col_gid.reset();
        g->blk_row0_global = 0; g->blk_row0_buf = 0;
        return GNX_OK;
    }
    GNX_CHECK_ARG(row0_global >= 0 && row0_buf >= 0 && row0_buf + g->a.n_rows <= g->a.n_cols,
                  "gnx_graph_set_block: the %lld rows do not fit behind column %lld of %lld", (long long)g->a.n_rows,
                  (long long)row0_buf, (long long)g->a.n_cols);
    if (!g->blk_col_gid) GNX_HIP(g->blk_col_gid.alloc(g->a.n_cols));
    GNX_HIP(hipMemcpyAsync(g->blk_col_gid, d_col_gid, g->a.n_cols * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    g->blk_row0_global = row0_global; g->blk_row0_buf = row0_buf;
    return GNX_OK;
}

int gnx_graph_enable_entry_dropout(gnx_graph_t g, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_enable_entry_dropout: NULL handle");
    if (!g->has_dups || g->entry_drop) return GNX_OK;
    hipStream_t s = (hipStream_t)stream;
    GNX_CHECK_ARG(!stream_is_capturing(s), "gnx_graph_enable_entry_dropout: the stream is being captured -- enable before the capture begins");
    int rc = ensure_transpose(g, s);
    if (rc != GNX_OK) return rc;
    const int64_t nnz = g->a.nnz;
    DevArray<uint8_t> m, tm;                                  // handed to the handle once all four are made
    DevArray<float> v, tv;
    GNX_HIP(m.alloc(nnz));
    GNX_HIP(tm.alloc(nnz));
    GNX_HIP(v.alloc(nnz));
    GNX_HIP(tv.alloc(nnz));
    hipLaunchKernelGGL(k_entry_tables, dim3(blocks_for(nnz)), dim3(256), 0, s, g->e_vals, g->slot_ptr, nnz, m, v);
    hipLaunchKernelGGL(k_permute_entry_tables, dim3(blocks_for(nnz)), dim3(256), 0, s, g->t_perm, nnz, m, v, tm, tv);
    GNX_HIP(hipGetLastError());
    GNX_HIP(hipStreamSynchronize(s));
    g->ed_mult = std::move(m); g->t_ed_mult = std::move(tm); g->ed_vals = std::move(v); g->t_ed_vals = std::move(tv);
    g->entry_drop = true;
    return GNX_OK;
}

int gnx_graph_colsum(gnx_graph_t g, float dropout_p, uint64_t seed, uint64_t stream_id, float *d_colsum_out, void *stream) {
    GNX_CHECK_ARG(g != nullptr && d_colsum_out != nullptr, "gnx_graph_colsum: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_transpose(g, s);
    if (rc != GNX_OK) return rc;
    Drop d;
    rc = make_drop(g, dropout_p, seed, stream_id, d);
    if (rc != GNX_OK) return rc;
    const Csr &t = g->t;
    if (t.n_rows == 0) return GNX_OK;
    with_dropout(dropout_p, [&](auto DROPOUT) { launch_colsums(t, slot_term<DROPOUT()>(g, d), 1, false, d_colsum_out, s); });
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_graph_colsum_streams(gnx_graph_t g, float dropout_p, uint64_t seed, uint64_t first_stream, int n_streams, float *d_colsum_out,
                             void *stream) {
    GNX_CHECK_ARG(g != nullptr && d_colsum_out != nullptr, "gnx_graph_colsum_streams: NULL argument");
    GNX_CHECK_ARG(n_streams >= 1 && n_streams <= 4096, "gnx_graph_colsum_streams: bad stream count %d", n_streams);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = g->a.n_cols;
    const bool tables = g->has_dups && g->entry_drop;        // gnx_graph_enable_entry_dropout
    if (dropout_p <= 0.f || (g->has_dups && !tables)) {      // no dropout / entry lists: one stream at a time through gnx_graph_colsum
        for (int k = 0; k < n_streams; ++k) {
            int rc = gnx_graph_colsum(g, dropout_p, seed, first_stream + k, d_colsum_out + (int64_t)k * n, stream);
            if (rc != GNX_OK) return rc;
        }
        return GNX_OK;
    }
    int rc = ensure_transpose(g, s);
    if (rc != GNX_OK) return rc;
    const Csr &t = g->t;
    if (t.n_rows == 0) return GNX_OK;
    // without entry tables, two passes per batch: keep bits with every lane busy, then the column walk over 2-byte masks
    const bool masked = !tables && n_streams >= 2 && t.nnz > 0;
    if (masked && !g->t_mask) {
        if (stream_is_capturing(s)) {
            set_error("gnx_graph_colsum_streams: the keep-bit scratch of this handle would have to be allocated while the stream is being "
                      "captured: call gnx_graph_reserve(handle, C, GNX_RESERVE_TRANSPOSED) or run the call once eagerly before capturing");
            return GNX_ERR_UNSUPPORTED;
        }
        GNX_HIP(g->t_mask.alloc(t.nnz));
    }
    const int per_batch = tables || masked ? 16 : 1;         // one stream (or no entry at all): a single pass per stream
    for (int k0 = 0; k0 < n_streams; k0 += per_batch) {
        const int ns = n_streams - k0 < per_batch ? n_streams - k0 : per_batch;
        Drop d;
        rc = make_drop(g, dropout_p, seed, first_stream + k0, d);
        if (rc != GNX_OK) return rc;
        float *out = d_colsum_out + (int64_t)k0 * n;
        if (tables) {
            launch_colsums(t, EntryTerm{t.colidx, g->t_perm, g->t_ed_mult, g->t_ed_vals, d}, ns, false, out, s);
        } else if (masked) {
            hipLaunchKernelGGL(k_keep_masks, dim3(blocks_for(t.nnz)), dim3(256), 0, s, g->t_rowidx, t.colidx, t.nnz, d, ns, g->t_mask);
            // only the columns that have entries; the sums of the others are zero
            const bool trim = t.nonempty_rows != nullptr && t.n_nonempty < t.n_rows;
            if (trim) GNX_HIP(hipMemsetAsync(out, 0, (size_t)ns * (size_t)n * sizeof(float), s));
            launch_colsums(t, MaskTerm{g->t_raw, g->t_mask, d.scale}, ns, trim, out, s);
        } else {
            launch_colsums(t, StreamTerm{t.colidx, g->t_raw, d}, 1, false, out, s);
        }
    }
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_degree_scale(float *d_deg, int64_t n, int normalized, int add_eye_before, void *stream) {
    GNX_CHECK_ARG(n >= 0 && (n == 0 || d_deg != nullptr), "gnx_degree_scale: NULL array");
    GNX_CHECK_ARG(normalized == GNX_NORM_SYMMETRIC || normalized == GNX_NORM_BIPARTITE,
                  "Invalid matrix normalization");
    if (n == 0) return GNX_OK;
    hipLaunchKernelGGL(k_degree_scale, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, d_deg, n, normalized,
                       add_eye_before ? 1.0f : 0.0f);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

// the values in slot order or in transposed order (k_scale_values)
static int scale_values_any(gnx_graph_t g, bool transposed, float dropout_p, uint64_t seed, uint64_t stream_id,
                            const float *rs, const float *cs, float *out, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    int rc = transposed ? ensure_transpose(g, s) : GNX_OK;
    if (rc != GNX_OK) return rc;
    Drop d;
    rc = make_drop(g, dropout_p, seed, stream_id, d);
    if (rc != GNX_OK) return rc;
    const int64_t nnz = g->a.nnz;
    if (nnz == 0) return GNX_OK;
    with_dropout(dropout_p, [&](auto DROPOUT) {
        if (transposed) hipLaunchKernelGGL((k_scale_values<DROPOUT(), true>), dim3(blocks_for(nnz)), dim3(256), 0, s, g->t.colidx, g->t_rowidx,
                                           g->t_perm, g->raw_vals, g->t_raw, d, rs, cs, nnz, out);
        else            hipLaunchKernelGGL((k_scale_values<DROPOUT(), false>), dim3(blocks_for(nnz)), dim3(256), 0, s, g->rowidx, g->a.colidx,
                                           nullptr, g->raw_vals, nullptr, d, rs, cs, nnz, out);
    });
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_graph_scale_values(gnx_graph_t g, float dropout_p, uint64_t seed, uint64_t stream_id, const float *d_row_scale,
                           const float *d_col_scale, float *d_vals_out, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_scale_values: NULL handle");
    GNX_CHECK_ARG(g->a.nnz == 0 || d_vals_out != nullptr, "gnx_graph_scale_values: NULL output");
    return scale_values_any(g, false, dropout_p, seed, stream_id, d_row_scale, d_col_scale, d_vals_out, stream);
}

static int normalize_impl(const char *fn, gnx_graph_t g, bool transposed, int normalized, int add_eye, float dropout_p,
                          uint64_t seed, uint64_t stream_id, float *d_vals_out, float *d_diag_out, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(normalized == GNX_NORM_NONE || normalized == GNX_NORM_SYMMETRIC || normalized == GNX_NORM_BIPARTITE,
                  "Invalid matrix normalization");
    GNX_CHECK_ARG(add_eye == GNX_EYE_NONE || add_eye == GNX_EYE_BEFORE || add_eye == GNX_EYE_AFTER,
                  "%s: invalid add_eye %d", fn, add_eye);
    GNX_CHECK_ARG(g->a.nnz == 0 || d_vals_out != nullptr, "%s: NULL output", fn);
    GNX_CHECK_ARG(add_eye == GNX_EYE_NONE || d_diag_out != nullptr, "%s: add_eye needs d_diag_out", fn);
    GNX_CHECK_ARG((normalized == GNX_NORM_NONE && add_eye == GNX_EYE_NONE) || g->a.n_rows == g->a.n_cols,
                  "%s: normalisation / add_eye need a square graph (%lld x %lld)", fn,
                  (long long)g->a.n_rows, (long long)g->a.n_cols);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = g->a.n_rows;
    int rc;
    if (normalized == GNX_NORM_NONE) {
        rc = scale_values_any(g, transposed, dropout_p, seed, stream_id, nullptr, nullptr, d_vals_out, stream);
        if (rc != GNX_OK) return rc;
        if (add_eye != GNX_EYE_NONE && n > 0)
            hipLaunchKernelGGL(k_diag, dim3(blocks_for(n)), dim3(256), 0, s, (const float *)nullptr, n, 0, d_diag_out);
        GNX_HIP(hipGetLastError());
        return GNX_OK;
    }
    rc = ensure_deg(g);
    if (rc != GNX_OK) return rc;
    rc = gnx_graph_colsum(g, dropout_p, seed, stream_id, g->deg, stream);
    if (rc != GNX_OK) return rc;
    rc = gnx_degree_scale(g->deg, g->a.n_cols, normalized, add_eye == GNX_EYE_BEFORE, stream);
    if (rc != GNX_OK) return rc;
    rc = scale_values_any(g, transposed, dropout_p, seed, stream_id, g->deg,
                          normalized == GNX_NORM_SYMMETRIC ? g->deg : nullptr, d_vals_out, stream);
    if (rc != GNX_OK) return rc;
    if (add_eye != GNX_EYE_NONE && n > 0) {
        const int mode = add_eye == GNX_EYE_AFTER ? 0 : (normalized == GNX_NORM_SYMMETRIC ? 1 : 2);
        hipLaunchKernelGGL(k_diag, dim3(blocks_for(n)), dim3(256), 0, s, g->deg, n, mode, d_diag_out);
    }
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_graph_normalize(gnx_graph_t g, int normalized, int add_eye, float dropout_p, uint64_t seed, uint64_t stream_id,
                        float *d_vals_out, float *d_diag_out, void *stream) {
    return normalize_impl("gnx_graph_normalize", g, false, normalized, add_eye, dropout_p, seed, stream_id, d_vals_out,
                          d_diag_out, stream);
}

int gnx_graph_normalize_t(gnx_graph_t g, int normalized, int add_eye, float dropout_p, uint64_t seed, uint64_t stream_id,
                          float *d_vals_t_out, float *d_diag_out, void *stream) {
    return normalize_impl("gnx_graph_normalize_t", g, true, normalized, add_eye, dropout_p, seed, stream_id, d_vals_t_out,
                          d_diag_out, stream);
}

}  // extern "C"
