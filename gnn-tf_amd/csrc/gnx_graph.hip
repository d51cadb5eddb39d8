// Graph handle: COO -> sorted entries -> coalesced CSR (+ lazy transposed structure) on gfx950.
// Replaces the tf.sparse.SparseTensor that gnntf's graph2adj returns
// (reference gnntf/core/gnn/graph_manipulation.py:24-31) as the container of the adjacency.
#include <cstring>
#include <string.h>

#include "gnx_internal.h"
#include <algorithm>
#include <memory>
#include <type_traits>
#include <utility>

#include <rocprim/rocprim.hpp>

namespace gnx {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static unsigned bits_for(uint64_t max_key_exclusive) {
    unsigned b = 1;
    while (b < 64 && (max_key_exclusive >> b) != 0) ++b;
    return b;
}

// ---- kernels ---------------------------------------------------------------------------
__global__ void k_make_keys(const int64_t *__restrict__ indices, int64_t nnz, int64_t n_rows, int64_t n_cols,
                            uint64_t *__restrict__ keys, int *__restrict__ bad) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    int64_t r = indices[2 * e], c = indices[2 * e + 1];
    if (r < 0 || r >= n_rows || c < 0 || c >= n_cols) {
        atomicExch(bad, 1);
        r = 0; c = 0;
    }
    keys[e] = (uint64_t)r * (uint64_t)n_cols + (uint64_t)c;
}

__global__ void k_heads(const uint64_t *__restrict__ keys, int64_t nnz, int32_t *__restrict__ head) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    head[e] = (e == 0 || keys[e] != keys[e - 1]) ? 1 : 0;
}

// slot = inclusive_scan(head) - 1
__global__ void k_fill_slots(const uint64_t *__restrict__ keys, const int32_t *__restrict__ scan, int64_t nnz,
                             int64_t n_cols, int32_t *__restrict__ colidx, int32_t *__restrict__ rowidx,
                             int64_t *__restrict__ slot_ptr /* may be null */) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const bool is_head = (e == 0) || (scan[e] != scan[e - 1]);
    if (!is_head) return;
    const int32_t s = scan[e] - 1;
    const uint64_t k = keys[e];
    rowidx[s] = (int32_t)(k / (uint64_t)n_cols);
    colidx[s] = (int32_t)(k % (uint64_t)n_cols);
    if (slot_ptr) slot_ptr[s] = e;
}

__global__ void k_sum_slots(const float *__restrict__ e_vals, const int64_t *__restrict__ slot_ptr, int64_t nslots,
                            float *__restrict__ out) {
    int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    float acc = 0.f;
    for (int64_t e = slot_ptr[s]; e < slot_ptr[s + 1]; ++e) acc += e_vals[e];  // input order
    out[s] = acc;
}

// ptr[r] = first position p with sorted_rows[p] >= r  (r in [0, n_rows]); sorted_rows int32 ascending
__global__ void k_lower_bound_rows(const int32_t *__restrict__ sorted_rows, int64_t nnz, int64_t n_rows,
                                   int64_t *__restrict__ ptr) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rows) return;
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if ((int64_t)sorted_rows[mid] < r) lo = mid + 1; else hi = mid;
    }
    ptr[r] = lo;
}

__global__ void k_rows_from_ptr(const int64_t *__restrict__ rowptr, int64_t n_rows, int32_t *__restrict__ rowidx) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    for (int64_t e = rowptr[r]; e < rowptr[r + 1]; ++e) rowidx[e] = (int32_t)r;
}

__global__ void k_check_csr(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t n_rows,
                            int64_t n_cols, int64_t nnz, int *__restrict__ bad) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    int64_t b = rowptr[r], e = rowptr[r + 1];
    if (b > e || b < 0 || e > nnz || (r == 0 && b != 0) || (r == n_rows - 1 && e != nnz)) { atomicExch(bad, 1); return; }
    for (int64_t k = b; k < e; ++k) {
        int32_t c = colidx[k];
        if (c < 0 || c >= n_cols || (k > b && colidx[k - 1] >= c)) { atomicExch(bad, 1); return; }
    }
}

__global__ void k_flag_long(const int64_t *__restrict__ rowptr, int64_t n_rows, int long_row, int long_chunk,
                            int32_t *__restrict__ flag, int64_t *__restrict__ cnt) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    int64_t d = rowptr[r + 1] - rowptr[r];
    bool lg = d > long_row;
    flag[r] = lg ? 1 : 0;
    cnt[r] = lg ? (d + long_chunk - 1) / long_chunk : 0;
}

// sort key of the degree-binned row order: clamp - min(entries, clamp), so an ascending stable sort puts the
// heaviest rows first and keeps ascending row ids inside a bin.  The clamp covers every row the sub-wave kernels take
// (up to the threshold entries): the rows that share a wave then have EQUAL lengths, also in the 256..512 range
__global__ void k_order_keys(const int64_t *__restrict__ rowptr, int64_t n_rows, int clamp, uint16_t *__restrict__ keys,
                             int32_t *__restrict__ ids) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    int64_t d = rowptr[r + 1] - rowptr[r];
    keys[r] = (uint16_t)(clamp - (d < clamp ? d : clamp));
    ids[r] = (int32_t)r;
}

// The same bins inside WINDOWS of the caller's numbering (Csr::order_window): key = (window, bin); rows without entries get the
// window past the last one, so that they still trail the whole order (the launchers cut the order there)
__global__ void k_order_keys_windowed(const int64_t *__restrict__ rowptr, int64_t n_rows, int clamp, int64_t window, uint32_t n_windows,
                                      unsigned bin_bits, uint32_t *__restrict__ keys, int32_t *__restrict__ ids) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    int64_t d = rowptr[r + 1] - rowptr[r];
    const uint32_t w = d == 0 ? n_windows : (uint32_t)(r / window);
    keys[r] = (w << bin_bits) | (uint32_t)(clamp - (d < clamp ? d : clamp));
    ids[r] = (int32_t)r;
}

__global__ void k_slot_ptrs(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ row_order, int64_t n_rows,
                            int64_t *__restrict__ slot_beg, int32_t *__restrict__ slot_cnt) {
    int64_t sidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (sidx >= n_rows) return;
    const int64_t r = row_order[sidx], b = rowptr[r], e = rowptr[r + 1];
    slot_beg[sidx] = b;
    slot_cnt[sidx] = (int32_t)(e - b < 0x7fffffff ? e - b : 0x7fffffff);
}

__global__ void k_count_nonempty(const int64_t *__restrict__ rowptr, int64_t n_rows, unsigned long long *__restrict__ count) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool has = r < n_rows && rowptr[r + 1] > rowptr[r];
    const unsigned long long votes = __popcll(__ballot(has));
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(count, votes);
}

__global__ void k_mark_referenced(const int32_t *__restrict__ colidx, int64_t nnz, uint8_t *__restrict__ flag) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nnz) flag[colidx[k]] = 1;
}

__global__ void k_count_empty_referenced(const int64_t *__restrict__ rowptr, int64_t n, const uint8_t *__restrict__ flag, int *__restrict__ count) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n && rowptr[r + 1] == rowptr[r] && flag[r]) atomicAdd(count, 1);
}

__global__ void k_fill_long(const int64_t *__restrict__ rowptr, int64_t n_rows, int long_row, int long_chunk,
                            const int32_t *__restrict__ pos,
                            const int64_t *__restrict__ cpos, int32_t *__restrict__ long_rows,
                            int64_t *__restrict__ long_chunk_ptr, int32_t *__restrict__ chunk_long) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    int64_t d = rowptr[r + 1] - rowptr[r];
    if (d <= long_row) return;
    const int32_t p = pos[r];
    const int64_t c0 = cpos[r];
    const int64_t nc = (d + long_chunk - 1) / long_chunk;
    long_rows[p] = (int32_t)r;
    long_chunk_ptr[p] = c0;
    for (int64_t c = 0; c < nc; ++c) chunk_long[c0 + c] = p;
}

// key of a long-row chunk = the first column it touches: chunks are then processed in column-window order, so
// that at any time the long-row waves gather from one window of columns and its hub rows stay cached
__global__ void k_chunk_keys(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                             const int32_t *__restrict__ long_rows, const int64_t *__restrict__ long_chunk_ptr,
                             const int32_t *__restrict__ chunk_long, int64_t n_chunks, int long_chunk,
                             uint32_t *__restrict__ keys, int32_t *__restrict__ ids) {
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const int32_t li = chunk_long[c];
    const int64_t beg = rowptr[long_rows[li]] + (c - long_chunk_ptr[li]) * long_chunk;
    keys[c] = (uint32_t)colidx[beg];
    ids[c] = (int32_t)c;
}

__global__ void k_make_tkeys(const int32_t *__restrict__ rowidx, const int32_t *__restrict__ colidx, int64_t nnz,
                             int64_t n_rows, uint64_t *__restrict__ keys, int32_t *__restrict__ payload) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz) return;
    keys[k] = (uint64_t)colidx[k] * (uint64_t)n_rows + (uint64_t)rowidx[k];
    payload[k] = (int32_t)k;
}

// relabelling (vertex row_order[i] -> i): newid = inverse of row_order; key of an entry = newid[row] * n + newid[col]
__global__ void k_invert_order(const int32_t *__restrict__ order, int64_t n, int32_t *__restrict__ newid) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) newid[order[i]] = (int32_t)i;
}

__global__ void k_make_rkeys(const int32_t *__restrict__ rowidx, const int32_t *__restrict__ colidx, const int32_t *__restrict__ newid,
                             int64_t nnz, int64_t n, uint64_t *__restrict__ keys, int32_t *__restrict__ payload) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz) return;
    keys[k] = (uint64_t)newid[rowidx[k]] * (uint64_t)n + (uint64_t)newid[colidx[k]];
    payload[k] = (int32_t)k;
}

// relabelling order inside a degree bin: key[v] = smallest degree rank among v's neighbours (its most popular neighbour)
__global__ void k_min_neighbour_rank(const int32_t *__restrict__ rowidx, const int32_t *__restrict__ colidx, const int32_t *__restrict__ rank,
                                     int64_t nnz, int32_t *__restrict__ key) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nnz) atomicMin(&key[rowidx[k]], rank[colidx[k]]);
}

__global__ void k_relabel_keys(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ key, int64_t n, int clamp,
                               uint64_t *__restrict__ keys, int32_t *__restrict__ ids) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int64_t d = rowptr[r + 1] - rowptr[r];
    const uint64_t bin = (uint64_t)(clamp - (d < clamp ? d : clamp));          // k_order_keys' bins: heaviest first
    keys[r] = (bin << 32) | (uint64_t)(uint32_t)key[r];
    ids[r] = (int32_t)r;
}

// gcol[k] = rank[colidx[k]]: the position of every entry's column in the gather order
__global__ void k_gather_columns(const int32_t *__restrict__ colidx, const int32_t *__restrict__ rank, int64_t nnz,
                                 int32_t *__restrict__ gcol) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nnz) gcol[k] = rank[colidx[k]];
}

// gather hints: rows by descending entry count (a stable sort of these keys keeps ties in id order) ...
__global__ void k_hint_keys(const int64_t *__restrict__ rowptr, int64_t n, uint64_t *__restrict__ keys, int32_t *__restrict__ ids) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    keys[r] = (uint64_t)(0x7fffffff - (rowptr[r + 1] - rowptr[r]));
    ids[r] = (int32_t)r;
}

// ... and per entry its column, bit 31 set when the column is not among the first `hot` rows of that order
__global__ void k_hint_columns(const int32_t *__restrict__ colidx, const int32_t *__restrict__ rank, int64_t nnz, int64_t hot,
                               int32_t *__restrict__ hint_cols) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz) return;
    const int32_t c = colidx[k];
    hint_cols[k] = rank[c] < hot ? c : (int32_t)((uint32_t)c | 0x80000000u);
}

// pendant elision, plan.  A candidate: one entry (i, h), h != i, and h stores at least two ...
__global__ void k_pend_candidates(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t n, uint8_t *__restrict__ flag) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t b = rowptr[i];
    uint8_t f = 0;
    if (rowptr[i + 1] - b == 1) {
        const int64_t h = colidx[b];
        f = h != i && rowptr[h + 1] - rowptr[h] >= 2;
    }
    flag[i] = f;
}

// ... which no row but h stores as a column (an integer store of 0; every writer writes the same value)
__global__ void k_pend_disqualify(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const int32_t *__restrict__ rowidx,
                                  int64_t nnz, uint8_t *__restrict__ flag) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz) return;
    const int32_t c = colidx[k];
    if (flag[c] && colidx[rowptr[c]] != rowidx[k]) flag[c] = 0;
}

// rows with flag f (count[0]) and rows of exactly one entry (count[1])
__global__ void k_pend_count(const int64_t *__restrict__ rowptr, const uint8_t *__restrict__ flag, int64_t n, unsigned long long *__restrict__ count) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < n;
    const unsigned long long f = __popcll(__ballot(in && flag[i])), one = __popcll(__ballot(in && rowptr[i + 1] - rowptr[i] == 1));
    if ((threadIdx.x & 63) == 0) {
        if (f) atomicAdd(count, f);
        if (one) atomicAdd(count + 1, one);
    }
}

// out[k] = flag[rows[k]]: the sort key that moves the elidable rows of the one-entry bin behind the others, and the per-slot mark
__global__ void k_pend_gather_flag(const int32_t *__restrict__ rows, const uint8_t *__restrict__ flag, int64_t n, uint8_t *__restrict__ out) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = flag[rows[k]];
}

// per entry the hinted column with PEND_COL_BIT where the column is elidable; a row that stores such an entry is marked
__global__ void k_pend_columns(const int32_t *__restrict__ hint_cols, const int32_t *__restrict__ rowidx, const uint8_t *__restrict__ flag,
                               int64_t nnz, int32_t *__restrict__ pend_cols, uint8_t *__restrict__ row_mark) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz) return;
    const int32_t j = hint_cols[k];
    if (flag[j & 0x7fffffff]) {
        pend_cols[k] = j | PEND_COL_BIT;
        row_mark[rowidx[k]] = 1;
    } else {
        pend_cols[k] = j;
    }
}

// per call: pend_w[i] = the value of the one entry of every elidable row i (`rows` = their slots of the row order)
__global__ void k_pend_weights(const int32_t *__restrict__ rows, int64_t n, const int64_t *__restrict__ rowptr, const float *__restrict__ vals,
                               float *__restrict__ pend_w) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int32_t i = rows[k];
    pend_w[i] = vals[rowptr[i]];
}

__global__ void k_permute_vals(const float *__restrict__ vals, const int32_t *__restrict__ perm, int64_t n,
                               float *__restrict__ out) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = vals[perm[k]];
}

__global__ void k_split_tkeys(const uint64_t *__restrict__ keys, int64_t nnz, int64_t n_rows,
                              int32_t *__restrict__ t_row /* = column of A */, int32_t *__restrict__ t_col /* = row of A */) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnz) return;
    t_row[k] = (int32_t)(keys[k] / (uint64_t)n_rows);
    t_col[k] = (int32_t)(keys[k] % (uint64_t)n_rows);
}

// ---- helpers -------------------------------------------------------------------------------
#define GNX_TRY(...)                                                                    \
    do {                                                                                \
        const int _rc = (__VA_ARGS__);                                                  \
        if (_rc != GNX_OK) return _rc;                                                  \
    } while (0)

// rocprim's calling convention: with a null temporary a call only reports the bytes it needs, the same call again with that many
// does the work.  `call(tmp, bytes)` is that call.  Waits for the work, because the temporary goes when this returns.
template <class Call>
static int with_temporary(const char *what, Call call, hipStream_t s) {
    DevArray<char> tmp;
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e == hipSuccess) e = tmp.alloc(bytes);
    if (e == hipSuccess) e = call(tmp.get(), bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        set_error("rocprim::%s failed: %s", what, hipGetErrorString(e));
        return GNX_ERR_HIP;
    }
    return GNX_OK;
}

// Stable ascending sort of n (key, value) pairs by key bits [0, end_bit).  V is const where the caller's own array is sorted.
template <class K, class V>
static int sort_pairs(K *keys_in, K *keys_out, V *vals_in, std::remove_const_t<V> *vals_out, int64_t n, unsigned end_bit, hipStream_t s) {
    return with_temporary("radix_sort_pairs", [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, end_bit, s);
    }, s);
}

static int sort_keys(int32_t *keys_in, int32_t *keys_out, int64_t n, unsigned end_bit, hipStream_t s) {
    return with_temporary("radix_sort_keys", [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_keys(tmp, bytes, keys_in, keys_out, (size_t)n, 0u, end_bit, s);
    }, s);
}

template <class T>
static int exclusive_scan(T *in, T *out, int64_t n, hipStream_t s) {   // sums, from 0
    return with_temporary("exclusive_scan", [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, in, out, (T)0, (size_t)n, rocprim::plus<T>(), s);
    }, s);
}

static int inclusive_scan(int32_t *in, int32_t *out, int64_t n, hipStream_t s) {
    return with_temporary("inclusive_scan", [&](void *tmp, size_t &bytes) {
        return rocprim::inclusive_scan(tmp, bytes, in, out, (size_t)n, rocprim::plus<int32_t>(), s);
    }, s);
}

// one value of a device array, waited for
template <class T>
static int fetch(T &host, const T *dev, hipStream_t s) {
    GNX_HIP(hipMemcpyAsync(&host, dev, sizeof(T), hipMemcpyDeviceToHost, s));
    GNX_HIP(hipStreamSynchronize(s));
    return GNX_OK;
}

// m.row_order = the rows in stable ascending order of the key_bits-wide keys of type K that `make_keys(keys, ids)` launches
template <class K, class MakeKeys>
static int order_rows(Csr &m, unsigned key_bits, MakeKeys make_keys, hipStream_t s) {
    DevArray<K> k0, k1;
    DevArray<int32_t> ids;
    GNX_HIP(k0.alloc(m.n_rows)); GNX_HIP(k1.alloc(m.n_rows)); GNX_HIP(ids.alloc(m.n_rows));
    GNX_HIP(m.row_order.alloc(m.n_rows));
    make_keys(k0.get(), ids.get());
    return sort_pairs<K, int32_t>(k0, k1, ids, m.row_order, m.n_rows, key_bits, s);
}

int build_long_plan(Csr &m, hipStream_t s) {
    m.n_long = 0; m.n_chunks = 0;
    const bool small = m.n_rows >= TINY_ROWS && m.n_rows < SMALL_ROWS;       // see gnx_internal.h
    m.long_row = small ? SMALL_LONG_ROW : LONG_ROW;
    m.long_chunk = small ? SMALL_LONG_ROW : LONG_CHUNK;
    const int order_clamp = m.long_row < 65535 ? m.long_row : 65535;
    if (m.n_rows == 0) return GNX_OK;
    const dim3 row_blocks(blocks_for(m.n_rows)), threads(256);
    const unsigned bin_bits = bits_for((uint64_t)order_clamp + 1);
    if (m.order_window > 0) {   // degree bins inside windows of the caller's numbering
        const uint64_t n_windows = (uint64_t)((m.n_rows + m.order_window - 1) / m.order_window);
        const unsigned key_bits = bin_bits + bits_for(n_windows + 1);
        GNX_CHECK_ARG(key_bits <= 32, "row window: %lld windows of %lld rows do not fit the order key", (long long)n_windows,
                      (long long)m.order_window);
        GNX_TRY(order_rows<uint32_t>(m, key_bits, [&](uint32_t *keys, int32_t *ids) {
            hipLaunchKernelGGL(k_order_keys_windowed, row_blocks, threads, 0, s, m.rowptr, m.n_rows, order_clamp, m.order_window,
                               (uint32_t)n_windows, bin_bits, keys, ids);
        }, s));
    } else {   // degree-binned row order
        GNX_TRY(order_rows<uint16_t>(m, bin_bits, [&](uint16_t *keys, int32_t *ids) {
            hipLaunchKernelGGL(k_order_keys, row_blocks, threads, 0, s, m.rowptr, m.n_rows, order_clamp, keys, ids);
        }, s));
    }
    if (m.n_rows >= SMALL_ROWS) {   // big structures: the rows' entry ranges in slot order
        GNX_HIP(m.slot_beg.alloc(m.n_rows));
        GNX_HIP(m.slot_cnt.alloc(m.n_rows));
        hipLaunchKernelGGL(k_slot_ptrs, row_blocks, threads, 0, s, m.rowptr, m.row_order, m.n_rows, m.slot_beg, m.slot_cnt);
    }
    {   // rows with entries: they lead the order (heaviest first), the empty ones trail it
        DevArray<unsigned long long> count;
        GNX_HIP(count.alloc(1));
        GNX_HIP(hipMemsetAsync(count, 0, sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_count_nonempty, row_blocks, threads, 0, s, m.rowptr, m.n_rows, count);
        unsigned long long host = 0;
        GNX_TRY(fetch(host, count.get(), s));
        m.n_nonempty = (int64_t)host;
    }
    m.empty_rows_unreferenced = false;
    if (m.n_nonempty < m.n_rows) {
        if (m.n_nonempty > 0) {   // the rows with entries in ascending order: the leading slots of row_order, sorted by id
            GNX_HIP(m.nonempty_rows.alloc(m.n_nonempty));
            GNX_TRY(sort_keys(m.row_order, m.nonempty_rows, m.n_nonempty, bits_for((uint64_t)m.n_rows), s));
        }
        if (m.n_rows == m.n_cols) {   // does any entry point at a row that has no entries itself?
            DevArray<uint8_t> flag;
            DevArray<int> count;
            GNX_HIP(flag.alloc(m.n_rows)); GNX_HIP(count.alloc(1));
            GNX_HIP(hipMemsetAsync(flag, 0, m.n_rows, s));
            GNX_HIP(hipMemsetAsync(count, 0, sizeof(int), s));
            if (m.nnz > 0) hipLaunchKernelGGL(k_mark_referenced, dim3(blocks_for(m.nnz)), threads, 0, s, m.colidx, m.nnz, flag);
            hipLaunchKernelGGL(k_count_empty_referenced, row_blocks, threads, 0, s, m.rowptr, m.n_rows, flag, count);
            int host_count = 1;
            GNX_TRY(fetch(host_count, count.get(), s));
            m.empty_rows_unreferenced = host_count == 0;
        }
    }
    if (m.nnz == 0) return GNX_OK;
    DevArray<int32_t> flag, pos;
    DevArray<int64_t> cnt, cpos;
    GNX_HIP(flag.alloc(m.n_rows));
    GNX_HIP(cnt.alloc(m.n_rows));
    GNX_HIP(pos.alloc(m.n_rows));
    GNX_HIP(cpos.alloc(m.n_rows));
    hipLaunchKernelGGL(k_flag_long, row_blocks, threads, 0, s, m.rowptr, m.n_rows, m.long_row, m.long_chunk, flag, cnt);
    GNX_TRY(exclusive_scan<int32_t>(flag, pos, m.n_rows, s));
    GNX_TRY(exclusive_scan<int64_t>(cnt, cpos, m.n_rows, s));
    int32_t last_flag = 0, last_pos = 0;
    int64_t last_cnt = 0, last_cpos = 0;
    GNX_TRY(fetch(last_flag, flag + (m.n_rows - 1), s));
    GNX_TRY(fetch(last_pos, pos + (m.n_rows - 1), s));
    GNX_TRY(fetch(last_cnt, cnt + (m.n_rows - 1), s));
    GNX_TRY(fetch(last_cpos, cpos + (m.n_rows - 1), s));
    m.n_long = (int64_t)last_flag + last_pos;
    m.n_chunks = last_cnt + last_cpos;
    if (m.n_long == 0) return GNX_OK;
    GNX_HIP(m.long_rows.alloc(m.n_long));
    GNX_HIP(m.long_chunk_ptr.alloc(m.n_long + 1));
    GNX_HIP(m.chunk_long.alloc(m.n_chunks));
    hipLaunchKernelGGL(k_fill_long, row_blocks, threads, 0, s, m.rowptr, m.n_rows, m.long_row, m.long_chunk, pos, cpos, m.long_rows,
                       m.long_chunk_ptr, m.chunk_long);
    GNX_HIP(hipMemcpyAsync(m.long_chunk_ptr + m.n_long, &m.n_chunks, 8, hipMemcpyHostToDevice, s));
    // column-window order of the chunks
    DevArray<uint32_t> k0, k1;
    DevArray<int32_t> ids;
    GNX_HIP(k0.alloc(m.n_chunks)); GNX_HIP(k1.alloc(m.n_chunks)); GNX_HIP(ids.alloc(m.n_chunks));
    GNX_HIP(m.chunk_order.alloc(m.n_chunks));
    hipLaunchKernelGGL(k_chunk_keys, dim3(blocks_for(m.n_chunks)), threads, 0, s, m.rowptr, m.colidx, m.long_rows, m.long_chunk_ptr,
                       m.chunk_long, m.n_chunks, m.long_chunk, k0, ids);
    return sort_pairs<uint32_t, int32_t>(k0, k1, ids, m.chunk_order, m.n_chunks, 32u, s);
}

// A stream that is being captured into a hipGraph must not see hipMalloc / hipFree / synchronisation: the lazily built parts of
// a handle (long-row slab, transposed structure, relabelled copy, gather order) refuse to grow there and say how to prepare them.
bool stream_is_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}

#define GNX_NOT_WHILE_CAPTURING(s, what)                                                                                         \
    do {                                                                                                                         \
        if (stream_is_capturing(s)) {                                                                                            \
            set_error("%s would have to be allocated while the stream is being captured into a hipGraph: call "                  \
                      "gnx_graph_reserve(handle, C, flags) -- or run the same call once eagerly -- before the capture begins", what); \
            return GNX_ERR_UNSUPPORTED;                                                                                          \
        }                                                                                                                        \
    } while (0)

// A slab that only ever grows; growing frees, then allocates (one slab at the peak; an implicit device synchronisation), which is why
// it never happens under capture.
static int grow_slab(DevArray<float> &slab, size_t &held_bytes, size_t bytes) {
    held_bytes = 0;
    GNX_HIP(slab.alloc((bytes + sizeof(float) - 1) / sizeof(float)));
    held_bytes = bytes;
    return GNX_OK;
}

// The slab the long-row chunks of a launch write their partial sums to ([chunks x C] floats), grown on demand (gnx_graph_reserve
// sizes it ahead of time for the widest C a client will use).
int ensure_partial(gnx_graph *g, size_t bytes, hipStream_t s) {
    if (bytes <= g->partial_bytes) return GNX_OK;
    GNX_NOT_WHILE_CAPTURING(s, "the long-row slab of this handle");
    return grow_slab(g->partial, g->partial_bytes, bytes);
}

int ensure_relabel_features(gnx_graph *g, size_t bytes, hipStream_t s) {
    if (bytes <= g->r_feat_bytes) return GNX_OK;
    GNX_NOT_WHILE_CAPTURING(s, "the feature scratch of this handle's relabelled copy");
    return grow_slab(g->r_feat, g->r_feat_bytes, bytes);
}

// Dropping a lazy part = assigning a fresh one (the parts: gnx_internal.h).  The gather order and the per-entry gather columns go
// whenever the relabelled copy, which is numbered in that order, goes.
static void drop_transpose(gnx_graph *g) { static_cast<TransposedPart &>(*g) = TransposedPart(); }
static void drop_relabel(gnx_graph *g) { static_cast<RelabelledPart &>(*g) = RelabelledPart(); }
static void drop_gather_order(gnx_graph *g) { static_cast<GatherOrderPart &>(*g) = GatherOrderPart(); }
static void drop_gather_hints(gnx_graph *g) { static_cast<GatherHintsPart &>(*g) = GatherHintsPart(); }

// Built aside and moved into the handle when complete: no half-built state on failure.
int ensure_transpose(gnx_graph *g, hipStream_t s) {
    if (g->has_t) return GNX_OK;
    GNX_NOT_WHILE_CAPTURING(s, "the transposed structure of this handle");
    const Csr &a = g->a;
    TransposedPart part;
    Csr &t = part.t;
    t.n_rows = a.n_cols; t.n_cols = a.n_rows; t.nnz = a.nnz;
    t.order_window = a.n_rows == a.n_cols ? a.order_window : 0;     // a square graph's columns share the rows' numbering
    GNX_HIP(t.rowptr.alloc(t.n_rows + 1));
    GNX_HIP(t.colidx.alloc(t.nnz));
    GNX_HIP(part.t_perm.alloc(t.nnz));
    GNX_HIP(part.t_vals.alloc(t.nnz));
    GNX_HIP(part.t_raw.alloc(t.nnz));
    DevArray<uint64_t> k0, k1;
    DevArray<int32_t> p0;
    if (t.nnz == 0) {
        GNX_HIP(hipMemsetAsync(t.rowptr, 0, (t.n_rows + 1) * sizeof(int64_t), s));
    } else {
        const dim3 entry_blocks(blocks_for(t.nnz)), threads(256);
        GNX_HIP(k0.alloc(t.nnz)); GNX_HIP(k1.alloc(t.nnz));
        GNX_HIP(p0.alloc(t.nnz));
        GNX_HIP(part.t_rowidx.alloc(t.nnz));
        hipLaunchKernelGGL(k_make_tkeys, entry_blocks, threads, 0, s, g->rowidx, a.colidx, a.nnz, a.n_rows, k0, p0);
        GNX_TRY(sort_pairs<uint64_t, int32_t>(k0, k1, p0, part.t_perm, t.nnz, bits_for((uint64_t)a.n_rows * (uint64_t)a.n_cols), s));
        hipLaunchKernelGGL(k_split_tkeys, entry_blocks, threads, 0, s, k1, t.nnz, a.n_rows, part.t_rowidx, t.colidx);
        hipLaunchKernelGGL(k_lower_bound_rows, dim3(blocks_for(t.n_rows + 1)), threads, 0, s, part.t_rowidx, t.nnz, t.n_rows, t.rowptr);
        hipLaunchKernelGGL(k_permute_vals, entry_blocks, threads, 0, s, g->raw_vals, part.t_perm, t.nnz, part.t_raw);
    }
    GNX_HIP(hipStreamSynchronize(s));
    GNX_TRY(build_long_plan(t, s));
    part.has_t = true;
    static_cast<TransposedPart &>(*g) = std::move(part);
    return GNX_OK;
}

// The gather order of a square handle: the degree bins of a.row_order (heaviest first) and, inside a bin, the vertices by the degree
// rank of their most popular neighbour, then by id (profiles/NOTES.md round 4: -4 % time, -16 % of the long-row kernel's fabric bytes
// at C = 8 against the plain degree order).  Hub rows become neighbours in memory and share 128-byte lines, a hub's leaves sit in
// consecutive lines.  go_order[i] = the vertex at position i, go_rank = its inverse.  Built once, on first use.
int ensure_gather_order(gnx_graph *g, hipStream_t s) {
    if (g->go_order) return GNX_OK;
    GNX_NOT_WHILE_CAPTURING(s, "the gather order of this handle");
    const Csr &a = g->a;
    GNX_CHECK_ARG(a.n_rows == a.n_cols && a.row_order != nullptr && a.n_rows > 0, "the gather order needs a non-empty square graph");
    const int64_t n = a.n_rows, nnz = a.nnz;
    const dim3 row_blocks(blocks_for(n)), threads(256);
    DevArray<int32_t> order, rank, key, ids;
    DevArray<uint64_t> k0, k1;
    GNX_HIP(order.alloc(n)); GNX_HIP(rank.alloc(n)); GNX_HIP(key.alloc(n)); GNX_HIP(ids.alloc(n));
    GNX_HIP(k0.alloc(n)); GNX_HIP(k1.alloc(n));
    hipLaunchKernelGGL(k_invert_order, row_blocks, threads, 0, s, a.row_order, n, rank);   // degree rank
    GNX_HIP(hipMemsetAsync(key, 0x7f, n * 4, s));                              // 0x7f7f7f7f: "no neighbour" sorts last
    if (nnz > 0)
        hipLaunchKernelGGL(k_min_neighbour_rank, dim3(blocks_for(nnz)), threads, 0, s, g->rowidx, a.colidx, rank, nnz, key);
    const int clamp = a.long_row < 65535 ? a.long_row : 65535;                 // as build_long_plan binned the rows
    hipLaunchKernelGGL(k_relabel_keys, row_blocks, threads, 0, s, a.rowptr, key, n, clamp, k0, ids);
    GNX_TRY(sort_pairs<uint64_t, int32_t>(k0, k1, ids, order, n, 32u + bits_for((uint64_t)clamp + 1), s));
    hipLaunchKernelGGL(k_invert_order, row_blocks, threads, 0, s, order, n, rank);
    GNX_HIP(hipStreamSynchronize(s));
    GNX_HIP(hipGetLastError());
    g->go_order = std::move(order);
    g->go_rank = std::move(rank);
    return GNX_OK;
}

// The matrix with its vertices renumbered in the gather order: same entries, rows and columns permuted alike, columns ascending
// inside a row.  Built once, on the first narrow-width propagation of a large square graph -- aside, like the transposed structure.
int ensure_relabel(gnx_graph *g, hipStream_t s) {
    if (g->has_r) return GNX_OK;
    GNX_NOT_WHILE_CAPTURING(s, "the relabelled copy of this handle");
    const Csr &a = g->a;
    GNX_CHECK_ARG(a.n_rows == a.n_cols && a.row_order != nullptr && a.nnz > 0, "relabelling needs a non-empty square graph");
    GNX_TRY(ensure_gather_order(g, s));
    const int64_t n = a.n_rows, nnz = a.nnz;
    const dim3 entry_blocks(blocks_for(nnz)), threads(256);
    RelabelledPart part;
    Csr &r = part.r;
    r.n_rows = n; r.n_cols = n; r.nnz = nnz;
    GNX_HIP(r.rowptr.alloc(n + 1));
    GNX_HIP(r.colidx.alloc(nnz));
    GNX_HIP(part.r_perm.alloc(nnz));
    GNX_HIP(part.r_vals.alloc(nnz));
    DevArray<uint64_t> k0, k1;
    DevArray<int32_t> p0, rrow;
    GNX_HIP(k0.alloc(nnz)); GNX_HIP(k1.alloc(nnz)); GNX_HIP(p0.alloc(nnz)); GNX_HIP(rrow.alloc(nnz));
    hipLaunchKernelGGL(k_make_rkeys, entry_blocks, threads, 0, s, g->rowidx, a.colidx, g->go_rank, nnz, n, k0, p0);
    GNX_TRY(sort_pairs<uint64_t, int32_t>(k0, k1, p0, part.r_perm, nnz, bits_for((uint64_t)n * (uint64_t)n), s));
    hipLaunchKernelGGL(k_split_tkeys, entry_blocks, threads, 0, s, k1, nnz, n, rrow, r.colidx);
    hipLaunchKernelGGL(k_lower_bound_rows, dim3(blocks_for(n + 1)), threads, 0, s, rrow, nnz, n, r.rowptr);
    GNX_HIP(hipStreamSynchronize(s));
    GNX_TRY(build_long_plan(r, s));
    part.has_r = true;
    static_cast<RelabelledPart &>(*g) = std::move(part);
    return GNX_OK;
}

// What gnx_spmm_dropped_chained_ord / gnx_spmm_dropped_back_ord walk: the transposed structure, the gather order, and per entry of
// either structure the position of its column in that order (4 bytes per entry each).  Stand-alone square handles without
// duplicate entries and without a row window (whose numbering carries its locality already).
int ensure_train_gather(gnx_graph *g, const char *fn, hipStream_t s) {
    if (g->blk_col_gid != nullptr) {
        set_error("%s: the handle is a vertex block (gnx_graph_set_block): the gather order exists for stand-alone graphs only", fn);
        return GNX_ERR_UNSUPPORTED;
    }
    if (g->has_dups) {
        set_error("%s: the graph holds duplicate COO entries: the gather order exists for handles without duplicates only", fn);
        return GNX_ERR_UNSUPPORTED;
    }
    if (g->a.order_window != 0) {
        set_error("%s: the handle has a row window (gnx_graph_set_row_window): its numbering carries locality already, the gather "
                  "order is not built", fn);
        return GNX_ERR_UNSUPPORTED;
    }
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "%s: needs a square graph", fn);
    if (g->a_gcol != nullptr) return GNX_OK;
    if (g->a.n_rows == 0) return GNX_OK;                             // nothing is ever launched
    GNX_NOT_WHILE_CAPTURING(s, "the gather-order columns of this handle (GNX_RESERVE_TRAIN_GATHER)");
    GNX_TRY(ensure_transpose(g, s));
    GNX_TRY(ensure_gather_order(g, s));
    const int64_t nnz = g->a.nnz;
    DevArray<int32_t> ac, tc;
    GNX_HIP(ac.alloc(nnz)); GNX_HIP(tc.alloc(nnz));
    if (nnz > 0) {
        hipLaunchKernelGGL(k_gather_columns, dim3(blocks_for(nnz)), dim3(256), 0, s, g->a.colidx, g->go_rank, nnz, ac);
        hipLaunchKernelGGL(k_gather_columns, dim3(blocks_for(nnz)), dim3(256), 0, s, g->t.colidx, g->go_rank, nnz, tc);
    }
    GNX_HIP(hipStreamSynchronize(s));
    GNX_HIP(hipGetLastError());
    g->t_gcol = std::move(tc);
    g->a_gcol = std::move(ac);
    return GNX_OK;
}

// ---- gather hints (gnx_graph_set_gather_hints; GatherHintsPart) -----------------------------------------------------------------
static bool takes_gather_hints(const gnx_graph *g) {
    return g->a.n_rows == g->a.n_cols && g->blk_col_gid == nullptr && g->a.order_window == 0 && g->a.nnz > 0;
}

// the hot_rows in force for a launch of C columns; 0 = the launch takes no hints
static int64_t hint_hot_rows(const gnx_graph *g, int64_t C) {
    if (!takes_gather_hints(g) || g->hint_setting == 0 || C * (int64_t)sizeof(float) < HINT_MIN_ROW_BYTES) return 0;
    const int64_t n = g->a.n_rows;
    if (g->hint_setting > 0) return std::min(g->hint_setting, n);
    if (n < HINT_MIN_ROWS) return 0;
    return std::min(n, std::max<int64_t>(1, HINT_HOT_BYTES / (C * (int64_t)sizeof(float))));
}

// hint_cols marked for `hot` rows: the degree order and the array on first use (built aside; not under capture), one pass over
// the entries whenever `hot` changes (in place and stream-ordered: only bit 31 changes, a launch that reads the array meanwhile
// still reads the right columns; under capture the array stays as it is).  An allocation that fails turns the hints off.
static int ensure_gather_hints(gnx_graph *g, int64_t hot, hipStream_t s) {
    const Csr &a = g->a;
    const dim3 threads(256);
    if (g->hint_cols == nullptr) {
        GNX_NOT_WHILE_CAPTURING(s, "the gather hints of this handle (GNX_RESERVE_GATHER_HINTS)");
        GatherHintsPart part;
        DevArray<uint64_t> k0, k1;
        DevArray<int32_t> ids, order;
        const size_t n = (size_t)a.n_rows;
        hipError_t e = part.hint_cols.alloc(a.nnz);
        if (e == hipSuccess) e = part.hint_rank.alloc(n);
        if (e == hipSuccess) e = k0.alloc(n);
        if (e == hipSuccess) e = k1.alloc(n);
        if (e == hipSuccess) e = ids.alloc(n);
        if (e == hipSuccess) e = order.alloc(n);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            g->hint_failed = true;
            set_error("gather hints: %s while allocating %lld bytes for the hinted columns: this handle runs unhinted", hipGetErrorString(e),
                      (long long)a.nnz * 4);
            return GNX_OK;
        }
        hipLaunchKernelGGL(k_hint_keys, dim3(blocks_for(a.n_rows)), threads, 0, s, a.rowptr, a.n_rows, k0, ids);
        GNX_TRY(sort_pairs<uint64_t, int32_t>(k0, k1, ids, order, a.n_rows, 31u, s));
        hipLaunchKernelGGL(k_invert_order, dim3(blocks_for(a.n_rows)), threads, 0, s, order, a.n_rows, part.hint_rank);   // kept as ranks
        GNX_HIP(hipStreamSynchronize(s));
        GNX_HIP(hipGetLastError());
        part.hint_hot = -1;
        static_cast<GatherHintsPart &>(*g) = std::move(part);
    }
    if (g->hint_hot != hot && !stream_is_capturing(s)) {
        hipLaunchKernelGGL(k_hint_columns, dim3(blocks_for(a.nnz)), threads, 0, s, a.colidx, g->hint_rank, a.nnz, hot, g->hint_cols);
        GNX_HIP(hipGetLastError());
        g->hint_hot = hot;
    }
    return GNX_OK;
}

int gather_hints_for(gnx_graph *g, const Csr &m, int64_t C, hipStream_t s, const int32_t **hint_cols) {
    *hint_cols = nullptr;
    if (&m != &g->a || g->hint_failed) return GNX_OK;
    const int64_t hot = hint_hot_rows(g, C);
    if (hot == 0) return GNX_OK;
    if (g->hint_cols == nullptr || g->hint_hot != hot) GNX_TRY(ensure_gather_hints(g, hot, s));
    *hint_cols = g->hint_cols;     // (null after a failed allocation)
    return GNX_OK;
}

// ---- pendant elision (gnx_graph_set_pendant_elision; PendantPart) ---------------------------------------------------------------
static void drop_pendants(gnx_graph *g) { static_cast<PendantPart &>(*g) = PendantPart(); }

static bool takes_pendant_elision(const gnx_graph *g) { return takes_gather_hints(g) && g->a.n_cols < (int64_t)PEND_COL_BIT; }

// The elidable rows, their place at the end of the one-entry bin of a.row_order, and the marks.  Not under capture.  Launches in
// flight on any stream may walk the row order while its last bin is rearranged: the device is synchronised first.  An allocation
// that fails leaves the handle without elision (and the row order as it was).
static int ensure_pendant_plan(gnx_graph *g, hipStream_t s) {
    if (g->pend_built || g->pend_failed) return GNX_OK;
    GNX_NOT_WHILE_CAPTURING(s, "the pendant plan of this handle (GNX_RESERVE_GATHER_HINTS)");
    Csr &a = g->a;
    const int64_t n = a.n_rows;
    const dim3 threads(256), row_blocks(blocks_for(n));
    PendantPart part;
    DevArray<unsigned long long> count;
    hipError_t e = part.pend_flag.alloc(n);
    if (e == hipSuccess) e = part.pend_row_mark.alloc(n);
    if (e == hipSuccess) e = part.pend_slot_mark.alloc(n);
    if (e == hipSuccess) e = part.pend_cols.alloc(a.nnz);
    if (e == hipSuccess) e = part.pend_w.alloc(n);
    if (e == hipSuccess) e = count.alloc(2);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        g->pend_failed = true;
        set_error("pendant elision: %s while allocating %lld bytes for the plan: this handle runs without it", hipGetErrorString(e),
                  (long long)a.nnz * 4 + (long long)n * 7);
        return GNX_OK;
    }
    GNX_HIP(hipMemsetAsync(count, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_pend_candidates, row_blocks, threads, 0, s, a.rowptr, a.colidx, n, part.pend_flag);
    hipLaunchKernelGGL(k_pend_disqualify, dim3(blocks_for(a.nnz)), threads, 0, s, a.rowptr, a.colidx, g->rowidx, a.nnz, part.pend_flag);
    hipLaunchKernelGGL(k_pend_count, row_blocks, threads, 0, s, a.rowptr, part.pend_flag, n, count);
    unsigned long long host[2] = {0, 0};
    GNX_HIP(hipMemcpyAsync(host, count, sizeof(host), hipMemcpyDeviceToHost, s));
    GNX_HIP(hipStreamSynchronize(s));
    part.n_pend = (int64_t)host[0];
    part.pend_slot0 = a.n_nonempty - part.n_pend;
    const int64_t n_one = (int64_t)host[1], one0 = a.n_nonempty - n_one;     // the one-entry bin: the last slots with entries
    if (part.n_pend > 0 && part.n_pend < n_one) {
        DevArray<uint8_t> k0, k1;
        DevArray<int32_t> moved;
        e = k0.alloc(n_one);
        if (e == hipSuccess) e = k1.alloc(n_one);
        if (e == hipSuccess) e = moved.alloc(n_one);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            g->pend_failed = true;
            set_error("pendant elision: %s while allocating the scratch of the plan: this handle runs without it", hipGetErrorString(e));
            return GNX_OK;
        }
        hipLaunchKernelGGL(k_pend_gather_flag, dim3(blocks_for(n_one)), threads, 0, s, a.row_order + one0, part.pend_flag, n_one, k0);
        GNX_TRY((sort_pairs<uint8_t, int32_t>(k0, k1, a.row_order + one0, moved, n_one, 1u, s)));
        GNX_HIP(hipDeviceSynchronize());
        GNX_HIP(hipMemcpyAsync(a.row_order + one0, moved, (size_t)n_one * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        if (a.slot_beg != nullptr)
            hipLaunchKernelGGL(k_slot_ptrs, dim3(blocks_for(n_one)), threads, 0, s, a.rowptr, a.row_order + one0, n_one, a.slot_beg + one0,
                               a.slot_cnt + one0);
    }
    GNX_HIP(hipMemsetAsync(part.pend_row_mark, 0, (size_t)n, s));
    GNX_HIP(hipStreamSynchronize(s));
    GNX_HIP(hipGetLastError());
    part.pend_built = true;
    static_cast<PendantPart &>(*g) = std::move(part);
    return GNX_OK;
}

// whether a K loop of C columns elides under the handle's setting: 1 wherever its launches take hints, -1 where the automatic hints are on
static bool pendant_setting_on(const gnx_graph *g, int64_t C) {
    if (g->pend_setting == 0 || !takes_pendant_elision(g) || hint_hot_rows(g, C) == 0) return false;
    return g->pend_setting > 0 || g->hint_setting == -1;
}

int pendant_plan_for(gnx_graph *g, int64_t C, hipStream_t s, const int32_t **pend_cols) {
    *pend_cols = nullptr;
    if (!pendant_setting_on(g, C) || g->hint_cols == nullptr || g->pend_failed) return GNX_OK;
    if (!g->pend_built) GNX_TRY(ensure_pendant_plan(g, s));
    if (!g->pend_built || g->n_pend == 0) return GNX_OK;
    if (g->pend_hot != g->hint_hot) {       // bit 31 of the hinted columns changed (or first use): one pass over the entries
        if (stream_is_capturing(s)) {
            if (g->pend_hot == -2) GNX_NOT_WHILE_CAPTURING(s, "the pendant plan of this handle (GNX_RESERVE_GATHER_HINTS)");
        } else {
            hipLaunchKernelGGL(k_pend_columns, dim3(blocks_for(g->a.nnz)), dim3(256), 0, s, g->hint_cols, g->rowidx, g->pend_flag, g->a.nnz,
                               g->pend_cols, g->pend_row_mark);
            hipLaunchKernelGGL(k_pend_gather_flag, dim3(blocks_for(g->a.n_rows)), dim3(256), 0, s, g->a.row_order, g->pend_row_mark, g->a.n_rows,
                               g->pend_slot_mark);
            GNX_HIP(hipGetLastError());
            g->pend_hot = g->hint_hot;
        }
    }
    *pend_cols = g->pend_cols;
    return GNX_OK;
}

int pendant_weights(gnx_graph *g, const float *vals, hipStream_t s) {
    hipLaunchKernelGGL(k_pend_weights, dim3(blocks_for(g->n_pend)), dim3(256), 0, s, g->a.row_order + g->pend_slot0, g->n_pend, g->a.rowptr, vals,
                       g->pend_w);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

static int finish_graph(gnx_graph *g, hipStream_t s) {
    GNX_TRY(build_long_plan(g->a, s));
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

}  // namespace gnx

using namespace gnx;

extern "C" {

const char *gnx_last_error(void) { return g_err; }
int gnx_version(void) { return GNX_VERSION_NUM; }

int gnx_graph_destroy(gnx_graph_t g) {
    delete g;
    return GNX_OK;
}

int gnx_graph_reserve(gnx_graph_t g, int64_t C, int flags, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_reserve: NULL handle");
    GNX_CHECK_ARG(C >= 1 && (flags & ~(GNX_RESERVE_TRANSPOSED | GNX_RESERVE_K_LOOP | GNX_RESERVE_TRAIN_GATHER | GNX_RESERVE_GATHER_HINTS)) == 0,
                  "gnx_graph_reserve: bad width / flags");
    if (flags & GNX_RESERVE_TRAIN_GATHER) flags |= GNX_RESERVE_TRANSPOSED;
    hipStream_t s = (hipStream_t)stream;
    GNX_CHECK_ARG(!stream_is_capturing(s), "gnx_graph_reserve: the stream is being captured -- reserve before the capture begins");
    int64_t chunks = g->a.n_chunks;
    if (flags & GNX_RESERVE_TRANSPOSED) {
        GNX_TRY(ensure_transpose(g, s));
        chunks = std::max(chunks, g->t.n_chunks);
        if (!g->t_mask && !g->has_dups && g->t.nnz > 0)      // the keep-bit scratch of a training step's column sums
            GNX_HIP(g->t_mask.alloc(g->t.nnz));
    }
    if ((flags & GNX_RESERVE_K_LOOP) && g->a.order_window == 0 && C <= RELABEL_MAX_C && g->a.n_rows == g->a.n_cols &&
        g->a.n_rows >= (1 << 20) && g->a.nnz >= g->a.n_rows) {
        GNX_TRY(ensure_relabel(g, s));
        GNX_TRY(ensure_relabel_features(g, (size_t)g->a.n_rows * (size_t)C * sizeof(float), s));
        chunks = std::max(chunks, g->r.n_chunks);
    }
    if (flags & GNX_RESERVE_TRAIN_GATHER) GNX_TRY(ensure_train_gather(g, "gnx_graph_reserve(GNX_RESERVE_TRAIN_GATHER)", s));
    if (flags & GNX_RESERVE_GATHER_HINTS) {
        const int32_t *unused;
        GNX_TRY(gather_hints_for(g, g->a, C, s, &unused));
        if (unused != nullptr) GNX_TRY(pendant_plan_for(g, C, s, &unused));     // (the K loop's pendant plan rides on the hints)
    }
    if (chunks > 0) return ensure_partial(g, (size_t)chunks * (size_t)C * sizeof(float), s);
    return GNX_OK;
}

int gnx_graph_gather_order(gnx_graph_t g, const int32_t **d_order, const int32_t **d_rank) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_gather_order: NULL handle");
    if (g->a.order_window != 0) {
        set_error("gnx_graph_gather_order: the handle has a row window (gnx_graph_set_row_window): the gather order is not built");
        return GNX_ERR_UNSUPPORTED;
    }
    GNX_TRY(ensure_gather_order(g, nullptr));
    if (d_order) *d_order = g->go_order;
    if (d_rank) *d_rank = g->go_rank;
    return GNX_OK;
}

int gnx_graph_set_gather_hints(gnx_graph_t g, int64_t hot_rows, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_set_gather_hints: NULL handle");
    GNX_CHECK_ARG(hot_rows >= -1, "gnx_graph_set_gather_hints: hot_rows %lld is neither -1 (automatic), 0 (off) nor a row count", (long long)hot_rows);
    hipStream_t s = (hipStream_t)stream;
    GNX_CHECK_ARG(!stream_is_capturing(s), "gnx_graph_set_gather_hints: the stream is being captured -- set the hints before the capture begins");
    g->hint_setting = hot_rows;
    g->hint_failed = false;
    if (hot_rows == 0) {
        GNX_HIP(hipDeviceSynchronize());        // launches in flight on any stream may still gather through the array freed here
        drop_gather_hints(g);
    } else if (hot_rows > 0 && takes_gather_hints(g)) {
        GNX_TRY(ensure_gather_hints(g, std::min(hot_rows, g->a.n_rows), s));
    }
    return GNX_OK;
}

int gnx_graph_gather_hints(gnx_graph_t g, const int32_t **d_hint_cols, int64_t *hot_rows, int64_t *last_launch_hot_rows) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_gather_hints: NULL handle");
    const bool built = takes_gather_hints(g) && g->hint_cols != nullptr && g->hint_hot >= 0;
    if (d_hint_cols) *d_hint_cols = built ? g->hint_cols.get() : nullptr;
    if (hot_rows) *hot_rows = built ? g->hint_hot : 0;
    if (last_launch_hot_rows) *last_launch_hot_rows = g->last_hint_hot;
    return GNX_OK;
}

int gnx_graph_set_pendant_elision(gnx_graph_t g, int mode, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_set_pendant_elision: NULL handle");
    GNX_CHECK_ARG(mode >= -1 && mode <= 1, "gnx_graph_set_pendant_elision: mode %d is neither -1 (automatic), 0 (off) nor 1 (on)", mode);
    hipStream_t s = (hipStream_t)stream;
    GNX_CHECK_ARG(!stream_is_capturing(s), "gnx_graph_set_pendant_elision: the stream is being captured -- set the mode before the capture begins");
    g->pend_setting = mode;
    g->pend_failed = false;
    if (mode == 1 && takes_pendant_elision(g)) GNX_TRY(ensure_pendant_plan(g, s));
    return GNX_OK;
}

int gnx_graph_pendant_elision(gnx_graph_t g, int64_t *n_elidable, const uint8_t **d_elidable, int *last_loop_elided) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_pendant_elision: NULL handle");
    if (n_elidable) *n_elidable = g->pend_built ? g->n_pend : 0;
    if (d_elidable) *d_elidable = g->pend_built ? g->pend_flag.get() : nullptr;
    if (last_loop_elided) *last_loop_elided = g->last_pend ? 1 : 0;
    return GNX_OK;
}

int gnx_graph_set_row_window(gnx_graph_t g, int64_t window_rows, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_set_row_window: NULL handle");
    GNX_CHECK_ARG(window_rows >= 0, "gnx_graph_set_row_window: negative window");
    hipStream_t s = (hipStream_t)stream;
    GNX_CHECK_ARG(!stream_is_capturing(s), "gnx_graph_set_row_window: the stream is being captured -- set the window before the capture begins");
    if (g->a.order_window == window_rows) return GNX_OK;
    // launches in flight on this handle -- on ANY stream -- still read the old order's arrays, which are freed below
    GNX_HIP(hipDeviceSynchronize());
    const int64_t before = g->a.order_window;
    g->a.drop_plan();
    g->a.order_window = window_rows;
    int rc = build_long_plan(g->a, s);
    if (rc != GNX_OK) {                                              // (a window count that does not fit the key: back to what it was)
        g->a.drop_plan();
        g->a.order_window = before;
        const int rc2 = build_long_plan(g->a, s);
        return rc2 != GNX_OK ? rc2 : rc;
    }
    if (g->has_t) {
        g->t.drop_plan();
        g->t.order_window = g->a.n_rows == g->a.n_cols ? window_rows : 0;
        rc = build_long_plan(g->t, s);
        if (rc != GNX_OK) {       // a half-built transposed plan must never be launched: the structure goes, the next user rebuilds it
            drop_transpose(g);
            return rc;
        }
    }
    if (g->has_r) drop_relabel(g);                                   // the degree-relabelled copy belongs to the default order,
    drop_gather_order(g);                                            // and so do the gather order and its per-entry columns
    drop_gather_hints(g);                                            // (a handle with a window takes no hints; back at 0 they are rebuilt)
    drop_pendants(g);                                                // (nor pendant elision: its slots belong to the order dropped above)
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_graph_create_coo(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *d_indices, const float *d_values,
                         void *stream, gnx_graph_t *out) {
    GNX_CHECK_ARG(out != nullptr, "gnx_graph_create_coo: out is NULL");
    *out = nullptr;
    GNX_CHECK_ARG(n_rows >= 0 && n_cols >= 0 && nnz >= 0, "gnx_graph_create_coo: negative size");
    GNX_CHECK_ARG(n_rows < INT32_MAX && n_cols < INT32_MAX, "gnx_graph_create_coo: more than 2^31-1 rows/cols per handle");
    GNX_CHECK_ARG(nnz < INT32_MAX, "gnx_graph_create_coo: more than 2^31-1 entries per handle");
    GNX_CHECK_ARG(nnz == 0 || (d_indices && d_values), "gnx_graph_create_coo: NULL indices/values");
    hipStream_t s = (hipStream_t)stream;
    std::unique_ptr<gnx_graph> g(new gnx_graph());
    Csr &a = g->a;
    a.n_rows = n_rows; a.n_cols = n_cols;
    g->nnz_entries = nnz;
    GNX_HIP(a.rowptr.alloc(n_rows + 1));
    if (nnz == 0) {
        a.nnz = 0;
        GNX_HIP(hipMemsetAsync(a.rowptr, 0, (n_rows + 1) * sizeof(int64_t), s));
        GNX_HIP(a.colidx.alloc(0));
        GNX_HIP(g->raw_vals.alloc(0));
        GNX_HIP(g->rowidx.alloc(0));
        GNX_HIP(hipStreamSynchronize(s));
        GNX_TRY(finish_graph(g.get(), s));
        *out = g.release();
        return GNX_OK;
    }
    const dim3 entry_blocks(blocks_for(nnz)), threads(256);
    DevArray<uint64_t> k0, k1;
    DevArray<float> v1;
    DevArray<int> bad;
    GNX_HIP(k0.alloc(nnz)); GNX_HIP(k1.alloc(nnz));
    GNX_HIP(v1.alloc(nnz));
    GNX_HIP(bad.alloc(1));
    GNX_HIP(hipMemsetAsync(bad, 0, 4, s));
    hipLaunchKernelGGL(k_make_keys, entry_blocks, threads, 0, s, d_indices, nnz, n_rows, n_cols, k0, bad);
    GNX_TRY(sort_pairs<uint64_t, const float>(k0, k1, d_values, v1, nnz, bits_for((uint64_t)n_rows * (uint64_t)n_cols), s));
    // k0 is free again: reuse as head flags + scan (2 x int32 per entry fits in 8 bytes/entry)
    int32_t *d_head = reinterpret_cast<int32_t *>(k0.get());
    int32_t *d_scan = d_head + nnz;
    hipLaunchKernelGGL(k_heads, entry_blocks, threads, 0, s, k1, nnz, d_head);
    GNX_TRY(inclusive_scan(d_head, d_scan, nnz, s));
    int h_bad = 0; int32_t h_nslots = 0;
    GNX_TRY(fetch(h_bad, bad.get(), s));
    GNX_TRY(fetch(h_nslots, d_scan + (nnz - 1), s));
    GNX_CHECK_ARG(h_bad == 0, "gnx_graph_create_coo: an index lies outside the %lld x %lld shape", (long long)n_rows,
                  (long long)n_cols);
    a.nnz = h_nslots;
    g->has_dups = (a.nnz != nnz);
    GNX_HIP(a.colidx.alloc(a.nnz));
    GNX_HIP(g->rowidx.alloc(a.nnz));
    if (g->has_dups) GNX_HIP(g->slot_ptr.alloc(a.nnz + 1));
    hipLaunchKernelGGL(k_fill_slots, entry_blocks, threads, 0, s, k1, d_scan, nnz, n_cols, a.colidx, g->rowidx, g->slot_ptr);
    if (g->has_dups) {
        GNX_HIP(hipMemcpyAsync(g->slot_ptr + a.nnz, &nnz, 8, hipMemcpyHostToDevice, s));
        g->e_vals = std::move(v1);
        GNX_HIP(g->raw_vals.alloc(a.nnz));
        hipLaunchKernelGGL(k_sum_slots, dim3(blocks_for(a.nnz)), threads, 0, s, g->e_vals, g->slot_ptr, a.nnz, g->raw_vals);
    } else {
        g->raw_vals = std::move(v1);
    }
    hipLaunchKernelGGL(k_lower_bound_rows, dim3(blocks_for(n_rows + 1)), threads, 0, s, g->rowidx, a.nnz, n_rows, a.rowptr);
    GNX_HIP(hipStreamSynchronize(s));
    GNX_TRY(finish_graph(g.get(), s));
    *out = g.release();
    return GNX_OK;
}

int gnx_graph_create_csr(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *d_rowptr, const int32_t *d_colidx,
                         const float *d_values, void *stream, gnx_graph_t *out) {
    GNX_CHECK_ARG(out != nullptr, "gnx_graph_create_csr: out is NULL");
    *out = nullptr;
    GNX_CHECK_ARG(n_rows >= 0 && n_cols >= 0 && nnz >= 0, "gnx_graph_create_csr: negative size");
    GNX_CHECK_ARG(n_rows < INT32_MAX && n_cols < INT32_MAX && nnz < INT32_MAX, "gnx_graph_create_csr: size over 2^31-1");
    GNX_CHECK_ARG(d_rowptr && (nnz == 0 || (d_colidx && d_values)), "gnx_graph_create_csr: NULL array");
    hipStream_t s = (hipStream_t)stream;
    std::unique_ptr<gnx_graph> g(new gnx_graph());
    Csr &a = g->a;
    a.n_rows = n_rows; a.n_cols = n_cols; a.nnz = nnz; g->nnz_entries = nnz;
    GNX_HIP(a.rowptr.alloc(n_rows + 1));
    GNX_HIP(a.colidx.alloc(nnz));
    GNX_HIP(g->raw_vals.alloc(nnz));
    GNX_HIP(g->rowidx.alloc(nnz));
    GNX_HIP(hipMemcpyAsync(a.rowptr, d_rowptr, (n_rows + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (nnz) {
        GNX_HIP(hipMemcpyAsync(a.colidx, d_colidx, nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        GNX_HIP(hipMemcpyAsync(g->raw_vals, d_values, nnz * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    DevArray<int> bad;
    GNX_HIP(bad.alloc(1));
    GNX_HIP(hipMemsetAsync(bad, 0, 4, s));
    if (n_rows) {
        hipLaunchKernelGGL(k_check_csr, dim3(blocks_for(n_rows)), dim3(256), 0, s, a.rowptr, a.colidx, n_rows, n_cols, nnz, bad);
        hipLaunchKernelGGL(k_rows_from_ptr, dim3(blocks_for(n_rows)), dim3(256), 0, s, a.rowptr, n_rows, g->rowidx);
    }
    int h_bad = 0;
    GNX_TRY(fetch(h_bad, bad.get(), s));
    GNX_CHECK_ARG(h_bad == 0, "gnx_graph_create_csr: rowptr/colidx are not a valid sorted CSR for this shape");
    GNX_TRY(finish_graph(g.get(), s));
    *out = g.release();
    return GNX_OK;
}

int gnx_graph_info(gnx_graph_t g, int64_t *n_rows, int64_t *n_cols, int64_t *nnz_entries, int64_t *nnz_coalesced) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_info: NULL handle");
    if (n_rows) *n_rows = g->a.n_rows;
    if (n_cols) *n_cols = g->a.n_cols;
    if (nnz_entries) *nnz_entries = g->nnz_entries;
    if (nnz_coalesced) *nnz_coalesced = g->a.nnz;
    return GNX_OK;
}

int gnx_graph_hub_rows(gnx_graph_t g, int64_t *n_hub_rows, int64_t *threshold) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_hub_rows: NULL handle");
    if (n_hub_rows) *n_hub_rows = g->a.n_long;
    if (threshold) *threshold = g->a.long_row;
    return GNX_OK;
}

int gnx_graph_csr(gnx_graph_t g, const int64_t **d_rowptr, const int32_t **d_colidx, const float **d_raw_values) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_csr: NULL handle");
    if (d_rowptr) *d_rowptr = g->a.rowptr;
    if (d_colidx) *d_colidx = g->a.colidx;
    if (d_raw_values) *d_raw_values = g->raw_vals;
    return GNX_OK;
}

int gnx_graph_export(gnx_graph_t g, int64_t *d_rowptr_out, int32_t *d_colidx_out, float *d_raw_values_out,
                     int32_t *d_rowidx_out, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_graph_export: NULL handle");
    hipStream_t s = (hipStream_t)stream;
    const Csr &a = g->a;
    if (d_rowptr_out) GNX_HIP(hipMemcpyAsync(d_rowptr_out, a.rowptr, (a.n_rows + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (a.nnz > 0) {
        if (d_colidx_out) GNX_HIP(hipMemcpyAsync(d_colidx_out, a.colidx, a.nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        if (d_raw_values_out) GNX_HIP(hipMemcpyAsync(d_raw_values_out, g->raw_vals, a.nnz * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (d_rowidx_out) GNX_HIP(hipMemcpyAsync(d_rowidx_out, g->rowidx, a.nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    }
    return GNX_OK;
}

const char *gnx_graph_last_kernel(gnx_graph_t g) { return g ? g->last_kernel : ""; }

}  // extern "C"
