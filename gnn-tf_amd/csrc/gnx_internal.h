// Internal declarations shared by the libgnx.so translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>

#include "../../include/gnx.h"

#define GNX_VERSION_NUM GNX_ABI_VERSION /* the header's number (include/gnx.h) */

namespace gnx {

void set_error(const char *fmt, ...);

#define GNX_HIP(expr)                                                                   \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            gnx::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return GNX_ERR_HIP;                                                         \
        }                                                                               \
    } while (0)

#define GNX_CHECK_ARG(cond, ...)                                                        \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            gnx::set_error(__VA_ARGS__);                                                \
            return GNX_ERR_INVALID;                                                     \
        }                                                                               \
    } while (0)

// Rows whose entry count exceeds LONG_ROW are cut into chunks of LONG_CHUNK entries that
// separate waves sum into a partial slab; a second kernel adds a row's partials in chunk
// order (fixed order => bitwise reproducible) and applies the epilogue.
#ifndef GNX_LONG_ROW
#define GNX_LONG_ROW 512
#endif
#ifndef GNX_LONG_CHUNK
#define GNX_LONG_CHUNK GNX_LONG_ROW
#endif
constexpr int LONG_ROW = GNX_LONG_ROW;
constexpr int LONG_CHUNK = GNX_LONG_CHUNK;
// Small structures (a citation graph: 10^5 rows) are bound by the LATENCY of their longest walk, not by bandwidth: one
// 512-entry row is 128 dependent gather rounds of a 16-lane group (0.13 ms -- the whole launch).  Between 2^15 and
// 2^20 rows the plan therefore cuts rows at 128 entries into 128-entry chunks, and the sub-wave kernels take chunks and short rows in one launch.
constexpr int SMALL_ROWS = 1 << 20;
constexpr int TINY_ROWS = 1 << 15;      // below this everything is cache-resident and launch-bound: an extra reduce launch costs more than it saves
// widest feature rows (floats) the K loop runs on the degree-relabelled copy of a large square graph.  Measured round 4 (RMAT
// 10M / 100M, K = 10) with the threshold at 32: C = 32 gains 7 % from the order and pays it back for the value permutation, the
// H0 permutation and the scattered last iteration (22.77 vs 22.78 ms); C = 64 loses.  16 stays.
constexpr int RELABEL_MAX_C = 16;
// Gather hints (gnx_graph_set_gather_hints).  The automatic rule marks as hot the rows that fill HINT_HOT_BYTES, the 256 MiB of the
// Infinity Cache, at the width of the call, on structures of at least HINT_MIN_ROWS rows; rows narrower than HINT_MIN_ROW_BYTES
// never take hints (they run on the narrow kernels).  Measured (profiles/NOTES.md, gather hints; R-MAT, K = 10, hints against none in
// one process): an L2-sized hot set LOSES 9-34 % -- most "cold" rows are gathered a few times per launch and a non-temporal load
// gives that reuse up -- an Infinity-Cache-sized one gains with the size of the graph: C = 128 +6.5 % at 10M rows, +2.3 % at 20M,
// -1.1 % at 40M, -5.2 % at 80M; C = 64 -0.6 / +3.4 / -5.7 / -5.0 %.  Hence on from 2^25 rows, and opt-in below.
constexpr int64_t HINT_HOT_BYTES = (int64_t)256 << 20;
constexpr int64_t HINT_MIN_ROWS = 1 << 25;
constexpr int64_t HINT_MIN_ROW_BYTES = 256;
#ifndef GNX_GATHER_HINTS_DEFAULT
#define GNX_GATHER_HINTS_DEFAULT (-1)
#endif
// Pendant elision (gnx_graph_set_pendant_elision): -1 = automatic, on exactly where the automatic gather hints are on; 0 = only on request
#ifndef GNX_PENDANT_ELISION_DEFAULT
#define GNX_PENDANT_ELISION_DEFAULT (-1)
#endif
constexpr int32_t PEND_COL_BIT = 1 << 30;             // pend_cols: the column is an elidable row
constexpr int32_t PEND_COL_MASK = PEND_COL_BIT - 1;   // ... and its number (bit 31 stays the gather hint)
constexpr int SMALL_LONG_ROW = GNX_LONG_ROW < 128 ? GNX_LONG_ROW : 128;

// An owned device array.  Everything a handle keeps on the device, and every temporary of its builds, is one of these, so dropping a
// part of a handle is assigning a fresh value to it, and destroying a handle is `delete`.  Reads as the T * it holds: launches and
// pointer arithmetic take it as they took the raw pointer.  alloc() frees what was held first and never allocates fewer than 16
// bytes, so the array of a built part is never null, however empty the graph.
template <class T>
struct DevArray {
    DevArray() = default;
    DevArray(DevArray &&o) noexcept : p(o.release()) {}
    DevArray &operator=(DevArray &&o) noexcept {
        if (this != &o) { reset(); p = o.release(); }
        return *this;
    }
    ~DevArray() { reset(); }
    hipError_t alloc(size_t count) {
        reset();
        const size_t bytes = count * sizeof(T);
        const hipError_t e = hipMalloc((void **)&p, bytes < 16 ? 16 : bytes);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    T *release() { T *q = p; p = nullptr; return q; }
    T *get() const { return p; }
    operator T *() const { return p; }
private:
    T *p = nullptr;
};

// Everything build_long_plan makes of a structure: what Csr::drop_plan drops for a rebuild under another row order.
struct Plan {
    // long-row split plan
    int64_t n_long = 0, n_chunks = 0;
    int long_row = LONG_ROW, long_chunk = LONG_CHUNK;   // this structure's threshold / chunk length (set by build_long_plan)
    DevArray<int32_t> long_rows;        // [n_long] row ids
    DevArray<int64_t> long_chunk_ptr;   // [n_long+1] first chunk of each long row
    DevArray<int32_t> chunk_long;       // [n_chunks] index into long_rows
    DevArray<int32_t> chunk_order;      // [n_chunks] chunk ids sorted by the first column they touch (see gnx_graph.hip)
    // rows in stable order of descending (clamped) entry count: the rows that share a wave in the
    // sub-wave kernels then have similar lengths (power-law graphs otherwise leave most lanes idle)
    DevArray<int32_t> row_order;        // [n_rows]
    DevArray<int64_t> slot_beg;         // [n_rows] first entry of row row_order[slot] ...
    DevArray<int32_t> slot_cnt;         // [n_rows] ... and its entry count: what the sub-wave kernels read instead of rowptr[row_order[slot]]
                                        // (coalesced, and no load that depends on another load before the row's entries are known)
    int64_t n_nonempty = 0;             // rows with at least one entry: the first n_nonempty slots of row_order (the rest are the empty rows)
    DevArray<int32_t> nonempty_rows;    // [n_nonempty] the same rows in ASCENDING order (only when some row is empty): what the one-wave-per-row
                                        // kernels walk while rows without entries are skipped
    // square structures: no row WITHOUT entries is referenced as a column by any entry (always so for a symmetric pattern).  Such rows
    // are alpha * H0 after every iteration and nobody gathers them: loops write them into their result only, never into work buffers
    bool empty_rows_unreferenced = false;
};

// One CSR-like structure (the matrix itself, or its transpose) and its plan.
struct Csr : Plan {
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    DevArray<int64_t> rowptr;   // [n_rows+1]
    DevArray<int32_t> colidx;   // [nnz]
    // gnx_graph_set_row_window: > 0 = the caller's numbering carries locality; rows are then taken in windows of this many consecutive
    // ids (degree-binned INSIDE a window, rows without entries still trailing everything) so that the rows in flight together are
    // neighbours in the caller's order and gather from one neighbourhood
    int64_t order_window = 0;
    void drop_plan() { static_cast<Plan &>(*this) = Plan(); }
};

// The lazily built parts of a handle that are dropped as a whole (a failed build, another row order): gnx_graph inherits each, so the
// fields read as the handle's own, and dropping a part is assigning a fresh one (drop_transpose and its like, gnx_graph.hip).

// transposed structure (lazy)
struct TransposedPart {
    bool has_t = false;
    Csr t;                       // t.n_rows = a.n_cols
    DevArray<int32_t> t_perm;    // [a.nnz] coalesced slot of every transposed entry
    DevArray<float> t_vals;      // [a.nnz] scratch: values gathered into transposed order
    DevArray<float> t_raw;       // [a.nnz] raw values in transposed order (streaming column sums)
    DevArray<int32_t> t_rowidx;  // [a.nnz] row of the transposed structure (= column of A) per transposed position
    DevArray<uint16_t> t_mask;   // [a.nnz] scratch: keep bits of up to 16 dropout streams per transposed position (gnx_graph_colsum_streams)
};

// degree-relabelled copy of a square matrix (lazy; narrow feature widths): vertex go_order[i] becomes vertex i, so the
// rows of the hubs -- which most gathers hit -- are neighbours in memory and share cache lines.  go_order (below) = the degree bins
// of a.row_order (heaviest first) and, inside a bin, the vertices by the degree rank of their most popular neighbour: the
// leaves of one hub become neighbours too, so the hub's row gathers them from consecutive lines
struct RelabelledPart {
    bool has_r = false;
    Csr r;
    DevArray<int32_t> r_perm;    // [a.nnz] coalesced slot of every relabelled entry
    DevArray<float> r_vals;      // [a.nnz] scratch: values gathered into relabelled order
};

// the gather order of a square handle (lazy): the order the relabelled copy numbers its vertices in (above), kept on its own so
// that it can exist without that copy.  go_order: position -> vertex (what the relabelled copy calls new id -> old id), go_rank its
// inverse.  a_gcol / t_gcol (gnx_spmm_dropped_chained_ord / _back_ord): go_rank of every column of the matrix / of the transposed
// structure, i.e. the row of a matrix STORED in gather order that an entry gathers
struct GatherOrderPart {
    DevArray<int32_t> go_order;  // [n]
    DevArray<int32_t> go_rank;   // [n]
    DevArray<int32_t> a_gcol;    // [a.nnz]
    DevArray<int32_t> t_gcol;    // [a.nnz]
};

// gather hints of a square stand-alone handle without a row window (lazy; gnx_graph_set_gather_hints): per entry of the matrix its
// column with bit 31 set when that column is COLD, i.e. not among the hint_hot rows with the most stored entries (ties to the
// smaller id).  The wide f32 eval kernels gather a cold row non-temporally, so that the hot rows stay in the L2s.  Only bit 31 is a
// hint: an array built for another hot_rows still names the right columns, so a launch that must not rebuild (a captured stream)
// uses the array as it is.
struct GatherHintsPart {
    DevArray<int32_t> hint_cols;     // [a.nnz], or null: not built
    DevArray<int32_t> hint_rank;     // [n] position of every row in the order of descending entry count, ties to the smaller id (kept: another hot_rows is one pass)
    int64_t hint_hot = 0;            // the hot_rows hint_cols was built for
    bool hint_failed = false;        // the arrays could not be allocated: the handle runs unhinted and does not try again
};

// pendant elision of the K loop (lazy; gnx_graph_set_pendant_elision; handles that take gather hints, fewer than 2^30 columns).
// An ELIDABLE row i stores exactly one entry (i, h), h != i, h stores at least two entries, and no row but h stores an entry in
// column i: the iterates of i between H0 and the result are read by h alone, which can form them itself from H0[i], pend_w[i] and
// its own row of two iterations ago (gnx_spmm_eval.h, PEND).  Building the part moves the elidable rows to the END of the
// one-entry bin of a.row_order (order inside a bin is free: equal lengths), so that the launches of the iterations between leave
// them out by their slot numbers.
struct PendantPart {
    bool pend_built = false, pend_failed = false;
    int64_t n_pend = 0;                     // elidable rows = slots [pend_slot0, a.n_nonempty) of a.row_order
    int64_t pend_slot0 = 0;
    DevArray<uint8_t> pend_flag;            // [n] 1 = the row is elidable
    DevArray<uint8_t> pend_row_mark;        // [n] 1 = the row stores an entry whose column is elidable (read by the chunk kernels)
    DevArray<uint8_t> pend_slot_mark;       // [n] the same per slot of a.row_order (read by the row kernels, coalesced)
    DevArray<int32_t> pend_cols;            // [a.nnz] hint_cols with PEND_COL_BIT set where the column is elidable
    int64_t pend_hot = -2;                  // the hint_hot whose bit 31 pend_cols carries
    DevArray<float> pend_w;                 // [n] per call: the value of the one entry of every elidable row
};

}  // namespace gnx

struct gnx_graph : gnx::TransposedPart, gnx::RelabelledPart, gnx::GatherOrderPart, gnx::GatherHintsPart, gnx::PendantPart {
    gnx::Csr a;            // coalesced matrix
    gnx::DevArray<float> raw_vals;     // [a.nnz] summed duplicate values
    gnx::DevArray<int32_t> rowidx;     // [a.nnz] row of every coalesced entry
    // un-coalesced entries (only when duplicates exist; otherwise entries == coalesced)
    int64_t nnz_entries = 0;
    bool has_dups = false;
    gnx::DevArray<float> e_vals;       // [nnz_entries] entry values, sorted by (row, col), input order among dups
    gnx::DevArray<int64_t> slot_ptr;   // [a.nnz+1] entry range of every coalesced slot
    // entry dropout of a handle with duplicates (gnx_graph_enable_entry_dropout): per slot the multiplicity (ENTRY_GENERAL: walk the
    // entry list) and the value its entries share, in CSR order and in transposed order (t_perm depends on the structure alone, so
    // the transposed tables stay valid if the transposed structure is ever rebuilt)
    bool entry_drop = false;
    gnx::DevArray<uint8_t> ed_mult, t_ed_mult;
    gnx::DevArray<float> ed_vals, t_ed_vals;
    // partial slab for long rows (grown on demand)
    gnx::DevArray<float> partial;
    size_t partial_bytes = 0;
    gnx::DevArray<float> deg;          // [a.n_cols] scratch for column sums / degree scales (lazy)
    const uint64_t *stream_offset = nullptr;   // NOT owned: optional device counter added to every dropout stream id of this handle
    // vertex block of a larger graph (gnx_graph_set_block): dropout draws are keyed by GLOBAL (row, col), and the degree
    // scale of local row r sits at position blk_row0_buf + r of the per-column scale vector
    int64_t blk_row0_global = 0, blk_row0_buf = 0;
    gnx::DevArray<int32_t> blk_col_gid;        // [a.n_cols] global vertex id of every column (owned), or null
    gnx::DevArray<float> r_feat;       // scratch of the relabelled copy: H0 in relabelled row order (grown on demand, outlives the copy)
    size_t r_feat_bytes = 0;
    const char *last_kernel = "";      // NOT owned: a string literal of the launcher
    int64_t last_hint_hot = 0;         // hot rows the last SpMM launch over this handle gathered with; 0 = it took no hints
    int64_t hint_setting = GNX_GATHER_HINTS_DEFAULT;   // gnx_graph_set_gather_hints: -1 automatic, 0 off, n > 0 that many hot rows
    int pend_setting = GNX_PENDANT_ELISION_DEFAULT;    // gnx_graph_set_pendant_elision: -1 automatic, 0 off, 1 on wherever admissible
    bool last_pend = false;                            // the last K loop over this handle elided its pendant rows
};

namespace gnx {

int build_long_plan(Csr &m, hipStream_t s);
int ensure_transpose(gnx_graph *g, hipStream_t s);
int ensure_partial(gnx_graph *g, size_t bytes, hipStream_t s);
bool stream_is_capturing(hipStream_t s);
int ensure_relabel(gnx_graph *g, hipStream_t s);
int ensure_gather_order(gnx_graph *g, hipStream_t s);
// the transposed structure, the gather order and a_gcol / t_gcol; GNX_ERR_UNSUPPORTED (naming `fn`) on a vertex block, a handle with
// duplicate entries or a handle with a row window
int ensure_train_gather(gnx_graph *g, const char *fn, hipStream_t s);
int ensure_relabel_features(gnx_graph *g, size_t bytes, hipStream_t s);
// The hinted columns a wide f32 eval launch of C columns over structure m gathers through, or null: hints are off, the handle or
// the width does not take them, or their arrays could not be allocated (then gnx_last_error says so; never a failure).  Builds or
// re-marks the array on first use and when the hot_rows in force changes; GNX_ERR_UNSUPPORTED, naming gnx_graph_reserve, where
// that would allocate under capture.
int gather_hints_for(gnx_graph *g, const Csr &m, int64_t C, hipStream_t s, const int32_t **hint_cols);
// The pendant plan of a K loop of C columns over the handle's own matrix whose launches gather through `hint_cols` (not null), or
// *pend_cols = null: elision is off, the handle does not take it, it has no elidable row, or the arrays could not be allocated.
// Builds the part on first use and re-marks pend_cols when the hints' hot rows changed; GNX_ERR_UNSUPPORTED where that would
// allocate under capture.
int pendant_plan_for(gnx_graph *g, int64_t C, hipStream_t s, const int32_t **pend_cols);
int pendant_weights(gnx_graph *g, const float *vals, hipStream_t s);   // per call: g->pend_w from the call's values

// blocks of `per_block` items that cover n items
inline unsigned blocks_for(int64_t n, int per_block = 256) { return (unsigned)((n + per_block - 1) / per_block); }

// a dropout rate as the kernels take it: keep iff hash >= int(p * 2^24) (oracle/gnntf_oracle.py:dropout_threshold), kept values times
// the f32 scale 1 / (1 - p)
inline uint32_t drop_threshold(double p) { return (uint32_t)(p * 16777216.0); }
inline float drop_scale(float p) { return 1.0f / (1.0f - p); }

// ---- counter RNG of the edge dropout: the same integer arithmetic as oracle/gnntf_oracle.py:hash_u24 ----------
__device__ __forceinline__ uint64_t rng_fin(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// hash_u24 in two parts: the first two rounds depend on (seed, stream, row, col) only, the last one on the duplicate rank as well
__device__ __forceinline__ uint64_t hash_key(uint64_t seed, uint64_t stream, uint64_t row, uint64_t col) {
    const uint64_t k = seed ^ (stream * 0xD1342543DE82EF95ull);
    uint64_t x = rng_fin(k + row * 0x9E3779B97F4A7C15ull);
    return x ^ (col * 0xC2B2AE3D27D4EB4Full);
}
__device__ __forceinline__ uint32_t hash_rank(uint64_t key, uint64_t dup) {
    return (uint32_t)(rng_fin(key + dup * 0x165667B19E3779F9ull) >> 40);
}
__device__ __forceinline__ uint32_t hash_u24(uint64_t seed, uint64_t stream, uint64_t row, uint64_t col, uint64_t dup) {
    return hash_rank(hash_key(seed, stream, row, col), dup);
}

// Entry dropout on a handle with duplicate COO entries (gnx_graph_enable_entry_dropout): per coalesced slot a multiplicity byte;
// ENTRY_GENERAL marks a slot whose entries are not all the same float (or more than 254 of them), whose value is then the walk
// of its entry list.  Kept sum of a slot = its kept entries * 1/(1-p), added in input order exactly as slot_value (gnx_prep.hip)
// writes it.  For a uniform slot every term is the same float, so the m-fold loop over one value is bit for bit the walk of the list
// -- as long as both round alike.  kept_term spells the rounding out: the product is rounded on its own and then added, which is what
// the reference does (tf.nn.dropout scales the values, layered.py:50; the entries of a slot are summed afterwards).  Written as
// `sum += value * scale` the compiler contracts the walk of a list into fmaf(value, scale, sum) but hoists the product of a uniform
// slot out of its loop: with three or more kept entries and a scale that is no power of two (p = 0.1, 0.9) the two sums differed in
// the last bit, and a slot holding +v and -v, both kept, summed to the rounding residue of v * scale instead of 0 -- a negative
// column sum, hence a NaN degree scale, when nothing else of the column is kept.
// (the pragma and not __fmul_rn / __fadd_rn: HIP defines those as the plain operators, which are contracted all the same)
__device__ __forceinline__ float kept_term(float acc, float value, float scale) {
#pragma clang fp contract(off)
    const float term = value * scale;
    return acc + term;
}

constexpr uint32_t ENTRY_GENERAL = 255;

__device__ __forceinline__ float slot_kept_sum(uint64_t key, uint32_t thr, float scale, uint32_t m, float uval,
                                               const float *__restrict__ e_vals, const int64_t *__restrict__ slot_ptr, int64_t slot) {
    float acc = 0.f;
    if (m != ENTRY_GENERAL) {
        for (uint32_t i = 0; i < m; ++i)
            if (hash_rank(key, i) >= thr) acc = kept_term(acc, uval, scale);
    } else {
        const int64_t b = slot_ptr[slot], e = slot_ptr[slot + 1];
        for (int64_t i = b; i < e; ++i)
            if (hash_rank(key, (uint64_t)(i - b)) >= thr) acc = kept_term(acc, e_vals[i], scale);
    }
    return acc;
}

// gnx_spmm_dropped: the values of one training iteration's dropped + re-normalised adjacency are produced inside the
// SpMM, per entry, with exactly the arithmetic of k_scale_values (gnx_prep.hip): (D[row] * drop(raw)) * D[col].
struct DropFuse {
    const float *D;        // degree scales of this (seed, stream); null = not fused
    uint64_t seed, stream;
    const uint64_t *offset; // optional device counter added to the stream id (gnx_graph_set_dropout_counter)
    uint32_t thr;          // keep iff hash >= thr
    float scale;           // 1 / (1 - p)
    int transposed;        // the structure walked is the transpose: its entry (r, c) is A[c][r]
    int col_prescaled;     // the gathered rows already carry their column's scale (written by the previous iteration's epilogue)
    int64_t row0_key, row0_D;   // vertex block: global id of row 0 / position of row 0's scale in D (0, 0 otherwise)
    const int32_t *gid;         // vertex block: global id of every column (null: the column index itself)
    // entry dropout (the _entries kernels only): multiplicity of every slot of the structure walked, the handle's entry lists and,
    // for the transposed structure, the coalesced slot of every position (t_perm); SpmmArgs::vals holds each uniform slot's value
    const uint8_t *mult;
    const float *e_vals;
    const int64_t *slot_ptr;
    const int32_t *perm;
};

__device__ __forceinline__ float dropped_weight(const DropFuse &f, float raw, int64_t r, int64_t c) {
    const int64_t ar = f.transposed ? c : r, ac = f.transposed ? r : c;      // the entry's (row, col) in A
    const uint64_t stream = f.stream + (f.offset ? *f.offset : 0);
    const uint64_t kc = f.gid ? (uint64_t)f.gid[ac] : (uint64_t)ac;
    if (hash_u24(f.seed, stream, (uint64_t)(ar + f.row0_key), kc, 0) < f.thr) return 0.f;   // dropped: (D * 0) * D = 0 for finite scales
    if (f.col_prescaled && f.transposed)          // the gathered row (vertex ar) carries D[ar] already: what is left is the OUTPUT row's scale
        return (raw * f.scale) * f.D[ac];
    const float w = f.D[ar + f.row0_D] * (raw * f.scale);
    return f.col_prescaled ? w : w * f.D[ac];
}

// dropped_weight on a handle with duplicate entries: `uval` = the uniform value of the slot at position `pos` of the structure walked.
// Weight (D[row] * kept sum) * D[col], as k_scale_values makes it; a slot whose kept sum is 0 weighs 0 and is skipped like a dropped one.
__device__ __forceinline__ float dropped_weight_entries(const DropFuse &f, float uval, int64_t pos, int64_t r, int64_t c) {
    const int64_t ar = f.transposed ? c : r, ac = f.transposed ? r : c;
    const uint64_t stream = f.stream + (f.offset ? *f.offset : 0);
    const uint64_t kc = f.gid ? (uint64_t)f.gid[ac] : (uint64_t)ac;
    const uint32_t m = f.mult[pos];
    const int64_t slot = (m == ENTRY_GENERAL && f.perm) ? (int64_t)f.perm[pos] : pos;
    const float v = slot_kept_sum(hash_key(f.seed, stream, (uint64_t)(ar + f.row0_key), kc), f.thr, f.scale, m, uval, f.e_vals,
                                  f.slot_ptr, slot);
    if (v == 0.f) return 0.f;
    if (f.col_prescaled && f.transposed) return v * f.D[ac];
    const float w = f.D[ar + f.row0_D] * v;
    return f.col_prescaled ? w : w * f.D[ac];
}

template <bool ENTRIES>
__device__ __forceinline__ float dropped_weight_at(const DropFuse &f, float raw, int64_t pos, int64_t r, int64_t c) {
    if constexpr (ENTRIES) return dropped_weight_entries(f, raw, pos, r, c);
    else return dropped_weight(f, raw, r, c);
}

struct SpmmArgs {
    const int64_t *rowptr;
    const int32_t *colidx;
    const float *vals;
    const float *diag;
    const float *X;
    int64_t ldx;
    const float *H0;
    int64_t ldh0;
    float beta, alpha;
    int act;
    float *out;
    int64_t ldo;
    const int32_t *out_rows;   // optional destination row of every result row (gnx_spmm_scatter / gnx_spmm_rows)
    bool map_h0;               // H0 rows are indexed through out_rows as well (gnx_spmm_rows)
    const float *out_scale;    // optional per-row factor applied to the finished row (gnx_spmm_dropped_chained: the NEXT iteration's column scale)
    // optional SECOND result of the same sums (gnx_spmm_dropped_back): out2[row] = acc * beta2 * (out2_scale ? out2_scale[row] : 1) --
    // no mix term, no activation; `out` then carries the running gradient sum and out2 the pre-scaled operand of the next step
    float *out2;
    int64_t ldo2;
    float beta2;
    const float *out2_scale;
    int64_t n_rows;
    int64_t n_nonempty;        // rows with entries = leading slots of row_order (Csr::n_nonempty)
    int64_t slot0;             // first row slot of this launch (a launch holds at most 2^32 work-items: huge graphs are dealt in pieces)
    int C;
    // long rows
    const int32_t *long_rows;
    const int64_t *long_chunk_ptr;
    const int32_t *chunk_long;
    const int32_t *chunk_order;
    const int32_t *row_order;
    const int64_t *slot_beg;        // Csr::slot_beg / slot_cnt (or null)
    const int32_t *slot_cnt;
    const int32_t *nonempty_rows;   // Csr::nonempty_rows (or null)
    const int32_t *row_list;        // set by the launcher: the wave-per-row kernels take row = row_list[slot] (null: row = slot)
    float *partial;
    int64_t n_long, n_chunks;
    int long_row, long_chunk;
    int tune;
    bool skip_empty;           // GNX_ACT_SKIP_EMPTY: rows without entries are left untouched
    int64_t xcd_rows;          // > 0: the row order carries locality (= Csr::order_window): the blocks that share an XCD take whole CHUNKS
    uint32_t xcd_chunk;        // of xcd_chunk consecutive blocks = one window's worth of slots (xcd_block; set per launch from xcd_rows)
    DropFuse fuse;
};

// "Done once" per DEVICE, not per process: a process may drive several GPUs (gnntf's nat.on_device, vertex blocks as threads), and a
// kernel attribute set on one device says nothing about the next.  Concurrent first calls may both do the (idempotent) work.
struct PerDeviceOnce {
    std::atomic<uint64_t> done{0};
    static int device() { int d = 0; if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); d = -1; } return d; }
    bool need(int dev) const { return dev < 0 || dev >= 64 || !((done.load(std::memory_order_acquire) >> dev) & 1u); }
    void set(int dev) { if (dev >= 0 && dev < 64) done.fetch_or(uint64_t(1) << dev, std::memory_order_release); }
};

int launch_spmm(gnx_graph *g, const Csr &m, SpmmArgs &p, hipStream_t s);                      // gnx_spmm.hip
void launch_long_rows(const SpmmArgs &p, hipStream_t s);                                       // gnx_spmm.hip: long rows only
// gnx_spmm_bf16.hip, for gnx_gcnii_step_bf16: p with its rows gathered from bf16 Xb (p.X unused) and finished as f32 into `out` (p.out
// unused), per row in the summation order of the f32 launch over the same arguments: hub chunks are dealt to the lane groups of at most
// 4 columns per lane, as F32Rows deals them (short rows add their entries in ascending order at any lane width).
int launch_spmm_bf16_f32_order(gnx_graph *g, const Csr &m, const SpmmArgs &p, const uint16_t *Xb, float *out, hipStream_t s);
void launch_long_rows_bf16(const SpmmArgs &p, const uint16_t *Xb, float *out, hipStream_t s);   // launch_long_rows, likewise
const char *launch_spmm_dropped(const SpmmArgs &p, int vec, hipStream_t s);              // gnx_spmm_train.hip
void launch_long_rows_dropped(const SpmmArgs &p, hipStream_t s);                         // gnx_spmm_train.hip: launch_long_rows under p.fuse
// gnx_spmm_train.hip, shared with gnx_spmm_train_bf16.hip: a handle with duplicate entries needs gnx_graph_enable_entry_dropout
// (GNX_ERR_UNSUPPORTED otherwise); the per-slot values and entry tables a fused launch over the handle reads
int refuse_duplicates(const gnx_graph *g, const char *fn);
void set_values(const gnx_graph *g, bool transposed, SpmmArgs &p);
void set_drop_fuse(const gnx_graph *g, float dropout_p, uint64_t seed, uint64_t stream_id, const float *d_D, int transposed,
                   int x_prescaled, SpmmArgs &p);
// out[out_rows[r]] = act(X[in_rows[r]] . W + bias) on the matrix cores (gnx_dense.hip); row maps optional
int dense_rows(const float *X, int64_t ldx, int64_t n, int64_t F, const float *W, int64_t ldw, int64_t O, const float *bias, int act,
               const int32_t *in_rows, const int32_t *out_rows, float *out, int64_t ldo, hipStream_t s);
// out[e] = partial[0][e] + partial[1][e] + ... in slab order, e < elems (gnx_dense_wgrad.hip): the last pass of the weight gradients
void sum_slabs(const float *partial, int64_t n_slabs, int64_t elems, float *out, hipStream_t s);
// out[r, :] = drop(X[r, :]) for the rows listed (null: rows 0 .. n), the mask keyed by row id and column (gnx_feature_dropout.hip): the
// fused layers' rows that go through memory; out may be X
void launch_feature_dropout(const float *X, int64_t ldx, const int32_t *rows, int64_t n, int64_t C, const DropFuse &fd, float *out, int64_t ldo,
                            hipStream_t s);
// out[r, :] holds act(P') of the rows listed (null: rows 0 .. n) and leaves as 2 drop(act(P') - bias) in place, the rows' gate words
// [., ceil(C / 32)] written beside it (gnx_gcnii.hip, k_spectral_tail: the spectral layers' rows that go through memory); bias null:
// zeros, fd null: no mask, gate null: no words
void launch_spectral_tail(float *out, int64_t ldo, const int32_t *rows, int64_t n, int64_t C, const float *bias, const DropFuse *fd,
                          uint32_t *gate, hipStream_t s);
#ifdef GNX_TUNING
extern int tune_override;
#endif

}  // namespace gnx
