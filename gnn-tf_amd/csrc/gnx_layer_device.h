// What the fused layer units stand on (gnx_gcnii.hip, gnx_gcn.hip, gnx_ngcf.hip: a layer family each; gnx_feature_dropout.hip: the mask as
// a pass of its own): the tile kernels' 16-row frame, the gathers, the feature mask, and the launch plumbing of their host paths.  What
// stands here is shared by contract -- a row made again has the bits of the row the forward stored because both ran this code; what is
// private to a layer stands in its unit.  No kernel stands here: every kernel has exactly one unit.
//   the mask           drop_stream, drop_values (the counter RNG of the edge dropout, keyed by row and column); EdgeArgs / feature_mask:
//                      where the mask's parameters travel when p.fuse belongs to the edge dropout
//   the frame          Tile<NT> (the geometry of a width), slot_row, tile_times_Ms (the MFMA block); described once above Tile
//   the gathers        gathered_row (a row of A . X; edge_gather where the weights are made from the edge dropout: EDGE / ENTRIES),
//                      written once over the row-storage policy R of gnx_spmm_device.h
//   the checks         make_feat_drop (the mask of one call), EdgeDrop / admit_edge_drop, fused_width, refuse_unfused
//   the plumbing       bind_fused, bind_values (loaded values, or the edge dropout into p), reserve_partial (the hub rows' slab, before the
//                      first launch), with_tile_width x with_out_tiles x with_flags (runtime widths and switches -> template arguments),
//                      launch_row_pass (the row passes' vector width and grid), hub_rows_tail (the long-row kernels, then the caller's
//                      transform of those rows alone), spmm_back_composed (a backward's order at the widths without a fused launch),
//                      GNX_TILE_NAMES (what gnx_graph_last_kernel reports for a tile kernel)
// Hub rows share the long-row path of gnx_spmm.hip / gnx_spmm_bf16.hip (launch_long_rows, launch_long_rows_bf16: the f32 launch's
// summation order) and the dense kernel on those rows alone; rounding points in gnx.h.  The masks come from the counter RNG of the edge
// dropout.  The templates and the device code have internal linkage, as in gnx_spmm_device.h; the plain host functions are inline in
// namespace gnx.
#pragma once
#include "gnx_spmm_device.h"

namespace {

// Feature dropout of a [n, C] matrix from the counter RNG of the edge dropout (hash_u24, gnx_internal.h), its parameters in the DropFuse
// of the edge dropout (seed, stream, offset, thr, scale; nothing else of it is read): element (i, c) is kept iff
// hash_u24(seed, stream + counter, i, c, 0) >= thr -- i the row id, c the column, duplicate rank 0, counter the handle's device-side
// dropout counter (read when the kernel runs) -- and a kept value leaves as v * scale, a dropped one as +0.  thr == 0 keeps everything:
// nothing is hashed (p == 0: scale = 1, the values leave as they are).
__device__ __forceinline__ uint64_t drop_stream(const DropFuse &f) { return f.stream + (f.offset ? *f.offset : 0); }

// x[v] <- drop(x[v]) for columns c .. c + VEC - 1 of row `row` (the row's round of the hash is shared by the columns)
template <int VEC>
__device__ __forceinline__ void drop_values(const DropFuse &f, uint64_t stream, int64_t row, int64_t c, float (&x)[VEC]) {
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        x[v] = (f.thr == 0 || hash_u24(f.seed, stream, (uint64_t)row, (uint64_t)(c + v), 0) >= f.thr) ? x[v] * f.scale : 0.f;
}

// ---- the layer under edge dropout (gnx_gcnii_step_dropped, gnx_gcnii_step_back_dropped; EDGE) ---------------------------------------------
// p.fuse belongs to the edge dropout there -- the weights of the gather loop come from it (dropped_weight_at) -- so the feature mask of
// DROP arrives beside it; the instantiations without EDGE carry an empty struct and keep reading p.fuse.
template <bool EDGE> struct EdgeArgs {};
template <> struct EdgeArgs<true> {
    DropFuse feat;         // the mask of the finished rows (seed, stream, offset, thr, scale); read by the DROP instantiations only
};
template <bool EDGE>
__device__ __forceinline__ const DropFuse &feature_mask(const SpmmArgs &p, const EdgeArgs<EDGE> &ed) {
    if constexpr (EDGE) return ed.feat;
    else return p.fuse;
}

// ---- the 16-row tile frame of k_spmm_gcnii, k_spmm_gcn, k_spmm_gcnii_back, k_spmm_gcn_back and k_gcnii_wgrad ----------------------------
// A block is WPB = 8 waves; wave w of block b owns tile b WPB + w: 16 row SLOTS of the structure's launch order (slot_row).  At width
// C = 16 NT a row is held by G = 4 NT lanes of four columns each, so a wave holds RPP = 64 / G rows at a time and walks its tile in
// PASSES = 16 / RPP passes: in pass ps lane l holds slot rr = ps RPP + l / G of the tile and columns c = 4 (l % G) .. c + 3.  The wave's
// tile and the block's matrix (filled by the whole block before the waves past n_rows return) live in LDS with row stride C + 4 (= 4
// mod 32 banks).  A slot past n_rows -- the ragged last tile -- has row -1; a slot is LIVE when it has a row of at most p.long_row
// entries (hub rows are left to the long-row kernels + the dense kernel).  A dead slot holds zeros in the tile and stores nothing.  The
// three tile kernels fill the tile pass by pass (rows[] / live[] keep what a pass found), put a wave barrier behind it, multiply
// (tile_times_Ms) and walk the finished tile: a float4 of the lane's columns per live pass.
// The geometry and the slot's row are written once below.  The fill, the slot -> row -> extent -> live step and the walk stand in each
// kernel: written as __forceinline__ functions (over a lambda row body; the slot as a struct or through references) every one of them
// changed instructions of some instantiation (profiles/NOTES.md, "The layer kernels' tile frame"), and the kernels stay the ones measured.
template <int NT> struct Tile {
    static constexpr int C = 16 * NT, G = 4 * NT, RPP = 64 / G, PASSES = 16 / RPP, STRIDE = C + 4;
};

// the row of slot `slot` < p.n_rows: the launch order is p.row_order (degree-binned; another one under a row window), null = the rows as numbered
__device__ __forceinline__ int64_t slot_row(const SpmmArgs &p, int64_t slot) { return p.row_order ? (int64_t)p.row_order[slot] : slot; }

// tile <- act(tile . Ms) for one wave's 16-row tile T and the block's Ms (both row stride C + 4, C = 16 NT), on
// v_mfma_f32_16x16x4_f32: the block the forward layer and its backward (k_spmm_gcnii_back) share.  The caller has put a wave
// barrier between its writes of T and this call; on return the whole tile is written and visible to the wave.
// BIAS (the spectral form): tile <- act(tile . Ms + bias[c]), the bias added to the accumulator value as it leaves the MFMA block.
// NTN (k_spmm_gcn): Ms holds 16 NTN <= C columns -- a rectangular transform -- and the result tile has that many, over the tile's
// first columns; its bias has n_bias entries, the columns from there on add 0 (n_bias = 0: no bias at all, the pointer is not read).
// NTK (k_spmm_gcn_back): the k extent -- the tile's first 16 NTK <= C columns are the gathered ones and Ms has that many rows.
template <int NT, bool BIAS = false, int NTN = NT, int NTK = NT>
__device__ __forceinline__ void tile_times_Ms(float *__restrict__ T, const float *__restrict__ Ms, int lane, int act,
                                              const float *__restrict__ bias = nullptr, int n_bias = 16 * NTN) {
    constexpr int C = 16 * NTK, STRIDE = Tile<NT>::STRIDE;
    static_assert(NTN >= 1 && NTN <= NT, "the result tile overwrites the gathered one");
    static_assert(NTK >= 1 && NTK <= NT, "the gathered columns are the tile's first");
    // tile . M : A[m = lane & 15][k = 4 kk + (lane >> 4)] from the tile, B[k][n = lane & 15] from Ms
    const int cc = lane & 15, g = lane >> 4;
    [[maybe_unused]] float bv[NTN];
    if constexpr (BIAS) {
#pragma unroll
        for (int nt = 0; nt < NTN; ++nt) bv[nt] = 16 * nt + cc < n_bias ? bias[16 * nt + cc] : 0.f;
    }
    f32x4 d[NTN];
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
    // D: lane (cc, g), register r -> row 4g + r, column 16 nt + cc; back through the tile so that rows leave as whole float4 rows
#pragma unroll
    for (int nt = 0; nt < NTN; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = d[nt][r];
            if constexpr (BIAS) v += bv[nt];
            if (act == GNX_ACT_RELU) v = fmaxf(v, 0.f);
            T[(4 * g + r) * STRIDE + 16 * nt + cc] = v;
        }
    __builtin_amdgcn_wave_barrier();
}

// The gather loop of the EDGE forms (k_spmm_gcnii, k_spmm_gcnii_back under edge dropout), columns c .. c + 3 of row `row` into acc: the
// entries in ascending order, U in flight per lane and one fmaf chain, as in the loops that load their weights -- the weight of an entry is
// (D[row] * drop(raw)) * D[col] from p.fuse, the arithmetic of k_scale_values, so it has the bits of the value gnx_graph_normalize would
// have stored there (ENTRIES: a handle with duplicate entries, p.vals = each slot's uniform value).  The G lanes of a row share the work
// of making the weights, as the lane groups of k_spmm_group_drop do: lane `sub` draws entry base + sub of a round of G entries -- one hash
// per stored entry, not one per lane -- and the round is walked U entries at a time through shuffles inside the group (the lanes of a row
// run the loop together: same beg and end).  A weight of exactly 0 -- a dropped entry, or a slot past the end of the row -- gathers
// nothing and adds fmaf(0, 0, acc) = acc (the DroppedAdjacency precondition of finite features).
// `loads` (k_spmm_gcn_back, whose rows are narrower than its lane groups): a lane without columns of its own draws its share of the
// weights and takes part in the shuffles, and gathers nothing.
template <bool ENTRIES, int G, int U>
__device__ __forceinline__ void edge_gather(const SpmmArgs &p, const float *__restrict__ Xc, int64_t row, int64_t beg, int64_t end,
                                            float (&acc)[4], bool loads = true) {
    static_assert(G % U == 0, "a round of G entries is whole batches of U");
    const int sub = (int)(threadIdx.x % G);
    for (int64_t base = beg; base < end; base += G) {
        int mycol = 0;
        float myw = 0.f;
        if (base + sub < end) {
            mycol = p.colidx[base + sub];
            myw = dropped_weight_at<ENTRIES>(p.fuse, p.vals[base + sub], base + sub, row, mycol);
        }
        const int n = (int)(end - base < G ? end - base : G);
        for (int k = 0; k < n; k += U) {
            float x[U][4];
            float w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = __shfl(mycol, k + u, G);
                w[u] = __shfl(myw, k + u, G);
                if (w[u] != 0.f && loads) vload<4>(x[u], Xc + (int64_t)j * p.ldx);
                else {
#pragma unroll
                    for (int v = 0; v < 4; ++v) x[u][v] = 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
        }
    }
}

// One aggregated row sum_j A[row, j] X[j, c .. c + 3] (entries beg .. end) into acc (zeros on entry): the gather loop and the entry
// order, written once -- U entries in flight per lane and one fmaf chain.  The GCNII kernels mix the sum behind it (mixed_row), the GCN
// layer (k_spmm_gcn) takes it as it is.
// EDGE (G = the lanes of a row): the entry's weight is made, not loaded (edge_gather above).
template <typename R, int U, bool EDGE = false, bool ENTRIES = false, int G = 0>
__device__ __forceinline__ void gathered_row(const typename R::Args &p, int64_t row, int64_t beg, int64_t end, int c, float (&acc)[4]) {
    const typename R::Elem *__restrict__ Xc = R::X(p) + c;
    if constexpr (EDGE) {
        edge_gather<ENTRIES, G, U>(p, Xc, row, beg, end, acc);
    } else {
        for (int64_t e = beg; e < end; e += U) {
            float x[U][4];
            float w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (e + u < end) {
                    const int j = p.colidx[e + u];
                    w[u] = p.vals[e + u];
                    R::template load<4>(x[u], Xc + (int64_t)j * p.ldx);
                } else {
                    w[u] = 0.f;
#pragma unroll
                    for (int v = 0; v < 4; ++v) x[u][v] = 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
        }
    }
}

}  // namespace

// ---- the host side: checks and refusals ----------------------------------------------------------------------------------------------------
namespace gnx {

inline int64_t roundup4(int64_t x) { return (x + 3) / 4 * 4; }

// the fused launch takes C = 16, 32 or 64 (C = 128 fits the kernel -- 135 KB of LDS: one block of eight waves per CU -- and was measured:
// 19.2 ms against 11.8 ms for the two launches on the config-4 graph; eight waves per CU cannot keep the gathers fed)
inline bool fused_width(int64_t C) { return C == 16 || C == 32 || C == 64; }

// what the entries without a composed form answer to the other widths and alignments: the callers keep f32 there
inline int refuse_unfused(const char *fn, int64_t C) {
    if (!fused_width(C)) set_error("%s: width %lld is not supported (the fused launch takes C = 16, 32 or 64; keep f32 storage elsewhere)", fn, (long long)C);
    else set_error("%s: misaligned buffer (the f32 buffers must be 16-byte aligned, the bf16 buffers 8-byte aligned)", fn);
    return GNX_ERR_UNSUPPORTED;
}

// the mask of one call: keep iff hash >= int(p * 2^24) (oracle/gnntf_oracle.py:dropout_threshold, over the caller's double), kept values
// times the f32 scale of the edge dropout, 1.0f / (1.0f - (float)p); the handle lends its dropout counter
inline int make_feat_drop(const char *fn, const gnx_graph *g, double p, uint64_t seed, uint64_t stream_id, DropFuse &fd) {
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(p >= 0.0 && p < 1.0, "%s: dropout rate %g outside [0, 1)", fn, p);
    fd.seed = seed; fd.stream = stream_id; fd.offset = g->stream_offset;
    fd.thr = drop_threshold(p);
    fd.scale = drop_scale((float)p);
    return GNX_OK;
}

// the edge dropout of gnx_gcnii_step_dropped / gnx_gcnii_step_back_dropped: what gnx_spmm_dropped takes
struct EdgeDrop { const float *D; float p; uint64_t seed, stream; };

// what those two entries check before anything is built or launched, as gnx_spmm_dropped_back does
inline int admit_edge_drop(const char *fn, gnx_graph *g, const EdgeDrop &e) {
    GNX_CHECK_ARG(e.D != nullptr, "%s: NULL degree scales", fn);
    GNX_CHECK_ARG(e.p >= 0.f && e.p < 1.f, "%s: dropout rate %g outside [0, 1)", fn, (double)e.p);
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols && g->blk_col_gid == nullptr, "%s: needs a square stand-alone graph", fn);
    return refuse_duplicates(g, fn);
}

// the structure and the long-row plan of a fused launch (its short rows need nothing else of bind_csr)
inline void bind_fused(const Csr &m, SpmmArgs &p) {
    p.rowptr = m.rowptr; p.colidx = m.colidx; p.n_rows = m.n_rows; p.n_nonempty = m.n_nonempty; p.row_order = m.row_order;
    p.long_rows = m.long_rows; p.long_chunk_ptr = m.long_chunk_ptr; p.chunk_long = m.chunk_long; p.chunk_order = m.chunk_order;
    p.n_long = m.n_long; p.n_chunks = m.n_chunks; p.long_row = m.long_row; p.long_chunk = m.long_chunk;
}

// ---- the host side: binding and reservation ------------------------------------------------------------------------------------------------
// The values a fused launch walks with, into p: under `edge` they are made in the gather loop (p.fuse becomes the edge dropout's, over the
// handle's per-slot values of that side), else they are loaded -- the caller's d_vals, or the handle's raw values of that side.
inline void bind_values(const gnx_graph *g, const EdgeDrop *edge, bool transposed, const float *d_vals, SpmmArgs &p) {
    if (edge) {
        set_values(g, transposed, p);
        set_drop_fuse(g, edge->p, edge->seed, edge->stream, edge->D, transposed ? 1 : 0, 0, p);
    } else {
        p.vals = d_vals ? d_vals : transposed ? g->t_raw.get() : g->raw_vals.get();
    }
}

// The slab of the hub rows' chunked partial sums at width C, reserved before the first launch of a call: under capture a slab that would
// have to grow refuses the whole call.
inline int reserve_partial(gnx_graph *g, const Csr &m, int64_t C, hipStream_t s) {
    return m.n_long > 0 ? ensure_partial(g, (size_t)m.n_chunks * (size_t)C * sizeof(float), s) : GNX_OK;
}

// The composed order of a layer's backward, for the widths / alignments without a fused launch: gT = G . Wt ([n, C_g] times [C_g, C])
// into d_work [n, C], then out = beta At gT over the transposed structure, At from d_vals_t or made from `edge`.  The transpose and the
// hub rows' slab come before the first launch: under capture a part that would have to be built refuses the whole call.
inline int spmm_back_composed(gnx_graph *g, const float *d_vals_t, const EdgeDrop *edge, const float *d_G, int64_t ldg, int64_t C_g,
                              const float *d_Wt, int64_t ldwt, int64_t C, float beta, float *d_work, float *d_out, int64_t ldo, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    int rc = ensure_transpose(g, s);
    if (rc != GNX_OK) return rc;
    rc = reserve_partial(g, g->t, C, s);
    if (rc != GNX_OK) return rc;
    rc = gnx_dense(d_G, ldg, g->a.n_rows, C_g, d_Wt, ldwt, C, nullptr, GNX_ACT_NONE, d_work, C, stream);
    if (rc != GNX_OK) return rc;
    if (edge) return gnx_spmm_dropped(g, edge->D, edge->p, edge->seed, edge->stream, 1, d_work, C, C, nullptr, 0, beta, 0.f, GNX_ACT_NONE, d_out, ldo, stream);
    return gnx_spmm_tv(g, d_vals_t ? d_vals_t : g->t_raw.get(), nullptr, d_work, C, C, nullptr, 0, beta, 0.f, GNX_ACT_NONE, d_out, ldo, stream);
}

}  // namespace gnx

// what gnx_graph_last_kernel reports for a tile kernel at width c: {without hub rows, with them}
#define GNX_TILE_NAMES(kernel, c, tail) {kernel "<" c ">" tail, kernel "<" c ">" tail "+long"}

// ---- the host side: launch plumbing (templates: internal linkage) ---------------------------------------------------------------------------
namespace {

using Bf16Rows = Bf16RowsT<false>;

// f(IntC<NT>, grid) for the two fused kernels at width C = 16 NT in {16, 32, 64}: blocks of 512 threads, a 16-row tile per wave
template <typename F>
void with_tile_width(int64_t C, int64_t n_rows, F &&f) {
    const dim3 grid(blocks_for(blocks_for(n_rows, 16), 8));
    if (C == 64)      f(IntC<4>{}, grid);
    else if (C == 32) f(IntC<2>{}, grid);
    else              f(IntC<1>{}, grid);
}

// f(IntC<n_tiles>) for the 1 .. 4 blocks of 16 columns of a tile's second width (C_out <= C_in <= 64); f guards the counts that have no
// kernel with `if constexpr`
template <typename F>
void with_out_tiles(int n_tiles, F &&f) {
    if (n_tiles == 1)      f(IntC<1>{});
    else if (n_tiles == 2) f(IntC<2>{});
    else if (n_tiles == 3) f(IntC<3>{});
    else                   f(IntC<4>{});
}

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): runtime switches as template arguments.  Every combination of the flags is
// instantiated in f, which guards the ones that have no kernel with `if constexpr`.
template <typename F>
void with_flags(F &&f) { f(); }
template <typename F, typename... Flags>
void with_flags(F &&f, bool flag, Flags... rest) {
    if (flag) with_flags([&](auto... tail) { f(std::true_type{}, tail...); }, rest...);
    else      with_flags([&](auto... tail) { f(std::false_type{}, tail...); }, rest...);
}

// ---- the row passes: a thread per VEC columns of an [n, C] matrix, grid-stride above 2^20 blocks of 256 -------------------------------
// launch(IntC<VEC>, grid): VEC = 4 (16-byte f32 / 8-byte bf16 accesses) where C and every buffer of the pass allow it, else 1
struct RowsAt { const void *base; size_t align; int64_t ld; };      // a buffer of the pass: its base, the alignment VEC = 4 needs, its row stride

template <typename F>
void launch_row_pass(int64_t n, int64_t C, std::initializer_list<RowsAt> buffers, F &&launch) {
    bool v4 = C % 4 == 0;
    for (const RowsAt &b : buffers) v4 = v4 && b.ld % 4 == 0 && aligned(b.base, b.align);
    const unsigned grid = (unsigned)std::min<int64_t>(blocks_for(n * (v4 ? C / 4 : C), 256), 1 << 20);
    if (v4) launch(IntC<4>{}, grid);
    else    launch(IntC<1>{}, grid);
}

// the chunked partial sums of the hub rows of a fused launch, mixed as p says, into f32 rows at `out` (p.partial set)
// (`dropped`, f32 rows: p.fuse is an edge dropout and the chunks make their weights from it, launch_long_drop of gnx_spmm_drop.h)
template <typename R>
void launch_hub_rows(typename R::Args &p, const typename R::Elem *X, float *out, hipStream_t s, bool dropped = false) {
    if constexpr (R::BF16) launch_long_rows_bf16(p, X, out, s);
    else {
        p.out = out;
        if (dropped) launch_long_rows_dropped(p, s);
        else launch_long_rows(p, s);
    }
}

// The tail of a fused launch.  Hub rows: their chunked partial sums, finished as p says (the caller has set the p.act / p.ldo of rows that
// go through memory), into f32 rows at their row ids of `to`, then transform(m.long_rows, m.n_long) -- what the caller does with those
// rows alone.  Then, hub rows or none, the launches' error state.
template <typename R, typename F>
int hub_rows_tail(gnx_graph *g, const Csr &m, typename R::Args &p, const typename R::Elem *X, float *to, bool dropped, hipStream_t s, F &&transform) {
    if (m.n_long > 0) {
        p.partial = g->partial;
        launch_hub_rows<R>(p, X, to, s, dropped);
        const int rc = transform(m.long_rows, m.n_long);
        if (rc != GNX_OK) return rc;
    }
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

}  // namespace
