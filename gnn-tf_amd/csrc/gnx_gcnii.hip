// The GCNII layer (gcn.py:7-27,54-74), the GCN layer (gcn.py:77-89) and the NGCF layer (gcn.py:116-135) on gfx950: six kernels on one
// 16-row tile frame, the row passes around them, and ONE host path per kernel over the launch plumbing they share.
//   the frame          Tile<NT> (the geometry of a width), slot_row, tile_times_Ms (the MFMA block); described once above Tile
//   the gathers        gathered_row (a row of A . X; edge_gather where the weights are made from the edge dropout: EDGE / ENTRIES) and
//                      mixed_row (the residual mix behind it), written once over the row-storage policy R of gnx_spmm_device.h
//   k_spmm_gcnii       the GCNII layer in one launch: SpMM + mix + the C x C transform (DROP: + the feature mask in the store loop; SPEC:
//                      the spectral-preserving form, gnx_gcnii_step_spectral -- k_spectral_tail is its epilogue as a row pass,
//                      k_spectral_back the backward's first pass)
//   k_spmm_gcn         the GCN layer in one launch: the gather without the residual operand, a rectangular W [C_in, C_out <= C_in]
//   k_spmm_ngcf        the NGCF layer in one launch: k_spmm_gcn's fill, two matrices in LDS, the message product kept in the accumulators
//                      while the tile is multiplied by the rows' own X, the mask and the row norm in the store loop (k_ngcf_product and
//                      k_ngcf_tail: the same layer as row passes around the dense kernel; k_ngcf_back_gate: the backward's first pass)
//   k_spmm_gcnii_back  the GCNII layer's backward past the relu gate, one launch over the transposed structure
//   k_spmm_gcn_back    the GCN layer's input gradient past the gate, one launch over the transposed structure: the gated gradient
//                      gathered at the OUTPUT width, stored at the input width (two geometries of the one tile)
//   k_gcnii_wgrad      the GCNII weight gradient dM = T^T G with the mixed rows T made again in LDS (mixed_row) and never stored
//   row passes         k_round_rows (f32 rows -> bf16), k_feature_dropout (the mask as a pass of its own: hub rows, the other widths, the
//                      generic composition) and the backward's gate (k_feature_dropout_back, .._back_bf16); launch_row_pass picks
//                      their vector width and grid
//   the plumbing       bind_values (loaded values, or the edge dropout into p), reserve_partial (the hub rows' slab, before the first
//                      launch), with_tile_width x with_flags (runtime width and switches -> template arguments), hub_rows_tail (the
//                      long-row kernels, then the caller's transform of those rows alone)
//   gcnii_forward<R>   gnx_gcnii_step, _step_drop, _step_dropped, _step_spectral (F32Rows), _step_bf16, _step_train_bf16, _step_drop_bf16
//                      (Bf16Rows); a ForwardForm says what differs: the mask, where mixed rows are kept or pass through memory, the
//                      format of the result, and whether the widths other than 16 / 32 / 64 run as two launches or are refused
//   gcnii_backward<R>  gnx_gcnii_step_back, _step_back_dropped, _step_back_bf16; the composed form of the other widths is its f32 branch
//   gcnii_wgrad<R>     gnx_gcnii_wgrad, gnx_gcnii_wgrad_bf16
//   gcn_forward        gnx_gcn_step, gnx_gcn_step_dropped
//   gcn_backward       gnx_gcn_step_back, gnx_gcn_step_back_dropped; the composed order of the other widths / strides is its branch
//   ngcf_forward       gnx_ngcf_step (gnx_ngcf_back_gate is an entry of its own: one launch)
// Hub rows share the long-row path of gnx_spmm.hip / gnx_spmm_bf16.hip (launch_long_rows, launch_long_rows_bf16: the f32 launch's
// summation order) and the dense kernel on those rows alone; rounding points in gnx.h.  The masks come from the counter RNG of the edge
// dropout.
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

// ---- the spectral-preserving form (gcn.py:30-51, gnx_gcnii_step_spectral): out = 2 drop(act(P') - bias), P' = T . M + bias ------------
// What a launch needs beside the plain layer's arguments; the plain instantiations carry an empty struct.
template <bool SPEC> struct SpectralArgs {};
template <> struct SpectralArgs<true> {
    const float *bias;     // [C]
    uint32_t *gate;        // [n, ceil(C / 32)] or null: bit c & 31 of word row * ceil(C / 32) + (c >> 5) = (P'[row, c] > 0)
};

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

// x[v] = act(P') of columns c .. c + VEC - 1 of row `row`  ->  2 drop(x[v] - bias[v]): the ONE place the finished value is formed, for
// the store loop of the fused launch and for the row pass behind the dense kernel (k_spectral_tail), so that a row has the same bits
// whichever path made it.  Returns the gate bits of the VEC columns, bit v = (x[v] > 0): with the relu act(P') > 0 iff P' > 0, so the
// gate is that of the pre-activation itself and never a guess from the finished value (relu(P') - bias rounds to -bias for a tiny P').
template <int VEC, bool DROP>
__device__ __forceinline__ uint32_t spectral_finish(const DropFuse &f, uint64_t stream, int64_t row, int64_t c, const float (&bias)[VEC],
                                                    float (&x)[VEC]) {
    uint32_t bits = 0;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        bits |= (x[v] > 0.f ? 1u : 0u) << v;
        x[v] -= bias[v];
    }
    if constexpr (DROP) drop_values<VEC>(f, stream, row, c, x);
#pragma unroll
    for (int v = 0; v < VEC; ++v) x[v] *= 2.f;
    return bits;
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

// One mixed row of the fused layer, columns c .. c + 3 of row `row` (entries beg .. end) into acc (zeros on entry): the gather
// (gathered_row) and the mix, written once -- the forward (k_spmm_gcnii) and the weight gradient that makes T again (k_gcnii_wgrad) run
// this code, so a row made again has the bits of the row the forward stored.
template <typename R, int U, bool EDGE = false, bool ENTRIES = false, int G = 0>
__device__ __forceinline__ void mixed_row(const typename R::Args &p, int64_t row, int64_t beg, int64_t end, int c, float (&acc)[4]) {
    gathered_row<R, U, EDGE, ENTRIES, G>(p, row, beg, end, c, acc);
    float h0[4];
    vload<4>(h0, p.H0 + row * p.ldh0 + c);
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[v] = fmaf(acc[v], p.beta, h0[v] * p.alpha);      // filter.py:20-21 / gcn.py:25
}

// ---- GCNII layer: SpMM + mix + C x C transform on the matrix cores + activation, one launch ------------------------
//   out[i,:] = act( (beta * sum_j A[i,j] X[j,:] + alpha * H0[i,:]) . M ),   M = (1-b) I + b W   (gcn.py:22-27)
// The frame with mixed_row as the row's body (U entries in flight per lane): the mixed rows stay in the wave's LDS tile -- in inference
// they never go to HBM; in training (`mixed` given) each lane also stores its piece of the mixed row, which the backward needs for
// dM = T^T g, so that the row is written once and NOT read back for the transform -- meet M on v_mfma_f32_16x16x4_f32 (exact f32) and
// leave as whole rows.  C = 16 NT for NT in {1, 2, 4}.  (NT = 8, C = 128, fits -- 135 KB of the CU's 160 KB of LDS -- but leaves one
// block of eight waves per CU: measured 19.2 ms against 11.8 ms for SpMM+mix followed by the dense kernel, so wide layers keep the two
// launches.)
// Written once over the row-storage policy R (gnx_spmm_device.h): F32Rows gathers float4 pieces of f32 rows, Bf16RowsT 8-byte pieces of
// bf16 rows (four columns, widened exactly) and stores the finished row as f32 or rounded once to bf16; entry order, summation order,
// the mix and the transform are the same code, so the bf16 instantiation over bf16-representable rows gives the bits of the f32 one.
// DROP (gnx_gcnii_step_drop): the finished rows leave as drop(act(T . M)) -- the mask is made in the store loop, after the MFMA block,
// where a lane holds row rows[ps] and columns c .. c + 3, so that the hash costs the gather loop no register; `mixed` still gets the
// undropped T.  The mask's parameters are p.fuse (this kernel has no other use for it), so the
// switch is a template argument alone and the instantiations without it are the kernel as it was.
// SPEC (gnx_gcnii_step_spectral, f32 rows): the bias joins the accumulator in the MFMA block's epilogue, before the activation, and the
// store loop forms 2 drop(act(P') - bias) (spectral_finish); with sp.gate the launch also writes one bit per element, P' > 0, which is
// all the backward needs of the forward: a lane holds four columns of a row, the 4 NT lanes of a row (eight of them per 32-column
// word) OR their bits together through xor-shuffles and one lane stores the word.  Like DROP a template argument alone.
// EDGE (gnx_gcnii_step_dropped, f32 rows, with ENTRIES on a handle after gnx_graph_enable_entry_dropout): the gather loop makes its
// weights from p.fuse (mixed_row, edge_gather) and the mask of DROP comes from ed.feat; entry order, U, the fmaf chain, the mix and
// everything behind them are those of the other instantiations.
template <typename R, int NT, int U, int WPB, bool DROP = false, bool SPEC = false, bool EDGE = false, bool ENTRIES = false>
__global__ __launch_bounds__(64 * WPB) void k_spmm_gcnii(const typename R::Args p, const float *__restrict__ M, int64_t ldm, float *__restrict__ mixed,
                                                         const SpectralArgs<SPEC> sp = SpectralArgs<SPEC>{},
                                                         const EdgeArgs<EDGE> ed = EdgeArgs<EDGE>{}) {
    static_assert(!EDGE || (!SPEC && !R::BF16), "the edge-dropout form exists for the plain layer over f32 rows");
    using TL = Tile<NT>;
    constexpr int C = TL::C, G = TL::G, RPP = TL::RPP, PASSES = TL::PASSES, STRIDE = TL::STRIDE;
    __shared__ float Ms[C * STRIDE];
    __shared__ float Ts[WPB][16 * STRIDE];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int idx = threadIdx.x; idx < C * C; idx += 64 * WPB) Ms[(idx / C) * STRIDE + idx % C] = M[(int64_t)(idx / C) * ldm + idx % C];
    __syncthreads();
    const int64_t tile = (int64_t)blockIdx.x * WPB + wave;
    if (tile * 16 >= p.n_rows) return;
    float *__restrict__ T = Ts[wave];
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
            mixed_row<R, U, EDGE, ENTRIES, G>(p, row, beg, end, c, acc);
            if (mixed) vstore<4>(mixed + row * (int64_t)C + c, acc);
        }
        vstore<4>(T + rr * STRIDE + c, acc);
    }
    __builtin_amdgcn_wave_barrier();
    if constexpr (SPEC) {
        constexpr int GW = G < 8 ? G : 8, WORDS = (C + 31) / 32;      // lanes per gate word, words per row
        tile_times_Ms<NT, true>(T, Ms, lane, p.act, sp.bias);
        float b[4];
        vload<4>(b, sp.bias + c);
        uint64_t stream = 0;
        if constexpr (DROP) stream = drop_stream(p.fuse);
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
            const int rr = ps * RPP + lane / G;
            float o[4];
            vload<4>(o, T + rr * STRIDE + c);
            // (every lane of the wave takes part in the shuffles; a row's lanes are live or not together, and a dead row stores nothing)
            uint32_t word = spectral_finish<4, DROP>(p.fuse, stream, rows[ps], c, b, o) << (c & 31);
#pragma unroll
            for (int m = 1; m < GW; m <<= 1) word |= (uint32_t)__shfl_xor((int)word, m);
            if (!live[ps]) continue;
            R::template store<4>(p, rows[ps] * p.ldo, c, o);
            if (sp.gate != nullptr && sub % GW == 0) sp.gate[rows[ps] * WORDS + (c >> 5)] = word;
        }
        return;
    }
    tile_times_Ms<NT>(T, Ms, lane, p.act);
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        if (!live[ps]) continue;
        const int rr = ps * RPP + lane / G;
        float o[4];
        vload<4>(o, T + rr * STRIDE + c);
        if constexpr (DROP) {
            const DropFuse &fd = feature_mask<EDGE>(p, ed);
            drop_values<4>(fd, drop_stream(fd), rows[ps], c, o);
        }
        R::template store<4>(p, rows[ps] * p.ldo, c, o);
    }
}

// ---- GCN layer: SpMM + the C_in x C_out transform on the matrix cores + bias + activation, one launch (gnx_gcn_step) --------------------
//   out[i,:] = drop( act( (sum_j A[i,j] X[j,:]) . W + bias ) )      (gcn.py:88-89)
// The frame at C_in = 16 NTI with gathered_row (the loop the GCNII kernels mix behind) as the row's body.  The block's matrix is
// W [C_in, C_out], 1 <= C_out <= C_in, its columns from C_out to 16 NTO zero-filled (NTO = ceil(C_out / 16): the padding exists in LDS
// alone); the product is tile_times_Ms with NTN = NTO, the bias (null: none) joins the accumulator as it leaves the MFMA block, before the
// activation, and the result tile overwrites the gathered one (C_out <= C_in: no second tile; the LDS is k_spmm_gcnii's).  `agg` (null: not
// kept) gets the aggregated rows, [n, C_in] contiguous, from the lanes that made them: training keeps them for dW = agg^T G', and the
// transform never reads them back.  A lane stores its columns below C_out: a whole float4 where `vec_out` says the row starts of out allow
// it (ldo % 4 == 0 and a 16-byte aligned base) and the four columns exist, scalars otherwise -- nothing is written past column C_out - 1 of
// any row.  DROP (`feat`, keyed by row and column; agg stays undropped) and EDGE / ENTRIES as in k_spmm_gcnii.  f32 rows only.
template <typename R, int NTI, int NTO, int U, int WPB, bool DROP = false, bool EDGE = false, bool ENTRIES = false>
__global__ __launch_bounds__(64 * WPB) void k_spmm_gcn(const typename R::Args p, const float *__restrict__ W, int64_t ldw, int C_out,
                                                       const float *__restrict__ bias, float *__restrict__ agg, bool vec_out, const DropFuse feat) {
    static_assert(!R::BF16, "the GCN layer exists over f32 rows");
    static_assert(NTO >= 1 && NTO <= NTI, "C_out <= C_in: the result tile overwrites the gathered one");
    using TL = Tile<NTI>;
    constexpr int C = TL::C, CO = 16 * NTO, G = TL::G, RPP = TL::RPP, PASSES = TL::PASSES, STRIDE = TL::STRIDE;
    __shared__ float Ws[C * STRIDE];
    __shared__ float Ts[WPB][16 * STRIDE];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int idx = threadIdx.x; idx < C * CO; idx += 64 * WPB) {
        const int k = idx / CO, n = idx % CO;
        Ws[k * STRIDE + n] = n < C_out ? W[(int64_t)k * ldw + n] : 0.f;
    }
    __syncthreads();
    const int64_t tile = (int64_t)blockIdx.x * WPB + wave;
    if (tile * 16 >= p.n_rows) return;
    float *__restrict__ T = Ts[wave];
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
            gathered_row<R, U, EDGE, ENTRIES, G>(p, row, beg, end, c, acc);
            if (agg) vstore<4>(agg + row * (int64_t)C + c, acc);
        }
        vstore<4>(T + rr * STRIDE + c, acc);
    }
    __builtin_amdgcn_wave_barrier();
    tile_times_Ms<NTI, true, NTO>(T, Ws, lane, p.act, bias, bias ? C_out : 0);
    if (c >= C_out) return;
    const bool whole = vec_out && c + 4 <= C_out;
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        if (!live[ps]) continue;
        const int rr = ps * RPP + lane / G;
        float o[4];
        vload<4>(o, T + rr * STRIDE + c);
        if constexpr (DROP) drop_values<4>(feat, drop_stream(feat), rows[ps], c, o);
        float *__restrict__ dst = p.out + rows[ps] * p.ldo + c;
        if (whole) vstore<4>(dst, o);
        else {
#pragma unroll
            for (int v = 0; v < 4; ++v)
                if (c + v < C_out) dst[v] = o[v];
        }
    }
}

// ---- NGCF layer: SpMM + both transforms + the activations' sum + mask + row norm, one launch (gnx_ngcf_step) ------------------------------
//   A = sum_j Ahat[i,j] X[j,:]   P1 = (X[i,:] * A) . W1 + b1   P2 = A . W2 + b2   out = l2_normalize(drop(act(P1) + act(P2)))  (gcn.py:116-135)
// The pieces of the finished value that the fused launch and the row pass behind the dense kernel (k_ngcf_tail) share, so that a row is
// finished by the same code whichever path made its pre-activations:
//   ngcf_act        act(v): the identity, the relu of tile_times_Ms, or tf.nn.leaky_relu's v > 0 ? v : 0.2f v
//   ngcf_mask_sq    x <- drop(x) for columns c .. c + VEC - 1 of a row, then ss <- fmaf(x[v], x[v], ss) over the columns below C_out in
//                   ascending order: a lane's share of the row's sum of squares, one fmaf chain
//   ngcf_row_sum    the lanes of a row (GL consecutive lanes, GL a power of two) add their shares through xor-shuffles, strides 1, 2, ..
//                   GL / 2: every lane ends with the same bits, and lanes that hold +0 beyond a narrower row leave them unchanged
//   ngcf_rnorm      r = 1 / sqrt(max(ss, 1e-12f)) -- IEEE sqrt and divide, correctly rounded each -- and whether the clamp acted
__device__ __forceinline__ float ngcf_act(float v, int act) {
    if (act == GNX_ACT_RELU) return fmaxf(v, 0.f);
    if (act == GNX_ACT_LEAKY) return v > 0.f ? v : 0.2f * v;
    return v;
}

template <int VEC, bool DROP>
__device__ __forceinline__ float ngcf_mask_sq(const DropFuse &f, uint64_t stream, int64_t row, int64_t c, int64_t C_out, float (&x)[VEC], float ss) {
    if constexpr (DROP) drop_values<VEC>(f, stream, row, c, x);
#pragma unroll
    for (int v = 0; v < VEC; ++v)
        if (c + v < C_out) ss = fmaf(x[v], x[v], ss);
    return ss;
}

template <int GL>
__device__ __forceinline__ float ngcf_row_sum(float ss) {
#pragma unroll
    for (int m = 1; m < GL; m <<= 1) ss += __shfl_xor(ss, m);
    return ss;
}

__device__ __forceinline__ float ngcf_rnorm(float ss, bool &clamped) {
    clamped = !(ss >= 1e-12f);
    return 1.0f / sqrtf(fmaxf(ss, 1e-12f));
}

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

// ---- the layer's backward past the relu gate, one launch (gnx_gcnii_step_back) -----------------------------------------------
//   dH[r,:] = (beta * sum_c At[r,c] G[c,:]) . N        S_out[r,:] = s_alpha * S_in[r,:] + (alpha * G[r,:]) . N,    N = M^T
// (1-a) At (G N) = ((1-a) At G) N: the launch gathers the gated gradient G itself over the transposed structure (p), so g' M^T is
// never written or gathered back, and the row's own a G[r] N -- the layer's term of dH0 -- rides on the same Ms.  The frame over the
// transposed structure, with beta times the gather as the row's body.  The ONE tile of a wave serves both products, one after the other
// (first beta Z, then alpha G of the same 16 slots), so the kernel's LDS is the forward's (51 KB at C = 64: three blocks per CU; a
// second tile would leave two, and the forward's C = 128 experiment above shows what the gathers lose with fewer waves).  Every row
// below n takes part in the second product, hub rows and rows without entries included (rows[ps] >= 0, not live[ps]); a row without
// entries gets dH = 0, written.  S_in may be S_out (each lane reads the four values it overwrites); dH aliases nothing.
// Written once over the row-storage policy R, as the forward is: Bf16RowsT gathers 8-byte pieces of the bf16 copy Gb of the gated
// gradient (gnx_gcnii_step_back_bf16) and widens them exactly; dH (p.out) is f32 under either policy, and the row's own G[r] of the
// second product is read from the f32 p.X under either policy too -- the bf16 entry binds the f32 G there beside Gb, so the running dH0
// sum never sees a rounded addend.  Same entry order, sums and transform: over bf16-representable G both give the same bits.
// EDGE (gnx_gcnii_step_back_dropped, f32 rows; ENTRIES as in the forward): the weights of the transposed walk are made from p.fuse
// (fuse.transposed = 1; on an entry-dropout handle with its mult / perm / slot_ptr tables, as gnx_spmm_dropped_back walks it):
// edge_gather, the forward's loop.
template <typename R, int NT, int U, int WPB, bool EDGE = false, bool ENTRIES = false>
__global__ __launch_bounds__(64 * WPB) void k_spmm_gcnii_back(const typename R::Args p, const float *__restrict__ N, int64_t ldn, const float *S_in,
                                                              float s_alpha, float *S_out) {
    static_assert(!EDGE || !R::BF16, "the edge-dropout form exists for f32 rows");
    using TL = Tile<NT>;
    constexpr int C = TL::C, G = TL::G, RPP = TL::RPP, PASSES = TL::PASSES, STRIDE = TL::STRIDE;
    __shared__ float Ms[C * STRIDE];
    __shared__ float Ts[WPB][16 * STRIDE];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int idx = threadIdx.x; idx < C * C; idx += 64 * WPB) Ms[(idx / C) * STRIDE + idx % C] = N[(int64_t)(idx / C) * ldn + idx % C];
    __syncthreads();
    const int64_t tile = (int64_t)blockIdx.x * WPB + wave;
    if (tile * 16 >= p.n_rows) return;
    float *__restrict__ T = Ts[wave];
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
            row = p.row_order ? (int64_t)p.row_order[slot] : slot;      // (slot_row spelled out: through it 6 of the 12 instantiations move)
            beg = p.rowptr[row]; end = p.rowptr[row + 1];
        }
        live[ps] = row >= 0 && end - beg <= p.long_row;
        rows[ps] = row;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (live[ps]) {
            // (gathered_row's loop, copied by hand: with gathered_row<R, U, EDGE, ENTRIES, G> in its place -- tried again with the tile
            // frame -- all 12 instantiations of this kernel move, f32 and bf16 alike (register allocation and the order of the fmaf
            // chain's packed halves), and the kernel stays instruction for instruction the one measured so far)
            const typename R::Elem *__restrict__ Xc;
            if constexpr (R::BF16) Xc = p.Xb + c;
            else Xc = p.X + c;
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
                            if constexpr (R::BF16) bload<4>(x[u], Xc + (int64_t)j * p.ldx);
                            else vload<4>(x[u], Xc + (int64_t)j * p.ldx);
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
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[v] *= p.beta;
        }
        vstore<4>(T + rr * STRIDE + c, acc);
    }
    __builtin_amdgcn_wave_barrier();
    tile_times_Ms<NT>(T, Ms, lane, GNX_ACT_NONE);
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        if (!live[ps]) continue;
        const int rr = ps * RPP + lane / G;
        float o[4];
        vload<4>(o, T + rr * STRIDE + c);
        vstore<4>(p.out + rows[ps] * p.ldo + c, o);
    }
    if (S_out == nullptr) return;
    __builtin_amdgcn_wave_barrier();      // every lane has read its rows of the first product before the tile is filled again
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int rr = ps * RPP + lane / G;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (rows[ps] >= 0) {
            vload<4>(x, p.X + rows[ps] * p.ldx + c);
#pragma unroll
            for (int v = 0; v < 4; ++v) x[v] *= p.alpha;
        }
        vstore<4>(T + rr * STRIDE + c, x);
    }
    __builtin_amdgcn_wave_barrier();
    tile_times_Ms<NT>(T, Ms, lane, GNX_ACT_NONE);
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        if (rows[ps] < 0) continue;
        const int rr = ps * RPP + lane / G;
        const int64_t at = rows[ps] * (int64_t)C + c;
        float o[4];
        vload<4>(o, T + rr * STRIDE + c);
        if (S_in) {
            float s[4];
            vload<4>(s, S_in + at);
#pragma unroll
            for (int v = 0; v < 4; ++v) o[v] = fmaf(s_alpha, s[v], o[v]);
        }
        vstore<4>(S_out + at, o);
    }
}

// ---- the GCN layer's backward past the gate, one launch (gnx_gcn_step_back) ------------------------------------------------------------
//   dX[r, 0 .. C_in) = (sum_c At[r,c] G'[c, 0 .. C_out)) . Wt        Wt = W^T [C_out, C_in], 1 <= C_out <= C_in
// At (G' Wt) = (At G') Wt, as in k_spmm_gcnii_back -- and here the reassociation also narrows the gather: the rows of G' are gathered at
// the OUTPUT width, CG = 16 NTG >= C_out columns (NTG the smallest of 1, 2, 4), by 4 NTG lanes per row, and leave at the input width
// C_in = 16 NTI, by 4 NTI lanes per row.  The frame at C_in over the transposed structure (p), with two geometries of the one tile:
//   gather  Tile<NTG>'s lanes, rows per pass and passes (C_out <= 16: one pass fills the 16 rows) over Tile<NTI>'s row stride; the
//           gathered rows are the tile's first CG columns.  A row of G' is (p.X, p.ldx) with ldx % 4 == 0, ldx >= roundup4(C_out) and a
//           16-byte aligned base, so every gather is a whole 16-byte load; a lane whose columns start at or beyond roundup4(C_out)
//           loads nothing, and what a load brings of the columns C_out .. roundup4(C_out) - 1 is SELECTED away behind the loop, not
//           multiplied by 0: the padding of a row may hold anything, a NaN included.
//   store   Tile<NTI>'s.  The lane that stores a row is not the lane that gathered it, so the gather leaves each slot's row id -- -1
//           for a dead slot -- in the slot's first padding column of the tile (column C_in of the stride C_in + 4, which neither the
//           product nor the walk touches): no second tile and no LDS beyond the forward's.
// The block's matrix is Wt in LDS as [CG, C_in], its rows from C_out on zero-filled (the padding exists in LDS alone); the product is
// tile_times_Ms with the k loop over the gathered width (NTK = NTG) and all NTI result blocks in registers.  A row without entries gets
// dX = 0, written; a slot past n and a hub row write nothing (hub rows: the long-row kernels at width C_out, then the dense kernel on
// those rows alone).  EDGE / ENTRIES as in k_spmm_gcnii_back (edge_gather over the gather's lane groups).  f32 rows only.
template <typename R, int NTI, int NTG, int U, int WPB, bool EDGE = false, bool ENTRIES = false>
__global__ __launch_bounds__(64 * WPB) void k_spmm_gcn_back(const typename R::Args p, const float *__restrict__ Wt, int64_t ldwt, int C_out) {
    static_assert(!R::BF16, "the GCN layer exists over f32 rows");
    static_assert(NTG >= 1 && NTG <= NTI, "C_out <= C_in: the gathered rows are the tile's first columns");
    using TL = Tile<NTI>;
    using TG = Tile<NTG>;
    constexpr int C = TL::C, CG = TG::C, STRIDE = TL::STRIDE;
    __shared__ float Ws[CG * STRIDE];
    __shared__ float Ts[WPB][16 * STRIDE];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int idx = threadIdx.x; idx < CG * C; idx += 64 * WPB) {
        const int k = idx / C, n = idx % C;
        Ws[k * STRIDE + n] = k < C_out ? Wt[(int64_t)k * ldwt + n] : 0.f;
    }
    __syncthreads();
    const int64_t tile = (int64_t)blockIdx.x * WPB + wave;
    if (tile * 16 >= p.n_rows) return;
    float *__restrict__ T = Ts[wave];
    {
        constexpr int G = TG::G, RPP = TG::RPP, PASSES = TG::PASSES;
        const int sub = lane % G, c = sub * 4;
        const bool loads = c < ((C_out + 3) & ~3);
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
            const bool live = row >= 0 && end - beg <= p.long_row;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            if (live) {
                // (the lanes of a row run edge_gather together, those without columns included: they make weights for the others)
                if constexpr (EDGE) edge_gather<ENTRIES, G, U>(p, p.X + c, row, beg, end, acc, loads);
                else if (loads) gathered_row<R, U>(p, row, beg, end, c, acc);
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[v] = c + v < C_out ? acc[v] : 0.f;
            }
            vstore<4>(T + rr * STRIDE + c, acc);
            if (sub == 0) T[rr * STRIDE + C] = __int_as_float(live ? (int)row : -1);
        }
    }
    __builtin_amdgcn_wave_barrier();
    tile_times_Ms<NTI, false, NTI, NTG>(T, Ws, lane, GNX_ACT_NONE);
    constexpr int G = TL::G, RPP = TL::RPP, PASSES = TL::PASSES;
    const int c = (lane % G) * 4;
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int rr = ps * RPP + lane / G;
        const int row = __float_as_int(T[rr * STRIDE + C]);
        if (row < 0) continue;
        float o[4];
        vload<4>(o, T + rr * STRIDE + c);
        vstore<4>(p.out + (int64_t)row * p.ldo + c, o);
    }
}

// ---- the layer's weight gradient without stored mixed rows, one launch (gnx_gcnii_wgrad) -------------------------------------------
//   dM = T^T . G,   T = beta * A . X + alpha * H0 made again by mixed_row -- the forward's gather, entry order and mix, so T[r] has the
// bits the forward would have stored -- and never written.  The frame's tiles without a block matrix, and with a wave that walks several
// of them: it fills its tile, multiplies T_tile^T . G_tile into NT x NT accumulator blocks on v_mfma_f32_16x16x4_f32 (k =
// the tile's 16 row slots, four per instruction) and goes on to its next tile with the accumulators live.  Block (mt, nt) holds the
// columns NT m + mt of T against the columns NT n + nt of G: A[m][k] is then one 4 NT-byte LDS read of row k of the tile for all mt, and
// B[k][n] one 4 NT-byte global load of G's row for all nt (16 lanes read the row's 64 NT contiguous bytes; no second LDS tile: at C = 64
// the kernel keeps 34 KB of LDS and its registers set the occupancy: the 64 accumulators leave two blocks per CU, and only because the G
// rows of a tile are loaded AFTER its gather -- requested before it, they are live through the gather loop and cost the second block;
// profiles/NOTES.md has the compiler's report).  A slot past n holds zeros on both sides; a row without entries contributes alpha * H0[r]; a hub row's T
// comes from `hub`, where the long-row kernels put it before this launch.
// No float atomics, nothing depends on the device: wave w of block b takes the tiles b WPB + w + k gridDim.x WPB in ascending k (the
// tiles are in degree-binned order, so striding spreads every degree bin over all blocks), the block adds its waves' accumulators in
// wave order through LDS and writes one [C, C] partial, slab b of `work`; the host's grid is a function of (n, C, slabs) alone and the
// slabs are added in index order by sum_slabs (gnx_dense_wgrad.hip).
template <typename R, int NT, int U, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_gcnii_wgrad(const typename R::Args p, const float *__restrict__ Gm, const float *__restrict__ hub,
                                                          float *__restrict__ work) {
    using TL = Tile<NT>;
    constexpr int C = TL::C, G = TL::G, RPP = TL::RPP, PASSES = TL::PASSES, STRIDE = TL::STRIDE;
    static_assert(WPB * 16 * STRIDE >= C * C, "the block's partial reuses the tiles");
    __shared__ __attribute__((aligned(16))) float Ts[WPB * 16 * STRIDE];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int cc = lane & 15, g = lane >> 4, c = (lane % G) * 4;
    float *T = Ts + wave * 16 * STRIDE;
    f32x4 d[NT][NT];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) d[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t n_tiles = (p.n_rows + 15) / 16, step = (int64_t)gridDim.x * WPB;
    for (int64_t tile = (int64_t)blockIdx.x * WPB + wave; tile < n_tiles; tile += step) {
        // the tile as the forward fills it (4 NT lanes of float4 per row, RPP rows per pass), a hub row from `hub`
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
            const int rr = ps * RPP + lane / G;
            const int64_t slot = tile * 16 + rr;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            if (slot < p.n_rows) {
                const int64_t row = slot_row(p, slot);
                const int64_t beg = p.rowptr[row], end = p.rowptr[row + 1];
                if (end - beg <= p.long_row) mixed_row<R, U>(p, row, beg, end, c, acc);
                else vload<4>(acc, hub + row * (int64_t)C + c);
            }
            vstore<4>(T + rr * STRIDE + c, acc);
        }
        // B[k = 4 kk + g][n = cc] of block nt = G[row of slot k][NT cc + nt]
        float b[4][NT];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int64_t slot = tile * 16 + 4 * kk + g;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[kk][nt] = 0.f;
            if (slot < p.n_rows) {
                const int64_t row = slot_row(p, slot);
                vload<NT>(b[kk], Gm + row * (int64_t)C + NT * cc);
            }
        }
        __builtin_amdgcn_wave_barrier();
        // A[m = cc][k = 4 kk + g] of block mt = T[slot k][NT cc + mt]
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            float a[NT];
            vload<NT>(a, T + (4 * kk + g) * STRIDE + NT * cc);
#pragma unroll
            for (int mt = 0; mt < NT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) d[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[kk][nt], d[mt][nt], 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();      // every lane has read the tile before it is filled again
    }
    // D of block (mt, nt): lane (cc, g), register r -> dM[NT (4 g + r) + mt][NT cc + nt]; the waves in wave order into the block's partial
    __syncthreads();
    for (int w = 0; w < WPB; ++w) {
        if (wave == w) {
#pragma unroll
            for (int mt = 0; mt < NT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int at = (NT * (4 * g + r) + mt) * C + NT * cc + nt;
                        Ts[at] = w == 0 ? d[mt][nt][r] : Ts[at] + d[mt][nt][r];
                    }
        }
        __syncthreads();
    }
    float *__restrict__ slab = work + (int64_t)blockIdx.x * (C * C);
    for (int idx = threadIdx.x; idx < C * C; idx += 64 * WPB) slab[idx] = Ts[idx];
}

using Bf16Rows = Bf16RowsT<false>;

// f(IntC<NT>, grid) for the two fused kernels at width C = 16 NT in {16, 32, 64}: blocks of 512 threads, a 16-row tile per wave
template <typename F>
void with_tile_width(int64_t C, int64_t n_rows, F &&f) {
    const dim3 grid(blocks_for(blocks_for(n_rows, 16), 8));
    if (C == 64)      f(IntC<4>{}, grid);
    else if (C == 32) f(IntC<2>{}, grid);
    else              f(IntC<1>{}, grid);
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

// dst[r, :] = bf(src[r, :]) for the rows listed (null: rows 0 .. n), both [., C] contiguous; VEC = 4: 16-byte loads, 8-byte stores
template <int VEC>
__global__ __launch_bounds__(256) void k_round_rows(const float *__restrict__ src, const int32_t *__restrict__ rows, int64_t n, int64_t C,
                                                   uint16_t *__restrict__ dst) {
    const int64_t per_row = C / VEC, total = n * per_row, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / per_row, r = rows ? (int64_t)rows[i] : i, at = r * C + (e % per_row) * VEC;
        float x[VEC];
        vload<VEC>(x, src + at);
        bstore<VEC>(dst + at, x);
    }
}

void round_rows(const float *src, const int32_t *rows, int64_t n, int64_t C, uint16_t *dst, hipStream_t s) {
    if (n == 0) return;
    launch_row_pass(n, C, {{src, 16, C}, {dst, 8, C}}, [&](auto V, unsigned grid) { GNX_LAUNCH(k_round_rows<V()>, grid, src, rows, n, C, dst); });
}

// out[r, :] = drop(X[r, :]) for the rows listed (null: rows 0 .. n), r the row id the mask is keyed by; out may be X (each lane reads the
// values it overwrites).  VEC = 4: 16-byte accesses (C, both row strides and both bases allow them)
template <int VEC>
__global__ __launch_bounds__(256) void k_feature_dropout(const float *X, int64_t ldx, const int32_t *__restrict__ rows, int64_t n, int64_t C,
                                                        const DropFuse fd, float *out, int64_t ldo) {
    const int64_t per_row = C / VEC, total = n * per_row, stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t stream = drop_stream(fd);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / per_row, r = rows ? (int64_t)rows[i] : i, c = (e % per_row) * VEC;
        float x[VEC];
        vload<VEC>(x, X + r * ldx + c);
        drop_values<VEC>(fd, stream, r, c, x);
        vstore<VEC>(out + r * ldo + c, x);
    }
}

void launch_feature_dropout(const float *X, int64_t ldx, const int32_t *rows, int64_t n, int64_t C, const DropFuse &fd, float *out, int64_t ldo,
                            hipStream_t s) {
    if (n == 0 || C == 0) return;
    launch_row_pass(n, C, {{X, 16, ldx}, {out, 16, ldo}},
                    [&](auto V, unsigned grid) { GNX_LAUNCH(k_feature_dropout<V()>, grid, X, ldx, rows, n, C, fd, out, ldo); });
}

// The spectral form's row pass behind the dense kernel (hub rows; every row of the other widths): out[r, :] holds act(P') and leaves as
// 2 drop(act(P') - bias) in place, the row's gate words written beside it (gate may be null) -- spectral_finish, the store loop's own
// code.  A thread per gate word: up to 32 columns of row rows[i] (null: row i), any width and row stride.
template <bool DROP>
__global__ __launch_bounds__(256) void k_spectral_tail(float *out, int64_t ldo, const int32_t *__restrict__ rows, int64_t n, int64_t C,
                                                      const float *__restrict__ bias, const DropFuse fd, uint32_t *__restrict__ gate) {
    const int64_t words = (C + 31) / 32, total = n * words, stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t stream = 0;
    if constexpr (DROP) stream = drop_stream(fd);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / words, w = e % words, r = rows ? (int64_t)rows[i] : i;
        const int64_t c0 = 32 * w, c1 = c0 + 32 < C ? c0 + 32 : C;
        float *o = out + r * ldo;
        uint32_t word = 0;
        for (int64_t c = c0; c < c1; ++c) {
            float x[1] = {o[c]};
            const float b[1] = {bias[c]};
            word |= spectral_finish<1, DROP>(fd, stream, r, c, b, x) << (c - c0);
            o[c] = x[0];
        }
        if (gate != nullptr) gate[r * words + w] = word;
    }
}

void launch_spectral_tail(float *out, int64_t ldo, const int32_t *rows, int64_t n, int64_t C, const float *bias, const DropFuse *fd,
                          uint32_t *gate, hipStream_t s) {
    if (n == 0 || C == 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks_for(n * ((C + 31) / 32), 256), 1 << 20);
    if (fd) GNX_LAUNCH(k_spectral_tail<true>, grid, out, ldo, rows, n, C, bias, *fd, gate);
    else    GNX_LAUNCH(k_spectral_tail<false>, grid, out, ldo, rows, n, C, bias, DropFuse{}, gate);
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

// The first pass of the spectral form's backward (gnx_gcnii_spectral_back): u = 2 drop(g) with the forward's mask, G' = gate ? u : 0
// (RELU; the identity has no gate: G' = u) and the bias gradient dbias[c] = -sum_i (gate ? 0 : u[i, c]): act(P') - bias depends on
// the bias through the -bias alone where the relu is shut, and not at all where it is open.
// No float atomics, nothing depends on the device: block b takes the rows b rpb .. (b + 1) rpb - 1, rpb = ceil(n / gridDim.x); a
// thread holds VEC columns and walks its rows -- every RL-th of the block's, RL = 256 / (threads per row) -- in ascending order, the
// block adds its RL row lanes in lane order through LDS and writes slab b of `work` ([C] each); the host's grid is a function of
// (n, C) alone and the slabs are added in index order by sum_slabs.  blockIdx.y: panels of 256 VEC columns.  G may be g.
template <int VEC, bool RELU>
__global__ __launch_bounds__(256) void k_spectral_back(const float *g, int64_t ldg, const uint32_t *__restrict__ gate, int64_t n, int64_t C,
                                                      const DropFuse fd, float *G, int64_t ldG, float *__restrict__ work) {
    __shared__ float sm[256 * VEC];
    const int64_t per_row = C / VEC, first = (int64_t)blockIdx.y * 256, words = (C + 31) / 32;
    const int tpr = (int)(per_row - first < 256 ? per_row - first : 256), RL = 256 / tpr;
    const int cg = threadIdx.x % tpr, rl = threadIdx.x / tpr;
    const int64_t c = (first + cg) * VEC;
    const int64_t rpb = (n + gridDim.x - 1) / gridDim.x, row0 = (int64_t)blockIdx.x * rpb, row1 = row0 + rpb < n ? row0 + rpb : n;
    const uint64_t stream = drop_stream(fd);
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
    if (rl < RL) {
        for (int64_t r = row0 + rl; r < row1; r += RL) {
            float x[VEC];
            vload<VEC>(x, g + r * ldg + c);
            drop_values<VEC>(fd, stream, r, c, x);
#pragma unroll
            for (int v = 0; v < VEC; ++v) x[v] *= 2.f;
            if constexpr (RELU) {
                const uint32_t word = gate[r * words + (c >> 5)] >> (c & 31);      // (VEC columns from c: one word, c % VEC == 0)
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (!((word >> v) & 1u)) { acc[v] -= x[v]; x[v] = 0.f; }
            }
            vstore<VEC>(G + r * ldG + c, x);
        }
    }
    if constexpr (RELU) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) sm[threadIdx.x * VEC + v] = acc[v];
        __syncthreads();
        if (rl == 0) {
            for (int k = 1; k < RL; ++k)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] += sm[(k * tpr + cg) * VEC + v];
            vstore<VEC>(work + (int64_t)blockIdx.x * C + c, acc);
        }
    }
}

// The backward's gate in one pass: G = kept ? g * scale : +0, and with RELU also +0 where y <= 0 (y = the DROPPED forward output, so
// y > 0 implies kept: the hash is taken only where y lets the value through, the same bits either way).  G may be g.
template <int VEC, bool RELU>
__global__ __launch_bounds__(256) void k_feature_dropout_back(const float *g, int64_t ldg, const float *__restrict__ y, int64_t ldy, int64_t n,
                                                             int64_t C, const DropFuse fd, float *G, int64_t ldG) {
    const int64_t per_row = C / VEC, total = n * per_row, stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t stream = drop_stream(fd);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / per_row, c = (e % per_row) * VEC;
        float x[VEC];
        vload<VEC>(x, g + r * ldg + c);
        if constexpr (RELU) {
            float out[VEC];
            vload<VEC>(out, y + r * ldy + c);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (out[v] <= 0.f) x[v] = 0.f;
                else x[v] = (fd.thr == 0 || hash_u24(fd.seed, stream, (uint64_t)r, (uint64_t)(c + v), 0) >= fd.thr) ? x[v] * fd.scale : 0.f;
            }
        } else {
            drop_values<VEC>(fd, stream, r, c, x);
        }
        vstore<VEC>(G + r * ldG + c, x);
    }
}

// k_feature_dropout_back over the STORED bf16 forward output y (gnx_feature_dropout_back_bf16), the gated gradient written twice: G
// in f32 (what gnx_dense_wgrad and the row's own product of the backward read) and Gb = bf(G) (what the backward gathers).  The gate is
// on the stored value: a positive f32 output that rounded to bf16 zero was stored as zero and passes nothing.
template <int VEC, bool RELU>
__global__ __launch_bounds__(256) void k_feature_dropout_back_bf16(const float *g, int64_t ldg, const uint16_t *__restrict__ y, int64_t ldy,
                                                                  int64_t n, int64_t C, const DropFuse fd, float *G, int64_t ldG,
                                                                  uint16_t *__restrict__ Gb, int64_t ldGb) {
    const int64_t per_row = C / VEC, total = n * per_row, stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t stream = drop_stream(fd);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / per_row, c = (e % per_row) * VEC;
        float x[VEC];
        vload<VEC>(x, g + r * ldg + c);
        if constexpr (RELU) {
            float out[VEC];
            bload<VEC>(out, y + r * ldy + c);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (out[v] <= 0.f) x[v] = 0.f;
                else x[v] = (fd.thr == 0 || hash_u24(fd.seed, stream, (uint64_t)r, (uint64_t)(c + v), 0) >= fd.thr) ? x[v] * fd.scale : 0.f;
            }
        } else {
            drop_values<VEC>(fd, stream, r, c, x);
        }
        vstore<VEC>(G + r * ldG + c, x);
        bstore<VEC>(Gb + r * ldGb + c, x);
    }
}

// the mask of one call: keep iff hash >= int(p * 2^24) (oracle/gnntf_oracle.py:dropout_threshold, over the caller's double), kept values
// times the f32 scale of the edge dropout, 1.0f / (1.0f - (float)p); the handle lends its dropout counter
int make_feat_drop(const char *fn, const gnx_graph *g, double p, uint64_t seed, uint64_t stream_id, DropFuse &fd) {
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(p >= 0.0 && p < 1.0, "%s: dropout rate %g outside [0, 1)", fn, p);
    fd.seed = seed; fd.stream = stream_id; fd.offset = g->stream_offset;
    fd.thr = drop_threshold(p);
    fd.scale = drop_scale((float)p);
    return GNX_OK;
}

// gnx_feature_dropout_back (F32Rows: no Gb) and gnx_feature_dropout_back_bf16: one host path
template <typename R>
int feature_dropout_back(const char *fn, gnx_graph *g, const float *d_g, int64_t ldg, const typename R::Elem *d_y, int64_t ldy, int64_t n_rows,
                         int64_t C, double dropout_p, uint64_t seed, uint64_t stream_id, int act, float *d_G, int64_t ldG, uint16_t *d_Gb,
                         int64_t ldGb, void *stream) {
    constexpr bool BF = R::BF16 != 0;
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "%s: invalid activation %d", fn, act);
    GNX_CHECK_ARG(n_rows >= 0 && C >= 1, "%s: negative row count or C < 1", fn);
    GNX_CHECK_ARG(d_g != nullptr && d_G != nullptr && ldg >= C && ldG >= C && (!BF || (d_Gb != nullptr && ldGb >= C)),
                  "%s: NULL g / G%s or a row stride below C", fn, BF ? " / Gb" : "");
    GNX_CHECK_ARG(d_G != d_g || ldG == ldg, "%s: in place needs ldG == ldg", fn);
    GNX_CHECK_ARG(!BF || ((const void *)d_Gb != (const void *)d_g && (const void *)d_Gb != (const void *)d_G), "%s: Gb must not alias g / G", fn);
    const bool relu = act == GNX_ACT_RELU;
    const void *written = BF ? (const void *)d_Gb : (const void *)d_G;      // the result in y's format
    GNX_CHECK_ARG(!relu || (d_y != nullptr && ldy >= C && (const void *)d_y != written), "%s: relu needs y (not %s itself) with ldy >= C", fn,
                  BF ? "Gb" : "G");
    DropFuse fd{};
    int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    if (n_rows == 0) return GNX_OK;
    hipStream_t s = (hipStream_t)stream;
    const RowsAt y_rows = relu ? RowsAt{d_y, 4 * sizeof(typename R::Elem), ldy} : RowsAt{nullptr, 1, 0};      // y is read with relu only
    const RowsAt gb_rows = BF ? RowsAt{d_Gb, 8, ldGb} : RowsAt{nullptr, 1, 0};                                 // Gb exists for bf16 only
    auto gate = [&](auto V, auto RELU, unsigned grid) {
        if constexpr (BF) GNX_LAUNCH((k_feature_dropout_back_bf16<V(), RELU()>), grid, d_g, ldg, d_y, ldy, n_rows, C, fd, d_G, ldG, d_Gb, ldGb);
        else GNX_LAUNCH((k_feature_dropout_back<V(), RELU()>), grid, d_g, ldg, d_y, ldy, n_rows, C, fd, d_G, ldG);
    };
    launch_row_pass(n_rows, C, {{d_g, 16, ldg}, {d_G, 16, ldG}, gb_rows, y_rows}, [&](auto V, unsigned grid) {
        if (relu) gate(V, std::true_type{}, grid);
        else      gate(V, std::false_type{}, grid);
    });
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

// the structure and the long-row plan of a fused launch (its short rows need nothing else of bind_csr)
void bind_fused(const Csr &m, SpmmArgs &p) {
    p.rowptr = m.rowptr; p.colidx = m.colidx; p.n_rows = m.n_rows; p.n_nonempty = m.n_nonempty; p.row_order = m.row_order;
    p.long_rows = m.long_rows; p.long_chunk_ptr = m.long_chunk_ptr; p.chunk_long = m.chunk_long; p.chunk_order = m.chunk_order;
    p.n_long = m.n_long; p.n_chunks = m.n_chunks; p.long_row = m.long_row; p.long_chunk = m.long_chunk;
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

// the edge dropout of gnx_gcnii_step_dropped / gnx_gcnii_step_back_dropped: what gnx_spmm_dropped takes
struct EdgeDrop { const float *D; float p; uint64_t seed, stream; };

// what those two entries check before anything is built or launched, as gnx_spmm_dropped_back does
int admit_edge_drop(const char *fn, gnx_graph *g, const EdgeDrop &e) {
    GNX_CHECK_ARG(e.D != nullptr, "%s: NULL degree scales", fn);
    GNX_CHECK_ARG(e.p >= 0.f && e.p < 1.f, "%s: dropout rate %g outside [0, 1)", fn, (double)e.p);
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols && g->blk_col_gid == nullptr, "%s: needs a square stand-alone graph", fn);
    return refuse_duplicates(g, fn);
}

// ---- the launch plumbing the host paths share --------------------------------------------------------------------------------------------
// The values a fused launch walks with, into p: under `edge` they are made in the gather loop (p.fuse becomes the edge dropout's, over the
// handle's per-slot values of that side), else they are loaded -- the caller's d_vals, or the handle's raw values of that side.
void bind_values(const gnx_graph *g, const EdgeDrop *edge, bool transposed, const float *d_vals, SpmmArgs &p) {
    if (edge) {
        set_values(g, transposed, p);
        set_drop_fuse(g, edge->p, edge->seed, edge->stream, edge->D, transposed ? 1 : 0, 0, p);
    } else {
        p.vals = d_vals ? d_vals : transposed ? g->t_raw.get() : g->raw_vals.get();
    }
}

// The slab of the hub rows' chunked partial sums at width C, reserved before the first launch of a call: under capture a slab that would
// have to grow refuses the whole call.
int reserve_partial(gnx_graph *g, const Csr &m, int64_t C, hipStream_t s) {
    return m.n_long > 0 ? ensure_partial(g, (size_t)m.n_chunks * (size_t)C * sizeof(float), s) : GNX_OK;
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

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): runtime switches as template arguments.  Every combination of the flags is
// instantiated in f, which guards the ones that have no kernel with `if constexpr`.
template <typename F>
void with_flags(F &&f) { f(); }
template <typename F, typename... Flags>
void with_flags(F &&f, bool flag, Flags... rest) {
    if (flag) with_flags([&](auto... tail) { f(std::true_type{}, tail...); }, rest...);
    else      with_flags([&](auto... tail) { f(std::false_type{}, tail...); }, rest...);
}

// the fused launch takes C = 16, 32 or 64 (C = 128 fits the kernel -- 135 KB of LDS: one block of eight waves per CU -- and was measured:
// 19.2 ms against 11.8 ms for the two launches on the config-4 graph; eight waves per CU cannot keep the gathers fed)
bool fused_width(int64_t C) { return C == 16 || C == 32 || C == 64; }

// what the entries without a composed form answer to the other widths and alignments: the callers keep f32 there
int refuse_unfused(const char *fn, int64_t C) {
    if (!fused_width(C)) set_error("%s: width %lld is not supported (the fused launch takes C = 16, 32 or 64; keep f32 storage elsewhere)", fn, (long long)C);
    else set_error("%s: misaligned buffer (the f32 buffers must be 16-byte aligned, the bf16 buffers 8-byte aligned)", fn);
    return GNX_ERR_UNSUPPORTED;
}

// ---- the forward's host path, once over the row storage R of H --------------------------------------------------------------------------
struct ForwardForm {             // what differs between its entries
    const DropFuse *fd;          // the mask of the finished rows (gnx_gcnii_step_drop, gnx_gcnii_step_train_bf16 at a rate above 0) or null
    float *mixed;                // f32 [n, C] or null: where the mixed rows T are kept (training)
    float *work;                 // f32 [n, C] or null: the bf16 entries' rows on their way through memory
    int out_bf16;                // the result is stored as bf16 (the bf16 entries)
    bool composes;               // the other widths / alignments run as two launches; false: they are refused (refuse_unfused)
    const char *fused, *composed;   // what gnx_graph_last_kernel reports
    const float *bias = nullptr;    // [C]: the spectral form (gnx_gcnii_step_spectral, F32Rows only), out = 2 drop(act(T . M + bias) - bias)
    uint32_t *gate = nullptr;       // the spectral form's gate words [n, ceil(C / 32)], or null
    const EdgeDrop *edge = nullptr; // gnx_gcnii_step_dropped (F32Rows only): the weights are made in the gather loop; d_vals is null
};

template <typename R>
int gcnii_forward(const char *fn, gnx_graph *g, const float *d_vals, const typename R::Elem *d_H, const float *d_H0, float a, int64_t C,
                  const float *d_M, int64_t ldm, int act, typename R::Out *d_out, const ForwardForm &f, void *stream) {
    int rc = check_common(fn, g, d_H, C, C, d_H0, C, d_out, C);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "%s: invalid activation %d", fn, act);
    GNX_CHECK_ARG(f.out_bf16 == 0 || f.out_bf16 == 1, "%s: out_bf16 must be 0 or 1", fn);
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "%s: needs a square graph", fn);
    GNX_CHECK_ARG(d_H0 != nullptr && d_M != nullptr && ldm >= C, "%s: NULL H0 / M or ldm < C", fn);
    const void *out = d_out, *H = d_H;
    GNX_CHECK_ARG(out != d_H0 && out != d_M, "%s: out must not alias H0 / M", fn);
    GNX_CHECK_ARG(f.mixed == nullptr || (f.mixed != out && f.mixed != H && f.mixed != d_H0 && f.mixed != d_M && f.mixed != d_vals),
                  "%s: d_mixed must be a buffer of its own", fn);
    GNX_CHECK_ARG(f.work == nullptr || (f.work != out && f.work != H && f.work != d_H0 && f.work != d_M && f.work != d_vals && f.work != f.mixed),
                  "%s: d_work must be a buffer of its own", fn);
    auto own = [&](const void *b) { return b != out && b != H && b != d_H0 && b != d_M && b != d_vals && b != f.mixed && b != f.work; };
    GNX_CHECK_ARG(f.bias == nullptr || own(f.bias), "%s: d_bias must be a buffer of its own", fn);
    GNX_CHECK_ARG(f.gate == nullptr || (own(f.gate) && (const void *)f.gate != f.bias), "%s: d_gate must be a buffer of its own", fn);
    if (f.edge) {
        rc = admit_edge_drop(fn, g, *f.edge);
        if (rc != GNX_OK) return rc;
    }
    const bool fusable = fused_width(C) && aligned(d_H, 4 * sizeof(typename R::Elem)) && aligned(d_H0, 16) && aligned(d_out, f.out_bf16 ? 8 : 16) &&
                         aligned(f.mixed, 16) && aligned(f.work, 16) && aligned(f.bias, 16);
    if (!fusable && !f.composes) return refuse_unfused(fn, C);
    const Csr &m = g->a;
    // the rows that go through memory -- every row of the two launches, the hub rows of the fused one -- need a place to be
    if constexpr (R::BF16)
        GNX_CHECK_ARG(f.work != nullptr || (fusable && m.n_long == 0), "%s: needs d_work [n, C] f32 (%s)", fn,
                      !fusable ? "this width / alignment runs the SpMM and the transform as two launches"
                      : f.mixed ? "the graph has hub rows: they are transformed and masked in memory"
                                : "the graph has hub rows: their mixed rows go through memory");
    else
        GNX_CHECK_ARG(fusable || f.mixed != nullptr, "%s: width %lld needs d_mixed [n, C] (the mixed rows go through memory)", fn, (long long)C);
    hipStream_t s = (hipStream_t)stream;
    const float beta = (float)(1.0 - (double)a);
    typename R::Args p{};
    bind_values(g, f.edge, false, d_vals, p);
    if (!f.edge && f.fd) p.fuse = *f.fd;      // (under f.edge p.fuse is the edge dropout's; the mask travels beside it, EdgeArgs)
    set_operands<R>(p, d_H, C, d_H0, C, beta, a, act, d_out, f.out_bf16, C, C);
    // mixed rows at T (the n listed; null: rows 0 .. n) -> act(T . M) of those rows alone, into d_out, or into d_work where the result is
    // bf16 -> their mask, in place -> the rows rounded into d_out.  (T may be d_work itself: every wave of the dense kernels reads whole
    // rows of its own tile before it stores them, as long as the result is ONE column panel)
    auto transform_rows = [&](float *T, const int32_t *rows, int64_t n) -> int {
        float *to = f.out_bf16 ? f.work : static_cast<float *>(d_out);
        const int err = dense_rows(T, C, n, C, d_M, ldm, C, f.bias, act, rows, rows, to, C, s);
        if (err != GNX_OK) return err;
        if (f.bias) launch_spectral_tail(to, C, rows, n, C, f.bias, f.fd, f.gate, s);      // (- bias, the mask, x 2 and the gate words)
        else if (f.fd) launch_feature_dropout(to, C, rows, n, C, *f.fd, to, C, s);
        if (f.out_bf16) round_rows(to, rows, n, C, (uint16_t *)d_out, s);
        GNX_HIP(hipGetLastError());
        return GNX_OK;
    };
    if (!fusable) {   // other widths: the fused SpMM + mix into f32 rows (d_mixed, else d_work), then the transform on the matrix cores
        float *T = f.mixed ? f.mixed : f.work;
        if constexpr (R::BF16) {
            p.act = GNX_ACT_NONE;
            rc = launch_spmm_bf16_f32_order(g, m, p, d_H, T, s);
        } else if (f.edge) {
            rc = gnx_spmm_dropped(g, f.edge->D, f.edge->p, f.edge->seed, f.edge->stream, 0, d_H, C, C, d_H0, C, beta, a, GNX_ACT_NONE, T, C, stream);
        } else {
            rc = gnx_spmm(g, d_vals, nullptr, d_H, C, C, d_H0, C, beta, a, GNX_ACT_NONE, T, C, stream);
        }
        if (rc != GNX_OK) return rc;
        g->last_kernel = f.composed;
        if (f.out_bf16 && C > 256) {
            set_error("%s: a bf16 result needs C <= 256 (wider: out_bf16 = 0, then gnx_cast_bf16)", fn);
            return GNX_ERR_UNSUPPORTED;
        }
        return transform_rows(T, nullptr, m.n_rows);
    }
    if (m.n_rows == 0) return GNX_OK;
    bind_fused(m, p);
    rc = reserve_partial(g, m, C, s);
    if (rc != GNX_OK) return rc;
    // the edge-dropout form and the spectral form exist over f32 rows; ENTRIES goes with EDGE
    const bool edged = !R::BF16 && f.edge, spectral = !R::BF16 && f.bias && !f.edge;
    with_tile_width(C, m.n_rows, [&](auto NT, dim3 grid) {
        with_flags([&](auto DROP, auto SPEC, auto EDGE, auto ENTRIES) {
            if constexpr (!(R::BF16 && (SPEC() || EDGE())) && !(SPEC() && EDGE()) && (EDGE() || !ENTRIES())) {
                SpectralArgs<SPEC()> sp{};
                if constexpr (SPEC()) sp = {f.bias, f.gate};
                EdgeArgs<EDGE()> ed{};
                if constexpr (EDGE()) ed.feat = f.fd ? *f.fd : DropFuse{};
                hipLaunchKernelGGL((k_spmm_gcnii<R, NT(), 4, 8, DROP(), SPEC(), EDGE(), ENTRIES()>), grid, dim3(512), 0, s, p, d_M, ldm, f.mixed, sp, ed);
            }
        }, f.fd != nullptr, spectral, edged, edged && p.fuse.mult);
    });
    g->last_kernel = f.fused;
    // hub rows: chunked partial sums -> mixed rows (into d_mixed when kept, else d_work, else in place) -> the transform of those rows alone
    float *T = f.mixed ? f.mixed : f.work ? f.work : static_cast<float *>(d_out);
    p.act = GNX_ACT_NONE;
    return hub_rows_tail<R>(g, m, p, d_H, T, f.edge != nullptr, s, [&](const int32_t *rows, int64_t n) { return transform_rows(T, rows, n); });
}

// ---- the backward's host path, once over the row storage R of the gathered gradient X (the f32 G itself, or its bf16 copy Gb) ------------
template <typename R>
int gcnii_backward(const char *fn, gnx_graph *g, const float *d_vals_t, const typename R::Elem *d_X, const float *d_G, float a, int64_t C,
                   const float *d_Mt, int64_t ldmt, float *d_dH, const float *d_S_in, float s_alpha, float *d_S_out, float *d_work, void *stream,
                   const EdgeDrop *edge = nullptr) {
    int rc = check_common(fn, g, d_X, C, C, d_S_in, C, d_dH, C);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "%s: needs a square graph", fn);
    if (edge) {      // (gnx_gcnii_step_back_dropped, f32 rows: the weights of the transposed walk are made from the edge dropout; d_vals_t is null)
        rc = admit_edge_drop(fn, g, *edge);
        if (rc != GNX_OK) return rc;
    }
    GNX_CHECK_ARG(d_Mt != nullptr && ldmt >= C, "%s: NULL Mt or ldmt < C", fn);
    GNX_CHECK_ARG(d_S_in == nullptr || d_S_out != nullptr, "%s: S_in without S_out", fn);
    if constexpr (R::BF16)
        GNX_CHECK_ARG((d_G == nullptr) == (d_S_out == nullptr), "%s: d_G (the f32 gated gradient of the row's own product) goes with d_S_out: both or neither", fn);
    const void *X = d_X;
    GNX_CHECK_ARG(d_dH != d_S_in && d_dH != d_S_out && d_dH != d_Mt && d_dH != d_G, "%s: dH must not alias %sS_in / S_out / Mt", fn, R::BF16 ? "G / " : "");
    GNX_CHECK_ARG(d_S_out == nullptr || (d_S_out != d_G && d_S_out != d_Mt && d_S_out != X), "%s: S_out must not alias G / %sMt", fn, R::BF16 ? "Gb / " : "");
    GNX_CHECK_ARG(d_work == nullptr || (d_work != d_G && d_work != X && d_work != d_dH && d_work != d_S_in && d_work != d_S_out && d_work != d_Mt),
                  "%s: d_work must be a buffer of its own", fn);
    hipStream_t s = (hipStream_t)stream;
    const float beta = (float)(1.0 - (double)a);
    const bool fusable = fused_width(C) && aligned(d_X, 4 * sizeof(typename R::Elem)) && aligned(d_G, 16) && aligned(d_dH, 16) && aligned(d_S_in, 16) &&
                         aligned(d_S_out, 16);
    if constexpr (R::BF16) {
        if (!fusable) return refuse_unfused(fn, C);
    } else if (!fusable) {   // other widths / alignments, the composed order: gT = G . Mt into d_work, dH = (1-a) At gT, S = s_alpha S_in + a gT
        const int64_t n = g->a.n_rows;
        GNX_CHECK_ARG(d_work != nullptr, "%s: width %lld / this alignment needs d_work [n, C] (G . Mt goes through memory)", fn, (long long)C);
        GNX_CHECK_ARG(d_S_out == nullptr || (aligned(d_work, 16) && aligned(d_S_in, 16) && aligned(d_S_out, 16)),
                      "%s: S_in, S_out and d_work must be 16-byte aligned (gnx_linear_combination adds them)", fn);
        rc = ensure_transpose(g, s);   // (before the first launch: under capture a part that would have to be built refuses the whole call)
        if (rc != GNX_OK) return rc;
        if (g->t.n_long > 0) {
            rc = ensure_partial(g, (size_t)g->t.n_chunks * (size_t)C * sizeof(float), s);
            if (rc != GNX_OK) return rc;
        }
        rc = gnx_dense(d_G, C, n, C, d_Mt, ldmt, C, nullptr, GNX_ACT_NONE, d_work, C, stream);
        if (rc != GNX_OK) return rc;
        if (edge) rc = gnx_spmm_dropped(g, edge->D, edge->p, edge->seed, edge->stream, 1, d_work, C, C, nullptr, 0, beta, 0.f, GNX_ACT_NONE, d_dH, C, stream);
        else rc = gnx_spmm_tv(g, d_vals_t ? d_vals_t : g->t_raw.get(), nullptr, d_work, C, C, nullptr, 0, beta, 0.f, GNX_ACT_NONE, d_dH, C, stream);
        if (rc != GNX_OK) return rc;
        g->last_kernel = edge ? "dense+spmm_back_edrop" : "dense+spmm_back";
        if (d_S_out == nullptr || n == 0) return GNX_OK;
        const float *src[2] = {d_S_in, d_work};
        const float coef[2] = {s_alpha, a};
        return d_S_in ? gnx_linear_combination(2, src, coef, n * C, d_S_out, stream)
                      : gnx_linear_combination(1, src + 1, coef + 1, n * C, d_S_out, stream);
    }
    rc = ensure_transpose(g, s);   // (the two before the first launch, as above)
    if (rc != GNX_OK) return rc;
    const Csr &m = g->t;
    if (m.n_rows == 0) return GNX_OK;
    rc = reserve_partial(g, m, C, s);
    if (rc != GNX_OK) return rc;
    typename R::Args p{};
    bind_values(g, edge, true, d_vals_t, p);
    set_operands<R>(p, d_X, C, nullptr, 0, beta, a, GNX_ACT_NONE, d_dH, 0, C, C);
    p.X = d_G; p.out = d_dH;      // the row's own f32 row and the f32 dH are SpmmArgs' own under either policy (k_spmm_gcnii_back)
    bind_fused(m, p);
    const bool edged = !R::BF16 && edge;      // (the edge-dropout form exists over f32 rows; ENTRIES goes with EDGE)
    with_tile_width(C, m.n_rows, [&](auto NT, dim3 grid) {
        with_flags([&](auto EDGE, auto ENTRIES) {
            if constexpr (!(R::BF16 && EDGE()) && (EDGE() || !ENTRIES()))
                hipLaunchKernelGGL((k_spmm_gcnii_back<R, NT(), 4, 8, EDGE(), ENTRIES()>), grid, dim3(512), 0, s, p, d_Mt, ldmt, d_S_in, s_alpha, d_S_out);
        }, edged, edged && p.fuse.mult);
    });
    g->last_kernel = R::BF16 ? "spmm_gcnii_back_mfma_bf16" : edge ? "spmm_gcnii_back_mfma_edrop" : "spmm_gcnii_back_mfma";
    // hub rows of the transposed structure: chunked partial sums -> (1-a) Z into dH -> those rows alone times Mt, in place
    return hub_rows_tail<R>(g, m, p, d_X, d_dH, edge != nullptr, s, [&](const int32_t *rows, int64_t n) {
        return dense_rows(d_dH, C, n, C, d_Mt, ldmt, C, nullptr, GNX_ACT_NONE, rows, rows, d_dH, C, s);
    });
}

// ---- the weight gradient's host path, once over the row storage R of H (gnx_gcnii_wgrad, gnx_gcnii_wgrad_bf16) -------------------------
// No composed form: the other widths / alignments are refused (refuse_unfused) and the callers keep the stored rows there.
template <typename R>
int gcnii_wgrad(const char *fn, const char *reports, gnx_graph *g, const float *d_vals, const typename R::Elem *d_H, const float *d_H0, float a,
                int64_t C, const float *d_G, float *d_dM, float *d_hub_rows, float *d_work, int64_t work_floats, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(C >= 1 && C <= (1 << 20), "%s: feature width %lld not in [1, 2^20]", fn, (long long)C);
    GNX_CHECK_ARG(d_H != nullptr && d_H0 != nullptr && d_G != nullptr && d_dM != nullptr, "%s: NULL H / H0 / G / dM", fn);
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "%s: needs a square graph", fn);
    const void *H = d_H;
    auto own = [&](const void *b) { return b != H && b != d_H0 && b != d_G && b != d_vals; };
    GNX_CHECK_ARG(own(d_dM), "%s: dM must not alias H / H0 / G / the values", fn);
    GNX_CHECK_ARG(d_work != nullptr && own(d_work) && d_work != d_dM, "%s: d_work must be a buffer of its own", fn);
    GNX_CHECK_ARG(d_hub_rows == nullptr || (own(d_hub_rows) && d_hub_rows != d_dM && d_hub_rows != d_work), "%s: d_hub_rows must be a buffer of its own", fn);
    GNX_CHECK_ARG(work_floats >= C * C, "%s: work_floats %lld below C * C (every slab of d_work holds a [C, C] partial)", fn, (long long)work_floats);
    if (!(fused_width(C) && aligned(d_H, 4 * sizeof(typename R::Elem)) && aligned(d_H0, 16) && aligned(d_G, 16) && aligned(d_dM, 16) &&
          aligned(d_hub_rows, 16) && aligned(d_work, 16)))
        return refuse_unfused(fn, C);
    const Csr &m = g->a;
    GNX_CHECK_ARG(d_hub_rows != nullptr || m.n_long == 0, "%s: needs d_hub_rows [n, C] f32 (the graph has hub rows: their mixed rows go through memory)", fn);
    hipStream_t s = (hipStream_t)stream;
    if (m.n_rows == 0) {
        GNX_HIP(hipMemsetAsync(d_dM, 0, (size_t)(C * C) * sizeof(float), s));
        return GNX_OK;
    }
    int rc = reserve_partial(g, m, C, s);
    if (rc != GNX_OK) return rc;
    typename R::Args p{};
    bind_values(g, nullptr, false, d_vals, p);
    set_operands<R>(p, d_H, C, d_H0, C, (float)(1.0 - (double)a), a, GNX_ACT_NONE, static_cast<typename R::Out *>(d_hub_rows), 0, C, C);
    bind_fused(m, p);
    // hub rows: chunked partial sums -> mixed rows at their row ids of d_hub_rows, where the launch below finds them
    rc = hub_rows_tail<R>(g, m, p, d_H, d_hub_rows, false, s, [](const int32_t *, int64_t) { return GNX_OK; });
    if (rc != GNX_OK) return rc;
    // as many slabs as the scratch holds, at most 2048 (gnx_dense_wgrad's cap) and at most one per block of eight tiles: a function of
    // (n, C, work_floats) alone, like the tile -> wave -> block assignment that follows from it
    const int64_t slabs = std::min<int64_t>(std::min<int64_t>(work_floats / (C * C), 2048), blocks_for(blocks_for(m.n_rows, 16), 8));
    with_tile_width(C, m.n_rows, [&](auto NT, dim3) {
        hipLaunchKernelGGL((k_gcnii_wgrad<R, NT(), 4, 8>), dim3((unsigned)slabs), dim3(512), 0, s, p, d_G, m.n_long > 0 ? d_hub_rows : nullptr, d_work);
    });
    sum_slabs(d_work, slabs, C * C, d_dM, s);
    g->last_kernel = reports;
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

// ---- the GCN layer's host path (gnx_gcn_step, gnx_gcn_step_dropped) -----------------------------------------------------------------------
// what gnx_graph_last_kernel reports: [C_in = 16, 32, 64][mask << 1 | edge dropout][hub rows ran]; the composed form [..][..] alone
#define GNX_GCN_NAMES2(c, tail) {"k_spmm_gcn<" c ">" tail, "k_spmm_gcn<" c ">" tail "+long"}
#define GNX_GCN_NAMES(c) {GNX_GCN_NAMES2(c, ""), GNX_GCN_NAMES2(c, "_edrop"), GNX_GCN_NAMES2(c, "_drop"), GNX_GCN_NAMES2(c, "_edrop_drop")}
const char *const kGcnFused[3][4][2] = {GNX_GCN_NAMES("16"), GNX_GCN_NAMES("32"), GNX_GCN_NAMES("64")};
const char *const kGcnComposed[4] = {"spmm+dense_mfma_gcn", "spmm+dense_mfma_gcn_edrop", "spmm+dense_mfma_gcn_drop", "spmm+dense_mfma_gcn_edrop_drop"};
#undef GNX_GCN_NAMES
#undef GNX_GCN_NAMES2

struct GcnOut { float *out; int64_t ldo; float *agg, *work; };      // the result, and where aggregated rows are kept / may pass through memory

// out = drop(act((A . X) . W + bias)), A from d_vals or made from `edge`; `fd` the mask of the finished rows or null.  The fused launch
// takes C_in = 16, 32 or 64 with C_out <= C_in over 16-byte aligned rows; everything else runs the SpMM, the dense kernel and the mask
// pass inside this call, as gcnii_forward treats its other widths.  Nothing is launched before the last check has passed.
int gcn_forward(const char *fn, gnx_graph *g, const float *d_vals, const EdgeDrop *edge, const float *d_X, int64_t ldx, int64_t C_in,
                const float *d_W, int64_t ldw, int64_t C_out, const float *d_bias, int act, const DropFuse *fd, const GcnOut &o, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "%s: invalid activation %d", fn, act);
    GNX_CHECK_ARG(C_in >= 1 && C_in <= (1 << 20) && C_out >= 1 && C_out <= (1 << 20), "%s: widths %lld -> %lld not in [1, 2^20]", fn,
                  (long long)C_in, (long long)C_out);
    GNX_CHECK_ARG(d_X != nullptr && d_W != nullptr && o.out != nullptr, "%s: NULL X / W / out", fn);
    GNX_CHECK_ARG(ldx >= C_in, "%s: ldx %lld < C_in %lld", fn, (long long)ldx, (long long)C_in);
    GNX_CHECK_ARG(ldw >= C_out, "%s: ldw %lld < C_out %lld", fn, (long long)ldw, (long long)C_out);
    GNX_CHECK_ARG(o.ldo >= C_out, "%s: ldo %lld < C_out %lld", fn, (long long)o.ldo, (long long)C_out);
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "%s: needs a square graph", fn);
    const void *D = edge ? edge->D : nullptr;
    auto input = [&](const void *b) { return b == d_X || b == d_W || (d_bias && b == d_bias) || (d_vals && b == d_vals) || (D && b == D); };
    GNX_CHECK_ARG(!input(o.out), "%s: out must not alias an input (X / W / bias / the values)", fn);
    GNX_CHECK_ARG(o.agg == nullptr || (!input(o.agg) && o.agg != o.out), "%s: d_agg must be a buffer of its own", fn);
    GNX_CHECK_ARG(o.work == nullptr || (!input(o.work) && o.work != o.out && o.work != o.agg), "%s: d_work must be a buffer of its own", fn);
    if (edge) {
        const int rc = admit_edge_drop(fn, g, *edge);
        if (rc != GNX_OK) return rc;
    }
    const Csr &m = g->a;
    const bool fusable = fused_width(C_in) && C_out <= C_in && ldx % 4 == 0 && aligned(d_X, 16) && aligned(o.agg, 16) && aligned(o.work, 16);
    float *T = o.agg ? o.agg : o.work;      // where rows [n, C_in] go through memory: every row of the composed form, the hub rows of the fused one
    GNX_CHECK_ARG(fusable || T != nullptr, "%s: needs d_agg or d_work [n, C_in] f32 (%s: the SpMM and the transform run as two launches)", fn,
                  !fused_width(C_in) ? "C_in is not 16, 32 or 64" : C_out > C_in ? "C_out > C_in" : "misaligned rows");
    GNX_CHECK_ARG(!fusable || m.n_long == 0 || T != nullptr,
                  "%s: needs d_agg or d_work [n, C_in] f32 (the graph has hub rows: their aggregated rows go through memory)", fn);
    hipStream_t s = (hipStream_t)stream;
    const int mode = (fd ? 2 : 0) | (edge ? 1 : 0);
    // aggregated rows at T (the n listed; null: rows 0 .. n) -> act(T . W + bias) of those rows alone -> their mask, in place
    auto transform_rows = [&](const int32_t *rows, int64_t n) -> int {
        const int err = dense_rows(T, C_in, n, C_in, d_W, ldw, C_out, d_bias, act, rows, rows, o.out, o.ldo, s);
        if (err != GNX_OK) return err;
        if (fd) launch_feature_dropout(o.out, o.ldo, rows, n, C_out, *fd, o.out, o.ldo, s);
        GNX_HIP(hipGetLastError());
        return GNX_OK;
    };
    if (!fusable) {
        const int rc = edge ? gnx_spmm_dropped(g, edge->D, edge->p, edge->seed, edge->stream, 0, d_X, ldx, C_in, nullptr, 0, 1.f, 0.f, GNX_ACT_NONE, T,
                                               C_in, stream)
                            : gnx_spmm(g, d_vals, nullptr, d_X, ldx, C_in, nullptr, 0, 1.f, 0.f, GNX_ACT_NONE, T, C_in, stream);
        if (rc != GNX_OK) return rc;
        g->last_kernel = kGcnComposed[mode];
        return transform_rows(nullptr, m.n_rows);
    }
    if (m.n_rows == 0) return GNX_OK;
    int rc = reserve_partial(g, m, C_in, s);
    if (rc != GNX_OK) return rc;
    SpmmArgs p{};
    bind_values(g, edge, false, d_vals, p);      // (under `edge` p.fuse is the edge dropout's; the mask travels beside it, `feat`)
    set_operands<F32Rows>(p, d_X, ldx, nullptr, 0, 1.f, 0.f, act, o.out, 0, o.ldo, C_in);
    bind_fused(m, p);
    const bool vec_out = o.ldo % 4 == 0 && aligned(o.out, 16);
    const DropFuse feat = fd ? *fd : DropFuse{};
    const int nto = (int)blocks_for(C_out, 16);
    with_tile_width(C_in, m.n_rows, [&](auto NTI, dim3 grid) {
        auto with_mode = [&](auto NTO) {      // (C_out <= C_in: no NTO above NTI; ENTRIES goes with EDGE)
            with_flags([&](auto DROP, auto EDGE, auto ENTRIES) {
                if constexpr (NTO() <= NTI() && (EDGE() || !ENTRIES()))
                    hipLaunchKernelGGL((k_spmm_gcn<F32Rows, NTI(), NTO(), 4, 8, DROP(), EDGE(), ENTRIES()>), grid, dim3(512), 0, s, p, d_W, ldw,
                                       (int)C_out, d_bias, o.agg, vec_out, feat);
            }, fd != nullptr, edge != nullptr, edge && p.fuse.mult);
        };
        if (nto == 1)      with_mode(IntC<1>{});
        else if (nto == 2) with_mode(IntC<2>{});
        else if (nto == 3) with_mode(IntC<3>{});
        else               with_mode(IntC<4>{});
    });
    g->last_kernel = kGcnFused[C_in == 16 ? 0 : C_in == 32 ? 1 : 2][mode][m.n_long > 0];
    // hub rows: chunked partial sums -> aggregated rows at their row ids of T -> the transform and the mask of those rows alone
    p.act = GNX_ACT_NONE;
    p.ldo = C_in;
    return hub_rows_tail<F32Rows>(g, m, p, d_X, T, edge != nullptr, s, transform_rows);
}

// ---- the GCN layer's backward host path (gnx_gcn_step_back, gnx_gcn_step_back_dropped) ----------------------------------------------------
// what gnx_graph_last_kernel reports: [C_in = 16, 32, 64][edge dropout][hub rows ran]; the composed form [edge dropout]
#define GNX_GCN_BACK_NAMES(c) {{"k_spmm_gcn_back<" c ">", "k_spmm_gcn_back<" c ">+long"}, {"k_spmm_gcn_back<" c ">_edrop", "k_spmm_gcn_back<" c ">_edrop+long"}}
const char *const kGcnBackFused[3][2][2] = {GNX_GCN_BACK_NAMES("16"), GNX_GCN_BACK_NAMES("32"), GNX_GCN_BACK_NAMES("64")};
const char *const kGcnBackComposed[2] = {"dense+spmm_back_gcn", "dense+spmm_back_gcn_edrop"};
#undef GNX_GCN_BACK_NAMES

// dX = (At . G') . Wt, At from d_vals_t or made from `edge`.  The fused launch takes C_in = 16, 32 or 64 with C_out <= C_in over rows of
// G' padded to whole 16-byte pieces (ldg % 4 == 0, ldg >= roundup4(C_out), aligned base) and 16-byte aligned rows of dX; everything
// else runs today's order inside this call: gnx_dense(G', Wt) into d_work, then the transposed SpMM.  The checks that need no look at
// the handle come first; nothing is launched before the last check has passed.
int gcn_backward(const char *fn, gnx_graph *g, const float *d_vals_t, const EdgeDrop *edge, const float *d_G, int64_t ldg, int64_t C_out,
                 const float *d_Wt, int64_t ldwt, int64_t C_in, float *d_dX, int64_t lddx, float *d_work, int64_t work_floats, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(C_in >= 1 && C_in <= (1 << 20) && C_out >= 1 && C_out <= (1 << 20), "%s: widths %lld <- %lld not in [1, 2^20]", fn,
                  (long long)C_in, (long long)C_out);
    GNX_CHECK_ARG(d_G != nullptr && d_Wt != nullptr && d_dX != nullptr, "%s: NULL G / Wt / dX", fn);
    GNX_CHECK_ARG(ldg >= C_out, "%s: ldg %lld < C_out %lld", fn, (long long)ldg, (long long)C_out);
    GNX_CHECK_ARG(ldwt >= C_in, "%s: ldwt %lld < C_in %lld", fn, (long long)ldwt, (long long)C_in);
    GNX_CHECK_ARG(lddx >= C_in, "%s: lddx %lld < C_in %lld", fn, (long long)lddx, (long long)C_in);
    GNX_CHECK_ARG(work_floats >= 0 && (d_work != nullptr || work_floats == 0), "%s: work_floats %lld without d_work, or negative", fn,
                  (long long)work_floats);
    const void *D = edge ? edge->D : nullptr;
    auto input = [&](const void *b) { return b == d_G || b == d_Wt || (d_vals_t && b == d_vals_t) || (D && b == D); };
    GNX_CHECK_ARG(!input(d_dX), "%s: dX must not alias an input (G / Wt / the values)", fn);
    GNX_CHECK_ARG(d_work == nullptr || (!input(d_work) && d_work != d_dX), "%s: d_work must be a buffer of its own", fn);
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "%s: needs a square graph", fn);
    if (edge) {
        const int rc = admit_edge_drop(fn, g, *edge);
        if (rc != GNX_OK) return rc;
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = g->a.n_rows, c4 = (C_out + 3) / 4 * 4;
    const bool fusable = fused_width(C_in) && C_out <= C_in && ldg % 4 == 0 && ldg >= c4 && aligned(d_G, 16) && lddx % 4 == 0 &&
                         aligned(d_dX, 16) && aligned(d_work, 16);
    if (!fusable) {      // the composed order: gT = G' . Wt into d_work, dX = At gT
        GNX_CHECK_ARG(work_floats >= n * C_in, "%s: needs d_work of n * C_in = %lld floats, has %lld (%s: G' . Wt goes through memory, gnx_dense and the transposed SpMM run as two launches)",
                      fn, (long long)(n * C_in), (long long)work_floats,
                      !fused_width(C_in) ? "C_in is not 16, 32 or 64" : C_out > C_in ? "C_out > C_in"
                      : (ldg % 4 != 0 || ldg < c4) ? "the rows of G' are not padded to whole 16-byte pieces: ldg % 4 != 0 or ldg < roundup4(C_out)"
                                                   : "misaligned rows");
        int rc = ensure_transpose(g, s);   // (before the first launch: under capture a part that would have to be built refuses the whole call)
        if (rc != GNX_OK) return rc;
        rc = reserve_partial(g, g->t, C_in, s);
        if (rc != GNX_OK) return rc;
        rc = gnx_dense(d_G, ldg, n, C_out, d_Wt, ldwt, C_in, nullptr, GNX_ACT_NONE, d_work, C_in, stream);
        if (rc != GNX_OK) return rc;
        if (edge) rc = gnx_spmm_dropped(g, edge->D, edge->p, edge->seed, edge->stream, 1, d_work, C_in, C_in, nullptr, 0, 1.f, 0.f, GNX_ACT_NONE, d_dX, lddx, stream);
        else rc = gnx_spmm_tv(g, d_vals_t ? d_vals_t : g->t_raw.get(), nullptr, d_work, C_in, C_in, nullptr, 0, 1.f, 0.f, GNX_ACT_NONE, d_dX, lddx, stream);
        if (rc != GNX_OK) return rc;
        g->last_kernel = kGcnBackComposed[edge ? 1 : 0];
        return GNX_OK;
    }
    int rc = ensure_transpose(g, s);   // (the structure says whether hub rows need d_work; it and the slab before the first launch)
    if (rc != GNX_OK) return rc;
    const Csr &m = g->t;
    GNX_CHECK_ARG(m.n_long == 0 || work_floats >= n * C_out,
                  "%s: needs d_work of n * C_out = %lld floats, has %lld (the transposed structure has hub rows: their rows of At . G' go through memory)",
                  fn, (long long)(n * C_out), (long long)work_floats);
    if (m.n_rows == 0) return GNX_OK;
    rc = reserve_partial(g, m, C_out, s);
    if (rc != GNX_OK) return rc;
    SpmmArgs p{};
    bind_values(g, edge, true, d_vals_t, p);
    set_operands<F32Rows>(p, d_G, ldg, nullptr, 0, 1.f, 0.f, GNX_ACT_NONE, d_dX, 0, lddx, C_out);
    bind_fused(m, p);
    const int ntg = C_out <= 16 ? 1 : C_out <= 32 ? 2 : 4;
    with_tile_width(C_in, m.n_rows, [&](auto NTI, dim3 grid) {
        auto with_gather = [&](auto NTG) {      // (C_out <= C_in: no NTG above NTI; ENTRIES goes with EDGE)
            with_flags([&](auto EDGE, auto ENTRIES) {
                if constexpr (NTG() <= NTI() && (EDGE() || !ENTRIES()))
                    hipLaunchKernelGGL((k_spmm_gcn_back<F32Rows, NTI(), NTG(), 4, 8, EDGE(), ENTRIES()>), grid, dim3(512), 0, s, p, d_Wt, ldwt, (int)C_out);
            }, edge != nullptr, edge && p.fuse.mult);
        };
        if (ntg == 1)      with_gather(IntC<1>{});
        else if (ntg == 2) with_gather(IntC<2>{});
        else               with_gather(IntC<4>{});
    });
    g->last_kernel = kGcnBackFused[C_in == 16 ? 0 : C_in == 32 ? 1 : 2][edge ? 1 : 0][m.n_long > 0];
    // hub rows of the transposed structure: chunked partial sums -> At . G' at their row ids of d_work, width C_out -> those rows alone times Wt
    p.ldo = C_out;
    return hub_rows_tail<F32Rows>(g, m, p, d_G, d_work, edge != nullptr, s, [&](const int32_t *rows, int64_t k) {
        return dense_rows(d_work, C_out, k, C_out, d_Wt, ldwt, C_in, nullptr, GNX_ACT_NONE, rows, rows, d_dX, lddx, s);
    });
}

// ---- the NGCF layer's host path (gnx_ngcf_step) -------------------------------------------------------------------------------------------
// what gnx_graph_last_kernel reports: [C_in = 16, 32, 64][mask][norm][hub rows ran]; the composed form [mask][norm]
#define GNX_NGCF_NAMES2(c, tail) {"k_spmm_ngcf<" c ">" tail, "k_spmm_ngcf<" c ">" tail "+long"}
#define GNX_NGCF_NAMES(c) {{GNX_NGCF_NAMES2(c, ""), GNX_NGCF_NAMES2(c, "_norm")}, {GNX_NGCF_NAMES2(c, "_drop"), GNX_NGCF_NAMES2(c, "_drop_norm")}}
const char *const kNgcfFused[3][2][2][2] = {GNX_NGCF_NAMES("16"), GNX_NGCF_NAMES("32"), GNX_NGCF_NAMES("64")};
const char *const kNgcfComposed[2][2] = {{"spmm+dense_mfma_ngcf", "spmm+dense_mfma_ngcf_norm"}, {"spmm+dense_mfma_ngcf_drop", "spmm+dense_mfma_ngcf_drop_norm"}};
#undef GNX_NGCF_NAMES
#undef GNX_NGCF_NAMES2

struct NgcfOut { float *out; int64_t ldo; float *agg; uint32_t *gate; float *rnorm; float *work; int64_t work_floats; };

inline int64_t roundup4(int64_t x) { return (x + 3) / 4 * 4; }

// out = l2_normalize(drop(act((X * (A . X)) . W1 + b1) + act((A . X) . W2 + b2))).  The fused launch takes C_in = 16, 32 or 64 with
// C_out <= C_in over 16-byte aligned rows; its hub rows, and every row of everything else, are composed inside this call: the
// aggregated rows at T (d_agg, else the first roundup4(n C_in) floats of d_work), the product pass into compact rows, the dense kernel
// twice without activation (P1 compact, P2 into out), then k_ngcf_tail.  Nothing is launched before the last check has passed.
int ngcf_forward(const char *fn, gnx_graph *g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C_in, const float *d_W1, int64_t ldw1,
                 const float *d_W2, int64_t ldw2, int64_t C_out, const float *d_b1, const float *d_b2, int act, const DropFuse *fd, int normalize,
                 const NgcfOut &o, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU || act == GNX_ACT_LEAKY, "%s: invalid activation %d", fn, act);
    GNX_CHECK_ARG(normalize == 0 || normalize == 1, "%s: normalize must be 0 or 1", fn);
    GNX_CHECK_ARG(C_in >= 1 && C_in <= (1 << 20) && C_out >= 1 && C_out <= (1 << 20), "%s: widths %lld -> %lld not in [1, 2^20]", fn,
                  (long long)C_in, (long long)C_out);
    GNX_CHECK_ARG(d_X != nullptr && d_W1 != nullptr && d_W2 != nullptr && o.out != nullptr, "%s: NULL X / W1 / W2 / out", fn);
    GNX_CHECK_ARG(ldx >= C_in, "%s: ldx %lld < C_in %lld", fn, (long long)ldx, (long long)C_in);
    GNX_CHECK_ARG(ldw1 >= C_out && ldw2 >= C_out, "%s: ldw1 %lld or ldw2 %lld < C_out %lld", fn, (long long)ldw1, (long long)ldw2, (long long)C_out);
    GNX_CHECK_ARG(o.ldo >= C_out, "%s: ldo %lld < C_out %lld", fn, (long long)o.ldo, (long long)C_out);
    GNX_CHECK_ARG(o.rnorm == nullptr || normalize, "%s: d_rnorm without normalize", fn);
    GNX_CHECK_ARG(o.work_floats >= 0 && (o.work != nullptr || o.work_floats == 0), "%s: work_floats %lld without d_work, or negative", fn,
                  (long long)o.work_floats);
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "%s: needs a square graph", fn);
    auto input = [&](const void *b) {
        return b == d_X || b == d_W1 || b == d_W2 || (d_b1 && b == d_b1) || (d_b2 && b == d_b2) || (d_vals && b == d_vals);
    };
    const void *gate = o.gate, *rnorm = o.rnorm;
    GNX_CHECK_ARG(!input(o.out), "%s: out must not alias an input (X / W1 / W2 / the biases / the values)", fn);
    GNX_CHECK_ARG(o.agg == nullptr || (!input(o.agg) && o.agg != o.out), "%s: d_agg must be a buffer of its own", fn);
    GNX_CHECK_ARG(gate == nullptr || (!input(gate) && gate != o.out && gate != o.agg), "%s: d_gate must be a buffer of its own", fn);
    GNX_CHECK_ARG(rnorm == nullptr || (!input(rnorm) && rnorm != o.out && rnorm != o.agg && rnorm != gate), "%s: d_rnorm must be a buffer of its own", fn);
    GNX_CHECK_ARG(o.work == nullptr || (!input(o.work) && o.work != o.out && o.work != o.agg && o.work != gate && o.work != rnorm),
                  "%s: d_work must be a buffer of its own", fn);
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
    const int nto = (int)blocks_for(C_out, 16);
    with_tile_width(C_in, n, [&](auto NTI, dim3 grid) {
        auto with_mode = [&](auto NTO) {      // (C_out <= C_in: no NTO above NTI)
            with_flags([&](auto DROP) {
                if constexpr (NTO() <= NTI())
                    hipLaunchKernelGGL((k_spmm_ngcf<F32Rows, NTI(), NTO(), 4, 8, DROP()>), grid, dim3(512), 0, s, p, d_W1, ldw1, d_W2, ldw2, (int)C_out,
                                       d_b1, d_b2, act, o.agg, gate_words, o.rnorm, normalize != 0, vec_out, feat);
            }, fd != nullptr);
        };
        if (nto == 1)      with_mode(IntC<1>{});
        else if (nto == 2) with_mode(IntC<2>{});
        else if (nto == 3) with_mode(IntC<3>{});
        else               with_mode(IntC<4>{});
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
    GNX_CHECK_ARG(d_g != nullptr && d_G1 != nullptr && d_G2 != nullptr && ldg >= C_out && ldG >= C_out, "%s: NULL g / G1 / G2 or a row stride below C_out", fn);
    GNX_CHECK_ARG(d_rnorm == nullptr || (d_y != nullptr && ldy >= C_out), "%s: d_rnorm needs y (the normalised forward output) with ldy >= C_out", fn);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || d_gate != nullptr, "%s: relu / leaky_relu need d_gate", fn);
    const void *gate = d_gate;
    GNX_CHECK_ARG(d_G1 != d_G2 && d_G1 != d_g && d_G2 != d_g && d_G1 != d_y && d_G2 != d_y && d_G1 != d_rnorm && d_G2 != d_rnorm &&
                  (const void *)d_G1 != gate && (const void *)d_G2 != gate, "%s: G1 and G2 must be buffers of their own", fn);
    DropFuse fd{};
    const int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    if (n_rows == 0) return GNX_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t pad = std::min<int64_t>(ldG, (C_out + 3) / 4 * 4);
    const float slope = act == GNX_ACT_LEAKY ? 0.2f : act == GNX_ACT_RELU ? 0.f : 1.f;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks_for(n_rows, 16), 1 << 20);
    GNX_LAUNCH(k_ngcf_back_gate, grid, d_g, ldg, d_y, ldy, d_rnorm, act == GNX_ACT_NONE ? nullptr : d_gate, n_rows, C_out, pad, slope, fd, d_G1, d_G2, ldG);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_gcn_step(gnx_graph_t g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C_in, const float *d_W, int64_t ldw, int64_t C_out,
                 const float *d_bias, int act, double dropout_p, uint64_t seed, uint64_t stream_id, float *d_out, int64_t ldo, float *d_agg,
                 float *d_work, void *stream) {
    const char *fn = "gnx_gcn_step";
    DropFuse fd{};
    const int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    return gcn_forward(fn, g, d_vals, nullptr, d_X, ldx, C_in, d_W, ldw, C_out, d_bias, act, dropout_p != 0.0 ? &fd : nullptr,
                       GcnOut{d_out, ldo, d_agg, d_work}, stream);
}

// (dropout_p == 0: no feature mask -- nothing is hashed for the finished rows; the edge dropout acts at any rate in [0, 1))
int gnx_gcn_step_dropped(gnx_graph_t g, const float *d_D, float edge_p, uint64_t edge_seed, uint64_t edge_stream, const float *d_X, int64_t ldx,
                         int64_t C_in, const float *d_W, int64_t ldw, int64_t C_out, const float *d_bias, int act, double dropout_p, uint64_t seed,
                         uint64_t stream_id, float *d_out, int64_t ldo, float *d_agg, float *d_work, void *stream) {
    const char *fn = "gnx_gcn_step_dropped";
    DropFuse fd{};
    const int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    const EdgeDrop edge{d_D, edge_p, edge_seed, edge_stream};
    return gcn_forward(fn, g, nullptr, &edge, d_X, ldx, C_in, d_W, ldw, C_out, d_bias, act, dropout_p != 0.0 ? &fd : nullptr,
                       GcnOut{d_out, ldo, d_agg, d_work}, stream);
}

int gnx_gcn_step_back(gnx_graph_t g, const float *d_vals_t, const float *d_G, int64_t ldg, int64_t C_out, const float *d_Wt, int64_t ldwt,
                      int64_t C_in, float *d_dX, int64_t lddx, float *d_work, int64_t work_floats, void *stream) {
    return gcn_backward("gnx_gcn_step_back", g, d_vals_t, nullptr, d_G, ldg, C_out, d_Wt, ldwt, C_in, d_dX, lddx, d_work, work_floats, stream);
}

int gnx_gcn_step_back_dropped(gnx_graph_t g, const float *d_D, float edge_p, uint64_t edge_seed, uint64_t edge_stream, const float *d_G,
                              int64_t ldg, int64_t C_out, const float *d_Wt, int64_t ldwt, int64_t C_in, float *d_dX, int64_t lddx,
                              float *d_work, int64_t work_floats, void *stream) {
    const EdgeDrop edge{d_D, edge_p, edge_seed, edge_stream};
    return gcn_backward("gnx_gcn_step_back_dropped", g, nullptr, &edge, d_G, ldg, C_out, d_Wt, ldwt, C_in, d_dX, lddx, d_work, work_floats, stream);
}

int gnx_gcnii_step(gnx_graph_t g, const float *d_vals, const float *d_H, const float *d_H0, float a, int64_t C, const float *d_M,
                   int64_t ldm, int act, float *d_out, float *d_mixed, void *stream) {
    const ForwardForm f{nullptr, d_mixed, nullptr, 0, true, "spmm_gcnii_mfma", "spmm+dense_mfma"};
    return gcnii_forward<F32Rows>("gnx_gcnii_step", g, d_vals, d_H, d_H0, a, C, d_M, ldm, act, d_out, f, stream);
}

int gnx_gcnii_step_drop(gnx_graph_t g, const float *d_vals, const float *d_H, const float *d_H0, float a, int64_t C, const float *d_M,
                        int64_t ldm, int act, double dropout_p, uint64_t seed, uint64_t stream_id, float *d_out, float *d_mixed,
                        void *stream) {
    DropFuse fd{};
    int rc = make_feat_drop("gnx_gcnii_step_drop", g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    const bool drop = dropout_p != 0.0;      // p == 0 hashes nothing: the plain path
    const ForwardForm f{drop ? &fd : nullptr, d_mixed, nullptr, 0, true, drop ? "spmm_gcnii_mfma_drop" : "spmm_gcnii_mfma",
                        drop ? "spmm+dense_mfma_drop" : "spmm+dense_mfma"};
    return gcnii_forward<F32Rows>("gnx_gcnii_step_drop", g, d_vals, d_H, d_H0, a, C, d_M, ldm, act, d_out, f, stream);
}

// (feat_p == 0: no feature mask -- nothing is hashed for the finished rows; the edge dropout acts at any rate in [0, 1))
int gnx_gcnii_step_dropped(gnx_graph_t g, const float *d_D, float edge_p, uint64_t edge_seed, uint64_t edge_stream, const float *d_H,
                           const float *d_H0, float a, int64_t C, const float *d_M, int64_t ldm, int act, double feat_p, uint64_t feat_seed,
                           uint64_t feat_stream, float *d_out, float *d_mixed, void *stream) {
    const char *fn = "gnx_gcnii_step_dropped";
    DropFuse fd{};
    int rc = make_feat_drop(fn, g, feat_p, feat_seed, feat_stream, fd);
    if (rc != GNX_OK) return rc;
    const EdgeDrop edge{d_D, edge_p, edge_seed, edge_stream};
    const bool drop = feat_p != 0.0;
    ForwardForm f{drop ? &fd : nullptr, d_mixed, nullptr, 0, true, drop ? "spmm_gcnii_mfma_edrop_drop" : "spmm_gcnii_mfma_edrop",
                  drop ? "spmm+dense_mfma_edrop_drop" : "spmm+dense_mfma_edrop"};
    f.edge = &edge;
    return gcnii_forward<F32Rows>(fn, g, nullptr, d_H, d_H0, a, C, d_M, ldm, act, d_out, f, stream);
}

int gnx_gcnii_step_back_dropped(gnx_graph_t g, const float *d_D, float edge_p, uint64_t edge_seed, uint64_t edge_stream, const float *d_G, float a,
                                int64_t C, const float *d_Mt, int64_t ldmt, float *d_dH, const float *d_S_in, float s_alpha, float *d_S_out,
                                float *d_work, void *stream) {
    const EdgeDrop edge{d_D, edge_p, edge_seed, edge_stream};
    return gcnii_backward<F32Rows>("gnx_gcnii_step_back_dropped", g, nullptr, d_G, d_G, a, C, d_Mt, ldmt, d_dH, d_S_in, s_alpha, d_S_out, d_work,
                                   stream, &edge);
}

// (the gate words are the relu's: with the identity there is nothing to gate and d_gate is not looked at)
int gnx_gcnii_step_spectral(gnx_graph_t g, const float *d_vals, const float *d_H, const float *d_H0, float a, int64_t C, const float *d_M,
                            int64_t ldm, const float *d_bias, int act, double dropout_p, uint64_t seed, uint64_t stream_id, float *d_out,
                            float *d_mixed, uint32_t *d_gate, void *stream) {
    const char *fn = "gnx_gcnii_step_spectral";
    DropFuse fd{};
    int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(d_bias != nullptr, "%s: NULL bias", fn);
    // (at the other widths d_mixed is the buffer every call passes its mixed rows through, and says nothing about training)
    GNX_CHECK_ARG(act != GNX_ACT_RELU || d_mixed == nullptr || d_gate != nullptr || !fused_width(C),
                  "%s: relu with d_mixed (training) needs d_gate [n, ceil(C / 32)] (the backward's gate)", fn);
    const bool drop = dropout_p != 0.0;      // p == 0 hashes nothing
    const ForwardForm f{drop ? &fd : nullptr, d_mixed, nullptr, 0, true, drop ? "spmm_gcnii_spectral_mfma_drop" : "spmm_gcnii_spectral_mfma",
                        drop ? "spmm+dense_mfma_spectral_drop" : "spmm+dense_mfma_spectral", d_bias, act == GNX_ACT_RELU ? d_gate : nullptr};
    return gcnii_forward<F32Rows>(fn, g, d_vals, d_H, d_H0, a, C, d_M, ldm, act, d_out, f, stream);
}

int gnx_gcnii_spectral_back(gnx_graph_t g, const float *d_g, int64_t ldg, const uint32_t *d_gate, int64_t n_rows, int64_t C, int act,
                            double dropout_p, uint64_t seed, uint64_t stream_id, float *d_G, int64_t ldG, float *d_dbias, float *d_work,
                            int64_t work_floats, void *stream) {
    const char *fn = "gnx_gcnii_spectral_back";
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "%s: invalid activation %d", fn, act);
    GNX_CHECK_ARG(n_rows >= 0 && C >= 1 && C <= (1 << 20), "%s: negative row count or C not in [1, 2^20]", fn);
    GNX_CHECK_ARG(d_g != nullptr && d_G != nullptr && d_dbias != nullptr && ldg >= C && ldG >= C, "%s: NULL g / G / dbias or a row stride below C", fn);
    GNX_CHECK_ARG(d_G != d_g || ldG == ldg, "%s: in place needs ldG == ldg", fn);
    const bool relu = act == GNX_ACT_RELU;
    const int64_t slabs = std::max<int64_t>(1, std::min<int64_t>(2048, blocks_for(n_rows, 256)));      // a function of n alone
    const void *gate = d_gate, *work = d_work;
    GNX_CHECK_ARG(!relu || (gate != nullptr && gate != d_g && gate != d_G), "%s: relu needs d_gate (not g / G itself)", fn);
    GNX_CHECK_ARG(d_dbias != d_g && d_dbias != d_G && (!relu || d_dbias != gate), "%s: dbias must be a buffer of its own", fn);
    GNX_CHECK_ARG(!relu || (work != nullptr && work != d_g && work != d_G && work != gate && work != d_dbias),
                  "%s: d_work must be a buffer of its own", fn);
    GNX_CHECK_ARG(!relu || work_floats >= slabs * C, "%s: work_floats %lld below %lld = min(2048, ceil(n_rows / 256)) slabs of C floats", fn,
                  (long long)work_floats, (long long)(slabs * C));
    DropFuse fd{};
    int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (!relu || n_rows == 0) GNX_HIP(hipMemsetAsync(d_dbias, 0, (size_t)C * sizeof(float), s));      // the identity: exact zeros
    if (n_rows == 0) return GNX_OK;
    const bool v4 = C % 4 == 0 && ldg % 4 == 0 && ldG % 4 == 0 && aligned(d_g, 16) && aligned(d_G, 16) && (!relu || aligned(d_work, 16));
    const dim3 grid((unsigned)slabs, blocks_for(v4 ? C / 4 : C, 256));
    if (v4) {
        if (relu) GNX_LAUNCH((k_spectral_back<4, true>), grid, d_g, ldg, d_gate, n_rows, C, fd, d_G, ldG, d_work);
        else      GNX_LAUNCH((k_spectral_back<4, false>), grid, d_g, ldg, d_gate, n_rows, C, fd, d_G, ldG, d_work);
    } else {
        if (relu) GNX_LAUNCH((k_spectral_back<1, true>), grid, d_g, ldg, d_gate, n_rows, C, fd, d_G, ldG, d_work);
        else      GNX_LAUNCH((k_spectral_back<1, false>), grid, d_g, ldg, d_gate, n_rows, C, fd, d_G, ldG, d_work);
    }
    if (relu) sum_slabs(d_work, slabs, C, d_dbias, s);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_gcnii_step_bf16(gnx_graph_t g, const float *d_vals, const uint16_t *d_H, const float *d_H0, float a, int64_t C, const float *d_M,
                        int64_t ldm, int act, void *d_out, int out_bf16, float *d_work, void *stream) {
    const ForwardForm f{nullptr, nullptr, d_work, out_bf16, true, "spmm_gcnii_mfma_bf16", "spmm+dense_mfma_bf16"};
    return gcnii_forward<Bf16Rows>("gnx_gcnii_step_bf16", g, d_vals, d_H, d_H0, a, C, d_M, ldm, act, d_out, f, stream);
}

// (training: T is kept, so d_mixed is not optional; no composed form -- the callers keep f32 at the other widths)
int gnx_gcnii_step_train_bf16(gnx_graph_t g, const float *d_vals, const uint16_t *d_H, const float *d_H0, float a, int64_t C, const float *d_M,
                              int64_t ldm, int act, double dropout_p, uint64_t seed, uint64_t stream_id, void *d_out, int out_bf16,
                              float *d_mixed, float *d_work, void *stream) {
    const char *fn = "gnx_gcnii_step_train_bf16";
    DropFuse fd{};
    int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(d_mixed != nullptr, "%s: needs d_mixed [n, C] f32 (the mixed rows T are kept for the weight gradient)", fn);
    const ForwardForm f{dropout_p != 0.0 ? &fd : nullptr, d_mixed, d_work, out_bf16, false, "spmm_gcnii_mfma_train_bf16", nullptr};
    return gcnii_forward<Bf16Rows>(fn, g, d_vals, d_H, d_H0, a, C, d_M, ldm, act, d_out, f, stream);
}

// (gnx_gcnii_step_train_bf16 without d_mixed: the forward of a layer whose weight gradient makes T again, gnx_gcnii_wgrad_bf16)
int gnx_gcnii_step_drop_bf16(gnx_graph_t g, const float *d_vals, const uint16_t *d_H, const float *d_H0, float a, int64_t C, const float *d_M,
                             int64_t ldm, int act, double dropout_p, uint64_t seed, uint64_t stream_id, void *d_out, int out_bf16, float *d_work,
                             void *stream) {
    const char *fn = "gnx_gcnii_step_drop_bf16";
    DropFuse fd{};
    int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    const ForwardForm f{dropout_p != 0.0 ? &fd : nullptr, nullptr, d_work, out_bf16, false, "spmm_gcnii_mfma_drop_bf16", nullptr};
    return gcnii_forward<Bf16Rows>(fn, g, d_vals, d_H, d_H0, a, C, d_M, ldm, act, d_out, f, stream);
}

int gnx_gcnii_wgrad(gnx_graph_t g, const float *d_vals, const float *d_H, const float *d_H0, float a, int64_t C, const float *d_G, float *d_dM,
                    float *d_hub_rows, float *d_work, int64_t work_floats, void *stream) {
    return gcnii_wgrad<F32Rows>("gnx_gcnii_wgrad", "gcnii_wgrad_mfma", g, d_vals, d_H, d_H0, a, C, d_G, d_dM, d_hub_rows, d_work, work_floats, stream);
}

int gnx_gcnii_wgrad_bf16(gnx_graph_t g, const float *d_vals, const uint16_t *d_H, const float *d_H0, float a, int64_t C, const float *d_G,
                         float *d_dM, float *d_hub_rows, float *d_work, int64_t work_floats, void *stream) {
    return gcnii_wgrad<Bf16Rows>("gnx_gcnii_wgrad_bf16", "gcnii_wgrad_mfma_bf16", g, d_vals, d_H, d_H0, a, C, d_G, d_dM, d_hub_rows, d_work,
                                 work_floats, stream);
}

int gnx_gcnii_step_back(gnx_graph_t g, const float *d_vals_t, const float *d_G, float a, int64_t C, const float *d_Mt, int64_t ldmt,
                        float *d_dH, const float *d_S_in, float s_alpha, float *d_S_out, float *d_work, void *stream) {
    return gcnii_backward<F32Rows>("gnx_gcnii_step_back", g, d_vals_t, d_G, d_G, a, C, d_Mt, ldmt, d_dH, d_S_in, s_alpha, d_S_out, d_work, stream);
}

int gnx_gcnii_step_back_bf16(gnx_graph_t g, const float *d_vals_t, const uint16_t *d_Gb, const float *d_G, float a, int64_t C, const float *d_Mt,
                             int64_t ldmt, float *d_dH, const float *d_S_in, float s_alpha, float *d_S_out, float *d_work, void *stream) {
    return gcnii_backward<Bf16Rows>("gnx_gcnii_step_back_bf16", g, d_vals_t, d_Gb, d_G, a, C, d_Mt, ldmt, d_dH, d_S_in, s_alpha, d_S_out, d_work, stream);
}

int gnx_feature_dropout(gnx_graph_t g, const float *d_X, int64_t ldx, int64_t n_rows, int64_t C, const int32_t *d_rows, double dropout_p,
                        uint64_t seed, uint64_t stream_id, float *d_out, int64_t ldo, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_feature_dropout: NULL handle");
    GNX_CHECK_ARG(n_rows >= 0 && C >= 1, "gnx_feature_dropout: negative row count or C < 1");
    GNX_CHECK_ARG(d_X != nullptr && d_out != nullptr && ldx >= C && ldo >= C, "gnx_feature_dropout: NULL X / out or a row stride below C");
    GNX_CHECK_ARG(d_out != d_X || ldo == ldx, "gnx_feature_dropout: in place needs ldo == ldx");
    DropFuse fd{};
    int rc = make_feat_drop("gnx_feature_dropout", g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    if (dropout_p == 0.0 && d_out == d_X) return GNX_OK;
    launch_feature_dropout(d_X, ldx, d_rows, n_rows, C, fd, d_out, ldo, (hipStream_t)stream);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_feature_dropout_back(gnx_graph_t g, const float *d_g, int64_t ldg, const float *d_y, int64_t ldy, int64_t n_rows, int64_t C,
                             double dropout_p, uint64_t seed, uint64_t stream_id, int act, float *d_G, int64_t ldG, void *stream) {
    return feature_dropout_back<F32Rows>("gnx_feature_dropout_back", g, d_g, ldg, d_y, ldy, n_rows, C, dropout_p, seed, stream_id, act, d_G, ldG,
                                         nullptr, 0, stream);
}

int gnx_feature_dropout_back_bf16(gnx_graph_t g, const float *d_g, int64_t ldg, const uint16_t *d_y, int64_t ldy, int64_t n_rows, int64_t C,
                                  double dropout_p, uint64_t seed, uint64_t stream_id, int act, float *d_G, int64_t ldG, uint16_t *d_Gb,
                                  int64_t ldGb, void *stream) {
    return feature_dropout_back<Bf16Rows>("gnx_feature_dropout_back_bf16", g, d_g, ldg, d_y, ldy, n_rows, C, dropout_p, seed, stream_id, act, d_G,
                                          ldG, d_Gb, ldGb, stream);
}

}  // extern "C"
