// The GCNII layer family (gcn.py:7-27,54-74) on gfx950: three kernels on the 16-row tile frame of gnx_layer_device.h, the row passes
// around them, and ONE host path per kernel over the launch plumbing of that header.
//   mixed_row          the residual mix behind gathered_row, written once over the row-storage policy R of gnx_spmm_device.h
//   k_spmm_gcnii       the GCNII layer in one launch: SpMM + mix + the C x C transform (DROP: + the feature mask in the store loop; SPEC:
//                      the spectral-preserving form, gnx_gcnii_step_spectral -- k_spectral_tail is its epilogue as a row pass,
//                      k_spectral_back the backward's first pass)
//   k_spmm_gcnii_back  the GCNII layer's backward past the relu gate, one launch over the transposed structure
//   k_gcnii_wgrad      the GCNII weight gradient dM = T^T G with the mixed rows T made again in LDS (mixed_row) and never stored
//   row passes         k_round_rows (f32 rows -> bf16), k_spectral_tail, k_spectral_back; the mask as a pass of its own (hub rows, the
//                      other widths) is launch_feature_dropout of gnx_feature_dropout.hip
//   gcnii_forward<R>   gnx_gcnii_step, _step_drop, _step_dropped, _step_spectral (F32Rows), _step_bf16, _step_train_bf16, _step_drop_bf16
//                      (Bf16Rows); a ForwardForm says what differs: the mask, where mixed rows are kept or pass through memory, the
//                      format of the result, and whether the widths other than 16 / 32 / 64 run as two launches or are refused
//   gcnii_backward<R>  gnx_gcnii_step_back, _step_back_dropped, _step_back_bf16; the composed form of the other widths is its f32 branch
//   gcnii_wgrad<R>     gnx_gcnii_wgrad, gnx_gcnii_wgrad_bf16
// (gnx_gcnii_spectral_back is an entry of its own: one launch and the slab sum.  spectral_finish stands in gnx_spectral_device.h and
// k_spectral_tail is launched through gnx::launch_spectral_tail, for the spectral GCN layer of gnx_gcn.hip too.)
#include "gnx_spectral_device.h"

namespace {

// ---- the spectral-preserving form (gcn.py:30-51, gnx_gcnii_step_spectral): out = 2 drop(act(P') - bias), P' = T . M + bias ------------
// What a launch needs beside the plain layer's arguments; the plain instantiations carry an empty struct.
template <bool SPEC> struct SpectralArgs {};
template <> struct SpectralArgs<true> {
    const float *bias;     // [C]
    uint32_t *gate;        // [n, ceil(C / 32)] or null: bit c & 31 of word row * ceil(C / 32) + (c >> 5) = (P'[row, c] > 0)
};

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

// The spectral form's row pass behind the dense kernel (hub rows; every row of the other widths): out[r, :] holds act(P') and leaves as
// 2 drop(act(P') - bias) in place, the row's gate words written beside it (gate may be null) -- spectral_finish, the store loop's own
// code.  A thread per gate word: up to 32 columns of row rows[i] (null: row i), any width and row stride.
template <bool DROP, bool BIAS = true>
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
            float b[1] = {0.f};
            if constexpr (BIAS) b[0] = bias[c];
            word |= spectral_finish<1, DROP>(fd, stream, r, c, b, x) << (c - c0);
            o[c] = x[0];
        }
        if (gate != nullptr) gate[r * words + w] = word;
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
        rc = spmm_back_composed(g, d_vals_t, edge, d_G, C, C, d_Mt, ldmt, C, beta, d_work, d_dH, C, stream);
        if (rc != GNX_OK) return rc;
        g->last_kernel = edge ? "dense+spmm_back_edrop" : "dense+spmm_back";
        if (d_S_out == nullptr || n == 0) return GNX_OK;
        const float *src[2] = {d_S_in, d_work};
        const float coef[2] = {s_alpha, a};
        return d_S_in ? gnx_linear_combination(2, src, coef, n * C, d_S_out, stream)
                      : gnx_linear_combination(1, src + 1, coef + 1, n * C, d_S_out, stream);
    }
    rc = ensure_transpose(g, s);   // (it and the slab before the first launch: under capture a part that would have to be built refuses the whole call)
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

}  // namespace

// (declared in gnx_internal.h: gnx_gcn.hip launches the pass for its spectral form; a null bias is a bias of zeros)
void gnx::launch_spectral_tail(float *out, int64_t ldo, const int32_t *rows, int64_t n, int64_t C, const float *bias, const DropFuse *fd,
                               uint32_t *gate, hipStream_t s) {
    if (n == 0 || C == 0) return;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks_for(n * ((C + 31) / 32), 256), 1 << 20);
    if (bias == nullptr) {
        if (fd) GNX_LAUNCH((k_spectral_tail<true, false>), grid, out, ldo, rows, n, C, bias, *fd, gate);
        else    GNX_LAUNCH((k_spectral_tail<false, false>), grid, out, ldo, rows, n, C, bias, DropFuse{}, gate);
    } else {
        if (fd) GNX_LAUNCH(k_spectral_tail<true>, grid, out, ldo, rows, n, C, bias, *fd, gate);
        else    GNX_LAUNCH(k_spectral_tail<false>, grid, out, ldo, rows, n, C, bias, DropFuse{}, gate);
    }
}

extern "C" {

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

}  // extern "C"
