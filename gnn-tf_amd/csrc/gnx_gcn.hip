// The GCN layer (gcn.py:77-89) on gfx950: two kernels on the 16-row tile frame of gnx_layer_device.h and ONE host path per kernel over
// the launch plumbing of that header.
//   k_spmm_gcn         the GCN layer in one launch: the gather without the residual operand, a rectangular W [C_in, C_out <= C_in]
//   k_spmm_gcn_back    the GCN layer's input gradient past the gate, one launch over the transposed structure: the gated gradient
//                      gathered at the OUTPUT width, stored at the input width (two geometries of the one tile)
//   gcn_forward        gnx_gcn_step, gnx_gcn_step_dropped, and with the SPEC form of the kernel (GCNSpectralPreservingLayer, gcn.py:92-105)
//                      gnx_step_spectral_gcn, gnx_step_spectral_gcn_dropped
//   gcn_backward       gnx_gcn_step_back, gnx_gcn_step_back_dropped; the composed order of the other widths / strides is its branch
// The mask of the rows that go through memory is launch_feature_dropout of gnx_feature_dropout.hip.
#include "gnx_spectral_device.h"

namespace {

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
// SPEC (gnx_step_spectral_gcn, gcn.py:92-105): the store loop forms 2 drop(act(P') - bias), P' the value the bias joined in the MFMA
// block's epilogue, through spectral_finish (a null bias: zeros), and with sp.gate the launch writes one bit per element, P' > 0, in the
// words of k_spmm_gcnii's SPEC form at the OUTPUT width: [n, ceil(C_out / 32)].  The lanes of a gate word -- those without a column
// below C_out included, which is why this form has no early return -- OR their bits together through xor-shuffles; a column at or
// beyond C_out contributes a 0 bit by selection (the zero-filled columns of W in LDS are not relied upon, and the tile's columns from
// 16 NTO on still hold gathered values), stores nothing, and the word's lowest lane stores the word if the word exists.  A template
// argument alone: the instantiations without it are the kernel as it was.
template <bool SPEC> struct GateArgs {};
template <> struct GateArgs<true> {
    uint32_t *gate;        // [n, ceil(C_out / 32)] or null: bit c & 31 of word row * ceil(C_out / 32) + (c >> 5) = (P'[row, c] > 0)
};

template <typename R, int NTI, int NTO, int U, int WPB, bool DROP = false, bool EDGE = false, bool ENTRIES = false, bool SPEC = false>
__global__ __launch_bounds__(64 * WPB) void k_spmm_gcn(const typename R::Args p, const float *__restrict__ W, int64_t ldw, int C_out,
                                                       const float *__restrict__ bias, float *__restrict__ agg, bool vec_out, const DropFuse feat,
                                                       const GateArgs<SPEC> sp = GateArgs<SPEC>{}) {
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
    if constexpr (SPEC) {
        constexpr int GW = G < 8 ? G : 8;      // lanes per gate word
        const int words = (C_out + 31) >> 5;
        const int left = C_out - c;            // the lane's columns below C_out: all four, the first `left`, or none
        const uint32_t valid = left >= 4 ? 0xfu : left > 0 ? (1u << left) - 1u : 0u;
        float b[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) b[v] = bias != nullptr && v < left ? bias[c + v] : 0.f;
        uint64_t stream = 0;
        if constexpr (DROP) stream = drop_stream(feat);
        const bool whole = vec_out && left >= 4;
#pragma unroll
        for (int ps = 0; ps < PASSES; ++ps) {
            const int rr = ps * RPP + lane / G;
            float o[4];
            vload<4>(o, T + rr * STRIDE + c);
            // (every lane of the wave takes part in the shuffles; a row's lanes are live or not together, and a dead row stores nothing)
            uint32_t word = (spectral_finish<4, DROP>(feat, stream, rows[ps], c, b, o) & valid) << (c & 31);
#pragma unroll
            for (int m = 1; m < GW; m <<= 1) word |= (uint32_t)__shfl_xor((int)word, m);
            if (!live[ps] || left <= 0) continue;
            float *__restrict__ dst = p.out + rows[ps] * p.ldo + c;
            if (whole) vstore<4>(dst, o);
            else {
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (v < left) dst[v] = o[v];
            }
            if (sp.gate != nullptr && sub % GW == 0) sp.gate[rows[ps] * words + (c >> 5)] = word;
        }
        return;
    }
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

// ---- the GCN layer's host path (gnx_gcn_step, gnx_gcn_step_dropped) -----------------------------------------------------------------------
// what gnx_graph_last_kernel reports: [C_in = 16, 32, 64][mask << 1 | edge dropout][hub rows ran]; the composed form [..][..] alone
#define GNX_GCN_NAMES(c) {GNX_TILE_NAMES("k_spmm_gcn", c, ""), GNX_TILE_NAMES("k_spmm_gcn", c, "_edrop"), GNX_TILE_NAMES("k_spmm_gcn", c, "_drop"), GNX_TILE_NAMES("k_spmm_gcn", c, "_edrop_drop")}
const char *const kGcnFused[3][4][2] = {GNX_GCN_NAMES("16"), GNX_GCN_NAMES("32"), GNX_GCN_NAMES("64")};
const char *const kGcnComposed[4] = {"spmm+dense_mfma_gcn", "spmm+dense_mfma_gcn_edrop", "spmm+dense_mfma_gcn_drop", "spmm+dense_mfma_gcn_edrop_drop"};
// the spectral form (gnx_step_spectral_gcn), likewise
#define GNX_GCN_SPEC_NAMES(c) {GNX_TILE_NAMES("k_spmm_gcn_spectral", c, ""), GNX_TILE_NAMES("k_spmm_gcn_spectral", c, "_edrop"), GNX_TILE_NAMES("k_spmm_gcn_spectral", c, "_drop"), GNX_TILE_NAMES("k_spmm_gcn_spectral", c, "_edrop_drop")}
const char *const kGcnSpecFused[3][4][2] = {GNX_GCN_SPEC_NAMES("16"), GNX_GCN_SPEC_NAMES("32"), GNX_GCN_SPEC_NAMES("64")};
const char *const kGcnSpecComposed[4] = {"spmm+dense_mfma_gcn_spectral", "spmm+dense_mfma_gcn_spectral_edrop", "spmm+dense_mfma_gcn_spectral_drop",
                                         "spmm+dense_mfma_gcn_spectral_edrop_drop"};
#undef GNX_GCN_SPEC_NAMES
#undef GNX_GCN_NAMES

// the result, and where aggregated rows are kept / may pass through memory; `spectral`: out = 2 drop(act(P') - bias) and the gate words
// [n, ceil(C_out / 32)] of P' > 0 at `gate` (null: not kept)
struct GcnOut { float *out; int64_t ldo; float *agg, *work; bool spectral = false; uint32_t *gate = nullptr; };

// out = drop(act((A . X) . W + bias)), A from d_vals or made from `edge`; `fd` the mask of the finished rows or null.  The fused launch
// takes C_in = 16, 32 or 64 with C_out <= C_in over 16-byte aligned rows; everything else runs the SpMM, the dense kernel and the mask
// pass inside this call, as gcnii_forward treats its other widths.  o.spectral (gnx_step_spectral_gcn): the SPEC form of the launch, and
// for the rows that go through memory the dense kernel with the bias, then k_spectral_tail (- bias, the mask, x 2, the gate words) in
// the mask pass's place.  Nothing is launched before the last check has passed.
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
    const void *gate = o.gate;
    GNX_CHECK_ARG(gate == nullptr || (!input(gate) && gate != o.out && gate != o.agg && gate != o.work), "%s: d_gate must be a buffer of its own", fn);
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
        if (o.spectral) launch_spectral_tail(o.out, o.ldo, rows, n, C_out, d_bias, fd, o.gate, s);
        else if (fd) launch_feature_dropout(o.out, o.ldo, rows, n, C_out, *fd, o.out, o.ldo, s);
        GNX_HIP(hipGetLastError());
        return GNX_OK;
    };
    if (!fusable) {
        const int rc = edge ? gnx_spmm_dropped(g, edge->D, edge->p, edge->seed, edge->stream, 0, d_X, ldx, C_in, nullptr, 0, 1.f, 0.f, GNX_ACT_NONE, T,
                                               C_in, stream)
                            : gnx_spmm(g, d_vals, nullptr, d_X, ldx, C_in, nullptr, 0, 1.f, 0.f, GNX_ACT_NONE, T, C_in, stream);
        if (rc != GNX_OK) return rc;
        g->last_kernel = (o.spectral ? kGcnSpecComposed : kGcnComposed)[mode];
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
    with_tile_width(C_in, m.n_rows, [&](auto NTI, dim3 grid) {
        with_out_tiles((int)blocks_for(C_out, 16), [&](auto NTO) {      // (C_out <= C_in: no NTO above NTI; ENTRIES goes with EDGE)
            with_flags([&](auto DROP, auto EDGE, auto ENTRIES, auto SPEC) {
                if constexpr (NTO() <= NTI() && (EDGE() || !ENTRIES())) {
                    GateArgs<SPEC()> sp{};
                    if constexpr (SPEC()) sp.gate = o.gate;
                    hipLaunchKernelGGL((k_spmm_gcn<F32Rows, NTI(), NTO(), 4, 8, DROP(), EDGE(), ENTRIES(), SPEC()>), grid, dim3(512), 0, s, p, d_W,
                                       ldw, (int)C_out, d_bias, o.agg, vec_out, feat, sp);
                }
            }, fd != nullptr, edge != nullptr, edge && p.fuse.mult, o.spectral);
        });
    });
    g->last_kernel = (o.spectral ? kGcnSpecFused : kGcnFused)[C_in == 16 ? 0 : C_in == 32 ? 1 : 2][mode][m.n_long > 0];
    // hub rows: chunked partial sums -> aggregated rows at their row ids of T -> the transform and the mask of those rows alone
    p.act = GNX_ACT_NONE;
    p.ldo = C_in;
    return hub_rows_tail<F32Rows>(g, m, p, d_X, T, edge != nullptr, s, transform_rows);
}

// ---- the GCN layer's backward host path (gnx_gcn_step_back, gnx_gcn_step_back_dropped) ----------------------------------------------------
// what gnx_graph_last_kernel reports: [C_in = 16, 32, 64][edge dropout][hub rows ran]; the composed form [edge dropout]
#define GNX_GCN_BACK_NAMES(c) {GNX_TILE_NAMES("k_spmm_gcn_back", c, ""), GNX_TILE_NAMES("k_spmm_gcn_back", c, "_edrop")}
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
    const int64_t n = g->a.n_rows, c4 = roundup4(C_out);
    const bool fusable = fused_width(C_in) && C_out <= C_in && ldg % 4 == 0 && ldg >= c4 && aligned(d_G, 16) && lddx % 4 == 0 &&
                         aligned(d_dX, 16) && aligned(d_work, 16);
    if (!fusable) {      // the composed order: gT = G' . Wt into d_work, dX = At gT
        GNX_CHECK_ARG(work_floats >= n * C_in, "%s: needs d_work of n * C_in = %lld floats, has %lld (%s: G' . Wt goes through memory, gnx_dense and the transposed SpMM run as two launches)",
                      fn, (long long)(n * C_in), (long long)work_floats,
                      !fused_width(C_in) ? "C_in is not 16, 32 or 64" : C_out > C_in ? "C_out > C_in"
                      : (ldg % 4 != 0 || ldg < c4) ? "the rows of G' are not padded to whole 16-byte pieces: ldg % 4 != 0 or ldg < roundup4(C_out)"
                                                   : "misaligned rows");
        const int rc = spmm_back_composed(g, d_vals_t, edge, d_G, ldg, C_out, d_Wt, ldwt, C_in, 1.f, d_work, d_dX, lddx, stream);
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
    with_tile_width(C_in, m.n_rows, [&](auto NTI, dim3 grid) {
        // (the gather's width is the smallest of 16, 32, 64 that holds C_out: no NTG of 3, none above NTI; ENTRIES goes with EDGE)
        with_out_tiles(C_out <= 16 ? 1 : C_out <= 32 ? 2 : 4, [&](auto NTG) {
            with_flags([&](auto EDGE, auto ENTRIES) {
                if constexpr (NTG() != 3 && NTG() <= NTI() && (EDGE() || !ENTRIES()))
                    hipLaunchKernelGGL((k_spmm_gcn_back<F32Rows, NTI(), NTG(), 4, 8, EDGE(), ENTRIES()>), grid, dim3(512), 0, s, p, d_Wt, ldwt, (int)C_out);
            }, edge != nullptr, edge && p.fuse.mult);
        });
    });
    g->last_kernel = kGcnBackFused[C_in == 16 ? 0 : C_in == 32 ? 1 : 2][edge ? 1 : 0][m.n_long > 0];
    // hub rows of the transposed structure: chunked partial sums -> At . G' at their row ids of d_work, width C_out -> those rows alone times Wt
    p.ldo = C_out;
    return hub_rows_tail<F32Rows>(g, m, p, d_G, d_work, edge != nullptr, s, [&](const int32_t *rows, int64_t k) {
        return dense_rows(d_work, C_out, k, C_out, d_Wt, ldwt, C_in, nullptr, GNX_ACT_NONE, rows, rows, d_dX, lddx, s);
    });
}

}  // namespace

extern "C" {

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

// (the gate words are the relu's: with the identity there is nothing to gate and d_gate is not looked at)
int gnx_step_spectral_gcn(gnx_graph_t g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C_in, const float *d_W, int64_t ldw,
                          int64_t C_out, const float *d_bias, int act, double dropout_p, uint64_t seed, uint64_t stream_id, float *d_out, int64_t ldo,
                          float *d_agg, uint32_t *d_gate, float *d_work, void *stream) {
    const char *fn = "gnx_step_spectral_gcn";
    DropFuse fd{};
    const int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(act != GNX_ACT_RELU || d_agg == nullptr || d_gate != nullptr,
                  "%s: relu with d_agg (training) needs d_gate [n, ceil(C_out / 32)] (the backward's gate)", fn);
    return gcn_forward(fn, g, d_vals, nullptr, d_X, ldx, C_in, d_W, ldw, C_out, d_bias, act, dropout_p != 0.0 ? &fd : nullptr,
                       GcnOut{d_out, ldo, d_agg, d_work, true, act == GNX_ACT_RELU ? d_gate : nullptr}, stream);
}

int gnx_step_spectral_gcn_dropped(gnx_graph_t g, const float *d_D, float edge_p, uint64_t edge_seed, uint64_t edge_stream, const float *d_X,
                                  int64_t ldx, int64_t C_in, const float *d_W, int64_t ldw, int64_t C_out, const float *d_bias, int act,
                                  double dropout_p, uint64_t seed, uint64_t stream_id, float *d_out, int64_t ldo, float *d_agg, uint32_t *d_gate,
                                  float *d_work, void *stream) {
    const char *fn = "gnx_step_spectral_gcn_dropped";
    DropFuse fd{};
    const int rc = make_feat_drop(fn, g, dropout_p, seed, stream_id, fd);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(act != GNX_ACT_RELU || d_agg == nullptr || d_gate != nullptr,
                  "%s: relu with d_agg (training) needs d_gate [n, ceil(C_out / 32)] (the backward's gate)", fn);
    const EdgeDrop edge{d_D, edge_p, edge_seed, edge_stream};
    return gcn_forward(fn, g, nullptr, &edge, d_X, ldx, C_in, d_W, ldw, C_out, d_bias, act, dropout_p != 0.0 ? &fd : nullptr,
                       GcnOut{d_out, ldo, d_agg, d_work, true, act == GNX_ACT_RELU ? d_gate : nullptr}, stream);
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

}  // extern "C"
