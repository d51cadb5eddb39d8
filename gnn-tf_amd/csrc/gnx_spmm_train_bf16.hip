// Opt-in bf16 feature storage for the fused training propagation: the chained forward and backward loops of gnx_spmm_train.hip with
// the GATHERED operand stored as bf16 (gnx_spmm_dropped_chained_bf16, gnx_spmm_dropped_back_bf16).
//
// What is bf16: the rows a launch gathers (X) and the rows it hands to the next launch of the loop (the forward's pre-scaled
// iterate, the backward's pre-scaled gradient).  A gathered row is widened exactly to f32 as it arrives.  Every weight (the counter
// RNG, the kept sums, the degree scales: dropped_weight_at of gnx_internal.h, unchanged), every sum, H0, the mix, the running
// gradient sum and both results of a step are f32.  A row that leaves as bf16 is rounded ONCE, after its scale:
// bf(H[i] * D_next[i]) forward, bf(y_beta * acc[r] * D_next[r]) backward (round to nearest even, NaN stays NaN).
//
// Dispatch classes, row orders and summation orders are those of gnx_spmm_train.hip -- one wave per row above 32 lanes, 32/16/8-lane
// groups below, long rows cut into chunks whose f32 partial sums a second kernel adds in chunk order (no float atomics: two calls
// give the same bits) -- with up to 8 bf16 (16 bytes) per lane, so C = 128 runs on 16-lane groups.  Dropped entries (weight exactly
// 0) are not gathered.  Every kernel here is its own; the f32 kernels are not touched.
#include "gnx_bf16_device.h"

namespace {

struct TbArgs : SpmmArgs {     // SpmmArgs::X / ::out / ::out2 stay null: the typed buffers are here
    const uint16_t *Xb;        // bf16 [rows, ldx]: the gathered operand
    void *outv;                // f32 or bf16 [n_rows, ldo]
    int out_bf16;
    uint16_t *out2b;           // bf16 [n_rows, ldo2] or null: the backward's operand for the next call
};

// wave_accumulate<FUSE> (gnx_spmm_device.h) over bf16 rows: one weight per lane and round of 64 entries, the kept entries gathered in
// ascending order, U rows in flight
template <int VEC, int U, bool ENTRIES>
__device__ __forceinline__ void wave_accumulate_drop_bf16(const TbArgs &p, int64_t beg, int64_t end, int c, int lane, int64_t row,
                                                          float (&acc)[VEC]) {
    for (int64_t base = beg; base < end; base += 64) {
        const int n = (int)((end - base) < 64 ? (end - base) : 64);
        int mycol = 0;
        float myw = 0.f;
        if (lane < n) {
            mycol = p.colidx[base + lane];
            myw = dropped_weight_at<ENTRIES>(p.fuse, p.vals[base + lane], base + lane, row, mycol);
        }
        uint64_t keep = __ballot(myw != 0.f);
        while (keep) {
            float x[U][VEC];
            int idx[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                idx[u] = keep ? (int)__builtin_ctzll(keep) : -1;
                if (keep) keep &= keep - 1;
                if (idx[u] >= 0) bload<VEC>(x[u], p.Xb + (int64_t)readlane_i(mycol, idx[u]) * p.ldx + c);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (idx[u] >= 0) {
                    const float w = readlane_f(myw, idx[u]);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, x[u][v], acc[v]);
                }
            }
        }
    }
}

// epilogue_store (gnx_spmm_device.h) of the training entries: the backward's second result (bf16, rounded after its scale), the
// f32 mix with H0 / the running sum, the next iteration's column scale, and one rounding if the result is bf16
template <int VEC>
__device__ __forceinline__ void epilogue_train_bf16(const TbArgs &p, int64_t row, int c, bool active, float (&acc)[VEC]) {
    if (!active) return;
    if (p.out2b) {
        const float f2 = p.out2_scale ? p.out2_scale[row] : 1.f;
        float o2[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) o2[v] = (acc[v] * p.beta2) * f2;
        bstore<VEC>(p.out2b + row * p.ldo2 + c, o2);
    }
    float o[VEC];
    if (p.H0) {
        float h0[VEC];
        fload<VEC>(h0, p.H0 + row * p.ldh0 + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] = fmaf(acc[v], p.beta, h0[v] * p.alpha);
    } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] = acc[v] * p.beta;
    }
    if (p.act == GNX_ACT_RELU) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] = fmaxf(o[v], 0.f);
    }
    if (p.out_scale) {
        const float os = p.out_scale[row];
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] *= os;
    }
    if (p.out_bf16) bstore<VEC>(static_cast<uint16_t *>(p.outv) + row * p.ldo + c, o);
    else fstore<VEC>(static_cast<float *>(p.outv) + row * p.ldo + c, o);
}

// ---- wide rows: one wave per row (k_spmm_wave_drop) ------------------------------------------------------------------------
template <int VEC, int U, int WPB, bool ENTRIES>
__global__ __launch_bounds__(64 * WPB) void k_spmm_wave_drop_bf16(const TbArgs p) {
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = p.slot0 + xcd_block(p) * WPB + wib;
    if (slot >= p.n_rows) return;
    const int64_t row = p.row_list ? (int64_t)__builtin_amdgcn_readfirstlane(p.row_list[slot]) : slot;
    const int64_t beg = p.rowptr[row], end = p.rowptr[row + 1];
    if (end - beg > p.long_row) return;
    if (p.skip_empty && beg == end) return;   // GNX_ACT_SKIP_EMPTY
    for (int c0 = 0; c0 < p.C; c0 += 64 * VEC) {
        const int c = c0 + lane * VEC;
        const bool active = c < p.C;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        wave_accumulate_drop_bf16<VEC, U, ENTRIES>(p, beg, end, active ? c : 0, lane, row, acc);
        epilogue_train_bf16<VEC>(p, row, c, active, acc);
    }
}

// ---- narrow rows: G lanes per row, G entries per round (k_spmm_group_drop: lane `sub` draws the weight of entry base + sub, the
// group walks the kept entries of the round in order, U gathers in flight) ------------------------------------------------------
template <int VEC, int G, int U, bool ENTRIES>
__global__ __launch_bounds__(256) void k_spmm_group_drop_bf16(const TbArgs p) {
    constexpr int RPB = 256 / G;
    const int sub = threadIdx.x % G;
    const int64_t slot = p.slot0 + xcd_block(p) * RPB + threadIdx.x / G;
    if (slot >= p.n_rows) return;
    const int64_t row = p.row_order ? (int64_t)p.row_order[slot] : slot;
    int64_t beg, end;
    if (p.slot_beg) { beg = p.slot_beg[slot]; end = beg + p.slot_cnt[slot]; }
    else { beg = p.rowptr[row]; end = p.rowptr[row + 1]; }
    if (end - beg > p.long_row) return;
    if (p.skip_empty && beg == end) return;   // GNX_ACT_SKIP_EMPTY
    for (int c0 = 0; c0 < p.C; c0 += G * VEC) {
        const int c = c0 + sub * VEC;
        const bool active = c < p.C;
        const uint16_t *__restrict__ Xc = p.Xb + (active ? c : 0);
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        for (int64_t base = beg; base < end; base += G) {
            const int n = (int)((end - base) < G ? (end - base) : G);
            int mycol = 0;
            float myw = 0.f;
            if (sub < n) {
                mycol = p.colidx[base + sub];
                myw = dropped_weight_at<ENTRIES>(p.fuse, p.vals[base + sub], base + sub, row, mycol);
            }
            const uint64_t all = __ballot(myw != 0.f);
            uint32_t keep = (uint32_t)(all >> ((threadIdx.x & 63) / G * G)) & (G == 32 ? 0xFFFFFFFFu : ((1u << G) - 1u));
            while (keep) {
                float x[U][VEC];
                float w[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (keep) {
                        const int idx = __builtin_ctz(keep);
                        keep &= keep - 1;
                        const int j = __shfl(mycol, idx, G);
                        w[u] = __shfl(myw, idx, G);
                        bload<VEC>(x[u], Xc + (int64_t)j * p.ldx);
                    } else {
                        w[u] = 0.f;
#pragma unroll
                        for (int v = 0; v < VEC; ++v) x[u][v] = 0.f;
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
            }
        }
        epilogue_train_bf16<VEC>(p, row, c, active, acc);
    }
}

// ---- long rows: f32 partial sums per chunk (k_spmm_long_partial_drop / _group_drop), added in chunk order by the reduce ----------
template <int VEC, int U, bool ENTRIES>
__global__ __launch_bounds__(256) void k_spmm_long_partial_drop_bf16(const TbArgs p) {
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t cslot = (int64_t)blockIdx.x * 4 + wib;
    if (cslot >= p.n_chunks) return;
    const int64_t chunk = p.chunk_order ? (int64_t)p.chunk_order[cslot] : cslot;
    const int32_t li = p.chunk_long[chunk];
    const int64_t row = p.long_rows[li];
    const int64_t beg = p.rowptr[row] + (chunk - p.long_chunk_ptr[li]) * p.long_chunk;
    const int64_t rend = p.rowptr[row + 1];
    const int64_t end = beg + p.long_chunk < rend ? beg + p.long_chunk : rend;
    for (int c0 = 0; c0 < p.C; c0 += 64 * VEC) {
        const int c = c0 + lane * VEC;
        const bool active = c < p.C;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        wave_accumulate_drop_bf16<VEC, U, ENTRIES>(p, beg, end, active ? c : 0, lane, row, acc);
        if (active) fstore<VEC>(p.partial + chunk * (int64_t)p.C + c, acc);
    }
}

// narrow long rows: the wave draws 64 weights per round (one per lane); sub-group s takes entries s, s + NS, ... of the round, then
// a fixed xor tree over the sub-groups
template <int VEC, int G, int U, bool ENTRIES>
__global__ __launch_bounds__(256) void k_spmm_long_partial_group_drop_bf16(const TbArgs p) {
    constexpr int NS = 64 / G;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t cslot = (int64_t)blockIdx.x * 4 + wib;
    if (cslot >= p.n_chunks) return;
    const int64_t chunk = p.chunk_order ? (int64_t)p.chunk_order[cslot] : cslot;
    const int32_t li = p.chunk_long[chunk];
    const int64_t row = p.long_rows[li];
    const int64_t beg = p.rowptr[row] + (chunk - p.long_chunk_ptr[li]) * p.long_chunk;
    const int64_t rend = p.rowptr[row + 1];
    const int64_t end = beg + p.long_chunk < rend ? beg + p.long_chunk : rend;
    const int sub = lane / G;
    const int c = (lane % G) * VEC;
    const bool active = c < p.C;
    const uint16_t *__restrict__ Xc = p.Xb + (active ? c : 0);
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
    for (int64_t base = beg; base < end; base += 64) {
        const int n = (int)((end - base) < 64 ? (end - base) : 64);
        int mycol = 0;
        float myw = 0.f;
        if (lane < n) {
            mycol = p.colidx[base + lane];
            myw = dropped_weight_at<ENTRIES>(p.fuse, p.vals[base + lane], base + lane, row, mycol);
        }
#pragma unroll 1
        for (int k = 0; k < G; k += U) {
            float x[U][VEC];
            float w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int src = sub + (k + u) * NS;                  // entry of the round this sub-group takes in slot k + u
                const int j = __shfl(mycol, src);
                w[u] = __shfl(myw, src);
                if (k + u < G && src < n && w[u] != 0.f) bload<VEC>(x[u], Xc + (int64_t)j * p.ldx);   // dropped: not gathered
                else {
                    w[u] = 0.f;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) x[u][v] = 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
        }
    }
#pragma unroll
    for (int off = G; off < 64; off <<= 1)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] += __shfl_xor(acc[v], off);
    if (sub == 0 && active) fstore<VEC>(p.partial + chunk * (int64_t)p.C + c, acc);
}

template <int VEC>
__global__ __launch_bounds__(256) void k_spmm_long_reduce_drop_bf16(const TbArgs p) {
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t li = (int64_t)blockIdx.x * 4 + wib;
    if (li >= p.n_long) return;
    const int64_t row = p.long_rows[li];
    const int64_t cb = p.long_chunk_ptr[li], ce = p.long_chunk_ptr[li + 1];
    for (int c0 = 0; c0 < p.C; c0 += 64 * VEC) {
        const int c = c0 + lane * VEC;
        const bool active = c < p.C;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        if (active) {
            for (int64_t k = cb; k < ce; ++k) {  // chunk order
                float x[VEC];
                fload<VEC>(x, p.partial + k * (int64_t)p.C + c);
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] += x[v];
            }
        }
        epilogue_train_bf16<VEC>(p, row, c, active, acc);
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
// (the row kernels go out through launch_row_pieces of gnx_spmm_device.h: pieces of at most 2^31 work-items, the XCD map padded)

// the names gnx_graph_last_kernel reports: the f32 training names with "_bf16" appended ("_entries_bf16" over a handle with duplicate
// entries), "+long" after the row class when hub rows went through the chunk kernels
enum RowClass { ROWS_NONE, ROWS_WAVE, ROWS_G32, ROWS_G16, ROWS_G8 };
const char *const kNames[2][2][5] = {
    {{"spmm_none_drop_bf16", "spmm_wave_drop_bf16", "spmm_group32_drop_bf16", "spmm_group16_drop_bf16", "spmm_group8_drop_bf16"},
     {"spmm_none_drop_entries_bf16", "spmm_wave_drop_entries_bf16", "spmm_group32_drop_entries_bf16", "spmm_group16_drop_entries_bf16",
      "spmm_group8_drop_entries_bf16"}},
    {{"spmm_none+long_drop_bf16", "spmm_wave+long_drop_bf16", "spmm_group32+long_drop_bf16", "spmm_group16+long_drop_bf16",
      "spmm_group8+long_drop_bf16"},
     {"spmm_none+long_drop_entries_bf16", "spmm_wave+long_drop_entries_bf16", "spmm_group32+long_drop_entries_bf16",
      "spmm_group16+long_drop_entries_bf16", "spmm_group8+long_drop_entries_bf16"}}};

template <int VEC, bool E>
RowClass launch_rows_tb(const TbArgs &p0, hipStream_t s) {
    TbArgs p = p0;
    const int lanes = (p.C + VEC - 1) / VEC;
    if (p.skip_empty && p.n_nonempty < p.n_rows) {            // as launch_rows_drop: the slots of the rows without entries are not launched
        if (lanes <= 32 && p.row_order != nullptr) p.n_rows = p.n_nonempty;
        else if (lanes > 32 && p.nonempty_rows != nullptr) { p.row_list = p.nonempty_rows; p.n_rows = p.n_nonempty; }
    }
    if (p.n_rows == 0) return ROWS_NONE;
    if (lanes > 32) {
        if (p.C <= 64 * VEC) launch_row_pieces(k_spmm_wave_drop_bf16<VEC, 8, 8, E>, p, 8, 512, s);
        else                 launch_row_pieces(k_spmm_wave_drop_bf16<VEC, 8, 4, E>, p, 4, 256, s);
        return ROWS_WAVE;
    }
    if (lanes > 16) { launch_row_pieces(k_spmm_group_drop_bf16<VEC, 32, 4, E>, p, 8, 256, s); return ROWS_G32; }
    if (lanes > 8)  { launch_row_pieces(k_spmm_group_drop_bf16<VEC, 16, 4, E>, p, 16, 256, s); return ROWS_G16; }
    launch_row_pieces(k_spmm_group_drop_bf16<VEC, 8, 4, E>, p, 32, 256, s);   // (up to 4 lanes as well: the extra lanes fetch and draw)
    return ROWS_G8;
}

template <int VEC, bool E>
void launch_long_tb(const TbArgs &p, hipStream_t s) {
    const int lanes = (p.C + VEC - 1) / VEC;
    if (lanes > 32)      GNX_LAUNCH((k_spmm_long_partial_drop_bf16<VEC, 8, E>), blocks_for(p.n_chunks, 4), p);
    else if (lanes > 16) GNX_LAUNCH((k_spmm_long_partial_group_drop_bf16<VEC, 32, 4, E>), blocks_for(p.n_chunks, 4), p);
    else if (lanes > 8)  GNX_LAUNCH((k_spmm_long_partial_group_drop_bf16<VEC, 16, 4, E>), blocks_for(p.n_chunks, 4), p);
    else if (lanes > 4)  GNX_LAUNCH((k_spmm_long_partial_group_drop_bf16<VEC, 8, 4, E>), blocks_for(p.n_chunks, 4), p);
    else                 GNX_LAUNCH((k_spmm_long_partial_group_drop_bf16<VEC, 4, 4, E>), blocks_for(p.n_chunks, 4), p);
    GNX_LAUNCH((k_spmm_long_reduce_drop_bf16<VEC>), blocks_for(p.n_long, 4), p);
}

template <int VEC, bool E>
const char *launch_tb(const TbArgs &p, hipStream_t s) {
    const RowClass rows = launch_rows_tb<VEC, E>(p, s);
    if (p.n_long > 0) launch_long_tb<VEC, E>(p, s);
    return kNames[p.n_long > 0][E][rows];
}

// widest per-lane vector every row start allows (8 bf16 = 16 bytes of X)
int pick_vec_tb(const TbArgs &p) {
    const size_t ob = p.out_bf16 ? 2 : 4;
    for (int vec = 8; vec > 1; vec >>= 1) {
        if (p.C % vec == 0 && p.ldx % vec == 0 && p.ldo % vec == 0 && (p.H0 == nullptr || p.ldh0 % vec == 0) &&
            (p.out2b == nullptr || p.ldo2 % vec == 0) && aligned(p.Xb, 2 * vec) && aligned(p.outv, std::min<size_t>(ob * vec, 16)) &&
            aligned(p.H0, std::min<size_t>(4 * vec, 16)) && aligned(p.out2b, 2 * vec))
            return vec;
    }
    return 1;
}

int launch_train_bf16(gnx_graph *g, const Csr &m, TbArgs &p, hipStream_t s) {
    p.rowptr = m.rowptr; p.colidx = m.colidx; p.n_rows = m.n_rows; p.n_nonempty = m.n_nonempty; p.nonempty_rows = m.nonempty_rows; p.row_list = nullptr;
    p.slot_beg = m.slot_beg; p.slot_cnt = m.slot_cnt;
    p.long_rows = m.long_rows; p.long_chunk_ptr = m.long_chunk_ptr; p.chunk_long = m.chunk_long;
    p.row_order = m.row_order;
    p.xcd_rows = m.order_window;
    p.chunk_order = m.chunk_order;
    p.tune = 0;
    p.n_long = m.n_long; p.n_chunks = m.n_chunks; p.long_row = m.long_row; p.long_chunk = m.long_chunk;
    p.partial = nullptr;
    p.skip_empty = (p.act & GNX_ACT_SKIP_EMPTY) != 0;
    p.act &= ~GNX_ACT_SKIP_EMPTY;
    if (m.n_rows == 0) return GNX_OK;
    if (m.n_long > 0) {      // (grows outside a capture only: GNX_ERR_UNSUPPORTED naming gnx_graph_reserve otherwise)
        int rc = ensure_partial(g, (size_t)m.n_chunks * (size_t)p.C * sizeof(float), s);
        if (rc != GNX_OK) return rc;
        p.partial = g->partial;
    }
    const int vec = pick_vec_tb(p);
    const char *name;
    if (p.fuse.mult) {
        if (vec == 8)      name = launch_tb<8, true>(p, s);
        else if (vec == 4) name = launch_tb<4, true>(p, s);
        else if (vec == 2) name = launch_tb<2, true>(p, s);
        else               name = launch_tb<1, true>(p, s);
    } else {
        if (vec == 8)      name = launch_tb<8, false>(p, s);
        else if (vec == 4) name = launch_tb<4, false>(p, s);
        else if (vec == 2) name = launch_tb<2, false>(p, s);
        else               name = launch_tb<1, false>(p, s);
    }
    g->last_kernel = name;
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

// the checks of both entries that need a handle: square stand-alone graphs, duplicates only with their entry tables
int check_handle(const char *fn, gnx_graph *g) {
    GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    if (g->blk_col_gid != nullptr) {
        set_error("%s: the handle is a vertex block (gnx_graph_set_block): bf16 training storage covers stand-alone graphs only -- "
                  "use the f32 entry", fn);
        return GNX_ERR_UNSUPPORTED;
    }
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "%s: needs a square stand-alone graph", fn);
    return refuse_duplicates(g, fn);
}

}  // namespace

extern "C" {

int gnx_spmm_dropped_chained_bf16(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                                  const float *d_D_next, const uint16_t *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0,
                                  float beta, float alpha, int act, void *d_out, int out_bf16, int64_t ldo, void *stream) {
    const char *fn = "gnx_spmm_dropped_chained_bf16";
    // the checks that need no handle come first (so that they can be exercised without a device)
    GNX_CHECK_ARG(C >= 1 && C <= (1 << 20), "%s: feature width %lld not in [1, 2^20]", fn, (long long)C);
    GNX_CHECK_ARG(d_X != nullptr && d_out != nullptr, "%s: NULL X/out", fn);
    GNX_CHECK_ARG(ldx >= C && ldo >= C && (d_H0 == nullptr || ldh0 >= C || ldh0 == 0), "%s: leading dimension smaller than C", fn);
    GNX_CHECK_ARG((const void *)d_X != (const void *)d_out, "%s: out must not alias X", fn);
    GNX_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1, "%s: out_bf16 must be 0 or 1", fn);
    GNX_CHECK_ARG((act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_NONE || (act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_RELU, "%s: invalid activation %d", fn, act);
    GNX_CHECK_ARG(d_D != nullptr, "%s: NULL degree scales", fn);
    GNX_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout rate %g outside [0, 1)", fn, (double)dropout_p);
    int rc = check_handle(fn, g);
    if (rc != GNX_OK) return rc;
    if (!g->a.empty_rows_unreferenced) act &= ~GNX_ACT_SKIP_EMPTY;       // honoured only when nobody gathers the rows it would leave untouched
    TbArgs p{};
    set_values(g, false, p);
    p.Xb = d_X; p.ldx = ldx; p.H0 = d_H0; p.ldh0 = ldh0; p.beta = beta; p.alpha = alpha; p.act = act;
    p.outv = d_out; p.out_bf16 = out_bf16; p.ldo = ldo; p.C = (int)C;
    p.out_scale = d_D_next;
    set_drop_fuse(g, dropout_p, seed, stream_id, d_D, 0, x_prescaled, p);
    return launch_train_bf16(g, g->a, p, (hipStream_t)stream);
}

int gnx_spmm_dropped_back_bf16(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                               const float *d_D_next, const uint16_t *d_X, int64_t ldx, int64_t C, const float *d_S_in, int64_t lds_in,
                               float s_alpha, float s_beta, float *d_S_out, int64_t lds_out, float y_beta, uint16_t *d_Y_out, int64_t ldy,
                               int act, void *stream) {
    const char *fn = "gnx_spmm_dropped_back_bf16";
    GNX_CHECK_ARG(C >= 1 && C <= (1 << 20), "%s: feature width %lld not in [1, 2^20]", fn, (long long)C);
    GNX_CHECK_ARG(d_X != nullptr && d_S_out != nullptr, "%s: NULL X/out", fn);
    GNX_CHECK_ARG(ldx >= C && lds_out >= C && (d_S_in == nullptr || lds_in >= C || lds_in == 0), "%s: leading dimension smaller than C", fn);
    GNX_CHECK_ARG((const void *)d_X != (const void *)d_S_out, "%s: out must not alias X", fn);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_SKIP_EMPTY, "%s: act must be GNX_ACT_NONE or GNX_ACT_SKIP_EMPTY", fn);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || (const void *)d_S_in == (const void *)d_S_out, "%s: GNX_ACT_SKIP_EMPTY needs the sum updated in place", fn);
    GNX_CHECK_ARG(d_D != nullptr && d_S_in != nullptr, "%s: NULL degree scales / running sum", fn);
    GNX_CHECK_ARG(d_Y_out == nullptr || (ldy >= C && (const void *)d_Y_out != (const void *)d_X && (const void *)d_Y_out != (const void *)d_S_out
                                         && (const void *)d_Y_out != (const void *)d_S_in),
                  "%s: the pre-scaled output needs a buffer of its own", fn);
    GNX_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout rate %g outside [0, 1)", fn, (double)dropout_p);
    int rc = check_handle(fn, g);
    if (rc != GNX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_transpose(g, s);
    if (rc != GNX_OK) return rc;
    if (!g->t.empty_rows_unreferenced) act = GNX_ACT_NONE;               // honoured only when nobody gathers the rows it would leave untouched
    TbArgs p{};
    set_values(g, true, p);
    p.Xb = d_X; p.ldx = ldx; p.H0 = d_S_in; p.ldh0 = lds_in; p.beta = s_beta; p.alpha = s_alpha; p.act = act;
    p.outv = d_S_out; p.out_bf16 = 0; p.ldo = lds_out; p.C = (int)C;
    p.out2b = d_Y_out; p.ldo2 = ldy; p.beta2 = y_beta; p.out2_scale = d_Y_out ? d_D_next : nullptr;
    set_drop_fuse(g, dropout_p, seed, stream_id, d_D, 1, x_prescaled, p);
    return launch_train_bf16(g, g->t, p, s);
}

}  // extern "C"
