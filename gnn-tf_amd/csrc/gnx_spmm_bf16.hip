// Opt-in bf16 feature storage for eval-mode propagation: the SpMM of gnx_spmm.hip with the GATHERED operand stored as bf16.
//
//   out[i,:] = act( beta * ( sum_j A[i,j] X~[j,:] + diag[i] X~[i,:] ) + alpha * H0[i,:] )
//
// X~ is bf16, widened exactly to f32 (a 16-bit shift) as it arrives; the sums, H0 and the epilogue are f32, and the result is
// rounded once (round to nearest even, NaN stays NaN: the plain cast, v_cvt_pk_bf16_f32) when the caller asks for a bf16 result.
// The propagation is bound by the random gathers of neighbour rows (profiles/NOTES.md): halving a gathered row halves the lines
// it moves (C = 128: 512 -> 256 bytes; C = 40 padded to 64: one 128-byte line instead of 160 bytes over two).
//
// The dispatch classes, their row orders and their summation orders are those of gnx_spmm.hip -- one wave per row for rows wider
// than 32 lanes, 32/16/8-lane groups below, long rows cut into chunks whose f32 partial sums a second kernel adds in chunk order
// (no float atomics: two calls give the same bits) -- with up to 8 bf16 (16 bytes) per lane: C = 128 runs on 16-lane groups.
// Every kernel here is its own (the f32 kernels and the helpers of gnx_spmm_device.h are not touched).
// gnx_spmm_rows_bf16 (the interior / boundary handles of a vertex block): SpmmArgs::out_rows / map_h0 send result row r to
// out[rows[r]] and mix H0[rows[r]] in every row class; with a null map a row is its own destination, as before.
#include "gnx_bf16_device.h"   // bload / bstore / fload / fstore (shared with gnx_spmm_train_bf16.hip)

namespace {

struct BfArgs : SpmmArgs {     // SpmmArgs::X / ::out stay null: the operand and the result are typed here
    const uint16_t *Xb;        // bf16 [rows, ldx]
    void *outv;                // f32 or bf16 [n_rows, ldo]
    int out_bf16;
};

// wave_accumulate (gnx_spmm_device.h) over bf16 rows: the same (col, val) fetch, v_readlane broadcast and entry order
template <int VEC, int U>
__device__ __forceinline__ void wave_accumulate_bf16(const int32_t *__restrict__ colidx, const float *__restrict__ vals,
                                                     const uint16_t *__restrict__ X, int64_t ldx, int64_t beg, int64_t end, int c,
                                                     int lane, float (&acc)[VEC]) {
    for (int64_t base = beg; base < end; base += 64) {
        const int n = (int)((end - base) < 64 ? (end - base) : 64);
        int mycol = 0;
        float myval = 0.f;
        if (lane < n) {
            mycol = colidx[base + lane];
            myval = vals[base + lane];
        }
        int i = 0;
        for (; i + U <= n; i += U) {
            float x[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) bload<VEC>(x[u], X + (int64_t)readlane_i(mycol, i + u) * ldx + c);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float w = readlane_f(myval, i + u);
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, x[u][v], acc[v]);
            }
        }
        if (i < n) {
            float x[U][VEC];
#pragma unroll
            for (int u = 0; u < U - 1; ++u)
                if (i + u < n) bload<VEC>(x[u], X + (int64_t)readlane_i(mycol, i + u) * ldx + c);
#pragma unroll
            for (int u = 0; u < U - 1; ++u) {
                if (i + u < n) {
                    const float w = readlane_f(myval, i + u);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w, x[u][v], acc[v]);
                }
            }
        }
    }
}

// epilogue_store of gnx_spmm_device.h: the diagonal term (from the bf16 row), the f32 mix, relu, one rounding if the result is bf16
template <int VEC>
__device__ __forceinline__ void epilogue_bf16(const BfArgs &p, int64_t row, int c, bool active, float (&acc)[VEC]) {
    if (!active) return;
    if (p.diag) {
        const float d = p.diag[row];
        float xr[VEC];
        bload<VEC>(xr, p.Xb + row * p.ldx + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = fmaf(d, xr[v], acc[v]);
    }
    float o[VEC];
    const int64_t orow = p.out_rows ? (int64_t)p.out_rows[row] : row;   // gnx_spmm_rows_bf16: the handle holds a subset of the output rows
    if (p.H0) {
        const int64_t hrow = p.map_h0 ? orow : row;                     // ... and H0 is indexed like the output
        float h0[VEC];
        fload<VEC>(h0, p.H0 + hrow * p.ldh0 + c);
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
    if (p.out_bf16) bstore<VEC>(static_cast<uint16_t *>(p.outv) + orow * p.ldo + c, o);
    else fstore<VEC>(static_cast<float *>(p.outv) + orow * p.ldo + c, o);
}

// ---- wide rows: one wave per row ----------------------------------------------------------------
template <int VEC, int U, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_spmm_wave_bf16(const BfArgs p) {
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = p.slot0 + xcd_block(p) * WPB + wib;
    if (slot >= p.n_rows) return;
    const int64_t row = p.row_list ? (int64_t)__builtin_amdgcn_readfirstlane(p.row_list[slot]) : slot;
    const int64_t beg = p.rowptr[row], end = p.rowptr[row + 1];
    if (end - beg > p.long_row) return;
    if (p.skip_empty && beg == end) return;
    for (int c0 = 0; c0 < p.C; c0 += 64 * VEC) {
        const int c = c0 + lane * VEC;
        const bool active = c < p.C;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        wave_accumulate_bf16<VEC, U>(p.colidx, p.vals, p.Xb, p.ldx, beg, end, active ? c : 0, lane, acc);
        epilogue_bf16<VEC>(p, row, c, active, acc);
    }
}

// ---- narrow rows: G lanes per row, degree-binned slots (group_rows of gnx_spmm.hip, U entries in flight per lane) ----------
template <int VEC, int G, int U>
__device__ __forceinline__ void group_rows_bf16(const BfArgs &p, int64_t block) {
    constexpr int RPB = 256 / G;
    const int sub = threadIdx.x % G;
    const int64_t slot = p.slot0 + block * RPB + threadIdx.x / G;
    if (slot >= p.n_rows) return;
    const int64_t row = p.row_order ? (int64_t)p.row_order[slot] : slot;
    int64_t beg, end;
    if (p.slot_beg) { beg = p.slot_beg[slot]; end = beg + p.slot_cnt[slot]; }
    else { beg = p.rowptr[row]; end = p.rowptr[row + 1]; }
    if (end - beg > p.long_row) return;
    if (p.skip_empty && beg == end) return;
    for (int c0 = 0; c0 < p.C; c0 += G * VEC) {
        const int c = c0 + sub * VEC;
        const bool active = c < p.C;
        const uint16_t *__restrict__ Xc = p.Xb + (active ? c : 0);
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        for (int64_t e = beg; e < end; e += U) {
            float x[U][VEC];
            float w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (e + u < end) {
                    w[u] = p.vals[e + u];
                    bload<VEC>(x[u], Xc + (int64_t)p.colidx[e + u] * p.ldx);
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
        epilogue_bf16<VEC>(p, row, c, active, acc);
    }
}

// G <= 8: the cooperative (col, val) fetch of group_rows_coop (gnx_spmm.hip): lane `sub` loads entry base + sub, the group reads
// the pairs out of each other's registers, the next batch's pairs are fetched behind the gathers; entries in ascending order
template <int VEC, int G, int B>
__device__ __forceinline__ void group_rows_coop_bf16(const BfArgs &p, int64_t block) {
    constexpr int RPB = 256 / G;
    const int sub = threadIdx.x % G;
    const int64_t slot = p.slot0 + block * RPB + threadIdx.x / G;
    if (slot >= p.n_rows) return;
    const int64_t row = p.row_order ? (int64_t)p.row_order[slot] : slot;
    int64_t beg, end;
    if (p.slot_beg) { beg = p.slot_beg[slot]; end = beg + p.slot_cnt[slot]; }
    else { beg = p.rowptr[row]; end = p.rowptr[row + 1]; }
    if (end - beg > p.long_row) return;
    if (p.skip_empty && beg == end) return;
    for (int c0 = 0; c0 < p.C; c0 += G * VEC) {
        const int c = c0 + sub * VEC;
        const bool active = c < p.C;
        const uint16_t *__restrict__ Xc = p.Xb + (active ? c : 0);
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        int myj = -1;
        float myw = 0.f;
        if (sub < B && beg + sub < end) { myj = p.colidx[beg + sub]; myw = p.vals[beg + sub]; }
        for (int64_t e = beg; e < end; e += B) {
            float x[B][VEC];
            float w[B];
#pragma unroll
            for (int u = 0; u < B; ++u) {
                const int j = __shfl(myj, u, G);
                w[u] = __shfl(myw, u, G);
                if (j >= 0) bload<VEC>(x[u], Xc + (int64_t)j * p.ldx);
                else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) x[u][v] = 0.f;
                }
            }
            myj = -1; myw = 0.f;
            if (sub < B && e + B + sub < end) { myj = p.colidx[e + B + sub]; myw = p.vals[e + B + sub]; }
#pragma unroll
            for (int u = 0; u < B; ++u)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
        }
        epilogue_bf16<VEC>(p, row, c, active, acc);
    }
}

template <int VEC, int G>
__global__ __launch_bounds__(256) void k_spmm_group_bf16(const BfArgs p) {
    if (G <= 8) group_rows_coop_bf16<VEC, G, 4>(p, xcd_block(p));
    else group_rows_bf16<VEC, G, 4>(p, xcd_block(p));
}

// ---- long rows: f32 partial sums per chunk, added in chunk order by k_spmm_long_reduce_bf16 ------------------------------
template <int VEC, int U>
__global__ __launch_bounds__(256) void k_spmm_long_partial_bf16(const BfArgs p) {
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
        wave_accumulate_bf16<VEC, U>(p.colidx, p.vals, p.Xb, p.ldx, beg, end, active ? c : 0, lane, acc);
        if (active) fstore<VEC>(p.partial + chunk * (int64_t)p.C + c, acc);
    }
}

// narrow rows: a chunk's entries dealt round-robin to the wave's 64/G sub-groups, then a fixed xor tree (long_chunks_group)
template <int VEC, int G, int U>
__device__ __forceinline__ void long_chunks_group_bf16(const BfArgs &p, int64_t block) {
    constexpr int NS = 64 / G;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t cslot = block * 4 + wib;
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
    for (int64_t e = beg + sub; e < end; e += (int64_t)NS * U) {
        float x[U][VEC];
        float w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t eu = e + (int64_t)u * NS;
            if (eu < end) {
                w[u] = p.vals[eu];
                bload<VEC>(x[u], Xc + (int64_t)p.colidx[eu] * p.ldx);
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
#pragma unroll
    for (int off = G; off < 64; off <<= 1)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] += __shfl_xor(acc[v], off);
    if (sub == 0 && active) fstore<VEC>(p.partial + chunk * (int64_t)p.C + c, acc);
}

template <int VEC, int G>
__global__ __launch_bounds__(256) void k_spmm_long_partial_group_bf16(const BfArgs p) {
    long_chunks_group_bf16<VEC, G, 4>(p, blockIdx.x);
}

template <int VEC>
__global__ __launch_bounds__(256) void k_spmm_long_reduce_bf16(const BfArgs p) {
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
        epilogue_bf16<VEC>(p, row, c, active, acc);
    }
}

// small structures: the chunks and the short rows in one launch (k_spmm_group_and_chunks of gnx_spmm.hip)
template <int VEC, int G>
__global__ __launch_bounds__(256) void k_spmm_group_and_chunks_bf16(const BfArgs p, int chunk_blocks) {
    if ((int)blockIdx.x < chunk_blocks) long_chunks_group_bf16<VEC, G, 4>(p, blockIdx.x);
    else if (G <= 8) group_rows_coop_bf16<VEC, G, 4>(p, (int64_t)blockIdx.x - chunk_blocks);
    else group_rows_bf16<VEC, G, 4>(p, (int64_t)blockIdx.x - chunk_blocks);
}

// f32 -> bf16, any leading dimensions; VEC = 4 when every row start is 16-byte (src) / 8-byte (dst) aligned
template <int VEC>
__global__ __launch_bounds__(256) void k_cast_bf16(const float *__restrict__ src, int64_t lds, int64_t n_rows, int64_t C,
                                                  uint16_t *__restrict__ dst, int64_t ldd) {
    const int64_t per_row = C / VEC, total = n_rows * per_row, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t r = e / per_row, c = (e % per_row) * VEC;
        float x[VEC];
        vload<VEC>(x, src + r * lds + c);
        bstore<VEC>(dst + r * ldd + c, x);
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
// (the row kernels go out through launch_row_pieces of gnx_spmm_device.h: pieces of at most 2^31 work-items, the XCD map padded)

// dispatch classes of the short rows (launch_rows of gnx_spmm.hip); the names gnx_graph_last_kernel reports, "+long" when hub rows
// went through the chunk kernels
enum RowClass { ROWS_NONE, ROWS_WAVE, ROWS_G32, ROWS_G16, ROWS_G8 };
const char *const kRowNames[2][5] = {
    {"spmm_none_bf16", "spmm_wave_bf16", "spmm_group32_bf16", "spmm_group16_bf16", "spmm_group8_bf16"},
    {"spmm_none+long_bf16", "spmm_wave+long_bf16", "spmm_group32+long_bf16", "spmm_group16+long_bf16", "spmm_group8+long_bf16"}};

template <int VEC>
RowClass launch_rows_bf16(const BfArgs &p0, hipStream_t s) {
    BfArgs p = p0;
    const int lanes = (p.C + VEC - 1) / VEC;
    // GNX_ACT_SKIP_EMPTY: the group kernels do not launch the trailing (empty) slots of row_order, the wave kernel walks the
    // ascending list of the rows with entries
    if (lanes <= 32 && p.skip_empty && p.row_order != nullptr && p.n_nonempty < p.n_rows) p.n_rows = p.n_nonempty;
    if (lanes > 32 && p.skip_empty && p.nonempty_rows != nullptr && p.n_nonempty < p.n_rows) { p.row_list = p.nonempty_rows; p.n_rows = p.n_nonempty; }
    if (p.n_rows == 0) return ROWS_NONE;
    if (lanes > 32) {
        if (p.C <= 64 * VEC) launch_row_pieces(k_spmm_wave_bf16<VEC, 8, 8>, p, 8, 512, s);
        else                 launch_row_pieces(k_spmm_wave_bf16<VEC, 8, 4>, p, 4, 256, s);
        return ROWS_WAVE;
    }
    if (lanes > 16) { launch_row_pieces(k_spmm_group_bf16<VEC, 32>, p, 8, 256, s); return ROWS_G32; }
    if (lanes > 8)  { launch_row_pieces(k_spmm_group_bf16<VEC, 16>, p, 16, 256, s); return ROWS_G16; }
    launch_row_pieces(k_spmm_group_bf16<VEC, 8>, p, 32, 256, s);   // (up to 4 lanes as well: the extra lanes share the index fetch)
    return ROWS_G8;
}

template <int VEC>
const char *launch_rows_and_chunks_bf16(const BfArgs &p, hipStream_t s) {
    const int lanes = (p.C + VEC - 1) / VEC;
    if (lanes > 32 || p.n_long == 0 || p.n_rows >= SMALL_ROWS) return nullptr;
    const unsigned cb = blocks_for(p.n_chunks, 4);
    const char *name;
#define GNX_BOTH_BF16(G, RPB_) \
    hipLaunchKernelGGL((k_spmm_group_and_chunks_bf16<VEC, G>), dim3(cb + blocks_for(p.n_rows, RPB_)), dim3(256), 0, s, p, (int)cb)
    if (lanes > 16)     { GNX_BOTH_BF16(32, 8); name = "spmm_group32+chunks_bf16"; }
    else if (lanes > 8) { GNX_BOTH_BF16(16, 16); name = "spmm_group16+chunks_bf16"; }
    else if (lanes > 4) { GNX_BOTH_BF16(8, 32); name = "spmm_group8+chunks_bf16"; }
    else                { GNX_BOTH_BF16(4, 64); name = "spmm_group4+chunks_bf16"; }
#undef GNX_BOTH_BF16
    GNX_LAUNCH((k_spmm_long_reduce_bf16<VEC>), blocks_for(p.n_long, 4), p);
    return name;
}

template <int VEC>
void launch_long_bf16(const BfArgs &p, hipStream_t s) {
    const int lanes = (p.C + VEC - 1) / VEC;
    if (lanes > 32)      GNX_LAUNCH((k_spmm_long_partial_bf16<VEC, 8>), blocks_for(p.n_chunks, 4), p);
    else if (lanes > 16) GNX_LAUNCH((k_spmm_long_partial_group_bf16<VEC, 32>), blocks_for(p.n_chunks, 4), p);
    else if (lanes > 8)  GNX_LAUNCH((k_spmm_long_partial_group_bf16<VEC, 16>), blocks_for(p.n_chunks, 4), p);
    else if (lanes > 4)  GNX_LAUNCH((k_spmm_long_partial_group_bf16<VEC, 8>), blocks_for(p.n_chunks, 4), p);
    else                 GNX_LAUNCH((k_spmm_long_partial_group_bf16<VEC, 4>), blocks_for(p.n_chunks, 4), p);
    GNX_LAUNCH((k_spmm_long_reduce_bf16<VEC>), blocks_for(p.n_long, 4), p);
}

template <int VEC>
const char *launch_bf16(const BfArgs &p, hipStream_t s) {
    if (const char *name = launch_rows_and_chunks_bf16<VEC>(p, s)) return name;
    const RowClass rows = launch_rows_bf16<VEC>(p, s);
    if (p.n_long > 0) launch_long_bf16<VEC>(p, s);
    return kRowNames[p.n_long > 0][rows];
}

// widest per-lane vector every row start allows (8 bf16 = 16 bytes of X)
int pick_vec_bf16(const BfArgs &p) {
    const size_t ob = p.out_bf16 ? 2 : 4;
    for (int vec = 8; vec > 1; vec >>= 1) {
        if (p.C % vec == 0 && p.ldx % vec == 0 && p.ldo % vec == 0 && (p.H0 == nullptr || p.ldh0 % vec == 0) &&
            aligned(p.Xb, 2 * vec) && aligned(p.outv, std::min<size_t>(ob * vec, 16)) && aligned(p.H0, std::min<size_t>(4 * vec, 16)))
            return vec;
    }
    return 1;
}

int launch_spmm_bf16(gnx_graph *g, const Csr &m, BfArgs &p, hipStream_t s) {
    p.rowptr = m.rowptr; p.colidx = m.colidx; p.n_rows = m.n_rows; p.n_nonempty = m.n_nonempty; p.nonempty_rows = m.nonempty_rows; p.row_list = nullptr;
    p.slot_beg = m.slot_beg; p.slot_cnt = m.slot_cnt;
    p.long_rows = m.long_rows; p.long_chunk_ptr = m.long_chunk_ptr; p.chunk_long = m.chunk_long;
    p.row_order = m.row_order;
    p.xcd_rows = m.order_window;
    p.chunk_order = m.chunk_order;
    p.tune = 0;
    p.n_long = m.n_long; p.n_chunks = m.n_chunks; p.long_row = m.long_row; p.long_chunk = m.long_chunk;
    p.partial = nullptr;
    p.skip_empty = (p.act & GNX_ACT_SKIP_EMPTY) != 0 && p.diag == nullptr;
    p.act &= ~GNX_ACT_SKIP_EMPTY;
    if (m.n_rows == 0) return GNX_OK;
    if (m.n_long > 0) {
        int rc = ensure_partial(g, (size_t)m.n_chunks * (size_t)p.C * sizeof(float), s);
        if (rc != GNX_OK) return rc;
        p.partial = g->partial;
    }
    const int vec = pick_vec_bf16(p);
    const char *name;
    if (vec == 8)      name = launch_bf16<8>(p, s);
    else if (vec == 4) name = launch_bf16<4>(p, s);
    else if (vec == 2) name = launch_bf16<2>(p, s);
    else               name = launch_bf16<1>(p, s);
    g->last_kernel = name;
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int cast_bf16(const float *src, int64_t n_rows, int64_t C, int64_t lds, uint16_t *dst, int64_t ldd, hipStream_t s) {
    if (n_rows == 0) return GNX_OK;
    const bool v4 = C % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && aligned(src, 16) && aligned(dst, 8);
    const int64_t items = n_rows * (v4 ? C / 4 : C);
    const unsigned grid = (unsigned)std::min<int64_t>(blocks_for(items, 256), 1 << 20);
    if (v4) hipLaunchKernelGGL(k_cast_bf16<4>, dim3(grid), dim3(256), 0, s, src, lds, n_rows, C, dst, ldd);
    else    hipLaunchKernelGGL(k_cast_bf16<1>, dim3(grid), dim3(256), 0, s, src, lds, n_rows, C, dst, ldd);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

}  // namespace

extern "C" {

int gnx_cast_bf16(const float *d_src, int64_t n_rows, int64_t C, int64_t lds, uint16_t *d_dst, int64_t ldd, void *stream) {
    GNX_CHECK_ARG(n_rows >= 0, "gnx_cast_bf16: negative row count");
    GNX_CHECK_ARG(C >= 1 && C <= (1 << 20), "gnx_cast_bf16: feature width %lld not in [1, 2^20]", (long long)C);
    GNX_CHECK_ARG(lds >= C && ldd >= C, "gnx_cast_bf16: leading dimension smaller than C");
    GNX_CHECK_ARG(n_rows == 0 || (d_src != nullptr && d_dst != nullptr), "gnx_cast_bf16: NULL buffer");
    GNX_CHECK_ARG(n_rows == 0 || (const void *)d_src != (const void *)d_dst, "gnx_cast_bf16: dst must not alias src");
    return cast_bf16(d_src, n_rows, C, lds, d_dst, ldd, (hipStream_t)stream);
}

int gnx_spmm_bf16(gnx_graph_t g, const float *d_vals, const float *d_diag, const uint16_t *d_X, int64_t ldx, int64_t C,
                  const float *d_H0, int64_t ldh0, float beta, float alpha, int act, void *d_out, int out_bf16, int64_t ldo,
                  void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_spmm_bf16: NULL handle");
    GNX_CHECK_ARG(C >= 1 && C <= (1 << 20), "gnx_spmm_bf16: feature width %lld not in [1, 2^20]", (long long)C);
    GNX_CHECK_ARG(d_X != nullptr && d_out != nullptr, "gnx_spmm_bf16: NULL X/out");
    GNX_CHECK_ARG(ldx >= C && ldo >= C && (d_H0 == nullptr || ldh0 >= C || ldh0 == 0), "gnx_spmm_bf16: leading dimension smaller than C");
    GNX_CHECK_ARG((const void *)d_X != d_out, "gnx_spmm_bf16: out must not alias X");
    GNX_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1, "gnx_spmm_bf16: out_bf16 must be 0 or 1");
    GNX_CHECK_ARG((act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_NONE || (act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_RELU, "gnx_spmm_bf16: invalid activation %d", act);
    GNX_CHECK_ARG(d_diag == nullptr || g->a.n_rows == g->a.n_cols, "gnx_spmm_bf16: diag needs a square graph");
    BfArgs p{};
    p.vals = d_vals ? d_vals : g->raw_vals;
    p.diag = d_diag; p.Xb = d_X; p.ldx = ldx; p.H0 = d_H0; p.ldh0 = ldh0; p.beta = beta; p.alpha = alpha; p.act = act;
    p.outv = d_out; p.out_bf16 = out_bf16; p.ldo = ldo; p.C = (int)C;
    return launch_spmm_bf16(g, g->a, p, (hipStream_t)stream);
}

int gnx_spmm_rows_bf16(gnx_graph_t g, const float *d_vals, const uint16_t *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0,
                       float beta, float alpha, int act, const int32_t *d_rows, void *d_out, int out_bf16, int64_t ldo, void *stream) {
    GNX_CHECK_ARG(g != nullptr, "gnx_spmm_rows_bf16: NULL handle");
    GNX_CHECK_ARG(C >= 1 && C <= (1 << 20), "gnx_spmm_rows_bf16: feature width %lld not in [1, 2^20]", (long long)C);
    GNX_CHECK_ARG(d_X != nullptr && d_out != nullptr, "gnx_spmm_rows_bf16: NULL X/out");
    GNX_CHECK_ARG(ldx >= C && ldo >= C && (d_H0 == nullptr || ldh0 >= C || ldh0 == 0), "gnx_spmm_rows_bf16: leading dimension smaller than C");
    GNX_CHECK_ARG((const void *)d_X != d_out, "gnx_spmm_rows_bf16: out must not alias X");
    GNX_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1, "gnx_spmm_rows_bf16: out_bf16 must be 0 or 1");
    GNX_CHECK_ARG((act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_NONE || (act & ~GNX_ACT_SKIP_EMPTY) == GNX_ACT_RELU, "gnx_spmm_rows_bf16: invalid activation %d", act);
    GNX_CHECK_ARG(d_rows != nullptr || g->a.n_rows == 0, "gnx_spmm_rows_bf16: NULL row map");
    BfArgs p{};
    p.vals = d_vals ? d_vals : g->raw_vals;
    p.Xb = d_X; p.ldx = ldx; p.H0 = d_H0; p.ldh0 = ldh0; p.beta = beta; p.alpha = alpha; p.act = act;
    p.outv = d_out; p.out_bf16 = out_bf16; p.ldo = ldo; p.C = (int)C; p.out_rows = d_rows; p.map_h0 = true;
    return launch_spmm_bf16(g, g->a, p, (hipStream_t)stream);
}

int gnx_appnp_propagate_bf16(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_H0, float a, int K, int64_t C,
                             int act, float *d_out, uint16_t *d_work, void *stream) {
    // the checks that need no handle come first (so that they can be exercised without a device)
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "gnx_appnp_propagate_bf16: invalid activation %d", act);
    GNX_CHECK_ARG(K >= 0, "gnx_appnp_propagate_bf16: negative iteration count");
    GNX_CHECK_ARG(C >= 1 && C <= (1 << 20), "gnx_appnp_propagate_bf16: feature width %lld not in [1, 2^20]", (long long)C);
    GNX_CHECK_ARG(d_H0 && d_out && (K < 1 || d_work), "gnx_appnp_propagate_bf16: NULL buffer");
    GNX_CHECK_ARG((const void *)d_out != (const void *)d_H0 && (const void *)d_work != (const void *)d_H0 && (const void *)d_out != (const void *)d_work,
                  "gnx_appnp_propagate_bf16: H0, out and work must be distinct");
    GNX_CHECK_ARG(g != nullptr, "gnx_appnp_propagate_bf16: NULL handle");
    GNX_CHECK_ARG(g->a.n_rows == g->a.n_cols, "gnx_appnp_propagate_bf16: needs a square graph");
    const int64_t n = g->a.n_rows;
    hipStream_t s = (hipStream_t)stream;
    if (K == 0) {
        GNX_HIP(hipMemcpyAsync(d_out, d_H0, (size_t)n * C * sizeof(float), hipMemcpyDeviceToDevice, s));
        return GNX_OK;
    }
    // H~_0 = bf(H0) into the first half of d_work; iteration k < K-1 writes bf(H_{k+1}) into the other half, the last one f32 H_K
    uint16_t *buf[2] = {d_work, d_work + n * C};
    int rc = cast_bf16(d_H0, n, C, C, buf[0], C, s);
    if (rc != GNX_OK) return rc;
    for (int k = 0; k < K; ++k) {
        const bool last = k == K - 1;
        // rows without entries are act(a * H0) after every iteration: buf[1] has them after k = 0, buf[0] after k = 1 (it held
        // bf(H0) before); when nobody gathers them (empty_rows_unreferenced) the work buffers never need them at all.  The
        // last iteration writes every row of d_out.
        const bool settled = !last && (k >= 2 || g->a.empty_rows_unreferenced);
        BfArgs p{};
        p.vals = d_vals ? d_vals : g->raw_vals;
        p.diag = d_diag; p.Xb = buf[k % 2]; p.ldx = C; p.H0 = d_H0; p.ldh0 = C; p.beta = (float)(1.0 - (double)a); p.alpha = a;
        p.act = (settled && d_diag == nullptr) ? (act | GNX_ACT_SKIP_EMPTY) : act;
        p.outv = last ? (void *)d_out : (void *)buf[(k + 1) % 2]; p.out_bf16 = last ? 0 : 1; p.ldo = C; p.C = (int)C;
        rc = launch_spmm_bf16(g, g->a, p, s);
        if (rc != GNX_OK) return rc;
    }
    return GNX_OK;
}

}  // extern "C"
