// The eval-mode dispatch classes of the SpMM, each written once over the row-storage policy R (gnx_spmm_device.h) and instantiated for
// f32 rows by gnx_spmm.hip and for bf16 rows by gnx_spmm_bf16.hip, and the launcher layer that picks among them.  The design notes
// are at the top of gnx_spmm.hip.
#pragma once
#include "gnx_spmm_device.h"

namespace {

// ---- wide path: one wave per row -----------------------------------------------------------
// tune bits (GNX_TUNE, experiments): 1 = degree-binned row order (f32 rows only: R::EXPERIMENTS)
// HINT, here and in every kernel below: p.colidx holds the handle's hinted columns and a cold row is gathered non-temporally
// (gnx_spmm_device.h, hinted gathers); false = the kernel as it always was.
template <typename R, int VEC, int U, int WPB, bool HINT = false>
__global__ __launch_bounds__(64 * WPB) void k_spmm_wave(const typename R::Args p) {
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tune = R::EXPERIMENTS ? p.tune : 0;
    const int64_t slot = p.slot0 + xcd_block(p) * WPB + wib;
    if (slot >= p.n_rows) return;
    const auto [row, beg, end] = slot_row<true>(p, slot, (tune & 1) != 0);
    if (end - beg > p.long_row) return;       // the chunk kernels take it
    if (p.skip_empty && beg == end) return;   // GNX_ACT_SKIP_EMPTY: the row already holds alpha * H0, or a later launch writes it
    for (int c0 = 0; c0 < p.C; c0 += 64 * VEC) {
        const int c = c0 + lane * VEC;
        const bool active = c < p.C;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        wave_accumulate<R, VEC, U, false, false, false, HINT>(p.colidx, p.vals, R::X(p), p.ldx, beg, end, active ? c : 0, lane, acc);
        epilogue_store<R, VEC>(p, row, c, active, acc);
    }
}

// ---- narrow path: G lanes per row, 256/G rows per block ---------------------------------------
// PIPE: the (col, val) pairs of batch b+1 are fetched while the gathers of batch b are in flight.
// PEND, here and in long_chunks_group: the launch elides the handle's pendant rows (IS_PEND: the policy whose arguments are PendArgs).
template <typename R, int VEC, int G, int U, bool PIPE, bool HINT = false>
__device__ __forceinline__ void group_rows(const typename R::Args &p, int64_t block) {
    constexpr bool PEND = IS_PEND<R>;
    constexpr int RPB = 256 / G;
    const int sub = threadIdx.x % G;
    const int64_t slot = p.slot0 + block * RPB + threadIdx.x / G;
    if (slot >= p.n_rows) return;
    const auto [row, beg, end] = slot_row<false>(p, slot);
    if (end - beg > p.long_row) return;       // the chunk kernels take it
    if (p.skip_empty && beg == end) return;   // GNX_ACT_SKIP_EMPTY: the row already holds alpha * H0, or a later launch writes it
    if constexpr (PEND) {
        if (slot >= p.skip_beg && slot < p.skip_end) return;   // an elidable row: only the last iteration computes it
    }
    for (int c0 = 0; c0 < p.C; c0 += G * VEC) {
        const int c = c0 + sub * VEC;
        const bool active = c < p.C;
        const typename R::Elem *__restrict__ Xc = R::X(p) + (active ? c : 0);
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        if constexpr (PEND) {
            static_assert(HINT && VEC == 4 && !PIPE && G >= 16, "pendant elision: the hinted sub-wave kernels");
            // the row's own values of two iterations ago, read before this lane overwrites them (P may be the destination buffer)
            float prev[VEC] = {0.f, 0.f, 0.f, 0.f};
            if (p.pend_slot_mark[slot] && !p.pend_raw) vload<VEC>(prev, p.P + row * p.ldp + (active ? c : 0));
            const float *H0c = p.H0 + (active ? c : 0);
            for (int64_t e = beg; e < end; e += U) {   // the batches of the hinted form
                int j[U];
                float w[U], pw[U];
                f32x4 x[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool ok = e + u < end;
                    j[u] = ok ? p.colidx[e + u] : HINT_NONE;
                    w[u] = ok ? p.vals[e + u] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t col = j[u] & PEND_COL_MASK;
                    const bool pend = pend_col(j[u]);
                    x[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                    gather16_hinted(x[u], pend ? H0c + col * p.ldh0 : Xc + col * p.ldx, j[u]);
                    pw[u] = pend ? p.pend_w[col] : 0.f;
                }
                gather_wait<U>(x);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (pend_col(j[u]) && !p.pend_raw) {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) x[u][v] = pendant_iterate(pw[u], prev[v], x[u][v], p.beta, p.alpha, p.act);
                    }
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
                }
            }
        } else if constexpr (HINT) {
            static_assert(VEC == 4 && !PIPE && std::is_same_v<typename R::Elem, float>, "hinted gathers: f32 rows, 16 bytes per lane");
            for (int64_t e = beg; e < end; e += U) {   // the batches of the plain form; an entry past the row's end loads nothing
                int j[U];
                float w[U];
                f32x4 x[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool ok = e + u < end;
                    j[u] = ok ? p.colidx[e + u] : HINT_NONE;
                    w[u] = ok ? p.vals[e + u] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    x[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                    gather16_hinted(x[u], Xc + (int64_t)hint_col(j[u]) * p.ldx, j[u]);
                }
                gather_wait<U>(x);
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
            }
        } else if (PIPE) {
            int jn[U];
            float wn[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool ok = beg + u < end;
                jn[u] = ok ? p.colidx[beg + u] : -1;
                wn[u] = ok ? p.vals[beg + u] : 0.f;
            }
            for (int64_t e = beg; e < end; e += U) {
                float x[U][VEC];
                float w[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {          // gathers of this batch
                    w[u] = wn[u];
                    if (jn[u] >= 0) R::template load<VEC>(x[u], Xc + (int64_t)jn[u] * p.ldx);
                    else {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) x[u][v] = 0.f;
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {          // indices of the next batch, behind the gathers
                    const bool ok = e + U + u < end;
                    jn[u] = ok ? p.colidx[e + U + u] : -1;
                    wn[u] = ok ? p.vals[e + U + u] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
            }
        } else {
            for (int64_t e = beg; e < end; e += U) {   // U entries in flight per lane, ragged tail predicated
                float x[U][VEC];
                float w[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (e + u < end) {
                        const int j = p.colidx[e + u];
                        w[u] = p.vals[e + u];
                        R::template load<VEC>(x[u], Xc + (int64_t)j * p.ldx);
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
        epilogue_store<R, VEC>(p, row, c, active, acc);
    }
}

// The same rows with a COOPERATIVE index fetch, for the narrow groups (G <= 8 lanes per row, C <= 32).  In group_rows every lane of a
// row's group loads the same (col, val) pair, so a step of four entries costs four index loads + four value loads + four gathers
// per lane: twelve vector-memory instructions, each served line by line by the CU's L1 pipe (sixteen different lines per wave
// instruction).  At narrow widths that pipe is what a launch waits for next to the fabric (SQ counters at C = 8: 60 % of the
// wave cycles are issue stalls, the TCP is busy for the whole launch; with every gather made to hit, a launch still takes 57 %
// of its time -- profiles/notes/r03_narrow_*).  Here lane `sub` of the group loads the pair of entry base + sub -- ONE index
// load and one value load per four entries -- and the group reads them out of each other's registers (ds_bpermute, off the memory
// pipe); the next batch's pairs are fetched behind the gathers.  Entries are added in ascending order as before: same bits.
// Measured (RMAT 10M / 100M, K = 10): C = 8 17.2 -> 16.4 ms, C = 16 19.5 -> 19.0, C = 32 22.2 -> 21.9; the all-gathers-hit floor
// 9.8 -> 7.6 ms at C = 8.  The wider groups LOSE 2-4 % with it (their gathers dominate the pipe, the shuffles only add latency).
template <typename R, int VEC, int G, int B>
__device__ __forceinline__ void group_rows_coop(const typename R::Args &p, int64_t block) {
    constexpr int RPB = 256 / G;
    const int sub = threadIdx.x % G;
    const int64_t slot = p.slot0 + block * RPB + threadIdx.x / G;
    if (slot >= p.n_rows) return;
    const auto [row, beg, end] = slot_row<false>(p, slot);
    if (end - beg > p.long_row) return;       // the chunk kernels take it
    if (p.skip_empty && beg == end) return;   // GNX_ACT_SKIP_EMPTY: the row already holds alpha * H0, or a later launch writes it
    for (int c0 = 0; c0 < p.C; c0 += G * VEC) {
        const int c = c0 + sub * VEC;
        const bool active = c < p.C;
        const typename R::Elem *__restrict__ Xc = R::X(p) + (active ? c : 0);
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
            for (int u = 0; u < B; ++u) {                                   // gathers of this batch
                const int j = __shfl(myj, u, G);
                w[u] = __shfl(myw, u, G);
                if (j >= 0) R::template load<VEC>(x[u], Xc + (int64_t)j * p.ldx);
                else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) x[u][v] = 0.f;
                }
            }
            myj = -1; myw = 0.f;                                            // pairs of the next batch, behind the gathers
            if (sub < B && e + B + sub < end) { myj = p.colidx[e + B + sub]; myw = p.vals[e + B + sub]; }
#pragma unroll
            for (int u = 0; u < B; ++u)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
        }
        epilogue_store<R, VEC>(p, row, c, active, acc);
    }
}

template <typename R, int VEC, int G, int U, bool PIPE, bool HINT = false>
__global__ __launch_bounds__(256) void k_spmm_group(const typename R::Args p) {
    if (G <= 8) group_rows_coop<R, VEC, G, 4>(p, xcd_block(p));
    else group_rows<R, VEC, G, U, PIPE, HINT>(p, xcd_block(p));
}

// ---- long rows ---------------------------------------------------------------------------------
template <typename R, int VEC, int U, bool HINT = false>
__global__ __launch_bounds__(256) void k_spmm_long_partial(const typename R::Args p) {
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t cslot = (int64_t)blockIdx.x * 4 + wib;
    if (cslot >= p.n_chunks) return;
    const auto [chunk, row, beg, end] = slot_chunk(p, cslot);
    for (int c0 = 0; c0 < p.C; c0 += 64 * VEC) {
        const int c = c0 + lane * VEC;
        const bool active = c < p.C;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        wave_accumulate<R, VEC, U, false, false, false, HINT>(p.colidx, p.vals, R::X(p), p.ldx, beg, end, active ? c : 0, lane, acc);
        if (active) vstore<VEC>(p.partial + chunk * (int64_t)p.C + c, acc);
    }
}

// Narrow features: a chunk's entries are dealt round-robin to the wave's 64/G sub-groups of G lanes
// (each sub-group gathers whole C-wide rows), then the sub-group sums are added with a fixed xor tree.
template <typename R, int VEC, int G, int U, bool HINT = false>
__device__ __forceinline__ void long_chunks_group(const typename R::Args &p, int64_t block) {
    constexpr bool PEND = IS_PEND<R>;
    constexpr int NS = 64 / G;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t cslot = block * 4 + wib;
    if (cslot >= p.n_chunks) return;
    const auto [chunk, row, beg, end] = slot_chunk(p, cslot);
    const int sub = lane / G;
    const int c = (lane % G) * VEC;
    const bool active = c < p.C;
    const typename R::Elem *__restrict__ Xc = R::X(p) + (active ? c : 0);
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
    [[maybe_unused]] float prev[VEC];
    if constexpr (PEND) {
        static_assert(HINT && VEC == 4 && G >= 16, "pendant elision: the hinted sub-wave kernels");
        // the hub row's own values of two iterations ago (P may be the destination buffer: the reduce launch writes the row later)
#pragma unroll
        for (int v = 0; v < VEC; ++v) prev[v] = 0.f;
        if (p.pend_row_mark[row] && !p.pend_raw) vload<VEC>(prev, p.P + row * p.ldp + (active ? c : 0));
    }
    for (int64_t e = beg + sub; e < end; e += (int64_t)NS * U) {
        if constexpr (PEND) {
            const float *H0c = p.H0 + (active ? c : 0);
            int j[U];
            float w[U], pw[U];
            f32x4 x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t eu = e + (int64_t)u * NS;
                j[u] = eu < end ? p.colidx[eu] : HINT_NONE;
                w[u] = eu < end ? p.vals[eu] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t col = j[u] & PEND_COL_MASK;
                const bool pend = pend_col(j[u]);
                x[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                gather16_hinted(x[u], pend ? H0c + col * p.ldh0 : Xc + col * p.ldx, j[u]);
                pw[u] = pend ? p.pend_w[col] : 0.f;
            }
            gather_wait<U>(x);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (pend_col(j[u]) && !p.pend_raw) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) x[u][v] = pendant_iterate(pw[u], prev[v], x[u][v], p.beta, p.alpha, p.act);
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
            }
            continue;
        } else if constexpr (HINT) {
            static_assert(VEC == 4 && std::is_same_v<typename R::Elem, float>, "hinted gathers: f32 rows, 16 bytes per lane");
            int j[U];
            float w[U];
            f32x4 x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t eu = e + (int64_t)u * NS;
                j[u] = eu < end ? p.colidx[eu] : HINT_NONE;
                w[u] = eu < end ? p.vals[eu] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                x[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                gather16_hinted(x[u], Xc + (int64_t)hint_col(j[u]) * p.ldx, j[u]);
            }
            gather_wait<U>(x);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[u], x[u][v], acc[v]);
            continue;
        }
        float x[U][VEC];
        float w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t eu = e + (int64_t)u * NS;
            if (eu < end) {
                const int j = p.colidx[eu];
                w[u] = p.vals[eu];
                R::template load<VEC>(x[u], Xc + (int64_t)j * p.ldx);
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
    if (sub == 0 && active) vstore<VEC>(p.partial + chunk * (int64_t)p.C + c, acc);
}

template <typename R, int VEC, int G, int U, bool HINT = false>
__global__ __launch_bounds__(256) void k_spmm_long_partial_group(const typename R::Args p) {
    long_chunks_group<R, VEC, G, U, HINT>(p, blockIdx.x);
}

// Short rows and the chunks of the long rows in ONE launch, for graphs with few chunks (a citation-graph-sized matrix has a few
// hundred): a chunk is one wave walking 512 entries, so a launch of a few hundred waves is bound by the latency of that walk
// (0.11 ms at C = 128) while most of the card idles; here the chunk blocks are dealt first and the short rows fill the rest of
// the card under them.  Same per-row arithmetic as the two separate launches; k_spmm_long_reduce follows as before.
template <typename R, int VEC, int G, bool HINT = false>
__global__ __launch_bounds__(256) void k_spmm_group_and_chunks(const typename R::Args p, int chunk_blocks) {
    if ((int)blockIdx.x < chunk_blocks) long_chunks_group<R, VEC, G, 4, HINT>(p, blockIdx.x);
    else if (G <= 8) group_rows_coop<R, VEC, G, 4>(p, (int64_t)blockIdx.x - chunk_blocks);
    else group_rows<R, VEC, G, 4, false, HINT>(p, (int64_t)blockIdx.x - chunk_blocks);
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
// the short rows; the class that took them
template <typename R, int VEC, bool HINT = false>
RowClass launch_rows(const typename R::Args &p0, hipStream_t s) {
    typename R::Args p = p0;
    const int lanes = (p.C + VEC - 1) / VEC;  // lanes needed to cover one row
    bool trim = true;
#ifdef GNX_TUNING
    if ((p.tune & (1 << 21)) || (lanes > 32 && (p.tune & 1))) trim = false;   // (A/B switch of the tuning build; the degree-ordered wave rows)
#endif
    if (trim) trim_empty_rows(p, lanes);
    if (p.n_rows == 0) return ROWS_NONE;
    if (lanes > 32) {
        // measured: U = 8 rows in flight is the plateau (U=4 +0.7 %, U=16 +17 %, forcing 8 waves/SIMD +14 %,
        // degree-ordered rows +9 %; non-temporal index loads +-0 % -- the "non-temporal H0/out" switch measured beside them compiled
        // to plain accesses and said nothing: both switches are gone)
        // measured (tools/tune_spmm.py): 8 waves per block are 1.6 % faster than 4 when the row is one tile wide
        // (C = 256), 0.6 % slower at two tiles (C = 512); 2 and 16 waves per block lose 3-11 %
        if (p.C <= 64 * VEC) GNX_ROW_PIECES((k_spmm_wave<R, VEC, 8, 8, HINT>), 8, 512);
        else                 GNX_ROW_PIECES((k_spmm_wave<R, VEC, 8, 4, HINT>), 4, 256);
        return ROWS_WAVE;
    }
    // measured (tools/tune_spmm.py, RMAT 10M/100M): prefetching the next (col, val) batch behind the gathers pays for G <= 8
    // (C <= 32: -8..-12 %; group_rows_coop) and not for the wider groups, whose pipelined form only tuning builds hold
    // (round 2, one-process A/B at C = 128 / 64: 8 entries in flight per lane 8.86 / 4.57 ms, pipelined 8.98 / 4.37, 2 entries 8.24 / 4.37
    //  against 8.24 / 4.36 for the shipped 4 -- the sub-wave kernels sit on the bandwidth plateau, not on latency)
    // Rows of up to 4 lanes (C <= 16) run on 8-lane groups as well: the four lanes beyond the row's width only take part in the
    // cooperative index fetch (round 6, config-4 graph: C = 8 1.543 -> 1.509 ms per iteration, C = 16 1.777 -> 1.741; same bits;
    // 8 entries per batch: 1.515 / 1.755; 16-lane groups: 1.77 / 1.96).  (Round 2 tried the other direction, 2 lanes per row for
    // C <= 8: 2.40 vs 2.28 ms -- every gather is one 128-byte line whatever the width, lane use is not the limit.)
    return with_group<false>(lanes, [&](auto G) {
#ifdef GNX_TUNING
        if constexpr (R::EXPERIMENTS) {
            if (((p.tune >> 8) & 3) == 2) {          // experiments: 1 = force plain, 2 = force pipelined
                GNX_ROW_PIECES((k_spmm_group<R, VEC, G(), 4, true>), 256 / G(), 256);
                return;
            }
        }
#endif
        GNX_ROW_PIECES((k_spmm_group<R, VEC, G(), 4, false, HINT && G() >= 16>), 256 / G(), 256);
    });
}

// few chunks (see k_spmm_group_and_chunks): one launch for the short rows and the chunks, then the reduce; ROWS_NONE = not taken
template <typename R, int VEC, bool HINT = false>
RowClass launch_rows_and_chunks(const typename R::Args &p, hipStream_t s) {
    const int lanes = (p.C + VEC - 1) / VEC;
    // (tune bit 65536: tuning builds' A/B of the merged launch on big graphs)
    if (lanes > 32 || p.n_long == 0 || (p.n_rows >= SMALL_ROWS && !(p.tune & 65536)) || ((p.tune >> 8) & 3) != 0 || (p.tune & 4096)) return ROWS_NONE;
    const unsigned cb = blocks_for(p.n_chunks, 4);
    // (4-lane groups: these launches are latency-bound)
    const RowClass rows = with_group<true>(lanes, [&](auto G) {
        hipLaunchKernelGGL((k_spmm_group_and_chunks<R, VEC, G(), HINT && G() >= 16>), dim3(cb + blocks_for(p.n_rows, 256 / G())), dim3(256), 0, s, p, (int)cb);
    });
    GNX_LAUNCH((k_spmm_long_reduce<R, VEC>), blocks_for(p.n_long, 4), p);
    return rows;
}

// the long rows in launches of their own: partial sums per chunk, then the reduce
template <typename R, int VEC, bool HINT = false>
void launch_long(const typename R::Args &p, hipStream_t s) {
    const int lanes = (p.C + VEC - 1) / VEC;
    if (lanes > 32) GNX_LAUNCH((k_spmm_long_partial<R, VEC, 8, HINT>), blocks_for(p.n_chunks, 4), p);
    else with_group<true>(lanes, [&](auto G) { GNX_LAUNCH((k_spmm_long_partial_group<R, VEC, G(), 4, HINT && G() >= 16>), blocks_for(p.n_chunks, 4), p); });
    GNX_LAUNCH((k_spmm_long_reduce<R, VEC>), blocks_for(p.n_long, 4), p);
}

// one eval-mode SpMM over bound arguments (bind_csr); the name gnx_graph_last_kernel reports.  HINT: p.colidx holds the handle's
// hinted columns (the caller made sure that the launch runs 4 values per lane on at least 16 lanes: launch_spmm, gather_hints_for).
template <typename R, bool HINT = false>
const char *launch_eval(const typename R::Args &p, hipStream_t s) {
    return with_vec<R>(R::vec(p), [&](auto V) {
        constexpr bool H = HINT && V() == 4;
        RowClass rows = launch_rows_and_chunks<R, V(), H>(p, s);
        if (rows != ROWS_NONE) return kernel_name<R>(rows, MODE_EVAL, HUBS_CHUNKS);
        rows = launch_rows<R, V(), H>(p, s);
        if (p.n_long > 0) launch_long<R, V(), H>(p, s);
        return kernel_name<R>(rows, MODE_EVAL, p.n_long > 0 ? HUBS_LONG : HUBS_NONE);
    });
}

// launch_eval<F32Rows, true> for one iteration of a K loop that elides the handle's pendant rows (the caller made sure of 4 values
// per lane on 16 or 32 lanes, and set p.colidx to the handle's pend_cols): the same three launch shapes over the PEND kernels.  An
// iteration but the last leaves the slots [skip_beg, skip_end) out -- it is not launched beyond them where the rows without entries,
// which follow them in the row order, are left alone as well.  The reduce of the hub rows is the plain one: it reads nothing new.
[[maybe_unused]] const char *launch_eval_pend(const PendArgs &p0, hipStream_t s) {
    using R = F32RowsPend;
    PendArgs p = p0;
    const int lanes = (p.C + 3) / 4;
    const SpmmArgs &plain = p;
    if (p.n_long > 0 && p.n_rows < SMALL_ROWS) {      // launch_rows_and_chunks
        const unsigned cb = blocks_for(p.n_chunks, 4);
        if (p.skip_empty && p.skip_end > p.skip_beg) p.n_rows = p.skip_beg;
        const RowClass rows = with_group<true>(lanes, [&](auto G) {
            if constexpr (G() >= 16)
                hipLaunchKernelGGL((k_spmm_group_and_chunks<R, 4, G(), true>), dim3(cb + blocks_for(p.n_rows, 256 / G())), dim3(256), 0, s, p, (int)cb);
        });
        GNX_LAUNCH((k_spmm_long_reduce<F32Rows, 4>), blocks_for(p.n_long, 4), plain);
        return kernel_name<F32Rows>(rows, MODE_EVAL, HUBS_CHUNKS);
    }
    RowClass rows = ROWS_NONE;
    {   // launch_rows
        PendArgs q = p;
        trim_empty_rows(q, lanes);
        if (q.skip_end > q.skip_beg && q.n_rows <= q.skip_end) q.n_rows = q.skip_beg;
        if (q.n_rows > 0)
            rows = with_group<false>(lanes, [&](auto G) {
                if constexpr (G() >= 16) launch_row_pieces((k_spmm_group<R, 4, G(), 4, false, true>), q, 256 / G(), 256, s);
            });
    }
    if (p.n_long > 0) {                               // launch_long
        with_group<true>(lanes, [&](auto G) {
            if constexpr (G() >= 16) GNX_LAUNCH((k_spmm_long_partial_group<R, 4, G(), 4, true>), blocks_for(p.n_chunks, 4), p);
        });
        GNX_LAUNCH((k_spmm_long_reduce<F32Rows, 4>), blocks_for(p.n_long, 4), plain);
    }
    return kernel_name<F32Rows>(rows, MODE_EVAL, p.n_long > 0 ? HUBS_LONG : HUBS_NONE);
}

}  // namespace
