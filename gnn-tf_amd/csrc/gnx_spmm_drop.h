// The training-mode dispatch classes of the SpMM (fused edge dropout), each written once over the row-storage policy R
// (gnx_spmm_device.h) and instantiated for f32 rows by gnx_spmm_train.hip and for bf16 rows by gnx_spmm_train_bf16.hip, and the
// launcher layer that picks among them.
#pragma once
#include "gnx_spmm_device.h"

namespace {

// ---- training iterations: the dropped + re-normalised values are produced inside the SpMM (gnx_spmm_dropped) ------------
// Same row / lane mapping as the eval kernels (gnx_spmm_eval.h); what differs is where an entry's weight comes from: p.vals holds the RAW
// values and every weight is (D[row] * drop(raw)) * D[col] (layered.py:47-50 + gnn.py:41-42), computed ONCE per entry by one
// lane and handed to the lanes that need it (readlane / shuffles), so the hash costs one evaluation per stored entry.
// ENTRIES (the _entries instantiations, a handle with duplicate COO entries after gnx_graph_enable_entry_dropout): p.vals holds each
// slot's uniform value and the lane that owns a slot makes its kept sum (dropped_weight_entries) -- one more hash round per further
// duplicate; everything else, and the kernels without duplicates, as before.
// R::GATHER_ORDER (F32RowsOrd): the lane that owns an entry also loads its gather column and the gather address takes that one; the
// draw, the mask and D[col] keep the column (gather_cols).
template <typename R, int VEC, int U, int WPB, bool ENTRIES = false>
__global__ __launch_bounds__(64 * WPB) void k_spmm_wave_drop(const typename R::Args p) {
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t slot = p.slot0 + xcd_block(p) * WPB + wib;
    if (slot >= p.n_rows) return;
    const auto [row, beg, end] = slot_row<true>(p, slot);
    if (end - beg > p.long_row) return;
    if (p.skip_empty && beg == end) return;   // GNX_ACT_SKIP_EMPTY (chained training loops: nobody gathers this row, a later launch writes it)
    for (int c0 = 0; c0 < p.C; c0 += 64 * VEC) {
        const int c = c0 + lane * VEC;
        const bool active = c < p.C;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        wave_accumulate<R, VEC, U, true, ENTRIES, R::GATHER_ORDER>(p.colidx, p.vals, R::X(p), p.ldx, beg, end, active ? c : 0, lane, acc, false, &p.fuse,
                                                                  row, gather_cols<R>(p));
        epilogue_store<R, VEC>(p, row, c, active, acc);
    }
}

// PIPE: the (col, raw value) pair a lane owns in the NEXT round is loaded before this round's kept entries are gathered, so a row
// of more than G entries pays the index latency once instead of once per round.
template <typename R, int VEC, int G, int U, bool PIPE, bool ENTRIES = false>
__global__ __launch_bounds__(256) void k_spmm_group_drop(const typename R::Args p) {
    constexpr int RPB = 256 / G;
    const int sub = threadIdx.x % G;
    const int64_t slot = p.slot0 + xcd_block(p) * RPB + threadIdx.x / G;
    if (slot >= p.n_rows) return;
    const auto [row, beg, end] = slot_row<false>(p, slot);
    if (end - beg > p.long_row) return;
    if (p.skip_empty && beg == end) return;   // GNX_ACT_SKIP_EMPTY
    constexpr bool GC = R::GATHER_ORDER;
    [[maybe_unused]] const int32_t *__restrict__ gcol = gather_cols<R>(p);
    for (int c0 = 0; c0 < p.C; c0 += G * VEC) {
        const int c = c0 + sub * VEC;
        const bool active = c < p.C;
        const typename R::Elem *__restrict__ Xc = R::X(p) + (active ? c : 0);
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        int ncol = 0;
        float nraw = 0.f;
        if (PIPE && beg + sub < end) { ncol = p.colidx[beg + sub]; nraw = p.vals[beg + sub]; }
        for (int64_t base = beg; base < end; base += G) {          // G entries per round: lane `sub` owns entry base + sub
            const int n = (int)((end - base) < G ? (end - base) : G);
            int mycol = 0;
            [[maybe_unused]] int mygcol = 0;                           // GATHER_ORDER: the row of X the entry gathers
            float myw = 0.f;
            if (PIPE) {
                const int ccol = ncol;
                const float craw = nraw;
                if (base + G + sub < end) { ncol = p.colidx[base + G + sub]; nraw = p.vals[base + G + sub]; }
                if (sub < n) {
                    mycol = ccol; myw = dropped_weight_at<ENTRIES>(p.fuse, craw, base + sub, row, ccol);
                    if constexpr (GC) mygcol = gcol[base + sub];
                }
            } else if (sub < n) {
                mycol = p.colidx[base + sub];
                if constexpr (GC) mygcol = gcol[base + sub];
                myw = dropped_weight_at<ENTRIES>(p.fuse, p.vals[base + sub], base + sub, row, mycol);
            }
            // dropped entries (weight exactly 0) are not gathered: the group walks only the kept entries of its round, in order
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
                        int j;
                        if constexpr (GC) j = __shfl(mygcol, idx, G);
                        else j = __shfl(mycol, idx, G);
                        w[u] = __shfl(myw, idx, G);
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

template <typename R, int VEC, int U, bool ENTRIES = false>
__global__ __launch_bounds__(256) void k_spmm_long_partial_drop(const typename R::Args p) {
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
        wave_accumulate<R, VEC, U, true, ENTRIES, R::GATHER_ORDER>(p.colidx, p.vals, R::X(p), p.ldx, beg, end, active ? c : 0, lane, acc, false, &p.fuse,
                                                                  row, gather_cols<R>(p));
        if (active) vstore<VEC>(p.partial + chunk * (int64_t)p.C + c, acc);
    }
}

// narrow long rows: the wave computes 64 weights per round (one per lane); sub-group s then takes entries s, s + NS, ... of the
// round, which is the entry -> sub-group dealing of k_spmm_long_partial_group (so the partial sums are bitwise the same)
template <typename R, int VEC, int G, int U, bool ENTRIES = false>
__global__ __launch_bounds__(256) void k_spmm_long_partial_group_drop(const typename R::Args p) {
    constexpr int NS = 64 / G;
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t cslot = (int64_t)blockIdx.x * 4 + wib;
    if (cslot >= p.n_chunks) return;
    const auto [chunk, row, beg, end] = slot_chunk(p, cslot);
    const int sub = lane / G;
    const int c = (lane % G) * VEC;
    const bool active = c < p.C;
    const typename R::Elem *__restrict__ Xc = R::X(p) + (active ? c : 0);
    constexpr bool GC = R::GATHER_ORDER;
    [[maybe_unused]] const int32_t *__restrict__ gcol = gather_cols<R>(p);
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
    // the reference kernel walks e = beg + sub + k * NS (k = 0, 1, ...) in batches of U: entry index within the chunk = sub + k NS.
    // A round of 64 entries covers k = 0 .. 64/NS - 1 = G - 1 for every sub-group.
    for (int64_t base = beg; base < end; base += 64) {
        const int n = (int)((end - base) < 64 ? (end - base) : 64);
        int mycol = 0;
        [[maybe_unused]] int mygcol = 0;
        float myw = 0.f;
        if (lane < n) {
            mycol = p.colidx[base + lane];
            if constexpr (GC) mygcol = gcol[base + lane];
            myw = dropped_weight_at<ENTRIES>(p.fuse, p.vals[base + lane], base + lane, row, mycol);
        }
#pragma unroll 1
        for (int k = 0; k < G; k += U) {
            float x[U][VEC];
            float w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int src = sub + (k + u) * NS;                  // entry of the round this sub-group takes in slot k + u
                int j;
                if constexpr (GC) j = __shfl(mygcol, src);
                else j = __shfl(mycol, src);
                w[u] = __shfl(myw, src);
                if (k + u < G && src < n && w[u] != 0.f) R::template load<VEC>(x[u], Xc + (int64_t)j * p.ldx);   // dropped: not gathered
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
    if (sub == 0 && active) vstore<VEC>(p.partial + chunk * (int64_t)p.C + c, acc);
}

[[maybe_unused]] constexpr bool DROP_U8 = false, DROP_PIPE = false;     // product defaults of the training row kernels (see launch_rows_drop)
constexpr int DROP_LONG_U = 4;

// ---- launchers ------------------------------------------------------------------------------------------------------------
template <typename R, int VEC, bool E>
RowClass launch_rows_drop(const typename R::Args &p0, hipStream_t s) {
    typename R::Args p = p0;
    const int lanes = (p.C + VEC - 1) / VEC;
    trim_empty_rows(p, lanes);
    if (p.n_rows == 0) return ROWS_NONE;
    if (lanes > 32) {
        if (p.C <= 64 * VEC) GNX_ROW_PIECES((k_spmm_wave_drop<R, VEC, 8, 8, E>), 8, 512);
        else                 GNX_ROW_PIECES((k_spmm_wave_drop<R, VEC, 8, 4, E>), 4, 256);
        return ROWS_WAVE;
    }
    // A group of G lanes takes G entries per round (lane `sub` draws the weight of entry base + sub), so G is also how many index
    // loads and draws are in flight per row.  Round 6 (profiles/NOTES.md, config-4 graph, middle iteration): rows of up to 4 lanes
    // (C <= 16) on 8-lane groups instead of 4-lane ones -- half the lanes then only fetch and draw, their gather repeats a
    // neighbour's line -- C = 8: 1.94 -> 1.52 ms forward, 2.03 -> 1.61 backward; C = 16: 2.00 -> 1.56 / 2.08 -> 1.63; same bits.
    // 16 lanes: 1.83 / 1.85 ms, 32 lanes: 2.7 ms (fewer rows per wave than the gathers need in flight).
    return with_group<false>(lanes, [&](auto G) {
        if constexpr (R::EXPERIMENTS) {
            // U gathers in flight per lane and the index prefetch: round-4 A/B on the config-4 graph (tuning build bits 1 << 17 = U 8,
            // 1 << 19 = PIPE; profiles/NOTES.md)
#ifdef GNX_TUNING
            const bool u8 = (p.tune & (1 << 17)) != 0, pipe = (p.tune & (1 << 19)) != 0;
#else
            const bool u8 = DROP_U8, pipe = DROP_PIPE;
#endif
            if (u8 && pipe)  GNX_ROW_PIECES((k_spmm_group_drop<R, VEC, G(), 8, true, E>), 256 / G(), 256);
            else if (u8)     GNX_ROW_PIECES((k_spmm_group_drop<R, VEC, G(), 8, false, E>), 256 / G(), 256);
            else if (pipe)   GNX_ROW_PIECES((k_spmm_group_drop<R, VEC, G(), 4, true, E>), 256 / G(), 256);
            else             GNX_ROW_PIECES((k_spmm_group_drop<R, VEC, G(), 4, false, E>), 256 / G(), 256);
        } else {
            GNX_ROW_PIECES((k_spmm_group_drop<R, VEC, G(), 4, false, E>), 256 / G(), 256);
        }
    });
}

template <typename R, int VEC, bool E>
void launch_long_drop(const typename R::Args &p, hipStream_t s) {
    const int lanes = (p.C + VEC - 1) / VEC;
    if (lanes > 32) GNX_LAUNCH((k_spmm_long_partial_drop<R, VEC, 8, E>), blocks_for(p.n_chunks, 4), p);
    else with_group<true>(lanes, [&](auto G) {
        constexpr int U = G() == 4 ? 4 : DROP_LONG_U;
#ifdef GNX_TUNING
        if constexpr (R::EXPERIMENTS) {
            if (p.tune & (1 << 18)) {
                GNX_LAUNCH((k_spmm_long_partial_group_drop<R, VEC, G(), (G() == 4 ? 4 : 8), E>), blocks_for(p.n_chunks, 4), p);
                return;
            }
        }
#endif
        GNX_LAUNCH((k_spmm_long_partial_group_drop<R, VEC, G(), U, E>), blocks_for(p.n_chunks, 4), p);
    });
    GNX_LAUNCH((k_spmm_long_reduce<R, VEC>), blocks_for(p.n_long, 4), p);
}

// one training-mode SpMM over bound arguments (bind_csr), E = the handle holds duplicate entries (p.fuse.mult); the name
// gnx_graph_last_kernel reports
template <typename R>
const char *launch_drop(const typename R::Args &p, int vec, hipStream_t s) {
    return with_vec<R>(vec, [&](auto V) {
        const RowClass rows = p.fuse.mult ? launch_rows_drop<R, V(), true>(p, s) : launch_rows_drop<R, V(), false>(p, s);
        if (p.n_long > 0) {
            if (p.fuse.mult) launch_long_drop<R, V(), true>(p, s);
            else launch_long_drop<R, V(), false>(p, s);
        }
        return kernel_name<R>(rows, p.fuse.mult ? MODE_DROP_ENTRIES : MODE_DROP, p.n_long > 0 ? HUBS_LONG : HUBS_NONE);
    });
}

// ---- the fused-dropout entry points, written once over the policy ------------------------------------------------------------------
// gnx_spmm_dropped_chained / _back and their _ord and _bf16 forms are calls of the two templates below with their own name.  Per
// storage differ: where the NULL-handle check sits (bf16 rows: in `admit`, behind the handle-free checks, so that those can be
// exercised without a device; f32 rows: first), which handles `admit(g, s)` lets through -- it runs behind the last handle-free check
// and before anything is built or launched --, how X and the results are typed (the policy's binders) and, under a GATHER_ORDER
// policy, `order`.  Only the messages of the bf16 entries name the entry in front of the dropout rate.
template <typename R>
int check_rate(const char *fn, float dropout_p) {
    const bool ok = dropout_p >= 0.f && dropout_p < 1.f;
    if constexpr (R::BF16) GNX_CHECK_ARG(ok, "%s: dropout rate %g outside [0, 1)", fn, (double)dropout_p);
    else GNX_CHECK_ARG(ok, "dropout rate %g outside [0, 1)", (double)dropout_p);
    return GNX_OK;
}

template <typename R>
int check_handle_and_operands(const char *fn, gnx_graph *g, const void *X, int64_t ldx, int64_t C, const float *H0, int64_t ldh0, const void *out,
                              int64_t ldo) {
    if constexpr (!R::BF16) GNX_CHECK_ARG(g != nullptr, "%s: NULL handle", fn);
    return check_operands(fn, X, ldx, C, H0, ldh0, out, ldo);
}

// the handle-free checks of the forward entries (gnx_spmm_dropped and the chained ones); act_flags = the bits `act` may carry beside
// the activation
template <typename R>
int check_dropped_forward(const char *fn, gnx_graph *g, const void *X, int64_t ldx, int64_t C, const float *H0, int64_t ldh0, const void *out,
                          int64_t ldo, int act, int act_flags, const float *d_D, float dropout_p) {
    int rc = check_handle_and_operands<R>(fn, g, X, ldx, C, H0, ldh0, out, ldo);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG((act & ~act_flags) == GNX_ACT_NONE || (act & ~act_flags) == GNX_ACT_RELU, "%s: invalid activation %d", fn, act);
    GNX_CHECK_ARG(d_D != nullptr, "%s: NULL degree scales", fn);
    return check_rate<R>(fn, dropout_p);
}

// f32 rows launch through gnx_spmm.hip (where a tuning build switches kernel variants), the other storages from their own unit
template <typename R>
int launch_train(gnx_graph *g, const Csr &m, typename R::Args &p, hipStream_t s) {
    if constexpr (std::is_same_v<typename R::Args, SpmmArgs>) return launch_spmm(g, m, p, s);
    else return launch_bound(g, m, p, s, [&](typename R::Args &q) { return launch_drop<R>(q, R::vec(q), s); });
}

template <typename R, typename Admit>
int spmm_dropped_chained(const char *fn, Admit admit, gnx_graph *g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id,
                         int x_prescaled, const float *d_D_next, const typename R::Elem *d_X, int64_t ldx, int64_t C, const float *d_H0,
                         int64_t ldh0, float beta, float alpha, int act, typename R::Out *d_out, int out_bf16, int64_t ldo, int order,
                         void *stream) {
    int rc = check_dropped_forward<R>(fn, g, d_X, ldx, C, d_H0, ldh0, d_out, ldo, act, GNX_ACT_SKIP_EMPTY, d_D, dropout_p);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(out_bf16 == 0 || out_bf16 == 1, "%s: out_bf16 must be 0 or 1", fn);
    GNX_CHECK_ARG((order & ~(GNX_ORD_X | GNX_ORD_OUT)) == 0, "%s: invalid order flags %d", fn, order);
    hipStream_t s = (hipStream_t)stream;
    rc = admit(g, s);
    if (rc != GNX_OK) return rc;
    if (!g->a.empty_rows_unreferenced) act &= ~GNX_ACT_SKIP_EMPTY;       // honoured only when nobody gathers the rows it would leave untouched
    typename R::Args p{};
    set_values(g, false, p);
    set_operands<R>(p, d_X, ldx, d_H0, ldh0, beta, alpha, act, d_out, out_bf16, ldo, C);
    p.out_scale = d_D_next ? d_D_next + g->blk_row0_buf : nullptr;       // (the offset is 0 on every handle that is no vertex block)
    if constexpr (R::GATHER_ORDER) {
        p.gcol = (order & GNX_ORD_X) ? g->a_gcol : nullptr;
        p.out_rows = (order & GNX_ORD_OUT) ? g->go_rank : nullptr;       // H0 and the scales stay indexed by the caller's row (map_h0 false)
    }
    set_drop_fuse(g, dropout_p, seed, stream_id, d_D, 0, x_prescaled, p);
    return launch_train<R>(g, g->a, p, s);
}

template <typename R, typename Admit>
int spmm_dropped_back(const char *fn, Admit admit, gnx_graph *g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id,
                      int x_prescaled, const float *d_D_next, const typename R::Elem *d_X, int64_t ldx, int64_t C, const float *d_S_in,
                      int64_t lds_in, float s_alpha, float s_beta, float *d_S_out, int64_t lds_out, float y_beta, typename R::Out2 *d_Y_out,
                      int64_t ldy, int act, int order, void *stream) {
    int rc = check_handle_and_operands<R>(fn, g, d_X, ldx, C, d_S_in, lds_in, d_S_out, lds_out);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG((order & ~(GNX_ORD_X | GNX_ORD_OUT)) == 0, "%s: invalid order flags %d", fn, order);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_SKIP_EMPTY, "%s: act must be GNX_ACT_NONE or GNX_ACT_SKIP_EMPTY", fn);
    GNX_CHECK_ARG(act == GNX_ACT_NONE || (const void *)d_S_in == (const void *)d_S_out, "%s: GNX_ACT_SKIP_EMPTY needs the sum updated in place", fn);
    GNX_CHECK_ARG(d_D != nullptr && d_S_in != nullptr, "%s: NULL degree scales / running sum", fn);
    GNX_CHECK_ARG(d_Y_out == nullptr || (ldy >= C && (const void *)d_Y_out != (const void *)d_X && (const void *)d_Y_out != (const void *)d_S_out
                                         && (const void *)d_Y_out != (const void *)d_S_in),
                  "%s: the pre-scaled output needs a buffer of its own", fn);
    rc = check_rate<R>(fn, dropout_p);
    if (rc != GNX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = admit(g, s);
    if (rc != GNX_OK) return rc;
    if constexpr (!R::GATHER_ORDER) {                                    // (ensure_train_gather, the admission of _ord, built it)
        rc = ensure_transpose(g, s);
        if (rc != GNX_OK) return rc;
    }
    if (!g->t.empty_rows_unreferenced) act = GNX_ACT_NONE;               // honoured only when nobody gathers the rows it would leave untouched
    typename R::Args p{};
    set_values(g, true, p);
    set_operands<R>(p, d_X, ldx, d_S_in, lds_in, s_beta, s_alpha, act, d_S_out, 0, lds_out, C);   // the running sum: f32, in the caller's order
    R::bind_out2(p, d_Y_out); p.ldo2 = ldy; p.beta2 = y_beta; p.out2_scale = d_Y_out ? d_D_next : nullptr;
    if constexpr (R::GATHER_ORDER) {
        p.gcol = (order & GNX_ORD_X) ? g->t_gcol : nullptr;
        p.out2_rows = (d_Y_out && (order & GNX_ORD_OUT)) ? g->go_rank : nullptr;
    }
    set_drop_fuse(g, dropout_p, seed, stream_id, d_D, 1, x_prescaled, p);   // (stand-alone handle: the block keys are 0 / null)
    return launch_train<R>(g, g->t, p, s);
}

}  // namespace
