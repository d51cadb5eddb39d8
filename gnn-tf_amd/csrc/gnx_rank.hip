// The ranking evaluation of the link task on the device: what MeanLinkPrediction.evaluate does per source node
// (reference gnntf/core/gnn/graph_predictor.py:154-203), for all sources in three launches.
//
//   gnx_rank_candidates   per source: the counts behind the rank-statistic AUC of its held-out neighbours against every non-linked
//                         candidate, and the k best entries of that list, without the [S, K] score matrix reaching memory
//
//   k_rank_prepare  one wave per source: checks it, scores its held-out neighbours (16 at a time on the matrix pipe) into the workspace
//   k_rank_tiles    a block of RANK_WAVES waves shares every tile of RANK_TILE gathered candidate rows in LDS; a wave owns 16 sources,
//                   whose rows -- scaled by r -- stay in registers across the candidate loop; the next tile's rows are gathered into
//                   registers under the MFMAs of the current one.  The score tile leaves the accumulators into
//                   the epilogue: compares against the source's positive scores (integer counts over ALL candidates) and a per-row
//                   running top-k in LDS whose threshold rejects almost everything; only an entry that would enter is looked up in the
//                   adjacency.  One partial list per (source, candidate part) goes to the workspace.
//   k_rank_finish   one wave per source: scores the EXCLUDED pairs (the source itself and its out- and in-neighbours that are candidates,
//                   found in the ascending candidate array) and subtracts what they added to the counts; merges the positives and the
//                   partial lists into the top-k.
//
// Every score of a (source, node) pair is the same chain of v_mfma_f32_16x16x4_f32 steps over the same operands in all three kernels,
// so the positives' scores, the tile's and the correction's agree bit for bit.  The top-k order is total and the counts are integers:
// the outputs do not depend on the number of parts or on the schedule.  No float atomics.  Ids are range-checked, never dereferenced
// out of range; nothing allocates or waits once the handle's transposed structure exists (gnx_graph_reserve).
#include "gnx_internal.h"

namespace {

using namespace gnx;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RANK_WAVES = 4;                 // waves (16 sources each) per block of k_rank_tiles
constexpr int RANK_TILE = 64;                 // candidates per LDS tile: 4 MFMA column tiles per wave and fill
constexpr int RANK_CK = 64;                   // columns of F per LDS fill
constexpr int RANK_PITCH = RANK_CK + 4;       // floats per LDS row: 16-byte aligned, and 16 rows at one column hit 16 bank quads
constexpr int RANK_MAX_K = GNX_RANK_MAX_K;
constexpr int RANK_POS_PASS = GNX_RANK_POS_PASS;   // positive scores per source kept in LDS; further ones are read from the workspace
constexpr int64_t RANK_TARGET_BLOCKS = 1024;  // splits == 0: parts until about 4 blocks per CU are in flight
constexpr int64_t RANK_MAX_SPLITS = 256;

struct RankArgs {
    const int64_t *g_rowptr;
    const int32_t *g_colidx;
    int64_t g_rows;
    const int64_t *t_rowptr;
    const int32_t *t_colidx;
    int64_t t_rows;
    const float *F;
    int64_t ldf, n_rows_F;
    int C;
    const float *r;
    int vec;                                  // 16-byte loads of F rows are aligned
    const int64_t *sources;
    int64_t S;
    const int64_t *pos_ptr, *pos_ids;
    int64_t P;
    const int64_t *cand;
    int64_t K;
    int k, splits;
    int64_t tiles_per_part;
    int64_t *n_pos, *n_neg;
    unsigned long long *less, *equal;
    int64_t *top_ids;
    float *top_scores;
    uint8_t *top_is_pos;
    float *scores;
    float *pos_scores;                        // workspace [P]
    uint64_t *part_keys;                      // workspace [S, splits, k]
};

// ---- the order --------------------------------------------------------------------------------------------------------------------------
// An entry of a source's list is one 64-bit key, larger = earlier in the top-k: the score as an order-preserving integer above the
// entry's place in the list (positive i: i; stranger at candidate index j: 2^31 + j).  0 is no entry (no finite score maps to 0).
__device__ __forceinline__ uint64_t rank_key(float x, uint32_t code) {
    const uint32_t b = __float_as_uint(x + 0.0f);                        // -0 orders as +0, as the comparison of the counts does
    const uint32_t ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)ord << 32) | code;
}
__device__ __forceinline__ float rank_key_score(uint64_t key) {
    const uint32_t ord = (uint32_t)(key >> 32);
    return __uint_as_float((ord & 0x80000000u) ? (ord & 0x7FFFFFFFu) : ~ord);
}

// the whole wave inserts `key` into the descending list of k keys at `list` (LDS)
__device__ __forceinline__ void topk_insert(volatile uint64_t *list, int k, uint64_t key, int lane) {
    const uint64_t cur = lane < k ? list[lane] : 0;
    const int at = __popcll(__ballot(lane < k && cur > key));             // the keys above it are a prefix
    __builtin_amdgcn_wave_barrier();
    if (lane >= at && lane + 1 < k) list[lane + 1] = cur;
    if (lane == at && at < k) list[at] = key;
    __builtin_amdgcn_wave_barrier();
}

// every lane that has `pass` set hands its key to the wave, lowest lane first
__device__ __forceinline__ bool topk_offer(volatile uint64_t *list, int k, bool pass, uint64_t key, int lane) {
    uint64_t mask = __ballot(pass);
    const bool any = mask != 0;
    while (mask) {
        const int src = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        const uint64_t kk = ((uint64_t)(uint32_t)__shfl((int)(key >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)key, src);
        topk_insert(list, k, kk, lane);
    }
    return any;
}

// ---- shared pieces ----------------------------------------------------------------------------------------------------------------------
// whether (row, col) is a stored entry of a CSR pattern whose columns ascend inside a row; a row or column beyond it stores nothing
__device__ __forceinline__ bool rank_stored(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t n_rows,
                                            int64_t row, int64_t col) {
    if (row < 0 || row >= n_rows) return false;
    int64_t lo = rowptr[row];
    const int64_t end = rowptr[row + 1];
    int64_t hi = end;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)colidx[mid] < col) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && (int64_t)colidx[lo] == col;
}

// first index of the ascending candidate array whose id is not below v
__device__ __forceinline__ int64_t cand_lower(const int64_t *__restrict__ cand, int64_t K, int64_t v) {
    int64_t lo = 0, hi = K;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cand[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// columns c0 .. c0 + 3 of a row, zeros from column C on (nothing beyond C is read)
__device__ __forceinline__ f32x4 load_cols4(const float *__restrict__ row, int c0, int C, bool vec) {
    if (vec && c0 + 3 < C) return *reinterpret_cast<const f32x4 *>(row + c0);
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (c0 + t < C) v[t] = row[c0 + t];
    return v;
}

// the A operand of columns c0 .. c0 + 3 of a source row: fl(F[s, c] * r[c]), or F[s, c] without r
__device__ __forceinline__ f32x4 load_a4(const RankArgs &a, const float *__restrict__ row, int c0) {
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!row) return v;
    v = load_cols4(row, c0, a.C, a.vec);
    if (a.r) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (c0 + t < a.C) v[t] = v[t] * a.r[c0 + t];
    }
    return v;
}

// The score chain, part of the interface: step (G, t), G ascending over groups of 16 columns and t = 0 .. 3 inside, multiplies k-slot
// g of the MFMA by column 16 G + 4 g + t.  Here for one source (every A row) against the node of lane column c; row null = zeros.
__device__ __forceinline__ float wave_pair_scores(const RankArgs &a, const float *__restrict__ src_row, const float *__restrict__ node_row,
                                                  int g) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 4 * g; c0 - 4 * g < a.C; c0 += 16) {
        const f32x4 av = load_a4(a, src_row, c0);
        const f32x4 bv = node_row ? load_cols4(node_row, c0, a.C, a.vec) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv[t], acc, 0, 0, 0);
    }
    return acc[0];
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (unsigned long long)__shfl_xor((long long)v, d);
    return v;
}

// the held-out range of a source, or false where the pointer array does not describe one inside [0, P]
__device__ __forceinline__ bool pos_range(const RankArgs &a, int64_t i, int64_t &lo, int64_t &n) {
    lo = a.pos_ptr[i];
    const int64_t hi = a.pos_ptr[i + 1];
    n = hi - lo;
    if (lo < 0 || hi < lo || hi > a.P) {
        lo = 0;
        n = 0;
        return false;
    }
    return true;
}

// ---- prepare ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rank_prepare(const RankArgs a) {
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.S) return;
    const int64_t s = a.sources[i];
    int64_t lo, n;
    bool ok = pos_range(a, i, lo, n);
    ok = ok && s >= 0 && s < a.n_rows_F;
    const float *__restrict__ src_row = ok ? a.F + s * a.ldf : nullptr;
    bool bad = false;
    for (int64_t base = 0; base < n; base += 16) {
        const int64_t e = base + c;
        int64_t v = -1;
        if (e < n) {
            v = a.pos_ids[lo + e];
            if (v < 0 || v >= a.n_rows_F) {
                bad = true;
                v = -1;
            }
        }
        const float x = wave_pair_scores(a, src_row, v >= 0 ? a.F + v * a.ldf : nullptr, g);
        if (e < n && g == 0) a.pos_scores[lo + e] = x;
    }
    ok = ok && __ballot(bad) == 0;
    if (lane == 0) {
        a.n_pos[i] = n;
        a.n_neg[i] = ok ? 0 : -1;
        a.less[i] = 0;
        a.equal[i] = 0;
    }
}

// ---- the tiles --------------------------------------------------------------------------------------------------------------------------
// NG: groups of 16 columns whose A operand stays in registers (C <= 16 NG); 0: any C, the A operand is read again for every tile
template <int NG>
__global__ __launch_bounds__(64 * RANK_WAVES, 2) void k_rank_tiles(const RankArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[RANK_TILE * RANK_PITCH];
    __shared__ int64_t tile_id[2][RANK_TILE];                            // this tile's candidates and the next one's
    __shared__ uint64_t topk[RANK_WAVES][16][RANK_MAX_K];
    __shared__ __attribute__((aligned(16))) float pos_lds[RANK_WAVES][16][RANK_POS_PASS];      // padded with NaN to a multiple of 4
    __shared__ float pos_min[RANK_WAVES][16], pos_max[RANK_WAVES][16];
    __shared__ int64_t src_id[RANK_WAVES][16], pos_lo[RANK_WAVES][16];       // read on the rare paths only: kept out of the registers
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int64_t src0 = ((int64_t)blockIdx.x * RANK_WAVES + wave) * 16;
    const int part = blockIdx.y;
    const int k = a.k;

    // the wave's 16 sources: their lists and the positive scores
    for (int rr = 0; rr < 16; ++rr) {
        const int64_t i = src0 + rr;
        int64_t lo = 0, n = 0;
        if (i < a.S && a.n_neg[i] != -1) pos_range(a, i, lo, n);
        float mn = __builtin_inff(), mx = -__builtin_inff();
        if (lane < RANK_POS_PASS && lane >= n) pos_lds[wave][rr][lane] = __builtin_nanf("");
        for (int64_t p = lane; p < n; p += 64) {
            const float ps = a.pos_scores[lo + p];
            if (p < RANK_POS_PASS) pos_lds[wave][rr][p] = ps;
            mn = fminf(mn, ps);
            mx = fmaxf(mx, ps);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, d));
            mx = fmaxf(mx, __shfl_xor(mx, d));
        }
        if (lane == 0) {
            pos_min[wave][rr] = mn;
            pos_max[wave][rr] = mx;
            src_id[wave][rr] = i < a.S ? a.sources[i] : -1;
            pos_lo[wave][rr] = lo;
        }
        if (lane < RANK_MAX_K) topk[wave][rr][lane] = 0;
    }
    __syncthreads();
    // D rows of this lane: 4 g + i
    int row_np[4];
    float row_mn[4], row_mx[4];
    bool row_ok[4], row_in[4];                                           // the source's outputs are valid; the source is a row of F
    uint64_t thr[4];
    unsigned long long n_less[4], n_equal[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t idx = src0 + 4 * g + i;
        row_ok[i] = idx < a.S && a.n_neg[idx] != -1;
        const int64_t s = src_id[wave][4 * g + i];
        row_in[i] = s >= 0 && s < a.n_rows_F;
        int64_t lo = 0, n = 0;
        if (row_ok[i]) pos_range(a, idx, lo, n);
        row_np[i] = (int)n;                                              // P < 2^31
        row_mn[i] = pos_min[wave][4 * g + i];
        row_mx[i] = pos_max[wave][4 * g + i];
        thr[i] = 0;
        n_less[i] = n_equal[i] = 0;
    }
    // A row of this lane: c
    const float *__restrict__ a_row = nullptr;
    {
        const int64_t idx = src0 + c, s = idx < a.S ? a.sources[idx] : -1;
        if (s >= 0 && s < a.n_rows_F) a_row = a.F + s * a.ldf;           // also where a held-out id is out of range: the raw scores stand
    }
    f32x4 areg[NG > 0 ? NG : 1];
    if constexpr (NG > 0) {
#pragma unroll
        for (int G = 0; G < NG; ++G) areg[G] = load_a4(a, a_row, 16 * G + 4 * g);
    }

    const int64_t n_tiles = (a.K + RANK_TILE - 1) / RANK_TILE;
    const int64_t tile_beg = (int64_t)part * a.tiles_per_part;
    const int64_t tile_end = tile_beg + a.tiles_per_part < n_tiles ? tile_beg + a.tiles_per_part : n_tiles;
    const int n_chunks = (a.C + RANK_CK - 1) / RANK_CK;
    // the candidate of this thread's slot of tile tl (the first RANK_TILE threads), -1: beyond K, or no row of F -- skipped, never dereferenced
    auto load_id = [&](int64_t tl) {
        int64_t id = -1;
        if (threadIdx.x < RANK_TILE && tl < tile_end) {
            const int64_t j = tl * RANK_TILE + threadIdx.x;
            if (j < a.K) id = a.cand[j];
            if (id < 0 || id >= a.n_rows_F) id = -1;
        }
        return id;
    };
    // this thread's quads of columns ck RANK_CK ... of the rows `ids` names, and their place in the LDS tile
    constexpr int FILL = RANK_TILE * (RANK_CK / 4) / (64 * RANK_WAVES);
    auto gather = [&](const int64_t *ids, int ck, f32x4 (&v)[FILL]) {
#pragma unroll
        for (int u = 0; u < FILL; ++u) {
            const int idx = threadIdx.x + u * 64 * RANK_WAVES, t = idx / (RANK_CK / 4), q = idx % (RANK_CK / 4);
            const int64_t id = ids[t];
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (id >= 0) v[u] = load_cols4(a.F + id * a.ldf, ck * RANK_CK + 4 * q, a.C, a.vec);
        }
    };
    auto put = [&](const f32x4 (&v)[FILL]) {
#pragma unroll
        for (int u = 0; u < FILL; ++u) {
            const int idx = threadIdx.x + u * 64 * RANK_WAVES, t = idx / (RANK_CK / 4), q = idx % (RANK_CK / 4);
            *reinterpret_cast<f32x4 *>(tile + t * RANK_PITCH + 4 * q) = v[u];
        }
    };
    // The rows of the NEXT tile (their first RANK_CK columns) are gathered into registers while this tile runs, and its ids one tile
    // further ahead: the gather's latency hides under the MFMAs and the epilogue.
    f32x4 pre[FILL];
    int64_t next_id = load_id(tile_beg);
    if (tile_beg < tile_end) {
        if (threadIdx.x < RANK_TILE) tile_id[0][threadIdx.x] = next_id;
        __syncthreads();
        gather(tile_id[0], 0, pre);
        next_id = load_id(tile_beg + 1);
    }
    for (int64_t tl = tile_beg; tl < tile_end; ++tl) {
        const int64_t j0 = tl * RANK_TILE;
        const int buf = (int)((tl - tile_beg) & 1);
        __syncthreads();                                                 // the previous tile and the other id buffer have been consumed
        put(pre);
        if (threadIdx.x < RANK_TILE) tile_id[buf ^ 1][threadIdx.x] = next_id;
        __syncthreads();
        if (tl + 1 < tile_end) gather(tile_id[buf ^ 1], 0, pre);
        next_id = load_id(tl + 2);
        f32x4 acc[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) acc[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto chunk = [&](int ck, auto a_of) {
            if (ck > 0) {                                                // further columns: filled in place
                __syncthreads();
                f32x4 v[FILL];
                gather(tile_id[buf], ck, v);
                put(v);
                __syncthreads();
            }
#pragma unroll
            for (int T = 0; T < RANK_CK / 16; ++T) {
                if (ck * RANK_CK + 16 * T >= a.C) break;
                const f32x4 av = a_of(ck * (RANK_CK / 16) + T);
                f32x4 bv[4];
#pragma unroll
                for (int sub = 0; sub < 4; ++sub)
                    bv[sub] = *reinterpret_cast<const f32x4 *>(tile + (16 * sub + c) * RANK_PITCH + 16 * T + 4 * g);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int sub = 0; sub < 4; ++sub) acc[sub] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv[sub][t], acc[sub], 0, 0, 0);
            }
        };
        if constexpr (NG > 0) {
#pragma unroll
            for (int ck = 0; ck < (NG + 3) / 4; ++ck) {
                if (ck >= n_chunks) break;
                chunk(ck, [&](int G) { return areg[G < NG ? G : NG - 1]; });
            }
        } else {
            for (int ck = 0; ck < n_chunks; ++ck) chunk(ck, [&](int G) { return load_a4(a, a_row, 16 * G + 4 * g); });
        }

        // the epilogue: D register i of column tile sub = (row 4 g + i, candidate j0 + 16 sub + c)
        bool cand_ok[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) cand_ok[sub] = tile_id[buf][16 * sub + c] >= 0;
        if (a.scores) {
#pragma unroll
            for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (cand_ok[sub] && row_in[i]) a.scores[(src0 + 4 * g + i) * a.K + j0 + 16 * sub + c] = acc[sub][i];
        }
        // the counts over ALL candidates.  A score below (above) every positive score of its row adds n_pos (nothing); when one of the
        // lane's four scores of a row lies between them, all four are compared with the row's positives, four per LDS read (the list
        // is padded with NaN, which compares false).
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!row_ok[i] || row_np[i] == 0) continue;
            bool between = false;
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) between |= cand_ok[sub] && !(acc[sub][i] < row_mn[i]) && !(acc[sub][i] > row_mx[i]);
            if (!between) {
#pragma unroll
                for (int sub = 0; sub < 4; ++sub)
                    if (cand_ok[sub] && acc[sub][i] < row_mn[i]) n_less[i] += (unsigned long long)row_np[i];
                continue;
            }
            uint32_t below = 0, same = 0;                                // at most 4 RANK_POS_PASS each
            const int in_lds = row_np[i] < RANK_POS_PASS ? row_np[i] : RANK_POS_PASS;
            for (int p = 0; p < in_lds; p += 4) {
                const f32x4 ps = *reinterpret_cast<const f32x4 *>(&pos_lds[wave][4 * g + i][p]);
#pragma unroll
                for (int sub = 0; sub < 4; ++sub) {
                    if (!cand_ok[sub]) continue;
                    const float x = acc[sub][i];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        below += x < ps[t];
                        same += x == ps[t];
                    }
                }
            }
            n_less[i] += below;
            n_equal[i] += same;
            for (int p = RANK_POS_PASS; p < row_np[i]; ++p) {
                const float ps = a.pos_scores[pos_lo[wave][4 * g + i] + p];
#pragma unroll
                for (int sub = 0; sub < 4; ++sub) {
                    n_less[i] += cand_ok[sub] && acc[sub][i] < ps;
                    n_equal[i] += cand_ok[sub] && acc[sub][i] == ps;
                }
            }
        }
        // the running top-k: an entry above the row's threshold is looked up in the adjacency, and enters if the pair is not linked
        bool inserted = false;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const int64_t j = j0 + 16 * sub + c;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float x = acc[sub][i];
                const bool live = cand_ok[sub] && row_ok[i];
                const uint64_t key = rank_key(x, 0x80000000u | (uint32_t)j);
                bool pass = live && key > thr[i];
                if (pass) {                                              // only now: is the pair linked?
                    const int64_t s = src_id[wave][4 * g + i], id = tile_id[buf][16 * sub + c];
                    pass = id != s && !rank_stored(a.g_rowptr, a.g_colidx, a.g_rows, s, id) &&
                           !rank_stored(a.g_rowptr, a.g_colidx, a.g_rows, id, s);
                }
                uint64_t mask = __ballot(pass);
                while (mask) {
                    const int src = __ffsll((unsigned long long)mask) - 1;
                    mask &= mask - 1;
                    const uint64_t kk = ((uint64_t)(uint32_t)__shfl((int)(key >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)key, src);
                    topk_insert(topk[wave][4 * (src >> 4) + i], k, kk, lane);
                    inserted = true;
                }
            }
            if (inserted) {
#pragma unroll
                for (int i = 0; i < 4; ++i) thr[i] = ((volatile uint64_t *)topk[wave][4 * g + i])[k - 1];
            }
        }
    }

    // the counts of a row sit in the 16 lanes of its g
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) {
            n_less[i] += (unsigned long long)__shfl_xor((long long)n_less[i], d);
            n_equal[i] += (unsigned long long)__shfl_xor((long long)n_equal[i], d);
        }
        if (c == 0 && row_ok[i]) {
            if (n_less[i]) atomicAdd(a.less + src0 + 4 * g + i, n_less[i]);
            if (n_equal[i]) atomicAdd(a.equal + src0 + 4 * g + i, n_equal[i]);
        }
    }
    __builtin_amdgcn_wave_barrier();
    for (int rr = 0; rr < 16; ++rr) {
        const int64_t i = src0 + rr;
        if (i < a.S && lane < k) a.part_keys[(i * a.splits + part) * k + lane] = ((volatile uint64_t *)topk[wave][rr])[lane];
    }
}

// ---- finish -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_rank_finish(const RankArgs a) {
    __shared__ uint64_t list[RANK_MAX_K];
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const int64_t i = blockIdx.x;
    const int k = a.k;
    int64_t *__restrict__ ids = a.top_ids + i * k;
    float *__restrict__ sc = a.top_scores + i * k;
    uint8_t *__restrict__ isp = a.top_is_pos + i * k;
    if (a.n_neg[i] == -1) {                                              // a source or a held-out id out of range: the outputs say so
        if (lane < k) {
            ids[lane] = -1;
            sc[lane] = -__builtin_inff();
            isp[lane] = 0;
        }
        return;
    }
    const int64_t s = a.sources[i];
    int64_t lo, n;
    pos_range(a, i, lo, n);
    if (lane < RANK_MAX_K) list[lane] = 0;
    __builtin_amdgcn_wave_barrier();

    // the list's best k: the positives, then the parts in part order (any order gives the same list: the order of the keys is total)
    uint64_t thr = 0;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t p = base + lane;
        const uint64_t key = p < n ? rank_key(a.pos_scores[lo + p], (uint32_t)p) : 0;
        if (topk_offer(list, k, key > thr, key, lane)) thr = ((volatile uint64_t *)list)[k - 1];
    }
    const uint64_t *__restrict__ parts = a.part_keys + i * a.splits * k;
    for (int64_t base = 0; base < (int64_t)a.splits * k; base += 64) {
        const int64_t p = base + lane;
        const uint64_t key = p < (int64_t)a.splits * k ? parts[p] : 0;
        if (topk_offer(list, k, key > thr, key, lane)) thr = ((volatile uint64_t *)list)[k - 1];
    }

    // the excluded pairs: out-neighbours, in-neighbours that are not out-neighbours too, the source itself unless its loop is stored
    const float *__restrict__ src_row = a.F + s * a.ldf;
    const int64_t out_beg = s < a.g_rows ? a.g_rowptr[s] : 0, n_out = s < a.g_rows ? a.g_rowptr[s + 1] - out_beg : 0;
    const int64_t in_beg = s < a.t_rows ? a.t_rowptr[s] : 0, n_in = s < a.t_rows ? a.t_rowptr[s + 1] - in_beg : 0;
    const int64_t n_list = n_out + n_in + 1;
    unsigned long long d_less = 0, d_equal = 0, n_excluded = 0;
    for (int64_t base = 0; base < n_list; base += 64) {                  // 64 lookups at a time, then 16 pairs per MFMA pass
        const int64_t e = base + lane;
        int64_t v = -1;
        if (e < n_out) v = a.g_colidx[out_beg + e];
        else if (e < n_out + n_in) {
            v = a.t_colidx[in_beg + e - n_out];
            if (rank_stored(a.g_rowptr, a.g_colidx, a.g_rows, s, v)) v = -1;
        } else if (e == n_out + n_in && !rank_stored(a.g_rowptr, a.g_colidx, a.g_rows, s, s)) v = s;
        if (v >= a.n_rows_F) v = -1;                                     // such a candidate was skipped
        if (v >= 0) {
            const int64_t j = cand_lower(a.cand, a.K, v);
            if (j >= a.K || a.cand[j] != v) v = -1;
        }
        if (__ballot(v >= 0) == 0) continue;
        for (int sub = 0; sub < 4 && base + 16 * sub < n_list; ++sub) {
            const int64_t vv = __shfl((long long)v, 16 * sub + c);
            const bool ok = vv >= 0;
            const float x = wave_pair_scores(a, src_row, ok ? a.F + vv * a.ldf : nullptr, g);
            n_excluded += ok && g == 0;
            for (int64_t p = g; p < n; p += 4) {
                const float ps = a.pos_scores[lo + p];
                d_less += ok && x < ps;
                d_equal += ok && x == ps;
            }
        }
    }
    d_less = wave_sum(d_less);
    d_equal = wave_sum(d_equal);
    n_excluded = wave_sum(n_excluded);
    if (lane == 0) {
        const int64_t in_range = cand_lower(a.cand, a.K, a.n_rows_F) - cand_lower(a.cand, a.K, 0);
        a.n_neg[i] = in_range - (int64_t)n_excluded;
        a.less[i] -= d_less;
        a.equal[i] -= d_equal;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < k) {
        const uint64_t key = ((volatile uint64_t *)list)[lane];
        const uint32_t code = (uint32_t)key;
        if (key == 0) {
            ids[lane] = -1;
            sc[lane] = -__builtin_inff();
            isp[lane] = 0;
        } else {
            const bool stranger = (code & 0x80000000u) != 0;
            ids[lane] = stranger ? a.cand[code & 0x7FFFFFFFu] : a.pos_ids[lo + code];
            sc[lane] = rank_key_score(key);
            isp[lane] = stranger ? 0 : 1;
        }
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// the number of candidate parts a launch runs: what was asked for, or enough parts to fill the device, never more than there are tiles
inline int64_t rank_splits(int64_t S, int64_t K, int64_t splits) {
    const int64_t n_tiles = (K + RANK_TILE - 1) / RANK_TILE;
    const int64_t blocks = (S + 16 * RANK_WAVES - 1) / (16 * RANK_WAVES);
    int64_t want = splits > 0 ? splits : (RANK_TARGET_BLOCKS + blocks - 1) / (blocks > 0 ? blocks : 1);
    if (want > RANK_MAX_SPLITS) want = RANK_MAX_SPLITS;
    if (want > n_tiles) want = n_tiles;
    return want < 1 ? 1 : want;
}

inline bool rank_sizes_ok(int64_t S, int64_t P, int64_t K, int64_t k, int64_t splits) {
    return S >= 0 && S < ((int64_t)1 << 31) && P >= 0 && P < ((int64_t)1 << 31) && K >= 0 && K < ((int64_t)1 << 31) && k >= 1 &&
           k <= RANK_MAX_K && splits >= 0 && splits <= RANK_MAX_SPLITS;
}

inline size_t rank_bytes(int64_t S, int64_t P, int64_t K, int64_t k, int64_t splits) {
    return align256((size_t)P * sizeof(float)) + align256((size_t)S * (size_t)rank_splits(S, K, splits) * (size_t)k * sizeof(uint64_t));
}

}  // namespace

extern "C" {

int64_t gnx_rank_candidates_bytes(int64_t S, int64_t P, int64_t K, int64_t k, int64_t splits) {
    if (!rank_sizes_ok(S, P, K, k, splits)) {
        gnx::set_error("gnx_rank_candidates_bytes: S, P and K must be in [0, 2^31), k in [1, %d], splits in [0, %d]", RANK_MAX_K,
                       (int)RANK_MAX_SPLITS);
        return -1;
    }
    return (int64_t)rank_bytes(S, P, K, k, splits);
}

int gnx_rank_candidates(gnx_graph_t g, const float *d_F, int64_t ldf, int64_t n_rows_F, int64_t C, const float *d_r, const int64_t *d_sources,
                        int64_t S, const int64_t *d_pos_ptr, const int64_t *d_pos_ids, int64_t P, const int64_t *d_candidates, int64_t K,
                        int64_t k, int64_t splits, int64_t *d_n_pos, int64_t *d_n_neg, int64_t *d_less, int64_t *d_equal, int64_t *d_top_ids,
                        float *d_top_scores, uint8_t *d_top_is_pos, float *d_scores, void *d_workspace, int64_t bytes, void *stream) {
    GNX_CHECK_ARG(S >= 0 && S < ((int64_t)1 << 31) && P >= 0 && P < ((int64_t)1 << 31) && K >= 0 && K < ((int64_t)1 << 31),
                  "gnx_rank_candidates: S, P and K must be in [0, 2^31)");
    GNX_CHECK_ARG(k >= 1 && k <= RANK_MAX_K, "gnx_rank_candidates: k must be in [1, %d]", RANK_MAX_K);
    GNX_CHECK_ARG(splits >= 0 && splits <= RANK_MAX_SPLITS, "gnx_rank_candidates: splits must be in [0, %d]", (int)RANK_MAX_SPLITS);
    GNX_CHECK_ARG(C >= 1 && C < ((int64_t)1 << 31) && ldf >= C && n_rows_F >= 0 && n_rows_F < ((int64_t)1 << 31),
                  "gnx_rank_candidates: bad sizes (C >= 1, ldf >= C, n_rows_F in [0, 2^31))");
    GNX_CHECK_ARG(g != nullptr, "gnx_rank_candidates: NULL handle");
    if (S == 0) return GNX_OK;
    GNX_CHECK_ARG(d_F && d_sources && d_pos_ptr, "gnx_rank_candidates: NULL pointer (d_F, d_sources, d_pos_ptr)");
    GNX_CHECK_ARG(d_pos_ids || P == 0, "gnx_rank_candidates: NULL pointer (d_pos_ids) with P > 0");
    GNX_CHECK_ARG(d_candidates || K == 0, "gnx_rank_candidates: NULL pointer (d_candidates) with K > 0");
    GNX_CHECK_ARG(d_n_pos && d_n_neg && d_less && d_equal && d_top_ids && d_top_scores && d_top_is_pos,
                  "gnx_rank_candidates: NULL pointer (an output)");
    GNX_CHECK_ARG(d_workspace, "gnx_rank_candidates: NULL pointer (d_workspace)");
    GNX_CHECK_ARG(aligned16(d_workspace), "gnx_rank_candidates: d_workspace must be 16-byte aligned");
    const size_t need = rank_bytes(S, P, K, k, splits);
    GNX_CHECK_ARG(bytes >= (int64_t)need, "gnx_rank_candidates: d_workspace holds %lld bytes, gnx_rank_candidates_bytes(S, P, K, k, splits) = %lld",
                  (long long)bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    const int rc = gnx::ensure_transpose(g, s);                          // the in-neighbours; built once (gnx_graph_reserve before a capture)
    if (rc != GNX_OK) return rc;

    RankArgs a;
    a.g_rowptr = g->a.rowptr.get(); a.g_colidx = g->a.colidx.get(); a.g_rows = g->a.n_rows;
    a.t_rowptr = g->t.rowptr.get(); a.t_colidx = g->t.colidx.get(); a.t_rows = g->t.n_rows;
    a.F = d_F; a.ldf = ldf; a.n_rows_F = n_rows_F; a.C = (int)C; a.r = d_r;
    a.vec = ldf % 4 == 0 && aligned16(d_F);
    a.sources = d_sources; a.S = S;
    a.pos_ptr = d_pos_ptr; a.pos_ids = d_pos_ids; a.P = P;
    a.cand = d_candidates; a.K = K;
    a.k = (int)k;
    a.splits = (int)rank_splits(S, K, splits);
    const int64_t n_tiles = (K + RANK_TILE - 1) / RANK_TILE;
    a.tiles_per_part = (n_tiles + a.splits - 1) / a.splits;
    a.n_pos = d_n_pos; a.n_neg = d_n_neg;
    a.less = reinterpret_cast<unsigned long long *>(d_less); a.equal = reinterpret_cast<unsigned long long *>(d_equal);
    a.top_ids = d_top_ids; a.top_scores = d_top_scores; a.top_is_pos = d_top_is_pos; a.scores = d_scores;
    char *ws = static_cast<char *>(d_workspace);
    a.pos_scores = reinterpret_cast<float *>(ws);
    a.part_keys = reinterpret_cast<uint64_t *>(ws + align256((size_t)P * sizeof(float)));

    hipLaunchKernelGGL(k_rank_prepare, dim3(blocks_for(S, 4)), dim3(256), 0, s, a);
    const dim3 grid(blocks_for(S, 16 * RANK_WAVES), (unsigned)a.splits), block(64 * RANK_WAVES);
    if (C <= 16) hipLaunchKernelGGL(k_rank_tiles<1>, grid, block, 0, s, a);
    else if (C <= 64) hipLaunchKernelGGL(k_rank_tiles<4>, grid, block, 0, s, a);
    else if (C <= 128) hipLaunchKernelGGL(k_rank_tiles<8>, grid, block, 0, s, a);
    else if (C <= 256) hipLaunchKernelGGL(k_rank_tiles<16>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_rank_tiles<0>, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_rank_finish, dim3((unsigned)S), dim3(64), 0, s, a);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

}  // extern "C"
