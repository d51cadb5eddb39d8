// The link task on the device: what LinkPrediction does around the link head (gnx_heads.hip: gnx_edge_scores) every step.
//
//   gnx_sample_negatives              every positive pair followed by `samples` corrupted pairs   reference gnntf/core/gnn/graph_predictor.py:52-98
//   gnx_edge_plan                     the endpoints of an edge list, stably sorted by node
//   gnx_edge_scores_backward_sorted   dF[x, :] += the terms of the positions that name x, in a FIXED order: no float atomics
//                                                                                                  reference gnntf/core/gnn/graph_predictor.py:122-146
//
// Ids are range-checked in the kernels, never dereferenced out of bounds.  Nothing here allocates or waits: every entry records into a
// hipGraph (the sort and the compaction of the plan run in the caller's workspace).
#include <cstring>
#include <string.h>

#include "gnx_internal.h"

#include <rocprim/rocprim.hpp>

namespace {

using namespace gnx;

// ---- the sampler ------------------------------------------------------------------------------------------------------------------------
// whether (row, col) is a stored entry: the columns of a row ascend, values are not read
__device__ __forceinline__ bool stored(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t row, int64_t col) {
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

// one thread per slot e = i * samples + s; the thread of s == 0 copies the positive row as well.  At most max_tries draws per slot.
__global__ __launch_bounds__(256) void k_sample_negatives(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t n_rows,
                                                           const int64_t *__restrict__ positive, int64_t m, int64_t samples,
                                                           const int64_t *__restrict__ candidates, uint64_t K, int64_t max_tries, uint64_t seed,
                                                           uint64_t stream, const uint64_t *__restrict__ counter, int64_t *__restrict__ edges,
                                                           unsigned long long *__restrict__ fallbacks) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m * samples) return;
    const int64_t i = e / samples, s = e - i * samples;
    const int64_t u = positive[2 * i], v = positive[2 * i + 1];
    int64_t *__restrict__ group = edges + 2 * i * (1 + samples);
    if (s == 0) {
        group[0] = u;
        group[1] = v;
    }
    int64_t *__restrict__ slot = group + 2 * (1 + s);
    slot[0] = u;
    if (u < 0 || u >= n_rows || v < 0 || v >= n_rows) {                 // nothing to look up: the score kernel answers -1 with NaN
        slot[1] = -1;
        return;
    }
    const uint64_t st = stream + (counter ? *counter : 0);
    const uint64_t key = seed ^ (st * 0xD1342543DE82EF95ull);            // hash_key's first round depends on (seed, stream, slot) alone
    const uint64_t slot_key = rng_fin(key + (uint64_t)e * 0x9E3779B97F4A7C15ull);
    int64_t w = -1;
    bool accepted = false;
    for (int64_t t = 0; t < max_tries && !accepted; ++t) {
        const uint64_t hi = hash_rank(slot_key ^ ((uint64_t)(2 * t) * 0xC2B2AE3D27D4EB4Full), 0);
        const uint64_t lo = hash_rank(slot_key ^ ((uint64_t)(2 * t + 1) * 0xC2B2AE3D27D4EB4Full), 0);
        const uint64_t x = (hi << 24) | lo;                              // 48 bits
        const uint64_t j = __umul64hi(x << 16, K);                       // floor(x K / 2^48) < K
        w = candidates ? candidates[j] : (int64_t)j;
        accepted = w != u && w != v && !stored(rowptr, colidx, u, w) && !(w >= 0 && w < n_rows && stored(rowptr, colidx, w, u));
    }
    if (!accepted) atomicAdd(fallbacks, 1ull);
    slot[1] = w;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------------
constexpr int EDGE_CHUNK = 256;      // positions of one node that one lane group adds up; part of the interface (include/gnx.h)

__global__ __launch_bounds__(256) void k_plan_keys(const int64_t *__restrict__ edges, int64_t n2, int64_t n_rows, uint32_t *__restrict__ keys,
                                                    int32_t *__restrict__ pos) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n2) return;
    const int64_t x = edges[q], y = edges[q ^ 1];
    keys[q] = (x < 0 || x >= n_rows || y < 0 || y >= n_rows) ? (uint32_t)n_rows : (uint32_t)x;
    pos[q] = (int32_t)q;
}

// flag[p] = sorted index p begins a chunk: its distance to the first index of its key is a multiple of EDGE_CHUNK
__global__ __launch_bounds__(256) void k_plan_heads(const uint32_t *__restrict__ keys, int64_t n2, uint32_t bucket, uint8_t *__restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n2) return;
    const uint32_t key = keys[p];
    bool head = false;
    if (key < bucket) {
        if (p == 0 || keys[p - 1] != key) head = true;
        else if (p >= EDGE_CHUNK && keys[p - EDGE_CHUNK] == key) {       // only then can the distance reach EDGE_CHUNK
            int64_t lo = 0, hi = p - EDGE_CHUNK;                         // the first index of the key: keys[hi] == key already
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (keys[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            head = ((p - lo) & (EDGE_CHUNK - 1)) == 0;
        }
    }
    flag[p] = head ? 1 : 0;
}

struct PlanLayout {
    size_t keys_in, pos_in, flags, temp, temp_bytes, total;
};

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline unsigned key_bits(int64_t n_rows) {
    unsigned b = 1;
    while (b < 32 && ((uint64_t)n_rows >> b) != 0) ++b;
    return b;
}

// rocprim's calling convention: with a null temporary a call only reports the bytes it needs
hipError_t plan_sort(void *tmp, size_t &bytes, uint32_t *k_in, uint32_t *k_out, int32_t *p_in, int32_t *p_out, size_t n2, unsigned bits,
                     hipStream_t s) {
    return rocprim::radix_sort_pairs(tmp, bytes, k_in, k_out, p_in, p_out, n2, 0u, bits, s);
}

hipError_t plan_select(void *tmp, size_t &bytes, uint8_t *flags, int32_t *out, int32_t *count, size_t n2, hipStream_t s) {
    return rocprim::select(tmp, bytes, rocprim::counting_iterator<int32_t>(0), flags, out, count, n2, s);
}

int plan_layout(int64_t m, PlanLayout &l) {
    const size_t n2 = 2 * (size_t)m;
    size_t sort_bytes = 0, select_bytes = 0;
    GNX_HIP(plan_sort(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, n2, 32u, nullptr));
    GNX_HIP(plan_select(nullptr, select_bytes, nullptr, nullptr, nullptr, n2, nullptr));
    l.keys_in = 0;
    l.pos_in = l.keys_in + align256(n2 * sizeof(uint32_t));
    l.flags = l.pos_in + align256(n2 * sizeof(int32_t));
    l.temp = l.flags + align256(n2);
    l.temp_bytes = align256(sort_bytes > select_bytes ? sort_bytes : select_bytes);
    l.total = l.temp + l.temp_bytes;
    return GNX_OK;
}

// ---- the backward -----------------------------------------------------------------------------------------------------------------------
// Sorted index p of the plan holds position q = pos[p] = 2 i + side of the edge list: it names node keys[p] = edges[q], whose row of dF
// receives t_q[c] = fl(fl(g_i r[c]) F[edges[q ^ 1], c]).  The positions of a node are consecutive in p and ascend in q (the sort is
// stable); they are cut into chunks of EDGE_CHUNK counted from the node's first index, and chunks[1 ..] lists the first index of every
// chunk.  One lane group adds a chunk up, term after term; a node of one chunk is finished there, the chunk sums of a longer one go
// through the slab and are added in chunk order by k_edge_back_long.
struct EdgeBack {
    const float *F;
    int64_t ldf, n_rows;
    int C;
    const int64_t *edges;
    const float *r, *g;
    float *dF;
    int64_t ldg;
    const uint32_t *keys;
    const int32_t *pos, *chunks;
    int64_t n2;
    float *slab;          // [2 * half, C]: a full chunk that starts at p in row (p + 255) / 256 -- the one multiple of 256 it covers --, a
    int64_t half;         // shorter (last) one in row half + p / 256: the last chunks of two long nodes start more than 256 apart
    int vec_g, vec_slab;  // 16-byte accesses of dF / of the slab are aligned
};

__device__ __forceinline__ int64_t slab_row(const EdgeBack &a, int64_t p, bool full) {
    return full ? (p + EDGE_CHUNK - 1) / EDGE_CHUNK : a.half + p / EDGE_CHUNK;
}

// the term and the running sum, each rounded on its own (the pragma and not __fmul_rn / __fadd_rn, which HIP defines as the plain operators)
__device__ __forceinline__ float edge_term(float gi, float rc, bool has_r, float f) {
#pragma clang fp contract(off)
    const float w = has_r ? gi * rc : gi;
    return w * f;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

template <int PER>
__device__ __forceinline__ void load_cols(const float *__restrict__ src, float (&v)[PER]) {
    if constexpr (PER == 4) {
        const float4 x = *reinterpret_cast<const float4 *>(src);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
        v[0] = src[0];
    }
}

// dst[0 .. PER) = (accumulate ? dst : 0) + v, with one 16-byte access where `vec` says it is aligned
template <int PER>
__device__ __forceinline__ void put_cols(float *__restrict__ dst, const float (&v)[PER], bool vec, bool accumulate) {
    if constexpr (PER == 4) {
        if (vec) {
            float4 x = make_float4(v[0], v[1], v[2], v[3]);
            if (accumulate) {
                const float4 d = *reinterpret_cast<const float4 *>(dst);
                x = make_float4(add_rn(d.x, x.x), add_rn(d.y, x.y), add_rn(d.z, x.z), add_rn(d.w, x.w));
            }
            *reinterpret_cast<float4 *>(dst) = x;
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) dst[k] = accumulate ? add_rn(dst[k], v[k]) : v[k];
}

__device__ __forceinline__ int64_t chunk_count(const EdgeBack &a) {
    const int64_t n = a.chunks[0];
    return n < 0 ? 0 : (n > a.n2 ? a.n2 : n);
}

// W lanes per chunk; a lane owns PER = 4 (VEC: 16-byte loads of F) or 1 consecutive columns of every pass of W * PER columns
template <int W, bool VEC>
__global__ __launch_bounds__(256) void k_edge_back_chunks(EdgeBack a) {
    constexpr int PER = VEC ? 4 : 1;
    const int lane = threadIdx.x & (W - 1);
    const int shift = (threadIdx.x & 63) & ~(W - 1);                     // the group's first lane in its wave
    const uint64_t group_mask = ~0ull >> (64 - W);
    const int64_t n_groups = (int64_t)gridDim.x * (256 / W), n_chunks = chunk_count(a);
    const bool has_r = a.r != nullptr;
    for (int64_t k = (int64_t)blockIdx.x * (256 / W) + threadIdx.x / W; k < n_chunks; k += n_groups) {
        const int64_t p0 = a.chunks[1 + k];
        if (p0 < 0 || p0 >= a.n2) continue;
        const uint32_t key = a.keys[p0];
        if ((int64_t)key >= a.n_rows) continue;
        const bool first = p0 == 0 || a.keys[p0 - 1] != key;
        for (int base = 0; base < a.C; base += W * PER) {
            const int c0 = base + lane * PER;
            const bool active = c0 < a.C;
            float rr[PER], acc[PER];
#pragma unroll
            for (int x = 0; x < PER; ++x) { rr[x] = (has_r && active) ? a.r[c0 + x] : 1.0f; acc[x] = 0.f; }
            bool have = false;
            int len = 0;
            for (int b = 0; b < EDGE_CHUNK; b += W) {                    // W positions at a time: lane j reads what position b + j needs
                const int64_t p = p0 + b + lane;
                const bool in = p < a.n2 && a.keys[p] == key;
                int64_t other = -1;
                float gi = 0.f;
                if (in) {
                    const int64_t q = a.pos[p];
                    if (q >= 0 && q < a.n2) {
                        other = a.edges[q ^ 1];
                        gi = a.g[q >> 1];
                        if (other < 0 || other >= a.n_rows) other = -1;  // a list that changed since it was planned: never dereferenced
                    }
                }
                const int cnt = __popcll((__ballot(in) >> shift) & group_mask);      // the positions of a key are consecutive
                for (int j = 0; j < cnt; j += 4) {
                    float f[4][PER], gg[4];
                    bool ok[4];
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        const int64_t o = __shfl(other, (j + x) & (W - 1), W);
                        gg[x] = __shfl(gi, (j + x) & (W - 1), W);
                        ok[x] = j + x < cnt && o >= 0 && active;
                        if (ok[x]) load_cols<PER>(a.F + o * a.ldf + c0, f[x]);
                    }
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        if (!ok[x]) continue;
#pragma unroll
                        for (int y = 0; y < PER; ++y) {
                            const float t = edge_term(gg[x], rr[y], has_r, f[x][y]);
                            acc[y] = have ? add_rn(acc[y], t) : t;
                        }
                        have = true;
                    }
                }
                len += cnt;
                if (cnt < W) break;
            }
            if (!active) continue;
            const bool full = len == EDGE_CHUNK;
            const bool longer = !first || (full && p0 + EDGE_CHUNK < a.n2 && a.keys[p0 + EDGE_CHUNK] == key);
            if (longer) put_cols<PER>(a.slab + slab_row(a, p0, full) * a.C + c0, acc, a.vec_slab, false);
            else if (have) put_cols<PER>(a.dF + (int64_t)key * a.ldg + c0, acc, a.vec_g, true);
        }
    }
}

// the nodes of more than one chunk: the group of a node's FIRST chunk adds its chunk sums in chunk order and then once into dF
template <int W>
__global__ __launch_bounds__(256) void k_edge_back_long(EdgeBack a) {
    const int lane = threadIdx.x & (W - 1);
    const int64_t n_groups = (int64_t)gridDim.x * (256 / W), n_chunks = chunk_count(a);
    for (int64_t k = (int64_t)blockIdx.x * (256 / W) + threadIdx.x / W; k < n_chunks; k += n_groups) {
        const int64_t p0 = a.chunks[1 + k];
        if (p0 < 0 || p0 + EDGE_CHUNK >= a.n2) continue;
        const uint32_t key = a.keys[p0];
        if ((int64_t)key >= a.n_rows || (p0 > 0 && a.keys[p0 - 1] == key) || a.keys[p0 + EDGE_CHUNK] != key) continue;
        for (int c = lane; c < a.C; c += W) {
            float s = a.slab[slab_row(a, p0, true) * a.C + c];
            for (int64_t p = p0 + EDGE_CHUNK; p < a.n2 && a.keys[p] == key; p += EDGE_CHUNK) {
                const bool full = p + EDGE_CHUNK - 1 < a.n2 && a.keys[p + EDGE_CHUNK - 1] == key;
                s = add_rn(s, a.slab[slab_row(a, p, full) * a.C + c]);
            }
            float *__restrict__ dst = a.dF + (int64_t)key * a.ldg + c;
            *dst = add_rn(*dst, s);
        }
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// at most this many blocks walk the chunk list: 8 blocks of 4 waves per CU of the largest part
constexpr int64_t BACK_BLOCKS = 2048;

template <int W>
void launch_edge_back(const EdgeBack &a, bool vec, hipStream_t s) {
    const int64_t want = (a.n2 + 256 / W - 1) / (256 / W);
    const dim3 grid((unsigned)(want < BACK_BLOCKS ? want : BACK_BLOCKS));
    if (vec) hipLaunchKernelGGL((k_edge_back_chunks<W, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_edge_back_chunks<W, false>), grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_edge_back_long<W>), grid, dim3(256), 0, s, a);
}

inline int64_t slab_half(int64_t m) { return 2 * m / EDGE_CHUNK + 2; }

}  // namespace

extern "C" {

int gnx_sample_negatives(gnx_graph_t g, const int64_t *d_positive, int64_t m, int64_t samples, const int64_t *d_candidates, int64_t K,
                         int64_t max_tries, uint64_t seed, uint64_t stream_id, int64_t *d_edges, unsigned long long *d_fallbacks,
                         void *stream) {
    GNX_CHECK_ARG(m >= 0, "gnx_sample_negatives: m is negative");
    GNX_CHECK_ARG(samples >= 1, "gnx_sample_negatives: samples must be at least 1");
    GNX_CHECK_ARG(max_tries >= 1, "gnx_sample_negatives: max_tries must be at least 1");
    GNX_CHECK_ARG(K >= 1 && K < ((int64_t)1 << 31), "gnx_sample_negatives: K must be in [1, 2^31)");
    GNX_CHECK_ARG(samples < ((int64_t)1 << 31) && m * samples < ((int64_t)1 << 31), "gnx_sample_negatives: m * samples must be below 2^31");
    GNX_CHECK_ARG(g != nullptr, "gnx_sample_negatives: NULL handle");
    GNX_CHECK_ARG(d_candidates || K == g->a.n_rows, "gnx_sample_negatives: K must be the handle's row count when d_candidates is NULL");
    if (m == 0) return GNX_OK;
    GNX_CHECK_ARG(d_positive && d_edges && d_fallbacks, "gnx_sample_negatives: NULL pointer (d_positive, d_edges, d_fallbacks)");
    hipLaunchKernelGGL(k_sample_negatives, dim3(blocks_for(m * samples)), dim3(256), 0, (hipStream_t)stream, g->a.rowptr.get(),
                       g->a.colidx.get(), g->a.n_rows, d_positive, m, samples, d_candidates, (uint64_t)K, max_tries, seed, stream_id,
                       g->stream_offset, d_edges, d_fallbacks);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int64_t gnx_edge_plan_bytes(int64_t m) {
    if (m < 0 || m >= ((int64_t)1 << 30)) {
        gnx::set_error("gnx_edge_plan_bytes: m must be in [0, 2^30)");
        return -1;
    }
    PlanLayout l;
    if (plan_layout(m, l) != GNX_OK) return -1;
    return (int64_t)l.total;
}

int gnx_edge_plan(const int64_t *d_edges, int64_t m, int64_t n_rows, uint32_t *d_keys, int32_t *d_pos, int32_t *d_chunks, void *d_workspace,
                  int64_t bytes, void *stream) {
    GNX_CHECK_ARG(m >= 0 && m < ((int64_t)1 << 30), "gnx_edge_plan: m must be in [0, 2^30)");
    GNX_CHECK_ARG(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "gnx_edge_plan: n_rows must be in [0, 2^31)");
    GNX_CHECK_ARG(d_chunks, "gnx_edge_plan: NULL pointer (d_chunks)");
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) {                                                        // an empty chunk list: the backward of no edges reads nothing else
        GNX_HIP(hipMemsetAsync(d_chunks, 0, sizeof(int32_t), s));
        return GNX_OK;
    }
    GNX_CHECK_ARG(d_edges && d_keys && d_pos && d_workspace, "gnx_edge_plan: NULL pointer (d_edges, d_keys, d_pos, d_workspace)");
    GNX_CHECK_ARG(aligned16(d_workspace), "gnx_edge_plan: d_workspace must be 16-byte aligned");
    PlanLayout l;
    const int rc = plan_layout(m, l);
    if (rc != GNX_OK) return rc;
    GNX_CHECK_ARG(bytes >= (int64_t)l.total, "gnx_edge_plan: d_workspace holds %lld bytes, gnx_edge_plan_bytes(m) = %lld", (long long)bytes,
                  (long long)l.total);
    const int64_t n2 = 2 * m;
    char *ws = static_cast<char *>(d_workspace);
    uint32_t *keys_in = reinterpret_cast<uint32_t *>(ws + l.keys_in);
    int32_t *pos_in = reinterpret_cast<int32_t *>(ws + l.pos_in);
    uint8_t *flags = reinterpret_cast<uint8_t *>(ws + l.flags);
    size_t temp_bytes = l.temp_bytes;
    hipLaunchKernelGGL(k_plan_keys, dim3(blocks_for(n2)), dim3(256), 0, s, d_edges, n2, n_rows, keys_in, pos_in);
    GNX_HIP(plan_sort(ws + l.temp, temp_bytes, keys_in, d_keys, pos_in, d_pos, (size_t)n2, key_bits(n_rows), s));
    hipLaunchKernelGGL(k_plan_heads, dim3(blocks_for(n2)), dim3(256), 0, s, d_keys, n2, (uint32_t)n_rows, flags);
    temp_bytes = l.temp_bytes;
    GNX_HIP(plan_select(ws + l.temp, temp_bytes, flags, d_chunks + 1, d_chunks, (size_t)n2, s));
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int64_t gnx_edge_sorted_work_floats(int64_t m, int64_t C) {
    if (m < 0 || m >= ((int64_t)1 << 30) || C < 1) {
        gnx::set_error("gnx_edge_sorted_work_floats: m must be in [0, 2^30) and C at least 1");
        return -1;
    }
    return 2 * slab_half(m) * C;
}

int gnx_edge_scores_backward_sorted(const float *d_F, int64_t ldf, int64_t n_rows, int64_t C, const int64_t *d_edges, int64_t m,
                                    const float *d_r, const float *d_grad_out, float *d_grad_F, int64_t ldg, const uint32_t *d_keys,
                                    const int32_t *d_pos, const int32_t *d_chunks, float *d_work, int64_t work_floats, void *stream) {
    GNX_CHECK_ARG(m >= 0 && m < ((int64_t)1 << 30) && C >= 1 && C < ((int64_t)1 << 31) && n_rows >= 0 && n_rows < ((int64_t)1 << 31) &&
                      ldf >= C && ldg >= C,
                  "gnx_edge_scores_backward_sorted: bad sizes");
    if (m == 0) return GNX_OK;
    GNX_CHECK_ARG(d_F && d_edges && d_grad_out && d_grad_F, "gnx_edge_scores_backward_sorted: NULL pointer");
    GNX_CHECK_ARG(d_keys && d_pos && d_chunks, "gnx_edge_scores_backward_sorted: NULL plan (d_keys, d_pos, d_chunks)");
    GNX_CHECK_ARG(d_work && work_floats >= 2 * slab_half(m) * C,
                  "gnx_edge_scores_backward_sorted: d_work must hold gnx_edge_sorted_work_floats(m, C) floats");
    EdgeBack a;
    a.F = d_F; a.ldf = ldf; a.n_rows = n_rows; a.C = (int)C;
    a.edges = d_edges; a.r = d_r; a.g = d_grad_out;
    a.dF = d_grad_F; a.ldg = ldg;
    a.keys = d_keys; a.pos = d_pos; a.chunks = d_chunks;
    a.n2 = 2 * m;
    a.slab = d_work; a.half = slab_half(m);
    const bool quads = C % 4 == 0;
    a.vec_g = quads && ldg % 4 == 0 && aligned16(d_grad_F);
    a.vec_slab = quads && aligned16(d_work);
    const bool vec = quads && ldf % 4 == 0 && aligned16(d_F);
    // the narrowest group whose lanes cover a row in one pass, as the SpMM picks its lane groups from C; 64 lanes pass over wider rows
    const int64_t per_pass = vec ? C / 4 : C;
    hipStream_t s = (hipStream_t)stream;
    if (per_pass <= 4) launch_edge_back<4>(a, vec, s);
    else if (per_pass <= 8) launch_edge_back<8>(a, vec, s);
    else if (per_pass <= 16) launch_edge_back<16>(a, vec, s);
    else if (per_pass <= 32) launch_edge_back<32>(a, vec, s);
    else launch_edge_back<64>(a, vec, s);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

}  // extern "C"
