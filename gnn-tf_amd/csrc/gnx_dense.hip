// The dense transform on gfx950 matrix cores: the pre-MLP, the Dense layers and the transform of the GCN / GCNII layers.
//
//   gnx_dense      out = act(X . W + b)                      reference gnntf/core/nn/layers.py:135-136 (Dense),
//                                                            gnntf/core/gnn/architectures/gcn.py:89 (the transform of GCNLayer)
//   gnx_dense_drop out = drop_out(act(drop_in(X) . W + b))   a Dropout layer, the Dense behind it and the Dense's own dropout
//                                                            (layers.py:125-136, 175-181) in the same launch: the DROP form of the
//                                                            three kernels below, the masks of drop_values (gnx_layer_device.h)
//
// gnx_dense is a tall-and-skinny GEMM (N rows in the millions, F and O in the tens to hundreds): float32 in, float32
// accumulate on v_mfma_f32_16x16x4_f32 (bit-for-bit a k-ordered fmaf chain, no reduced precision).  A 256-thread block owns
// 64 rows; each of its 4 waves keeps a 16-row x O accumulator strip in registers.  X is read ONCE, straight from HBM into
// the A operand (16 bytes per lane; the k index inside a 16-wide step is permuted so that a lane's four consecutive floats
// feed four MFMAs), W streams through LDS in K chunks shared by the block (row stride = 4 mod 32 banks: the four k-groups
// of a wave read disjoint banks).  Arithmetic intensity is O/2 flop per byte of X: HBM-bound up to O = 32, MFMA-bound beyond.
// Tall inputs (n >= 16K rows) take one of two persistent kernels instead: k_dense_wreg (W in registers, shapes up to 256 x 64) or
// k_dense_ring (W in LDS); both stream X through per-wave LDS-DMA rings and add the k terms in the same order as this kernel.
// Which of the three a column panel takes: dense_kernel_for.  (The weight gradient: gnx_dense_wgrad.hip; the task heads: gnx_heads.hip.)
// Tried and dropped (round 2): a persistent W-resident variant (W once in LDS, the whole K extent of a 16-row tile in
// registers, next tile prefetched, no barrier in the loop) -- 5.1 ms vs 4.2 ms at 10M x 256 -> 64: with two waves per SIMD the
// 64-byte-per-row A loads no longer hide (a 256 -> 7 product ran at 3.2 TB/s); the chunked kernel's eight blocks per CU do.
#include <mutex>

#include "gnx_dense_device.h"
#include "gnx_layer_device.h"

namespace {

struct DenseArgs {
    const float *X; int64_t ldx; int64_t n; int F;
    const float *W; int64_t ldw; int O;
    const float *bias;            // [O] or null
    int act;
    float *out; int64_t ldo;
    const int32_t *out_rows;      // optional: result row r goes to out[out_rows[r]]
    const int32_t *in_rows;       // optional: input row r is X[in_rows[r]]
    bool w_aligned;               // W rows start 16-byte aligned (ldw % 4 == 0, aligned base): float4 loads of W
    const float *zeros = nullptr; // 16 bytes of device zeros (k_dense_wreg with padded widths stages them for the columns past F)
};

// What the DROP instantiations take beside the panel (gnx_dense_drop): the two masks of out = drop_out(act(drop_in(X) . W + b)) as the
// feature-dropout pass takes them (DropFuse: seed, stream, offset, thr, scale; drop_values, gnx_layer_device.h) and the panel's first
// output column (the output mask is keyed by the column of the whole result).  thr == 0 on a side: nothing is hashed there.  The
// instantiations without DROP take DenseArgs as it stands.
template <bool DROP> struct DenseArgsD : DenseArgs {};
template <> struct DenseArgsD<true> : DenseArgs {
    DropFuse din, dout;
    int col0;
};

// x <- drop(x) for the four consecutive columns col .. col + 3 of row `row` that a lane holds as one fragment
__device__ __forceinline__ void drop_fragment(const DropFuse &f, uint64_t stream, int64_t row, int64_t col, f32x4 &x) {
    float v[4] = {x[0], x[1], x[2], x[3]};
    drop_values<4>(f, stream, row, col, v);
    x = f32x4{v[0], v[1], v[2], v[3]};
}

template <int NT> struct DenseCfg {
    static constexpr int OP = NT * 16;                 // padded output width
    static constexpr int KC = NT <= 4 ? 64 : 32;       // W rows per LDS chunk
    static constexpr int STRIDE = OP + 4;              // OP is a multiple of 16; +4 makes row stride = 4 (mod 8): see header
};

constexpr int DENSE_WAVES = 8;       // waves (16-row strips) per block: 128 rows share one W chunk in LDS

template <int NT, bool ALIGNED, bool DROP = false>
__global__ __launch_bounds__(64 * DENSE_WAVES) void k_dense_mfma(const DenseArgsD<DROP> p) {
    using Cfg = DenseCfg<NT>;
    __shared__ float Ws[Cfg::KC * Cfg::STRIDE];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * (16 * DENSE_WAVES) + wave * 16;
    int64_t arow = row0 + c < p.n ? row0 + c : p.n - 1;                  // rows past the end read a valid row and are not stored
    if (p.in_rows) arow = p.in_rows[arow];
    const float *__restrict__ xrow = p.X + arow * p.ldx;
    [[maybe_unused]] uint64_t in_stream = 0, out_stream = 0;
    if constexpr (DROP) { in_stream = drop_stream(p.din); out_stream = drop_stream(p.dout); }
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // A values of one K chunk: 16 bytes per lane and 16-wide step, straight from HBM into the MFMA operand registers
    auto load_a = [&](int k0, float (&a)[Cfg::KC / 16][4]) {
#pragma unroll
        for (int T = 0; T < Cfg::KC / 16; ++T) {
            const int kb = k0 + 16 * T + 4 * g;
            if (ALIGNED && kb + 3 < p.F) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(xrow + kb);
                a[T][0] = v[0]; a[T][1] = v[1]; a[T][2] = v[2]; a[T][3] = v[3];
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) a[T][t] = kb + t < p.F ? xrow[kb + t] : 0.f;
            }
            if constexpr (DROP) {                                          // the input mask, on the fragment as loaded (columns past F hold zeros)
                if (p.din.thr != 0 && kb < p.F) drop_values<4>(p.din, in_stream, arow, kb, a[T]);
            }
        }
    };
    float a[Cfg::KC / 16][4], a_next[Cfg::KC / 16][4];
    load_a(0, a);
    for (int k0 = 0; k0 < p.F; k0 += Cfg::KC) {
        __syncthreads();                                                   // the previous chunk has been consumed
        for (int idx = threadIdx.x; idx < Cfg::KC * (Cfg::OP / 4); idx += 64 * DENSE_WAVES) {      // 16 bytes of W per thread and step
            const int r = idx / (Cfg::OP / 4), cc = (idx % (Cfg::OP / 4)) * 4;
            const int k = k0 + r;
            f32x4 w = f32x4{0.f, 0.f, 0.f, 0.f};
            if (k < p.F) {
                const float *__restrict__ wr = p.W + (int64_t)k * p.ldw + cc;
                if (p.w_aligned && cc + 3 < p.O) w = *reinterpret_cast<const f32x4 *>(wr);
                else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) if (cc + t < p.O) w[t] = wr[t];
                }
            }
            *reinterpret_cast<f32x4 *>(Ws + r * Cfg::STRIDE + cc) = w;
        }
        if (k0 + Cfg::KC < p.F) load_a(k0 + Cfg::KC, a_next);              // the next chunk's rows are in flight under this chunk's MFMAs
        __syncthreads();
#pragma unroll
        for (int T = 0; T < Cfg::KC / 16; ++T) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float *__restrict__ wrow = Ws + (16 * T + 4 * g + t) * Cfg::STRIDE + c;   // B[k-slot g][col c] = W[k0 + 16T + 4g + t][16 nt + c]
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[T][t], wrow[16 * nt], acc[nt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int T = 0; T < Cfg::KC / 16; ++T)
#pragma unroll
            for (int t = 0; t < 4; ++t) a[T][t] = a_next[T][t];
    }
    // D layout: lane (c, g), register r -> row 4g + r, column 16 nt + c
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = 16 * nt + c;
        if (col >= p.O) continue;
        const float b = p.bias ? p.bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = row0 + 4 * g + r;
            if (row >= p.n) continue;
            float v = acc[nt][r] + b;
            if (p.act == GNX_ACT_RELU) v = fmaxf(v, 0.f);
            if constexpr (DROP) {                                          // the output mask, after bias and relu
                if (p.dout.thr != 0) {
                    float one[1] = {v};
                    drop_values<1>(p.dout, out_stream, row, p.col0 + col, one);
                    v = one[0];
                }
            }
            const int64_t orow = p.out_rows ? (int64_t)p.out_rows[row] : row;
            p.out[orow * p.ldo + col] = v;
        }
    }
}

// ---- the same product with X through LDS in full lines (LDS-DMA ring), W resident in LDS --------------------------------------
// k_dense_mfma loads the A operand "fragment-shaped": one wave instruction fetches 64 bytes of each of 16 rows, so every 128-byte
// line of X is touched twice and the CU's L1 pipe does twice the line work of a row-contiguous read; its 32 A registers per lane
// also cap the occupancy.  Here every wave owns 16-row tiles and streams their K chunks (64 floats = two whole lines per row)
// into a private RING of LDS stages by LDS-DMA (global_load_lds_dwordx4: no VGPR destination, four 1-KiB wave instructions per
// stage, each writing four rows), keeps RING - 1 stages in flight behind a counted s_waitcnt vmcnt, and reads the A fragments
// back with ds_read_b128.  The LDS image is lane-linear (an LDS-DMA cannot pad or scatter), so the 16-byte pieces of a row are
// XOR-swizzled by the row index on the SOURCE address; the fragment reads of a wave are then conflict-free.  W ([F, O], at most
// 64 KB) is laid out once per block as [k][column group][c][4] so that a lane's four accumulator columns are ONE ds_read_b128,
// again conflict-free (row stride = a multiple of the 256-byte bank row).  The block is persistent (one per CU, WAVES waves, no
// barrier inside the loop: a wave only ever reads what it staged itself), walks tiles of 16 rows, and adds the k terms in the same
// order as k_dense_mfma: same bits.
constexpr int RING_BK = 64;            // floats of one row per stage

// One stage of either ring is 16 rows x 64 floats, the 16-byte pieces of a row XOR-swizzled by the row index on the source address.
// Read back by lane (c, g): the A fragment X[row c][16 T + 4 g .. + 3] of the stage at A, one conflict-free ds_read_b128.
__device__ __forceinline__ f32x4 stage_fragment(const float *A, int c, int g, int T) {
    return *reinterpret_cast<const f32x4 *>(A + c * RING_BK + 4 * ((4 * T + g) ^ c));
}

template <int NT, int WAVES, int RING, bool DROP = false>
__global__ __launch_bounds__(64 * WAVES) void k_dense_ring(const DenseArgsD<DROP> p, int64_t n_tiles) {
    static_assert(NT % 4 == 0, "the W image groups the accumulator columns in fours");
    constexpr int NQ = NT / 4;                                    // column groups of 4 x 16 outputs
    constexpr int STAGE = 16 * RING_BK;                           // floats per stage: 16 rows x 64
    extern __shared__ float lds[];                                // ONE array: [W image: F * NT * 16 floats][WAVES][RING][STAGE]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int w_floats = p.F * NT * 16;
    float *__restrict__ Wl = lds;
    float *__restrict__ ring = lds + w_floats + wave * (RING * STAGE);
    // W image: Wl[(k * NQ + q) * 64 + cc * 4 + j] = W[k][16 (4 q + j) + cc]
    for (int idx = threadIdx.x; idx < p.F * NT * 16; idx += 64 * WAVES) {
        const int k = idx / (NT * 16), col = idx % (NT * 16);      // col = 16 nt + cc: coalesced reads of W's row
        const int nt = col >> 4, cc = col & 15;
        Wl[(k * NQ + (nt >> 2)) * 64 + cc * 4 + (nt & 3)] = col < p.O ? p.W[(int64_t)k * p.ldw + col] : 0.f;
    }
    float bias[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) bias[nt] = (p.bias && 16 * nt + c < p.O) ? p.bias[16 * nt + c] : 0.f;
    __syncthreads();                                              // the only barrier: W is in place
    [[maybe_unused]] uint64_t in_stream = 0, out_stream = 0;
    if constexpr (DROP) { in_stream = drop_stream(p.din); out_stream = drop_stream(p.dout); }

    const int kchunks = p.F / RING_BK;
    const int64_t tile_stride = (int64_t)gridDim.x * WAVES;
    const int64_t first = (int64_t)blockIdx.x * WAVES + wave;
    const int64_t my_tiles = first < n_tiles ? (n_tiles - first + tile_stride - 1) / tile_stride : 0;
    const int64_t steps = my_tiles * kchunks;                     // (tile, K chunk) pairs, walked in order

    // Staging runs RING - 1 steps ahead of the arithmetic: (pf_tile, pf_kc) is the next step to stage, counted up without divisions.
    // One stage = four LDS-DMA instructions, lane l -> row 4 i + l / 16, 16-byte slot l % 16 of that row, filled with piece slot ^ row.
    int64_t pf_tile = first, pf_step = 0;
    int pf_kc = 0;
    auto issue_next = [&]() {
        float *dst = ring + (pf_step % RING) * STAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * i + (lane >> 4);
            int64_t row = pf_tile * 16 + r;
            row = row < p.n ? row : p.n - 1;                      // rows past the end read a valid row and are not stored
            const float *src = p.X + row * p.ldx + pf_kc * RING_BK + 4 * ((lane & 15) ^ r);
            __builtin_amdgcn_global_load_lds(src, dst + i * 256, 16, 0, 0);
        }
        ++pf_step;
        if (++pf_kc == kchunks) { pf_kc = 0; pf_tile += tile_stride; }
    };
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < RING - 1 && s0 < steps; ++s0) issue_next();
    int64_t step = 0;
    for (int64_t tile = first; tile < n_tiles; tile += tile_stride) {
        for (int kc = 0; kc < kchunks; ++kc, ++step) {
            // the reads of stage step - 1 (the slot that stage step + RING - 1 overwrites) were consumed by its MFMAs: drain them, then restage
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (pf_step < steps) issue_next();
            // all but the youngest 4 (RING - 1) vector-memory operations are done => stage `step` has landed (stores issued in between only
            // make the wait stricter); near the end fewer stages are in flight behind it
            const int64_t behind = steps - 1 - step;
            if (behind >= RING - 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 * (RING - 1)) : "memory");
            else if (RING > 2 && behind == RING - 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 * (RING > 2 ? RING - 2 : 0)) : "memory");
            else if (RING > 3 && behind == RING - 3) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 * (RING > 3 ? RING - 3 : 0)) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const float *__restrict__ A = ring + (step % RING) * STAGE;
            if constexpr (NQ <= 2) {
                // the stage's A fragments up front (X[row c][16 T + 4 g .. + 3]), the B fragments one k step ahead of the MFMAs that use
                // them: the wave hides its own LDS latency instead of waiting for every fragment it has just asked for
                f32x4 a4[RING_BK / 16];
#pragma unroll
                for (int T = 0; T < RING_BK / 16; ++T) a4[T] = stage_fragment(A, c, g, T);
                if constexpr (DROP) {                                         // the input mask, on the fragments as read back (the LDS-DMA cannot mask)
                    if (p.din.thr != 0) {
#pragma unroll
                        for (int T = 0; T < RING_BK / 16; ++T) drop_fragment(p.din, in_stream, tile * 16 + c, kc * RING_BK + 16 * T + 4 * g, a4[T]);
                    }
                }
                const float *__restrict__ Wk = Wl + ((kc * RING_BK + 4 * g) * NQ) * 64 + c * 4;      // fragment of k = kc 64 + 4 g (+ 16 T + t)
                f32x4 b[2][NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) b[0][q] = *reinterpret_cast<const f32x4 *>(Wk + q * 64);
#pragma unroll
                for (int st = 0; st < RING_BK / 4; ++st) {                    // st = 4 T + t
                    const int T = st >> 2, t = st & 3;
                    if (st + 1 < RING_BK / 4) {
                        const int T1 = (st + 1) >> 2, t1 = (st + 1) & 3;
#pragma unroll
                        for (int q = 0; q < NQ; ++q) b[(st + 1) & 1][q] = *reinterpret_cast<const f32x4 *>(Wk + ((16 * T1 + t1) * NQ + q) * 64);
                    }
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[4 * q + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[T][t], b[st & 1][q][j], acc[4 * q + j], 0, 0, 0);
                }
                // pin that order for the scheduler (it would otherwise sink every read next to its first use and wait for all of them):
                // the A fragments and the first B fragment, then { next B fragment, this step's MFMAs } sixteen times
                __builtin_amdgcn_sched_group_barrier(0x100, RING_BK / 16 + NQ, 0);
#pragma unroll
                for (int st = 0; st < RING_BK / 4; ++st) {
                    if (st + 1 < RING_BK / 4) __builtin_amdgcn_sched_group_barrier(0x100, NQ, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 4 * NQ, 0);
                }
            } else {
                // wide outputs (O = 192 / 256): sixteen accumulator tiles leave no room for fragments in flight (measured: +5 % with them)
#pragma unroll
                for (int T = 0; T < RING_BK / 16; ++T) {
                    f32x4 a4 = stage_fragment(A, c, g, T);
                    if constexpr (DROP) {
                        if (p.din.thr != 0) drop_fragment(p.din, in_stream, tile * 16 + c, kc * RING_BK + 16 * T + 4 * g, a4);
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int k = kc * RING_BK + 16 * T + 4 * g + t;
#pragma unroll
                        for (int q = 0; q < NQ; ++q) {
                            const f32x4 b4 = *reinterpret_cast<const f32x4 *>(Wl + (k * NQ + q) * 64 + c * 4);
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                acc[4 * q + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[t], b4[j], acc[4 * q + j], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // the tile is complete.  D layout: lane (c, g), register r -> row 4 g + r, column 16 nt + c
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = 16 * nt + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = tile * 16 + 4 * g + r;
                float v = acc[nt][r] + bias[nt];
                if (p.act == GNX_ACT_RELU) v = fmaxf(v, 0.f);
                if constexpr (DROP) {                                         // the output mask, after bias and relu
                    if (p.dout.thr != 0 && col < p.O && row < p.n) {
                        float one[1] = {v};
                        drop_values<1>(p.dout, out_stream, row, p.col0 + col, one);
                        v = one[0];
                    }
                }
                if (col < p.O && row < p.n) p.out[row * p.ldo + col] = v;
            }
            acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

template <int NT, int WAVES, int RING, bool DROP>
int launch_ring_as(const DenseArgsD<DROP> &p, hipStream_t s) {
    const size_t lds_bytes = ((size_t)p.F * NT * 16 + (size_t)WAVES * RING * 16 * RING_BK) * sizeof(float);
    const int cus = persistent_launch<k_dense_ring<NT, WAVES, RING, DROP>>();
    if (cus < 0) return cus;
    const int64_t n_tiles = (p.n + 15) / 16;
    const unsigned grid = (unsigned)std::min<int64_t>((n_tiles + WAVES - 1) / WAVES, cus);
    hipLaunchKernelGGL((k_dense_ring<NT, WAVES, RING, DROP>), dim3(grid), dim3(64 * WAVES), lds_bytes, s, p, n_tiles);
    return GNX_OK;
}

// Waves per block: as many 2-stage rings (8 KB each) as fit beside the W image in the CU's 160 KB of LDS, up to 16 -- measured at
// 10M x 256 -> 64: 4 waves x 4 stages 4.14 ms, 8 x 2 3.54, 8 x 3 3.61, 12 x 2 3.41 (k_dense_mfma: 3.59); the matrix pipe wants
// three waves per SIMD more than it wants a deeper ring.
template <int NT, bool DROP>
int launch_ring(const DenseArgsD<DROP> &p, bool, hipStream_t s) {
    const size_t w_bytes = (size_t)p.F * NT * 16 * sizeof(float);
    const size_t rings = ((160u << 10) - w_bytes) / (2 * 16 * RING_BK * sizeof(float));
    // DROP: the hashes in flight need registers -- no more waves than build without scratch at NT accumulator tiles (12 at NT = 8, 8 above)
    constexpr int MOST = !DROP || NT <= 4 ? 16 : NT <= 8 ? 12 : 8;
    if constexpr (MOST >= 16) {
        if (rings >= 16) return launch_ring_as<NT, 16, 2, DROP>(p, s);
    }
    if constexpr (MOST >= 12) {
        if (rings >= 12) return launch_ring_as<NT, 12, 2, DROP>(p, s);
    }
    return launch_ring_as<NT, 8, 2, DROP>(p, s);
}

// ---- W in REGISTERS, X through a deep LDS-DMA ring ---------------------------------------------------------------------------------
// When the whole W fits the register file -- (F / 4) x NT fragments per lane, 256 for the pre-MLP's 256 -> 64 -- a wave keeps it there
// for the life of the (persistent) block: no LDS read per MFMA at all, and the CU's LDS is ALL staging ring.  One wave per SIMD (512
// registers each), so the matrix pipe is fed by a single straight-line instruction stream, and everything that is not an MFMA has to
// sit in the issue slots between two of them:
//   * W is the MFMA's A operand and the X fragment its B operand (out^T = W^T X^T): a lane then holds FOUR CONSECUTIVE output columns
//     of one row, so a tile is stored with four 16-byte stores instead of sixteen 4-byte ones;
//   * two accumulator sets: the stores of tile t are in the same basic block as the first MFMAs of the wave's next tile (no branch:
//     only the wave's LAST tile, the one that can be ragged, takes the guarded path);
//   * staging addresses are 32-bit row x 32-bit pitch (one v_mad_u64_u32 per load); the stage's K offset and LDS slot are compile-time;
//   * staging never stops (past the wave's last tile it re-stages the last row tile, which nobody reads), so "all but the youngest
//     4 (RING - 2) vector-memory operations" is the wait for every stage (stores in between only make it stricter).
// Same k order as the other two kernels: same bits.  Measured (10M x 256 -> 64, profiles/NOTES.md): the ring depth does not matter from
// 4 stages up and the staging waits are never taken -- what the launch costs beyond the MFMAs is issue slots and the clock.
// PAD: F < 64 KS and / or O < 16 NT (both multiples of 4): the columns of X past F are staged from a block of zeros (times the zero rows
// W gets there: exact, whatever X holds), the columns past O are neither loaded from W nor stored.
// DROP: the input mask is applied to a stage's fragments as they are read back from the ring (`fragments` is told the tile and the K
// chunk of the stage it reads), the output mask in `finish`; the hash runs in the issue slots between the MFMAs.
template <int NT, int KS, int RING, bool RELU, bool PAD, bool DROP = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_dense_wreg(const DenseArgsD<DROP> p, int64_t n_tiles64) {
    constexpr int STAGE = 16 * RING_BK;
    extern __shared__ float lds[];                                // [4 waves][RING][STAGE]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 15, g = lane >> 4;
    float *__restrict__ ring = lds + wave * (RING * STAGE);
    // W fragments: wreg[kc][T][t][nt] = W[64 kc + 16 T + 4 g + t][16 nt + c]
    float wreg[KS][4][4][NT];
#pragma unroll
    for (int kc = 0; kc < KS; ++kc)
#pragma unroll
        for (int T = 0; T < 4; ++T)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                {
                    const int k = 64 * kc + 16 * T + 4 * g + t, col = 16 * nt + c;
                    wreg[kc][T][t][nt] = (!PAD || (k < p.F && col < p.O)) ? p.W[(int64_t)k * p.ldw + col] : 0.f;
                    asm volatile("" : "+a"(wreg[kc][T][t][nt]));      // W lives in the accumulation half of the register file; the MFMAs read it there
                }
    f32x4 bias[NT];                                               // columns 16 nt + 4 g .. + 3
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) bias[nt][r] = (p.bias && (!PAD || 16 * nt + 4 * g + r < p.O)) ? p.bias[16 * nt + 4 * g + r] : 0.f;

    const uint32_t n_tiles = (uint32_t)n_tiles64, n_rows = (uint32_t)p.n;
    const uint32_t f_pieces = (uint32_t)p.F / 4;
    const uint32_t tile_stride = gridDim.x * 4, first = blockIdx.x * 4 + wave;
    const uint32_t x_pitch = (uint32_t)p.ldx * 4u, o_pitch = (uint32_t)p.ldo * 4u;      // bytes
    const char *__restrict__ Xb = reinterpret_cast<const char *>(p.X);
    char *__restrict__ Ob = reinterpret_cast<char *>(p.out);
    [[maybe_unused]] uint64_t in_stream = 0, out_stream = 0;
    if constexpr (DROP) { in_stream = drop_stream(p.din); out_stream = drop_stream(p.dout); }
    uint32_t piece[4];                                            // byte offset of this lane's 16-byte piece inside the stage's 256 bytes of row 4 i + g
#pragma unroll
    for (int i = 0; i < 4; ++i) piece[i] = 16u * (uint32_t)(c ^ (4 * i + g));
    uint32_t pf_tile = first;
    auto issue = [&](int pf_kc, int slot) {                       // both compile-time at every call site
        const uint32_t t16 = (pf_tile < n_tiles ? pf_tile : n_tiles - 1) * 16u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t row = t16 + 4 * i + g;
            row = row < n_rows ? row : n_rows - 1;                // rows past the end read a valid row and are not stored
            const char *src = Xb + (uint64_t)row * x_pitch + (uint32_t)(pf_kc * RING_BK * 4) + piece[i];
            if constexpr (PAD) {
                if ((uint32_t)(pf_kc * (RING_BK / 4)) + piece[i] / 16u >= f_pieces) src = reinterpret_cast<const char *>(p.zeros);
            }
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const float *>(src), ring + slot * STAGE + i * 256, 16, 0, 0);
        }
        if (pf_kc == KS - 1) pf_tile += tile_stride;
    };
    // X[row c][16 T + 4 g .. + 3] of the stage in `slot`; DROP: the stage is K chunk `kc` of tile `tile`
    auto fragments = [&](int slot, f32x4 (&a)[4], [[maybe_unused]] uint32_t tile, [[maybe_unused]] int kc) {
        const float *__restrict__ A = ring + slot * STAGE;
#pragma unroll
        for (int T = 0; T < 4; ++T) a[T] = stage_fragment(A, c, g, T);
        if constexpr (DROP) {
            if (p.din.thr != 0) {
#pragma unroll
                for (int T = 0; T < 4; ++T) {
                    const int col = kc * RING_BK + 16 * T + 4 * g;
                    if (!PAD || col < p.F) drop_fragment(p.din, in_stream, (int64_t)(tile * 16u + c), col, a[T]);     // (the zeros past F need no hash)
                }
            }
        }
    };
    // D layout with W as the A operand: lane (c, g), register r -> row c, column 16 nt + 4 g + r
    auto finish = [&](const f32x4 &acc, int nt, [[maybe_unused]] uint32_t row) {
        f32x4 v = acc + bias[nt];
        if constexpr (RELU) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        if constexpr (DROP) {                                     // the output mask, after bias and relu
            if (p.dout.thr != 0) drop_fragment(p.dout, out_stream, (int64_t)row, p.col0 + 16 * nt + 4 * g, v);
        }
        return v;
    };
    auto store_row = [&](f32x4 (&acc)[NT], uint32_t row) {
        char *o = Ob + (uint64_t)row * o_pitch + 16u * g;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            if (!PAD || 16 * nt + 4 * g < p.O) *reinterpret_cast<f32x4 *>(o + 64 * nt) = finish(acc[nt], nt, row);
    };
    auto store_tile = [&](f32x4 (&acc)[NT], uint32_t tile) { store_row(acc, tile * 16u + c); };      // a full tile: no guards
    auto store_last = [&](f32x4 (&acc)[NT], uint32_t tile) {      // the wave's last tile: may be the ragged one
        if (tile * 16u + c < n_rows) store_row(acc, tile * 16u + c);
    };
    f32x4 afrag[2][4];                                            // the X fragments of the stage being multiplied and of the next one
    // one tile: KS stages; `slot0` is the ring slot of its first stage (compile-time).  With EPI, the stores of the wave's previous tile
    // sit among the first stage's MFMAs.
    // `tile`: the tile being multiplied (DROP: the row key of the fragments read for its stages and for the first stage of the next one)
    auto tile_body = [&](auto epi, int slot0, f32x4 (&acc)[NT], f32x4 (&prev)[NT], uint32_t prev_tile, [[maybe_unused]] uint32_t tile) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < KS; ++kc) {
            const int slot = (slot0 + kc) % RING;
            f32x4 (&a_cur)[4] = afrag[kc & 1];
            f32x4 (&a_nxt)[4] = afrag[(kc + 1) & 1];
            // a_cur was read out of `slot`; the slot before it is free (its fragments were consumed by the previous stage's MFMAs)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            issue((kc + RING - 1) % KS, (slot + RING - 1) % RING);
            if constexpr (decltype(epi)::value) {
                if (kc == 0) store_tile(prev, prev_tile);
            }
#pragma unroll
            for (int T = 0; T < 3; ++T)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[kc][T][t][nt], a_cur[T][t], acc[nt], 0, 0, 0);
            // the next stage: RING - 2 younger stages may still be in flight behind it
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 * (RING - 2)) : "memory");
            fragments((slot + 1) % RING, a_nxt, kc == KS - 1 ? tile + tile_stride : tile, (kc + 1) % KS);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[kc][3][t][nt], a_cur[3][t], acc[nt], 0, 0, 0);
        }
    };
    static_assert(KS % 2 == 0, "the fragment registers alternate per stage: a tile must start on the same one every time");
    static_assert((2 * KS) % RING == 0, "two tiles must take a whole number of ring turns (their slots are compile-time)");
    if (first < n_tiles) {
#pragma unroll
        for (int s0 = 0; s0 < RING - 1; ++s0) issue(s0 % KS, s0);
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 * (RING - 2)) : "memory");          // stage 0 has landed
        fragments(0, afrag[0], first, 0);
        f32x4 accA[NT], accB[NT];
        uint32_t tile = first;
        constexpr int SLOT_B = KS % RING;                         // first slot of every second tile
        tile_body(std::false_type{}, 0, accA, accB, 0u, tile);
        for (;;) {
            if (tile + tile_stride >= n_tiles) { store_last(accA, tile); break; }
            tile_body(std::true_type{}, SLOT_B, accB, accA, tile, tile + tile_stride);
            tile += tile_stride;
            if (tile + tile_stride >= n_tiles) { store_last(accB, tile); break; }
            tile_body(std::true_type{}, 0, accA, accB, tile, tile + tile_stride);
            tile += tile_stride;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // nothing of this wave may still be writing LDS when the block retires
}

// a block of zeros on the CURRENT device (one per device the process drives; never freed)
const float *device_zeros() {
    static std::mutex lock;
    static float *z[64] = {};
    const int dev = PerDeviceOnce::device();
    if (dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> hold(lock);
    if (!z[dev]) {
        float *q = nullptr;
        if (hipMalloc((void **)&q, 256) != hipSuccess) return nullptr;
        if (hipMemset(q, 0, 256) != hipSuccess) { (void)hipFree(q); return nullptr; }
        z[dev] = q;
    }
    return z[dev];
}

template <int NT, int KS, int RING, bool RELU, bool PAD, bool DROP>
int launch_wreg_as(const DenseArgsD<DROP> &p, hipStream_t s) {
    const size_t lds_bytes = (size_t)4 * RING * 16 * RING_BK * sizeof(float);
    const int cus = persistent_launch<k_dense_wreg<NT, KS, RING, RELU, PAD, DROP>>();
    if (cus < 0) return cus;
    const int64_t n_tiles = (p.n + 15) / 16;
    const unsigned grid = (unsigned)std::min<int64_t>((n_tiles + 3) / 4, cus);
    hipLaunchKernelGGL((k_dense_wreg<NT, KS, RING, RELU, PAD, DROP>), dim3(grid), dim3(256), lds_bytes, s, p, n_tiles);
    return GNX_OK;
}

template <int NT, int KS, int RING, bool DROP>
int launch_wreg(const DenseArgsD<DROP> &p0, bool, hipStream_t s) {
    DenseArgsD<DROP> p = p0;
    const bool pad = p.F != 64 * KS || p.O != 16 * NT;
    if (pad) {
        p.zeros = device_zeros();
        if (!p.zeros) return GNX_ERR_ALLOC;
        return p.act == GNX_ACT_RELU ? launch_wreg_as<NT, KS, RING, true, true, DROP>(p, s) : launch_wreg_as<NT, KS, RING, false, true, DROP>(p, s);
    }
    return p.act == GNX_ACT_RELU ? launch_wreg_as<NT, KS, RING, true, false, DROP>(p, s) : launch_wreg_as<NT, KS, RING, false, false, DROP>(p, s);
}

template <int NT, bool DROP>
int launch_dense(const DenseArgsD<DROP> &p, bool aligned, hipStream_t s) {
    const unsigned grid = (unsigned)((p.n + 16 * DENSE_WAVES - 1) / (16 * DENSE_WAVES));
    if (aligned) hipLaunchKernelGGL((k_dense_mfma<NT, true, DROP>), dim3(grid), dim3(64 * DENSE_WAVES), 0, s, p);
    else         hipLaunchKernelGGL((k_dense_mfma<NT, false, DROP>), dim3(grid), dim3(64 * DENSE_WAVES), 0, s, p);
    return GNX_OK;
}

// Which kernel, with which template arguments, a column panel takes (p: the panel, at most 256 outputs, nt = its 16-column accumulator
// tiles; x_aligned: X in whole float4 rows, i.e. a 16-byte base and ldx % 4 == 0).  The rules, in this order:
//   tall = x_aligned, no row maps, n >= 16K rows: what both persistent kernels need.
//   1. k_dense_wreg<NT, KS, RING>: tall; n < 2^31 and ldx, ldo < 2^30 (it addresses by 32-bit row x byte pitch); out in whole float4 rows
//      (16-byte base, ldo % 4 == 0); F and O multiples of 4; and W within 256 registers per lane once padded to 64 KS x 16 NT:
//        128 < F <= 256:   O <= 32 -> <2, 4, 8>    O <= 64 -> <4, 4, 8>     wider: not this kernel
//         64 < F <= 128:   O <= 64 -> <4, 2, 4>    O <= 128 -> <8, 2, 4>    wider: not this kernel
//   2. k_dense_ring<NT = nt>: tall; F a multiple of 64; nt a multiple of 4 (accumulator columns go in groups of four); the W image of
//      F x 16 nt floats within 64 KB.
//   3. k_dense_mfma<NT, ALIGNED = x_aligned>: every other panel, row maps included; NT = nt rounded up to one of 1 2 3 4 6 8 12 16.
// The alignment of W decides nothing here: p.w_aligned only picks how k_dense_mfma loads W; the other two load it once, by the word.
// (tuning builds: GNX_DENSE_WREG=0 skips rule 1, GNX_DENSE_RING=0 rule 2, for A/B runs)
// DROP (gnx_dense_drop) takes the same rules: whichever kernel carries a shape adds the k terms in the same order and hashes the same keys.
template <bool DROP> using DenseLaunch = int (*)(const DenseArgsD<DROP> &p, bool x_aligned, hipStream_t s);

template <bool DROP>
DenseLaunch<DROP> dense_kernel_for(const DenseArgsD<DROP> &p, bool x_aligned) {
    const int nt = (p.O + 15) / 16;
    const bool tall = x_aligned && p.in_rows == nullptr && p.out_rows == nullptr && p.n >= 16 * 1024;
    const bool out_aligned = aligned(p.out, 16) && p.ldo % 4 == 0;
    if (tall && tuning_switch("GNX_DENSE_WREG") && out_aligned && p.F % 4 == 0 && p.O % 4 == 0 && p.n < (1ll << 31) && p.ldx < (1ll << 30) &&
        p.ldo < (1ll << 30)) {
        // DROP: with W in 256 registers (<4, 4, 8>, <8, 2, 4>) the hashes of a stage do not fit beside it (the build spills 132 .. 472
        // bytes per lane): those panels take rule 2 or 3
        if (p.F > 128 && p.F <= 256) {
            if (p.O <= 32) return launch_wreg<2, 4, 8, DROP>;
            if constexpr (!DROP) {
                if (p.O <= 64) return launch_wreg<4, 4, 8, DROP>;
            }
        } else if (p.F > 64 && p.F <= 128) {
            if (p.O <= 64) return launch_wreg<4, 2, 4, DROP>;
            if constexpr (!DROP) {
                if (p.O <= 128) return launch_wreg<8, 2, 4, DROP>;
            }
        }
    }
    if (tall && tuning_switch("GNX_DENSE_RING") && p.F % RING_BK == 0 && nt % 4 == 0 && (int64_t)p.F * nt * 16 * 4 <= (64 << 10))
        return nt == 4 ? launch_ring<4, DROP> : nt == 8 ? launch_ring<8, DROP> : nt == 12 ? launch_ring<12, DROP> : launch_ring<16, DROP>;
    return nt <= 1 ? launch_dense<1, DROP> : nt <= 2 ? launch_dense<2, DROP> : nt <= 3 ? launch_dense<3, DROP> : nt <= 4 ? launch_dense<4, DROP> :
           nt <= 6 ? launch_dense<6, DROP> : nt <= 8 ? launch_dense<8, DROP> : nt <= 12 ? launch_dense<12, DROP> : launch_dense<16, DROP>;
}

// the column panels of at most 256 outputs of one product, each through dense_kernel_for (DROP: p.col0 = the panel's first column)
template <bool DROP>
int dense_panels(const DenseArgsD<DROP> &p, hipStream_t s) {
    const float *W = p.W, *bias = p.bias;
    float *out = p.out;
    const int O = p.O;
    const bool al = p.ldx % 4 == 0 && aligned(p.X, 16);
    for (int o0 = 0; o0 < O; o0 += 256) {
        DenseArgsD<DROP> q = p;
        q.W = W + o0; q.bias = bias ? bias + o0 : nullptr; q.out = out + o0;
        q.w_aligned = p.ldw % 4 == 0 && aligned(q.W, 16);
        q.O = O - o0 < 256 ? O - o0 : 256;
        if constexpr (DROP) q.col0 = o0;
        const int rc = dense_kernel_for<DROP>(q, al)(q, al, s);
        if (rc != GNX_OK) return rc;
    }
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

}  // namespace

namespace gnx {

// used by the fused layer units too (their long rows go through the dense kernel with a row scatter)
int dense_rows(const float *X, int64_t ldx, int64_t n, int64_t F, const float *W, int64_t ldw, int64_t O, const float *bias, int act,
               const int32_t *in_rows, const int32_t *out_rows, float *out, int64_t ldo, hipStream_t s) {
    if (n == 0) return GNX_OK;
    DenseArgsD<false> p;
    static_cast<DenseArgs &>(p) = DenseArgs{X, ldx, n, (int)F, W, ldw, (int)O, bias, act, out, ldo, out_rows, in_rows, false};
    return dense_panels<false>(p, s);
}

}  // namespace gnx

extern "C" {

int gnx_dense(const float *d_X, int64_t ldx, int64_t n, int64_t F, const float *d_W, int64_t ldw, int64_t O, const float *d_bias,
              int act, float *d_out, int64_t ldo, void *stream) {
    GNX_CHECK_ARG(n >= 0 && F >= 1 && O >= 1 && F <= (1 << 24) && O <= (1 << 20), "gnx_dense: bad sizes (n=%lld, F=%lld, O=%lld)",
                  (long long)n, (long long)F, (long long)O);
    GNX_CHECK_ARG(ldx >= F && ldw >= O && ldo >= O, "gnx_dense: leading dimension smaller than the row");
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "gnx_dense: invalid activation %d", act);
    if (n == 0) return GNX_OK;
    GNX_CHECK_ARG(d_X && d_W && d_out, "gnx_dense: NULL pointer");
    GNX_CHECK_ARG((const void *)d_X != (const void *)d_out, "gnx_dense: out must not alias X");
    return dense_rows(d_X, ldx, n, F, d_W, ldw, O, d_bias, act, nullptr, nullptr, d_out, ldo, (hipStream_t)stream);
}

int gnx_dense_drop(gnx_graph_t g, const float *d_X, int64_t ldx, int64_t n, int64_t F, const float *d_W, int64_t ldw, int64_t O,
                   const float *d_bias, int act, double in_p, uint64_t in_seed, uint64_t in_stream, double out_p, uint64_t out_seed,
                   uint64_t out_stream, float *d_out, int64_t ldo, void *stream) {
    GNX_CHECK_ARG(n >= 0 && F >= 1 && O >= 1 && F <= (1 << 24) && O <= (1 << 20), "gnx_dense_drop: bad sizes (n=%lld, F=%lld, O=%lld)",
                  (long long)n, (long long)F, (long long)O);
    GNX_CHECK_ARG(ldx >= F && ldw >= O && ldo >= O, "gnx_dense_drop: leading dimension smaller than the row");
    GNX_CHECK_ARG(act == GNX_ACT_NONE || act == GNX_ACT_RELU, "gnx_dense_drop: invalid activation %d", act);
    // (the handle is read -- for its dropout counter -- only once every other argument has passed)
    GNX_CHECK_ARG(g != nullptr, "gnx_dense_drop: NULL handle");
    GNX_CHECK_ARG(in_p >= 0.0 && in_p < 1.0 && out_p >= 0.0 && out_p < 1.0, "gnx_dense_drop: dropout rate %g outside [0, 1)",
                  in_p >= 0.0 && in_p < 1.0 ? out_p : in_p);
    if (n == 0) return GNX_OK;
    GNX_CHECK_ARG(d_X && d_W && d_out, "gnx_dense_drop: NULL pointer");
    GNX_CHECK_ARG((const void *)d_X != (const void *)d_out, "gnx_dense_drop: out must not alias X");
    DenseArgsD<true> p;
    int rc = make_feat_drop("gnx_dense_drop", g, in_p, in_seed, in_stream, p.din);
    if (rc != GNX_OK) return rc;
    rc = make_feat_drop("gnx_dense_drop", g, out_p, out_seed, out_stream, p.dout);
    if (rc != GNX_OK) return rc;
    if (p.din.thr == 0 && p.dout.thr == 0)          // no mask on either side: the plain product (same kernels, same bits, nothing hashed)
        return dense_rows(d_X, ldx, n, F, d_W, ldw, O, d_bias, act, nullptr, nullptr, d_out, ldo, (hipStream_t)stream);
    static_cast<DenseArgs &>(p) = DenseArgs{d_X, ldx, n, (int)F, d_W, ldw, (int)O, d_bias, act, d_out, ldo, nullptr, nullptr, false};
    p.col0 = 0;
    return dense_panels<true>(p, (hipStream_t)stream);
}

}  // extern "C"
