// Standalone probe: does a cache-policy bit on COLD gathered rows keep HOT gathered rows in gfx950's L2 / Infinity Cache?
//   hipcc -O3 --offload-arch=gfx950 tools/gather_policy_probe.hip -o build/gather_policy_probe
//   build/gather_policy_probe [--rounds R] [--reps N] [--iters I] [--hot-mib 2|128]   (tools/gather_policy_probe.sh runs it with counters too)
// The access shape is the wide SpMM's: a 32-lane group gathers one 512-byte row with one 16-byte load per lane, two groups per
// wave, four rows in flight per group, 32 waves per CU.  One slot in HOT_EVERY is a uniformly random row of a small HOT table
// (always a plain load); the others are uniformly random rows of an 8 GB COLD table, loaded with the policy under test.  Row
// numbers come from a hash, so no index stream competes for the caches.  Every load goes through the same inline-asm statement
// and the same once-per-batch wait, so two variants differ in the cache bits of the cold loads and in nothing else; a pair of
// compiler-counted kernels (plain / __builtin_nontemporal_load) shows what the hand-counted wait costs.
// Prints per variant the median, minimum and maximum ms per launch over the rounds (variants alternate inside a round), the
// gathered TB/s, and a last JSON line with the same figures.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CHECK(e) do { hipError_t s_ = (e); if (s_ != hipSuccess) { printf("hip error %s line %d\n", hipGetErrorString(s_), __LINE__); exit(1); } } while (0)

enum { P_PLAIN = 0, P_NT = 1, P_SC1 = 2, P_SC0_SC1 = 3, P_BUILTIN_PLAIN = 4, P_BUILTIN_NT = 5 };

__device__ __forceinline__ unsigned mix32(unsigned x) {
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}

template <int POLICY>
__device__ __forceinline__ f32x4 load16(const f32x4 *p) {
    f32x4 v;
    if constexpr (POLICY == P_PLAIN) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
    else if constexpr (POLICY == P_NT) asm volatile("global_load_dwordx4 %0, %1, off nt" : "=v"(v) : "v"(p) : "memory");
    else if constexpr (POLICY == P_SC1) asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v) : "v"(p) : "memory");
    else if constexpr (POLICY == P_SC0_SC1) asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(v) : "v"(p) : "memory");
    else if constexpr (POLICY == P_BUILTIN_NT) v = __builtin_nontemporal_load(p);
    else v = *p;
    return v;
}

// HOT_EVERY: slot s of a group's stream is hot when s % HOT_EVERY == 0; 0 = no hot slot (cold only), 1 = hot only.
template <int POLICY, int HOT_EVERY>
__global__ void __launch_bounds__(256) k_probe(const f32x4 *__restrict__ hot, unsigned hot_mask, const f32x4 *__restrict__ cold,
                                               unsigned cold_mask, int iters, unsigned seed, float *__restrict__ sink) {
    constexpr bool kAsm = POLICY <= P_SC0_SC1;
    constexpr int kHotPolicy = kAsm ? P_PLAIN : P_BUILTIN_PLAIN;
    const unsigned lane = threadIdx.x & 31u;
    const unsigned group = (blockIdx.x * 256u + threadIdx.x) >> 5;
    unsigned key = mix32(group * 0x9e3779b9u + seed);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {                 // two batches of four, so that HOT_EVERY = 8 has a compile-time slot
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                key = mix32(key + 0x6d2b79f5u);
                const int s = b * 4 + u;
                const bool is_hot = HOT_EVERY > 0 && s % (HOT_EVERY > 0 ? HOT_EVERY : 1) == 0;
                if (is_hot) v[u] = load16<kHotPolicy>(hot + (size_t)(key & hot_mask) * 32 + lane);
                else v[u] = load16<POLICY>(cold + (size_t)(key & cold_mask) * 32 + lane);
            }
            // the compiler counts nothing inside asm: one wait per batch, naming every destination so none is read early
            if constexpr (kAsm) asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) : : "memory");
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += v[u];
        }
    }
    const float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    if (s == 12345.678f) sink[0] = s;                 // keeps the loads alive without a reduction
}

struct Variant {
    const char *name;
    void (*kernel)(const f32x4 *, unsigned, const f32x4 *, unsigned, int, unsigned, float *);
    double hot_share;
    std::vector<float> ms;
};

int main(int argc, char **argv) {
    int rounds = 5, reps = 3, iters = 256, only_hot_mib = 0;        // --hot-mib N: that hot table only (counter runs: one table per run)
    for (int i = 1; i + 1 < argc; i += 2) {
        if (!strcmp(argv[i], "--rounds")) rounds = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--reps")) reps = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--iters")) iters = atoi(argv[i + 1]);
        else if (!strcmp(argv[i], "--hot-mib")) only_hot_mib = atoi(argv[i + 1]);
        else { printf("unknown option %s\n", argv[i]); return 2; }
    }
    if (rounds < 1 || reps < 1 || iters < 1) { printf("rounds, reps and iters must be positive\n"); return 2; }
    const size_t row_bytes = 512;
    const size_t cold_bytes = 8ull << 30, cold_rows = cold_bytes / row_bytes;        // 2^24 rows
    const size_t hot_bytes_opts[2] = {2ull << 20, 128ull << 20};                     // one L2's half; Infinity-Cache sized
    const int blocks = 256 * 8, groups = blocks * 8;                                 // 8 blocks of 4 waves per CU
    f32x4 *cold, *hot;
    float *sink;
    CHECK(hipMalloc((void **)&cold, cold_bytes));
    CHECK(hipMalloc((void **)&hot, hot_bytes_opts[1]));
    CHECK(hipMalloc((void **)&sink, 256));
    CHECK(hipMemset(cold, 1, cold_bytes));
    CHECK(hipMemset(hot, 1, hot_bytes_opts[1]));
    CHECK(hipDeviceSynchronize());
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
    const double gathers = (double)groups * iters * 8;
    printf("rows of %zu B; cold table %zu MiB; %d groups x %d slots = %.1f M gathers (%.2f GB) per launch; %d rounds x %d reps\n",
           row_bytes, cold_bytes >> 20, groups, iters * 8, gathers / 1e6, gathers * row_bytes / 1e9, rounds, reps);
    std::string json = "{\"row_bytes\": 512, \"cold_mib\": 8192, \"gathers_per_launch\": " + std::to_string((long long)gathers) + ", \"results\": [";
    for (int h = 0; h < 2; ++h) {
        if (only_hot_mib && (size_t)only_hot_mib != hot_bytes_opts[h] >> 20) continue;
        const size_t hot_rows = hot_bytes_opts[h] / row_bytes;
        std::vector<Variant> vs = {
            {"hot_only", k_probe<P_PLAIN, 1>, 1.0, {}},
            {"cold_only_plain", k_probe<P_PLAIN, 0>, 0.0, {}},
            {"cold_only_nt", k_probe<P_NT, 0>, 0.0, {}},
            {"hot1of4_cold_plain", k_probe<P_PLAIN, 4>, 0.25, {}},
            {"hot1of4_cold_nt", k_probe<P_NT, 4>, 0.25, {}},
            {"hot1of4_cold_sc1", k_probe<P_SC1, 4>, 0.25, {}},
            {"hot1of4_cold_sc0sc1", k_probe<P_SC0_SC1, 4>, 0.25, {}},
            {"hot1of8_cold_plain", k_probe<P_PLAIN, 8>, 0.125, {}},
            {"hot1of8_cold_nt", k_probe<P_NT, 8>, 0.125, {}},
            {"hot1of8_cold_sc1", k_probe<P_SC1, 8>, 0.125, {}},
            {"hot1of8_cold_sc0sc1", k_probe<P_SC0_SC1, 8>, 0.125, {}},
            {"hot1of4_cold_plain_builtin", k_probe<P_BUILTIN_PLAIN, 4>, 0.25, {}},
            {"hot1of4_cold_nt_builtin", k_probe<P_BUILTIN_NT, 4>, 0.25, {}},
        };
        unsigned seed = 1;
        for (int r = -1; r < rounds; ++r)              // round -1 warms every kernel up and is not recorded
            for (Variant &v : vs) {
                CHECK(hipEventRecord(a, 0));
                for (int k = 0; k < reps; ++k)
                    hipLaunchKernelGGL(v.kernel, dim3(blocks), dim3(256), 0, 0, hot, (unsigned)(hot_rows - 1), cold,
                                       (unsigned)(cold_rows - 1), iters, seed++, sink);
                CHECK(hipEventRecord(b, 0));
                CHECK(hipEventSynchronize(b));
                CHECK(hipGetLastError());
                float ms;
                CHECK(hipEventElapsedTime(&ms, a, b));
                if (r >= 0) v.ms.push_back(ms / reps);
            }
        printf("\nhot table %zu MiB (%zu rows)\n%-28s %9s %9s %9s %9s\n", hot_bytes_opts[h] >> 20, hot_rows, "variant", "median ms",
               "min ms", "max ms", "TB/s");
        for (Variant &v : vs) {
            std::sort(v.ms.begin(), v.ms.end());
            const float med = v.ms[v.ms.size() / 2];
            printf("%-28s %9.3f %9.3f %9.3f %9.2f\n", v.name, med, v.ms.front(), v.ms.back(), gathers * row_bytes / med / 1e9);
            char buf[256];
            snprintf(buf, sizeof buf, "%s{\"hot_mib\": %zu, \"variant\": \"%s\", \"hot_share\": %.3f, \"ms_median\": %.4f, \"ms_min\": %.4f, \"ms_max\": %.4f}",
                     json.back() == '[' ? "" : ", ", hot_bytes_opts[h] >> 20, v.name, v.hot_share, med, v.ms.front(), v.ms.back());
            json += buf;
        }
        fflush(stdout);
    }
    printf("\n%s]}\n", json.c_str());
    CHECK(hipFree(cold)); CHECK(hipFree(hot)); CHECK(hipFree(sink));
    return 0;
}
