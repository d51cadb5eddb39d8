/* gnx_halo_pack_bf16 + gnx_halo_exchange_bf16 over a REAL RCCL communicator, from a plain C program (no Python, no torch).
 *
 * One rank on one GPU: the block lists ITSELF as its only peer (loop-back region after the local rows), so a one-rank
 * communicator carries real ncclSend / ncclRecv pairs of ncclBfloat16 elements.  Both halves of the message (pulled rows: copies
 * of bf16 rows; pushed partial sums: f32 sums rounded once) go through one group and then through two groups with bound entry
 * points; the received region must equal the packed send slices bit for bit, the pulled rows must be the local rows they name, and
 * the pushed sum must be the bf16 rounding of the sum (chosen so that it is exact).
 * Build: gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude tests/c_abi_rccl_bf16.c -Lgnn-tf_amd/lib -lgnx
 *        -L/opt/rocm/lib -lamdhip64 -lrccl -lm */
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gnx.h"

#define CHECK_HIP(e) do { hipError_t _s = (e); if (_s != hipSuccess) { printf("hip error %d at line %d\n", (int)_s, __LINE__); return 2; } } while (0)
#define CHECK_GNX(e) do { int _s = (e); if (_s != GNX_OK) { printf("gnx error %d: %s (line %d)\n", _s, gnx_last_error(), __LINE__); return 3; } } while (0)
#define CHECK_NCCL(e) do { ncclResult_t _s = (e); if (_s != ncclSuccess) { printf("rccl error %d at line %d\n", (int)_s, __LINE__); return 4; } } while (0)

static int upload(const void *src, size_t bytes, void **dst) {
    if (hipMalloc(dst, bytes) != hipSuccess) return 1;
    return hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess;
}

/* the bf16 bit pattern of a float that bf16 represents exactly (its low 16 bits are zero) */
static uint16_t bf16_exact(float x) {
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    if (u & 0xFFFFu) { printf("%g is not a bf16 value\n", x); exit(9); }
    return (uint16_t)(u >> 16);
}

int main(void) {
    enum { C = 3, NL = 4 };
    if (ncclBfloat16 != 9) { printf("ncclBfloat16 is %d, the library sends 9\n", (int)ncclBfloat16); return 10; }
    CHECK_HIP(hipSetDevice(0));
    ncclUniqueId id;
    ncclComm_t comm;
    CHECK_NCCL(ncclGetUniqueId(&id));
    CHECK_NCCL(ncclCommInitRank(&comm, 1, id, 0));
    hipStream_t stream;
    CHECK_HIP(hipStreamCreate(&stream));
    float H[NL * C];
    uint16_t Hb[NL * C];
    for (int i = 0; i < NL * C; ++i) { H[i] = 1.f + 0.25f * i; Hb[i] = bf16_exact(H[i]); }
    const int32_t pull_src[2] = {3, 1};                                       /* pulled rows: local rows 3 and 1, in this order */
    const int64_t push_idx[6] = {0, 0, 0, 2, 0, 3};                           /* pushed sum: 0.5 H[0] + 2 H[2] - H[3] (exact in bf16) */
    const float push_val[3] = {0.5f, 2.f, -1.f};
    void *d_src, *d_pi, *d_pv;
    if (upload(pull_src, sizeof pull_src, &d_src) || upload(push_idx, sizeof push_idx, &d_pi) || upload(push_val, sizeof push_val, &d_pv)) return 20;
    gnx_graph_t push_g = NULL;
    CHECK_GNX(gnx_graph_create_coo(1, NL, 3, (const int64_t *)d_pi, (const float *)d_pv, NULL, &push_g));
    const int64_t two[1] = {2}, one[1] = {1};
    gnx_halo_plan_t plan = NULL;
    CHECK_GNX(gnx_halo_plan_create(1, 0, NL, two, one, two, one, (const int32_t *)d_src, push_g, &plan));
    int64_t n_buf, local0, n_send, n_send_pull, recv0[1], spull0[1], spush0[1];
    CHECK_GNX(gnx_halo_plan_layout(plan, &n_buf, &local0, &n_send, &n_send_pull, recv0, spull0, spush0));
    if (n_buf != NL + 3 || local0 != 0 || n_send != 3 || n_send_pull != 2 || recv0[0] != NL || spull0[0] != 0 || spush0[0] != 2) { printf("layout\n"); return 21; }
    uint16_t *d_X, *d_send;
    CHECK_HIP(hipMalloc((void **)&d_X, (size_t)n_buf * C * sizeof(uint16_t)));
    CHECK_HIP(hipMalloc((void **)&d_send, (size_t)n_send * C * sizeof(uint16_t)));
    uint16_t want[3 * C];
    for (int c = 0; c < C; ++c) {
        want[0 * C + c] = Hb[3 * C + c];
        want[1 * C + c] = Hb[1 * C + c];
        want[2 * C + c] = bf16_exact(0.5f * H[0 * C + c] + 2.f * H[2 * C + c] - H[3 * C + c]);
    }
    /* variant 0: entry points found in the process (this program links librccl), both halves in one group;
     * variant 1: entry points bound by the caller, the two halves as two groups (pulled rows first) */
    for (int variant = 0; variant < 2; ++variant) {
        CHECK_HIP(hipMemsetAsync(d_X, 0, (size_t)n_buf * C * sizeof(uint16_t), stream));
        CHECK_HIP(hipMemsetAsync(d_send, 0xFF, (size_t)n_send * C * sizeof(uint16_t), stream));
        CHECK_HIP(hipMemcpyAsync(d_X, Hb, sizeof Hb, hipMemcpyHostToDevice, stream));
        if (variant == 0) {
            CHECK_GNX(gnx_halo_pack_bf16(plan, GNX_HALO_ALL, d_X, C, C, d_send, C, stream));
            CHECK_GNX(gnx_halo_exchange_bf16(plan, GNX_HALO_ALL, comm, d_send, d_X, C, stream));
        } else {
            CHECK_GNX(gnx_halo_bind_rccl((void *)ncclGroupStart, (void *)ncclGroupEnd, (void *)ncclSend, (void *)ncclRecv));
            CHECK_GNX(gnx_halo_pack_bf16(plan, GNX_HALO_PULL, d_X, C, C, d_send, C, stream));
            CHECK_GNX(gnx_halo_exchange_bf16(plan, GNX_HALO_PULL, comm, d_send, d_X, C, stream));
            CHECK_GNX(gnx_halo_pack_bf16(plan, GNX_HALO_PUSH, d_X, C, C, d_send, C, stream));
            CHECK_GNX(gnx_halo_exchange_bf16(plan, GNX_HALO_PUSH, comm, d_send, d_X, C, stream));
        }
        CHECK_HIP(hipStreamSynchronize(stream));
        uint16_t got[3 * C], sent[3 * C];
        CHECK_HIP(hipMemcpy(got, d_X + recv0[0] * C, sizeof got, hipMemcpyDeviceToHost));
        CHECK_HIP(hipMemcpy(sent, d_send, sizeof sent, hipMemcpyDeviceToHost));
        for (int i = 0; i < 3 * C; ++i) {
            if (got[i] != sent[i]) { printf("variant %d, element %d: received 0x%04x, packed 0x%04x\n", variant, i, got[i], sent[i]); return 22; }
            if (got[i] != want[i]) { printf("variant %d, region element %d: got 0x%04x want 0x%04x\n", variant, i, got[i], want[i]); return 23; }
        }
    }
    CHECK_GNX(gnx_halo_bind_rccl(NULL, NULL, NULL, NULL));
    CHECK_GNX(gnx_halo_plan_destroy(plan));
    CHECK_GNX(gnx_graph_destroy(push_g));
    CHECK_NCCL(ncclCommDestroy(comm));
    printf("RCCL bf16 loop-back OK (pulled bf16 rows and rounded pushed sums through ncclSend / ncclRecv, one group and two groups)\n");
    return 0;
}
