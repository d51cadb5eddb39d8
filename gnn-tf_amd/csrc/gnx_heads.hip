// The task heads: what a model's output rows go through on their way to a loss or a prediction.  None of it is a GEMM.
//
//   gnx_node_ce      mean_i CE(log_softmax(logits[nodes_i]))   reference gnntf/core/gnn/graph_predictor.py:19-25
//   gnx_node_argmax  argmax(logits[nodes_i])                   reference gnntf/core/gnn/graph_predictor.py:16-17, 27-31
//   gnx_edge_scores  sum_c F[u_i, c] * F[v_i, c] * (r[c] or 1) reference gnntf/core/gnn/graph_predictor.py:122-126
//
// Ids are range-checked in the kernels, never dereferenced out of bounds.  Fixed reduction trees: bitwise reproducible.
#include "gnx_internal.h"

namespace {

__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// one 16-lane group per listed item: 16 items per block, item i = 16 blockIdx.x + threadIdx.x / 16 in every kernel launched here
template <typename K, typename... Args>
void launch_items(K kernel, int64_t m, void *stream, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((m + 15) / 16)), dim3(256), 0, (hipStream_t)stream, args...);
}

// the row maximum and the sum of exp(x - max) of one row, across the group
__device__ __forceinline__ void softmax_stats(const float *__restrict__ x, int C, int sub, float &mx, float &se) {
    mx = -INFINITY;
    for (int c = sub; c < C; c += 16) mx = fmaxf(mx, x[c]);
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    se = 0.f;
    for (int c = sub; c < C; c += 16) se += expf(x[c] - mx);
    se = group16_sum(se);
}

// ---- node head: gather the row, max, sum of exponentials, loss_i = logsumexp - x[label] ------------------------------------------
// (graph_predictor.py:24-25: CE-from-logits applied to log_softmax(x); softmax(log_softmax(x)) = softmax(x), so this IS the
// plain cross entropy.)
__global__ __launch_bounds__(256) void k_node_ce_fwd(const float *__restrict__ logits, int64_t ldl, int C, int64_t n_rows,
                                                      const int64_t *__restrict__ nodes, const int64_t *__restrict__ labels, int64_t m,
                                                      float *__restrict__ loss) {
    const int sub = threadIdx.x & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (i >= m) return;
    const int64_t node = nodes[i], label = labels[i];
    if (node < 0 || node >= n_rows || label < 0 || label >= C) {      // never read out of bounds: the loss of such an item is NaN
        if (sub == 0) loss[i] = NAN;
        return;
    }
    const float *__restrict__ x = logits + node * ldl;
    float mx, se;
    softmax_stats(x, C, sub, mx, se);
    // log(se) - (x[label] - mx), not (log(se) + mx) - x[label]: the difference of two logits is exact where they share an offset,
    // while log(se) added to mx first is rounded to the spacing of mx (1e-3 at logits round 1e4) before the offset cancels
    if (sub == 0) loss[i] = logf(se) - (x[label] - mx);
}

// d logits[node_i, :] += scale * (softmax(x) - onehot(label)); atomics because a node may be listed twice
__global__ __launch_bounds__(256) void k_node_ce_bwd(const float *__restrict__ logits, int64_t ldl, int C, int64_t n_rows,
                                                      const int64_t *__restrict__ nodes, const int64_t *__restrict__ labels, int64_t m,
                                                      const float *__restrict__ gout, float inv_m, float *__restrict__ grad, int64_t ldg) {
    const int sub = threadIdx.x & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (i >= m) return;
    const int64_t node = nodes[i], label = labels[i];
    if (node < 0 || node >= n_rows || label < 0 || label >= C) return;
    const float *__restrict__ x = logits + node * ldl;
    float mx, se;
    softmax_stats(x, C, sub, mx, se);
    // the label's column gets softmax - 1 = -(the other columns' share): formed as pr - 1 it is a difference of nearly equal numbers
    // wherever the model is sure of the label, and keeps only the absolute accuracy of pr (1e-7) in a term of 1e-3 or less
    float rest = 0.f;
    for (int c = sub; c < C; c += 16) rest += c == label ? 0.f : expf(x[c] - mx);
    rest = group16_sum(rest);
    const float scale = gout[0] * inv_m, inv = 1.0f / se;
    for (int c = sub; c < C; c += 16) {
        const float pr = (c == label ? -rest : expf(x[c] - mx)) * inv;
        atomicAdd(grad + node * ldg + c, scale * pr);
    }
}

// mean of m values in a fixed order: MEAN_BLOCKS blocks each reduce a contiguous slice (strided partial sums + a fixed LDS
// tree) into partial[block]; one block then adds the partials in the same way and divides
constexpr int MEAN_BLOCKS = 256;

// the sum of v[b + thread], v[b + thread + 256], ... below e per thread, then of the block's 256 threads by the LDS tree; valid in thread 0
__device__ __forceinline__ float block256_sum(const float *__restrict__ v, int64_t b, int64_t e) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int64_t i = b + threadIdx.x; i < e; i += 256) acc += v[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void k_mean_partial(const float *__restrict__ v, int64_t m, float *__restrict__ partial) {
    const int64_t per = (m + MEAN_BLOCKS - 1) / MEAN_BLOCKS;
    const int64_t b = (int64_t)blockIdx.x * per, e = b + per < m ? b + per : m;
    const float sum = block256_sum(v, b, e);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void k_mean(const float *__restrict__ v, int64_t n_partial, int64_t m, float *__restrict__ out) {
    const float sum = block256_sum(v, 0, n_partial);
    if (threadIdx.x == 0) out[0] = sum / (float)m;
}

// first index of the row maximum (tf.argmax / np.argmax tie rule)
__global__ __launch_bounds__(256) void k_node_argmax(const float *__restrict__ logits, int64_t ldl, int C, int64_t n_rows,
                                                      const int64_t *__restrict__ nodes, int64_t m, int64_t *__restrict__ out) {
    const int sub = threadIdx.x & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (i >= m) return;
    const int64_t node = nodes ? nodes[i] : i;
    if (node < 0 || node >= n_rows) {                                   // out of range: -1
        if (sub == 0) out[i] = -1;
        return;
    }
    const float *__restrict__ x = logits + node * ldl;
    float best = -INFINITY;
    int arg = C;                                           // rows of NaNs: no element compares greater; report 0 like np.argmax of all-equal
    for (int c = sub; c < C; c += 16) {
        const float v = x[c];
        if (v > best || (v == best && c < arg)) { best = v; arg = c; }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oa = __shfl_xor(arg, off);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (sub == 0) out[i] = arg < C ? arg : 0;
}

// ---- link head: logit_i = sum_c F[u_i, c] * F[v_i, c] * (r[c] or 1)   (graph_predictor.py:122-126) ---------------------
__global__ __launch_bounds__(256) void k_edge_scores(const float *__restrict__ F, int64_t ldf, int C, int64_t n_rows,
                                                      const int64_t *__restrict__ edges, int64_t m, const float *__restrict__ r,
                                                      float *__restrict__ out) {
    const int sub = threadIdx.x & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (i >= m) return;
    const int64_t u = edges[2 * i], v = edges[2 * i + 1];
    if (u < 0 || u >= n_rows || v < 0 || v >= n_rows) {                 // out of range: NaN
        if (sub == 0) out[i] = NAN;
        return;
    }
    const float *__restrict__ fu = F + u * ldf, *__restrict__ fv = F + v * ldf;
    float acc = 0.f;
    for (int c = sub; c < C; c += 16) acc = fmaf(fu[c] * fv[c], r ? r[c] : 1.0f, acc);
    acc = group16_sum(acc);
    if (sub == 0) out[i] = acc;
}

// dF[u_i, :] += g_i * F[v_i, :] * r,  dF[v_i, :] += g_i * F[u_i, :] * r   (atomics: endpoints repeat across edges)
__global__ __launch_bounds__(256) void k_edge_scores_bwd(const float *__restrict__ F, int64_t ldf, int C, int64_t n_rows,
                                                          const int64_t *__restrict__ edges, int64_t m, const float *__restrict__ r,
                                                          const float *__restrict__ g, float *__restrict__ dF, int64_t ldg) {
    const int sub = threadIdx.x & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (i >= m) return;
    const int64_t u = edges[2 * i], v = edges[2 * i + 1];
    if (u < 0 || u >= n_rows || v < 0 || v >= n_rows) return;
    const float gi = g[i];
    for (int c = sub; c < C; c += 16) {
        const float w = gi * (r ? r[c] : 1.0f);
        atomicAdd(dF + u * ldg + c, w * F[v * ldf + c]);
        atomicAdd(dF + v * ldg + c, w * F[u * ldf + c]);
    }
}

}  // namespace

extern "C" {

int gnx_node_ce(const float *d_logits, int64_t ldl, int64_t n_rows, int64_t C, const int64_t *d_nodes, const int64_t *d_labels, int64_t m,
                float *d_loss_per_node, float *d_mean_loss, void *stream) {
    GNX_CHECK_ARG(m >= 1 && C >= 1 && n_rows >= 1 && ldl >= C, "gnx_node_ce: bad sizes");
    GNX_CHECK_ARG(d_logits && d_nodes && d_labels && d_loss_per_node && d_mean_loss, "gnx_node_ce: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    launch_items(k_node_ce_fwd, m, stream, d_logits, ldl, (int)C, n_rows, d_nodes, d_labels, m, d_loss_per_node);
    if (m > 4096) {      // two-level mean; the partial sums live in the scratch tail of d_loss_per_node
        float *partial = d_loss_per_node + m;
        hipLaunchKernelGGL(k_mean_partial, dim3(MEAN_BLOCKS), dim3(256), 0, s, d_loss_per_node, m, partial);
        hipLaunchKernelGGL(k_mean, dim3(1), dim3(256), 0, s, partial, (int64_t)MEAN_BLOCKS, m, d_mean_loss);
    } else {
        hipLaunchKernelGGL(k_mean, dim3(1), dim3(256), 0, s, d_loss_per_node, m, m, d_mean_loss);
    }
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_node_ce_backward(const float *d_logits, int64_t ldl, int64_t n_rows, int64_t C, const int64_t *d_nodes, const int64_t *d_labels,
                         int64_t m, const float *d_grad_loss, float *d_grad_logits, int64_t ldg, void *stream) {
    GNX_CHECK_ARG(m >= 1 && C >= 1 && n_rows >= 1 && ldl >= C && ldg >= C, "gnx_node_ce_backward: bad sizes");
    GNX_CHECK_ARG(d_logits && d_nodes && d_labels && d_grad_loss && d_grad_logits, "gnx_node_ce_backward: NULL pointer");
    launch_items(k_node_ce_bwd, m, stream, d_logits, ldl, (int)C, n_rows, d_nodes, d_labels, m, d_grad_loss, 1.0f / (float)m, d_grad_logits, ldg);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_edge_scores(const float *d_F, int64_t ldf, int64_t n_rows, int64_t C, const int64_t *d_edges, int64_t m, const float *d_r,
                    float *d_out, void *stream) {
    GNX_CHECK_ARG(m >= 0 && C >= 1 && n_rows >= 0 && ldf >= C, "gnx_edge_scores: bad sizes");
    if (m == 0) return GNX_OK;
    GNX_CHECK_ARG(d_F && d_edges && d_out, "gnx_edge_scores: NULL pointer");
    launch_items(k_edge_scores, m, stream, d_F, ldf, (int)C, n_rows, d_edges, m, d_r, d_out);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_edge_scores_backward(const float *d_F, int64_t ldf, int64_t n_rows, int64_t C, const int64_t *d_edges, int64_t m, const float *d_r,
                             const float *d_grad_out, float *d_grad_F, int64_t ldg, void *stream) {
    GNX_CHECK_ARG(m >= 0 && C >= 1 && ldf >= C && ldg >= C, "gnx_edge_scores_backward: bad sizes");
    if (m == 0) return GNX_OK;
    GNX_CHECK_ARG(d_F && d_edges && d_grad_out && d_grad_F, "gnx_edge_scores_backward: NULL pointer");
    launch_items(k_edge_scores_bwd, m, stream, d_F, ldf, (int)C, n_rows, d_edges, m, d_r, d_grad_out, d_grad_F, ldg);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

int gnx_node_argmax(const float *d_logits, int64_t ldl, int64_t n_rows, int64_t C, const int64_t *d_nodes, int64_t m, int64_t *d_out,
                    void *stream) {
    GNX_CHECK_ARG(m >= 0 && C >= 1 && n_rows >= 0 && ldl >= C, "gnx_node_argmax: bad sizes");
    if (m == 0) return GNX_OK;
    GNX_CHECK_ARG(d_logits && d_out, "gnx_node_argmax: NULL pointer");
    launch_items(k_node_argmax, m, stream, d_logits, ldl, (int)C, n_rows, d_nodes, m, d_out);
    GNX_HIP(hipGetLastError());
    return GNX_OK;
}

}  // extern "C"
