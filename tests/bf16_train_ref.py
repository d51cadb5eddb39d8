"""Emulation of the bf16 training loops (gnx_spmm_dropped_chained_bf16 / gnx_spmm_dropped_back_bf16) for the tests: numpy, float64 sums,
built from the oracle's own pieces -- keep_mask / sparse_dropout for the dropped raw matrix B_k, its column sums with divide_no_nan for
the f32 degree scales D_k -- with bf() (tests/bf16_ref.py) at exactly the points where the library rounds:

  forward   X_0 = bf(H0); iteration 0: acc[i] = sum_j ((D_0[i] b_ij) D_0[j]) X_0[j]; k >= 1: acc[i] = sum_j (D_k[i] b_ij) X_k[j];
            H_{k+1} = (1-a) acc + a H0; X_{k+1} = bf(H_{k+1} * D_{k+1}) for k < K-1; the last iteration returns H_K.
  backward  first call gathers bf(g) unscaled, S_in = g; acc[r] = sum_c A_k[c][r] X[c]; S = s_beta acc + s_alpha S_in;
            Y = bf((1-a) acc * D_{k-1}) unless it is the last call; dH0 = S.  Coefficients: those of sparse._backward_chained.

With ``bf`` the identity and float64 coefficients this is the reference arithmetic itself (tests/test_bf16_train_host.py)."""
import numpy as np
import scipy.sparse as sp

from oracle import gnntf_oracle as oracle
from bf16_ref import bf16_round


def bf(x):
    return bf16_round(x).astype(np.float64)


def identity(x):
    return np.asarray(x, dtype=np.float64)


def dropped_matrices(indices, values, shape, p, seed, first_stream, K):
    """[(B_k as float64 CSR, D_k float32)] for k = 0 .. K-1: B_k = the dropped raw COO (kept entries scaled by 1/(1-p) in f32,
    duplicates added), D_k = divide_no_nan(1, sqrt(column sums of B_k)) in f32 (gnn.py:41)."""
    indices = np.asarray(indices, dtype=np.int64).reshape(-1, 2)
    values = np.asarray(values, dtype=np.float32)
    out = []
    for k in range(K):
        v = oracle.sparse_dropout(indices, values, p, True, seed, first_stream + k)
        D = oracle.divide_no_nan(np.float32(1.0), np.sqrt(oracle.sparse_reduce_sum_axis0(indices, v, shape)))
        B = sp.coo_matrix((v.astype(np.float64), (indices[:, 0], indices[:, 1])), shape=shape).tocsr()
        out.append((B, D.astype(np.float32)))
    return out


def forward(mats, H0, a, rnd=bf, coef=np.float32):
    """H_K (float64) of the chained forward loop over ``mats`` = dropped_matrices(...)."""
    H0 = np.asarray(H0, dtype=np.float32).astype(np.float64)
    K = len(mats)
    beta, alpha = float(coef(1.0 - float(a))), float(coef(a))
    X = rnd(H0)
    H = H0
    for k, (B, D) in enumerate(mats):
        D = D.astype(np.float64)[:, None]
        acc = D * (B @ (D * X)) if k == 0 else D * (B @ X)
        H = beta * acc + alpha * H0
        if k < K - 1:
            X = rnd(H * mats[k + 1][1].astype(np.float64)[:, None])
    return H


def backward(mats, g, a, rnd=bf, coef=np.float32):
    """dH0 (float64) of the chained backward loop for the upstream gradient ``g``."""
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    K = len(mats)
    a = float(a)
    X, S = rnd(g), g
    for k in range(K - 1, -1, -1):
        first, last = k == K - 1, k == 0
        B, D = mats[k]
        D = D.astype(np.float64)[:, None]
        acc = D * (B.T @ (D * X)) if first else D * (B.T @ X)
        s_alpha = float(coef(a)) if first else 1.0
        s_beta = float(coef(1.0 - a)) if last else float(coef(a * (1.0 - a)))
        S = s_beta * acc + s_alpha * S
        if not last:
            X = rnd(float(coef(1.0 - a)) * acc * mats[k - 1][1].astype(np.float64)[:, None])
    return S


def oracle_forward(indices, values, shape, H0, a, K, p, seed, first_stream, dtype=np.float64):
    """The reference's training loop (oracle.appnp_propagate), no bf16 anywhere."""
    return oracle.appnp_propagate(indices, np.asarray(values), shape, H0, a, K, graph_dropout=p, training=True, seed=seed,
                                  first_stream=first_stream, dtype=dtype)


def oracle_backward(indices, values, shape, g, a, K, p, seed, first_stream, dtype=np.float64):
    """dH0 by K applications of oracle.ppr_iteration_backward: g_k = dL/dH_k, dH0 = g_0 + sum of the a g_{k+1} terms."""
    g = np.asarray(g).astype(dtype)
    total = np.zeros_like(g)
    for k in range(K - 1, -1, -1):
        ai, av = oracle.get_adjacency(indices, np.asarray(values), shape, p, "symmetric", "none", True, seed, first_stream + k, dtype)
        g, gH0 = oracle.ppr_iteration_backward(ai, av, shape, g, a)
        total = total + gH0
    return total + g


def rel_fro(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / max(np.linalg.norm(want), 1e-300))
