"""Float64 numpy emulation of a GCNII training run over bf16 row storage (sparse.gcnii_train_run_bf16), with exactly the rounding
points of include/gnx.h -- bf() = tests/bf16_ref.py:bf16_round -- and the oracle's mask integers:

  forward    X_0 = bf(H);   T_l = beta (A X_l) + alpha H0_l;   Y_l = mask_l * act(T_l M_l);   X_{l+1} = bf(Y_l), the last Y stays as it is
  backward   g = upstream;  G_l = mask_l * g, with relu 0 where the STORED output (X_{l+1}, the last: Y) <= 0;   Gb_l = bf(G_l)
             dM_l = T_l^T G_l;   g <- (beta A^T Gb_l) M_l^T;   dH0 += (alpha G_l) M_l^T  (the f32 G, not Gb);   dH = the last g

beta = coef(1 - a), alpha = coef(a) (the library: f32), mask_l = 0 / s with s the f32 1 / (1 - p).  ``rnd=identity, coef=np.float64``
switches every rounding off: the plain float64 stack."""
import numpy as np

from oracle import gnntf_oracle as oracle
from bf16_ref import bf16_round


def bf(x):
    return bf16_round(x).astype(np.float64)


def identity(x):
    return np.asarray(x, dtype=np.float64)


def mask_scale(seed, stream, p, n, C):
    """The feature-dropout mask of (seed, stream) as a float64 [n, C] of 0 / s: kept iff hash_u24(seed, stream, row, col, 0) >=
    dropout_threshold(p) (the oracle's integers), s = the f32 1 / (1 - p)."""
    rows, cols = np.repeat(np.arange(n), C), np.tile(np.arange(C), n)
    keep = oracle.hash_u24(seed, stream, rows, cols, np.zeros(n * C, dtype=np.int64)) >= oracle.dropout_threshold(p)
    s = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(keep.reshape(n, C), np.float64(s), 0.0)


def run(A, H, steps, up, rnd=bf, coef=np.float32):
    """``A``: the normalised adjacency as a float64 scipy CSR; ``steps``: per layer (h0_key, H0, a, M, relu, mask) with mask = a
    mask_scale() array or None; ``up``: the upstream gradient of the run's output.  Returns a dict: ``out``, ``dH``, ``dH0`` = {h0_key:
    the sum over the layers with that key}, ``dM`` = [per layer]."""
    X = rnd(np.asarray(H, dtype=np.float64))
    kept = []
    n_layers = len(steps)
    for k, (_, H0, a, M, relu, mask) in enumerate(steps):
        beta, alpha = float(coef(1.0 - float(coef(a)))), float(coef(a))
        M = np.asarray(M, dtype=np.float64)
        T = beta * (A @ X) + alpha * np.asarray(H0, dtype=np.float64)
        Y = T @ M
        if relu:
            Y = np.maximum(Y, 0.0)
        if mask is not None:
            Y = Y * mask
        X = rnd(Y) if k < n_layers - 1 else Y
        kept.append((T, X, beta, alpha, M))
    out = X
    g = np.asarray(up, dtype=np.float64)
    dH0, dM = {}, [None] * n_layers
    for k in range(n_layers - 1, -1, -1):
        key, _, _, _, relu, mask = steps[k]
        T, stored, beta, alpha, M = kept[k]
        G = g if mask is None else g * mask
        if relu:
            G = np.where(stored <= 0.0, 0.0, G)
        Gb = rnd(G)
        dM[k] = T.T @ G
        g = (beta * (A.T @ Gb)) @ M.T
        dH0[key] = dH0.get(key, 0.0) + (alpha * G) @ M.T
    return dict(out=out, dH=g, dH0=dH0, dM=dM)


def rel_fro(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / max(np.linalg.norm(want), 1e-300))
