"""numpy helpers for the fused NGCF backward (gnx_step_back_ngcf, sparse.ngcf_step(backward="fused")): the float64 intermediates that
ngcf_fused_ref.backward_ref does not return, their bounds, and a float32 emulation of the entry's stated rounding points that the bounds
must admit.  Everything else -- graphs, operands, forward_ref, back_gate_ref, backward_ref, ``ratio`` -- is tests/ngcf_fused_ref.py's,
imported.  numpy and scipy only: imports without a GPU.

With G1, G2 and their bounds e_G1, e_G2 from back_gate_ref (u = 2^-24):
    Q1 = G1 W1^T     Q2 = G2 W2^T     e_Q = e_G |W^T| + (C_out + 2) u |G| |W^T|                       as in backward_ref
    dA = Q1 * X + Q2                  e_dA = e_Q1 |X| + e_Q2 + 2 u (|Q1| |X| + |Q2|)                  ngcf_fused_ref's docstring
    R  = Q1 * A32                     e_R  = e_Q1 |A32| + 2 u |Q1| |A32|
A32 is the float32 A . X the launch reads, taken as DATA: R is judged as the product with the very operand the kernel multiplied by (its
distance from the float64 A . X enters dX's bound, e_Q1 |agg| + |Q1| e_agg, not R's).  One u of each 2 u is the rounding of the product
(dA: of the fused multiply-add), the other covers the second-order remainder, as everywhere in ngcf_fused_ref.  In every bound |Q|
stands for |G| |W^T| (>= |G W^T|), the majorant ngcf_fused_ref.backward_ref uses for it: a bound never below the letter of the formula.

The entry's rounding points, emulated by ``backward_f32``: G1 / G2 given (the gate pass's float32 results); P = X * A32 one multiply;
each Q a float32 sum over the output columns ascending, product and add fused (the MFMA's k-ordered fmaf chain); dA one fused
multiply-add; R one multiply; db the float32 column sums (row order); dX = A_hat^T dA in the library's order, + R once."""
import numpy as np
import scipy.sparse as sp

import ngcf_fused_ref as nref
from ngcf_fused_ref import U32, f64


def products_ref(X, A32, W1, W2, G1, e_G1, G2, e_G2):
    """dict(Q1, e_Q1, Q2, e_Q2, dA, e_dA, R, e_R) in float64 from the gated gradients and their bounds."""
    C_out = G1.shape[1]
    X64, A64 = f64(X), f64(A32)
    W1t, W2t = f64(W1).T, f64(W2).T
    Q1, Q2 = G1 @ W1t, G2 @ W2t
    q1_abs, q2_abs = np.abs(G1) @ np.abs(W1t), np.abs(G2) @ np.abs(W2t)
    e_Q1 = e_G1 @ np.abs(W1t) + (C_out + 2) * U32 * q1_abs
    e_Q2 = e_G2 @ np.abs(W2t) + (C_out + 2) * U32 * q2_abs
    dA = Q1 * X64 + Q2
    e_dA = e_Q1 * np.abs(X64) + e_Q2 + 2 * U32 * (q1_abs * np.abs(X64) + q2_abs)
    R = Q1 * A64
    e_R = e_Q1 * np.abs(A64) + 2 * U32 * q1_abs * np.abs(A64)
    return dict(Q1=Q1, e_Q1=e_Q1, Q2=Q2, e_Q2=e_Q2, dA=dA, e_dA=e_dA, R=R, e_R=e_R)


def fma32(a, b, c):
    """fmaf(a, b, c) over float32 arrays: the product of two float32 is exact in float64 and the sum is rounded once there, then once more
    to float32 -- the double rounding differs from a true fused multiply-add in rare ties only, far inside any bound here."""
    return (f64(a) * f64(b) + f64(c)).astype(np.float32)


def matmul_fma32(G, Wt):
    """G . Wt in float32 as the matrix cores sum it: per element one fmaf chain over k ascending from +0."""
    G, Wt = np.asarray(G, dtype=np.float32), np.asarray(Wt, dtype=np.float32)
    acc = np.zeros((G.shape[0], Wt.shape[1]), dtype=np.float32)
    for k in range(G.shape[1]):
        acc = fma32(G[:, k:k + 1], Wt[k:k + 1, :], acc)
    return acc


def backward_f32(At32, X, A32, W1, W2, G1, G2, L, with_R=True, with_X=True):
    """dict(P, dA, R, db1, db2, dX) in float32 at the entry's rounding points.  ``with_R=False`` / ``with_X=False`` are the two broken
    backwards the bounds must reject: dX without the Q1 * A term, and dA without the product with X."""
    f32 = np.float32
    X, A32, G1, G2 = (np.asarray(t, dtype=f32) for t in (X, A32, G1, G2))
    Q1, Q2 = matmul_fma32(G1, np.asarray(W1, dtype=f32).T), matmul_fma32(G2, np.asarray(W2, dtype=f32).T)
    dA = fma32(Q1, X, Q2) if with_X else (Q1 + Q2).astype(f32)
    R = (Q1 * A32).astype(f32)
    gathered = nref.spmm_f32(At32, dA, "library", L)
    dX = (gathered + R).astype(f32) if with_R else gathered
    return dict(P=(X * A32).astype(f32), dA=dA, R=R, db1=G1.sum(axis=0, dtype=f32), db2=G2.sum(axis=0, dtype=f32), dX=dX)


def transposed32(A32):
    At32 = sp.csr_matrix(A32.T)
    At32.sort_indices()
    return At32
