"""float64 emulation of the bf16 propagation over vertex blocks (ShardedGraph.make_state(storage=torch.bfloat16)), with the
rounding points of include/gnx.h: the iterate is bf16 between the iterations, a pulled row is a copy of its owner's bf16 row, and a
pushed partial sum -- the entries of one row whose columns ONE peer owns -- is rounded once by its sender before it is added.

    S = A_keep . H~ + sum_q bf(P_q . H~),      H_{k+1} = (1-a) S + a H0,      H~_{k+1} = bf(H_{k+1}) for k < K-1

A_keep: the entries a block multiplies itself (local and pulled columns), P_q: the pushed entries whose column rank q owns.  Built
on tests/bf16_ref.py (numpy + scipy); with no pushed entry it is bf16_ref.appnp_bf16."""
import numpy as np
import scipy.sparse as sp

from bf16_ref import bf16_round


def split_entries(rows, cols, vals, pushed, bounds):
    """(A_keep, [P_q for every rank q]) as float64 CSR matrices from the global entries of ShardedGraph(keep_entries=True).entries
    (concatenated over the ranks) and the P + 1 partition bounds."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    n, world = int(bounds[-1]), len(bounds) - 1
    pushed = np.zeros(len(rows), dtype=bool) if pushed is None else np.asarray(pushed, dtype=bool)
    csr = lambda m: sp.csr_matrix((vals[m], (rows[m], cols[m])), shape=(n, n))
    owner = np.searchsorted(np.asarray(bounds[1:], dtype=np.int64), cols, side="right")
    row_owner = np.searchsorted(np.asarray(bounds[1:], dtype=np.int64), rows, side="right")
    assert not (pushed & (owner == row_owner)).any(), "a local entry is never pushed"
    return csr(~pushed), [csr(pushed & (owner == q)) for q in range(world)]


def sharded_appnp_bf16(rows, cols, vals, pushed, bounds, H0, a, K):
    """H_K (float64) of the bf16 propagation over the blocks ``bounds`` cuts."""
    H0 = np.asarray(H0, dtype=np.float32)
    if K == 0:
        return H0.astype(np.float64)
    keep, push = split_entries(rows, cols, vals, pushed, bounds)
    push = [P for P in push if P.nnz]
    beta, alpha = float(np.float32(1.0 - float(a))), float(np.float32(a))
    Ht = bf16_round(H0).astype(np.float64)
    H = None
    for k in range(K):
        S = keep @ Ht
        for P in push:
            S = S + bf16_round(P @ Ht).astype(np.float64)           # the sender's f32 sum, rounded once on its way to the link
        H = beta * S + alpha * H0.astype(np.float64)
        if k < K - 1:
            Ht = bf16_round(H).astype(np.float64)
    return H
