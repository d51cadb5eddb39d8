"""numpy helpers for the fused GCNLayer (gnx_gcn_step, gnx_gcn_step_dropped, sparse.gcn_step): the float64 reference of the forward and
of the backward, their derived bounds and the float32 emulations the bounds must admit.  Graphs, the first-order terms, ``ratio`` and the
float32 products are those of tests/gcnii_shapes_ref.py, imported.  numpy and scipy only: imports without a GPU.

The layer (gcn.py:88-89):  agg = A . X,  P = agg . W + b,  out = s m act(P)  -- m the keep mask, s the f32 1 / (1 - p) taken as it is.

The bounds are first-order bounds of a float32 evaluation of the same terms IN ANY ORDER, as in gcnii_shapes_ref.forward_ref: a sum of
t terms costs (t - 1) u sum |terms|, a row cut into chunks adds one term per chunk, the product with W adds C_in terms; the constants
cover the rounding of each product, the bias add, the scaling by s and the second-order remainder:
    agg_bound = (deg + chunks + 4) u |A| |X|
    out_bound = (deg + chunks + C_in + 7) u (|A| |X| |W| + |b|)         (times s where a mask scales the result; relu is 1-Lipschitz)
The backward over the gated gradient G' [n, C_out] the launches hold (float32, taken as data):
    dW = agg^T G'    bound (n + 2) u |agg|^T |G'|                        (agg = the float32 rows the forward kept)
    db = column sums of G'    bound (n + 2) u sum |G'|
    dX = A^T (G' W^T)         bound (deg^T + chunks^T + C_out + 6) u |A^T| (|G'| |W^T|)
The criterion everywhere is  max |got - want| / bound <= 1."""
import numpy as np
import scipy.sparse as sp

from gcnii_shapes_ref import (U32, chunk_counts, csr_of, f64, matmul_f32, plan_threshold, planted_graph, ratio, ratio_rows,  # noqa: F401
                              regime_graph, spmm_f32)

SHAPES = ((16, 16), (32, 32), (64, 64), (64, 48), (64, 40), (64, 7), (32, 1))      # (C_in, C_out) of the fused launch


def scale(p):
    """The f32 scale of the dropout as the kernels form it: 1.0f / (1.0f - (float)p)."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def operands(n, C_in, C_out, seed):
    """X, G seeded normal [n, C_in] / [n, C_out]; W = N / sqrt(C_in) [C_in, C_out]; bias uniform in +-0.3 [C_out]; float32, read-only."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, C_in)).astype(np.float32)
    G = rng.standard_normal((n, C_out)).astype(np.float32)
    W = (rng.standard_normal((C_in, C_out)) / np.sqrt(C_in)).astype(np.float32)
    bias = rng.uniform(-0.3, 0.3, size=C_out).astype(np.float32)
    out = dict(X=X, G=G, W=W, bias=bias)
    for x in out.values():
        x.setflags(write=False)
    return out


def terms_of(A, L):
    deg = np.diff(A.indptr)
    return (deg + chunk_counts(deg, L))[:, None]


def forward_ref(A, X, W, bias, relu, p=0.0, mask=None, L=None):
    """A: scipy CSR of the float32 weights.  float64: dict(agg, agg_bound, P, out, out_bound) -- see the module docstring."""
    n, C_in = X.shape
    L = plan_threshold(n) if L is None else L
    A = sp.csr_matrix(A, dtype=np.float64)
    terms = terms_of(A, L)
    agg = A @ f64(X)
    size = abs(A) @ np.abs(f64(X))
    b = np.zeros(W.shape[1]) if bias is None else f64(bias).reshape(-1)
    P = agg @ f64(W) + b[None, :]
    act = np.maximum(P, 0.0) if relu else P
    s = float(scale(p))
    m = np.ones(P.shape) if mask is None else f64(mask)
    return dict(agg=agg, agg_bound=(terms + 4) * U32 * size, P=P, out=s * m * act,
                out_bound=s * (terms + C_in + 7) * U32 * (size @ np.abs(f64(W)) + np.abs(b)[None, :]))


def forward_f32(A32, X, W, bias, relu, order, L):
    """(agg, out) of the layer in float32 under ``order`` ("library", "sequential", "chunked"), every operation rounded once."""
    agg = spmm_f32(A32, X, order, L)
    P = matmul_f32(agg, W, order)
    if bias is not None:
        P = (P + np.asarray(bias, dtype=np.float32).reshape(1, -1)).astype(np.float32)
    return agg, np.maximum(P, np.float32(0)) if relu else P


def gate_f32(g, out, relu, p=0.0, mask=None):
    """G' as the backward's first pass forms it in float32, bit for bit: kept ? g s : 0, with relu also 0 where out <= 0."""
    G = np.asarray(g, dtype=np.float32)
    if p != 0:
        G = np.where(mask, G * scale(p), np.float32(0)).astype(np.float32)
    return np.where(np.asarray(out) > 0, G, np.float32(0)) if relu else G


def backward_ref(A, agg32, G, W, L=None):
    """float64 over the float32 data (the gated gradient G and the kept rows agg32): dict(dX, dX_bound, dW, dW_bound, db, db_bound)."""
    n = G.shape[0]
    L = plan_threshold(n) if L is None else L
    At = sp.csr_matrix(sp.csr_matrix(A, dtype=np.float64).T)
    terms = terms_of(At, L)
    G, Wt = f64(G), f64(W).T
    C_out = G.shape[1]
    dX = At @ (G @ Wt)
    dX_bound = (terms + C_out + 6) * U32 * (abs(At) @ (np.abs(G) @ np.abs(Wt)))
    T = f64(agg32)
    return dict(dX=dX, dX_bound=dX_bound, dW=T.T @ G, dW_bound=(n + 2) * U32 * (np.abs(T).T @ np.abs(G)),
                db=G.sum(axis=0), db_bound=(n + 2) * U32 * np.abs(G).sum(axis=0))


def backward_f32(A32, agg32, G, W, order, L):
    """(dX, dW, db) in float32 under ``order``."""
    At32 = sp.csr_matrix(A32.T)
    At32.sort_indices()
    G = np.asarray(G, dtype=np.float32)
    dX = spmm_f32(At32, matmul_f32(G, np.ascontiguousarray(np.asarray(W, dtype=np.float32).T), order), order, L)
    dW = matmul_f32(np.ascontiguousarray(np.asarray(agg32, dtype=np.float32).T), G, order)
    db = G.sum(axis=0, dtype=np.float32) if order == "library" else matmul_f32(np.ones((1, len(G)), dtype=np.float32), G, order)[0]
    return dX, dW, db
