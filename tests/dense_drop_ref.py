"""References for the fused dropout around Dense (gnx_dense_drop, gnx_dense_wgrad_drop, sparse.dense_step): the masks from the oracle's
integers, a float64 reference over the float32 data, a float32 emulation with the stated rounding points, and first-order bounds.
numpy only: imports without a GPU.

The layer:  out = m_out s_out act((m_in s_in X) . W + b)  -- m the keep masks (hash_u24(seed, stream + counter, row, column, 0) >=
int(p 2^24)), s the f32 1 / (1 - p) taken as it is, the output mask keyed by the column of the WHOLE result.
Rounding points of the kernels (include/gnx.h): x' = fl(x s_in); the k-ascending fmaf chain over x'; + b; relu; fl(v s_out).

Bounds, first order, U = 2^-24:
  out   ((F + 2) U (sum_k |x s_in| |w| + |b|)) s_out + U |out|     the F products and sums, the rounding of x', the bias; then the scale
  dW    (n + 2) U (|x s_in|^T |g|)                                 an n-term sum in any order, the rounding of x'
  db    (n + 2) U sum_i |g|
  dX    ((O + 2) U (|g| |W|^T)) s_in + U |dX|"""
import numpy as np

from oracle import gnntf_oracle as orc

U32 = 2.0 ** -24


def scale(p):
    """The f32 1 / (1 - p) of the kernels (1.0f / (1.0f - (float)p)); 1 for p = 0."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(triple, n, C, counter=0, col0=0):
    """The keep mask [n, C] of ``triple`` = (p, seed, stream) or None (everything kept); columns keyed from ``col0`` on."""
    if triple is None or triple[0] == 0:
        return np.ones((n, C), dtype=bool)
    p, seed, stream = triple
    rows, cols = np.repeat(np.arange(n), C), np.tile(np.arange(col0, col0 + C), n)
    h = orc.hash_u24(seed, (int(stream) + int(counter)) & 0xFFFFFFFFFFFFFFFF, rows, cols, np.zeros(n * C, dtype=np.int64))
    return (h >= orc.dropout_threshold(p)).reshape(n, C)


def _s(triple):
    return np.float64(scale(triple[0])) if triple is not None else 1.0


def forward(X, W, b, relu, din, dout, counter=0):
    """float64 over the float32 data: dict(out, out_bound, pre) -- pre the float64 pre-activation (the relu's gate)."""
    n, F = X.shape
    O = W.shape[1]
    Xs = np.where(keep_mask(din, n, F, counter), X.astype(np.float64) * _s(din), 0.0)
    W64 = W.astype(np.float64)
    b64 = np.zeros(O) if b is None else b.astype(np.float64).reshape(-1)
    pre = Xs @ W64 + b64
    act = np.maximum(pre, 0.0) if relu else pre
    m_out = keep_mask(dout, n, O, counter)
    out = np.where(m_out, act * _s(dout), 0.0)
    magnitude = np.abs(Xs) @ np.abs(W64) + np.abs(b64)
    bound = np.where(m_out, (F + 2) * U32 * magnitude * _s(dout), 0.0) + U32 * np.abs(out)
    return dict(out=out, out_bound=bound, pre=pre)


def backward(X, W, G, din, counter=0):
    """float64 over the float32 data, G the gated gradient the backward starts from: dict(dW, dW_bound, db, db_bound, dX, dX_bound)."""
    n, F = X.shape
    O = W.shape[1]
    m_in = keep_mask(din, n, F, counter)
    Xs = np.where(m_in, X.astype(np.float64) * _s(din), 0.0)
    G64, W64 = G.astype(np.float64), W.astype(np.float64)
    dX = np.where(m_in, (G64 @ W64.T) * _s(din), 0.0)
    dX_bound = np.where(m_in, (O + 2) * U32 * (np.abs(G64) @ np.abs(W64).T) * _s(din), 0.0) + U32 * np.abs(dX)
    return dict(dW=Xs.T @ G64, dW_bound=(n + 2) * U32 * (np.abs(Xs).T @ np.abs(G64)),
                db=G64.sum(axis=0), db_bound=(n + 2) * U32 * np.abs(G64).sum(axis=0), dX=dX, dX_bound=dX_bound)


def gated(g, out, relu, dout, counter=0):
    """The gated gradient in float32, exactly as the gate pass makes it: kept ? fl(g s_out) : +0, with relu also +0 where out <= 0."""
    n, O = g.shape
    G = np.where(keep_mask(dout, n, O, counter), g.astype(np.float32) * (scale(dout[0]) if dout is not None else np.float32(1)), np.float32(0))
    if relu:
        G = np.where(out > 0, G, np.float32(0))
    return G.astype(np.float32)


def ratio(got, want, bound):
    """max |got - want| / bound (0 / 0 counts as 0: an element the bound says is exact must be exact)."""
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


# ---- the float32 emulation and the planted mistakes ------------------------------------------------------------------------------------
def _chain(Xs, W):
    """The k-ascending fmaf chain in float32: acc <- fl(acc + x_k w_k), the product exact (float64 holds it)."""
    acc = np.zeros((Xs.shape[0], W.shape[1]), dtype=np.float32)
    W64 = W.astype(np.float64)
    for k in range(Xs.shape[1]):
        acc = (acc.astype(np.float64) + Xs[:, k:k + 1].astype(np.float64) * W64[k:k + 1, :]).astype(np.float32)
    return acc


def emulate(X, W, b, relu, din, dout, counter=0, mistake=None, panel=256):
    """The kernels' arithmetic in numpy float32.  ``mistake``: None, or one of
      "panel_column"  the output mask keyed by the column inside its panel of ``panel`` outputs instead of the global column
      "scale_after"   the input scale applied to the finished product (bias included) instead of to x
      "mask_first"    the output mask applied to the product, ahead of bias and relu, instead of behind them"""
    n, F = X.shape
    O = W.shape[1]
    s_in = scale(din[0]) if din is not None else np.float32(1)
    s_out = scale(dout[0]) if dout is not None else np.float32(1)
    m_in = keep_mask(din, n, F, counter)
    if mistake == "panel_column":
        m_out = np.concatenate([keep_mask(dout, n, min(panel, O - o0), counter) for o0 in range(0, O, panel)], axis=1)
    else:
        m_out = keep_mask(dout, n, O, counter)
    b32 = np.zeros(O, dtype=np.float32) if b is None else b.astype(np.float32).reshape(-1)
    if mistake == "scale_after":
        v = (_chain(np.where(m_in, X, np.float32(0)).astype(np.float32), W) + b32) * s_in
    else:
        v = _chain(np.where(m_in, X * s_in, np.float32(0)).astype(np.float32), W)
        if mistake == "mask_first":
            v = np.where(m_out, v * s_out, np.float32(0)).astype(np.float32)
        v = v + b32
    v = np.maximum(v, np.float32(0)) if relu else v
    if mistake != "mask_first":
        v = np.where(m_out, v * s_out, np.float32(0))
    return v.astype(np.float32)
