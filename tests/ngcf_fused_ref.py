"""numpy helpers for the fused NGCFLayer (gnx_ngcf_step, gnx_ngcf_back_gate, sparse.ngcf_step): the float64 reference of the forward and of
the backward, their derived bounds and a float32 emulation the bounds must admit.  Graphs, ``ratio`` and the float32 products are those of
tests/gcnii_shapes_ref.py / tests/gcn_fused_ref.py, imported.  numpy and scipy only: imports without a GPU.

The layer (gcn.py:116-135), A the bipartite-normalised adjacency (float32 weights taken as data):
    agg = A . X      M = X * agg      P1 = M . W1 + b1      P2 = agg . W2 + b2      S = act(P1) + act(P2)
    x = s m S  (m the keep mask, s the f32 1 / (1 - p) taken as it is)      r = 1 / sqrt(max(sum_c x_c^2, 1e-12f))      y = x r
act is the identity, the relu or the leaky relu whose slope is the float32 0.2f taken as it is.

The forward bounds are first-order bounds of a float32 evaluation of the same terms IN ANY ORDER (u = 2^-24; a sum of t terms costs
(t - 1) u sum |terms|, a rounded product u |product|; one spare u per line covers the second-order remainder), with
|A| |X| =: a_abs, deg + chunks =: t (a row cut into chunks adds one term per chunk):
    e_agg = (t + 4) u a_abs                                             the GCN bound for agg (gcn_fused_ref.forward_ref)
    e_M   = |X| e_agg + u |X| a_abs  <=  (t + 5) u |X| a_abs            the product with the row's own X: one rounding
    e_P2  = e_agg |W2| + (C_in + 3) u (a_abs |W2| + |b2|)  <=  (t + C_in + 7) u (a_abs |W2| + |b2|)       the GCN bound for out
    e_P1  = e_M |W1| + (C_in + 3) u (|X| a_abs |W1| + |b1|)  <=  (t + C_in + 8) u ((|X| a_abs) |W1| + |b1|)
    e_S   = e_P1 + e_P2 + 2 u (|act P1| + |act P2|)                     act is 1-Lipschitz; the leaky multiply and the add round once each
    e_x   = s m e_S + u |x|                                             the mask's multiply by s (p = 0: no multiply, the term stays)
Through the norm, with y = x r and dr / r = -r^2 sum_k x_k dx_k to first order:
    dy_c = r (dx_c - y_c sum_k y_k dx_k)    =>    |dy_c| <= r (e_x_c + |y_c| sum_k |y_k| e_x_k)
and the norm's own arithmetic: the sum of C_out squares in any order is off by at most (C_out + 1) u relatively (C_out products, C_out - 1
adds, all terms >= 0; fused multiply-adds only lose roundings), which the square root halves; sqrtf and the division are IEEE
operations, correctly rounded (u each: the library is built without fast-math and the compiler's default for HIP keeps both exact to
0.5 ulp); the final multiply is one more u:
    e_y = r (e_x_c + |y_c| sum_k |y_k| e_x_k) + ((C_out + 1) / 2 + 4) u |y_c|
A row whose sum of squares is below the clamp leaves as x * 1e6 (r is a constant there):  e_y = 1e6 e_x + 2 u |y|.  Both forms agree at
the clamp to first order; the operands of the tests have no row near it but the rows of exact zeros.

The backward, given the gate bits (bit1 = P1 > 0, bit2 = P2 > 0: data, judged on their own) and the mask, for an upstream gradient g:
    d = sum_k y_k g_k      g_s = r (g - y d)  (clamped rows: r g)      g_u = s m g_s      G1 = g_u (bit1 ? 1 : slope)      G2 likewise
    db = column sums of G      dW1 = M^T G1      dW2 = agg^T G2      Q1 = G1 W1^T      Q2 = G2 W2^T
    dA = Q1 * X + Q2           dX = Q1 * agg + A^T dA
The launches read the FLOAT32 y, r, agg and M of the forward, so the forward's errors enter (rho = the relative error of r):
    rho   = r sum_k |y_k| e_x_k + ((C_out + 1) / 2 + 3) u
    e_d   = sum_k e_y_k |g_k| + (C_out + 1) u sum_k |y_k g_k|
    e_gs  = r (e_y |d|_abs + |y| e_d) + (rho + 4 u) r (|g| + |y| |d|_abs)          |d|_abs = sum_k |y_k g_k| >= |d|
    e_G   = s m e_gs + 2 u |G|                                                     the scale and the slope: one rounding each
    e_db  = sum_i e_G + (n + 2) u sum_i |G|
    e_dW1 = e_M^T |G1| + |M|^T e_G1 + (n + 2) u |M|^T |G1|                          dW2 likewise with agg, e_agg
    e_Q   = e_G |W^T| + (C_out + 2) u |G| |W^T|
    e_dA  = e_Q1 |X| + e_Q2 + 2 u (|Q1| |X| + |Q2|)
    e_dX  = e_Q1 |agg| + |Q1| e_agg + |A^T| e_dA + (t^T + 4) u |A^T| (|Q1| |X| + |Q2|) + 2 u (|Q1| |agg| + |A^T| (|Q1| |X| + |Q2|))
The criterion everywhere is  max |got - want| / bound <= 1."""
import numpy as np
import scipy.sparse as sp

from gcn_fused_ref import SHAPES, scale, terms_of                                      # noqa: F401
from gcnii_shapes_ref import (U32, chunk_counts, csr_of, f64, matmul_f32, plan_threshold, ratio, ratio_rows, regime_graph,  # noqa: F401
                              spmm_f32)

SLOPE32 = {"none": np.float32(1.0), "relu": np.float32(0.0), "leaky": np.float32(0.2)}
CLAMP = float(np.float32(1e-12))


def bipartite(coo, vals, shape):
    """The bipartite normalisation of gnx_graph_normalize (gnn.py:43-45): v_ij <- v_ij / colsum[i], the row scaled by the sum of the column of the same index -- (A64, A32): the
    float64 CSR and the same weights rounded once to float32.  The tests read the weights back from the handle; this is for the CPU."""
    A = csr_of(coo, vals, shape)
    d = np.asarray(A.sum(axis=0)).ravel()
    A64 = sp.csr_matrix(sp.diags(np.where(d > 0, 1.0 / np.where(d > 0, d, 1.0), 0.0)) @ A)
    A64.sort_indices()
    A32 = sp.csr_matrix(A64, dtype=np.float32)
    return sp.csr_matrix(A32, dtype=np.float64), A32


def operands(n, C_in, C_out, seed):
    """X, g seeded normal [n, C_in] / [n, C_out]; W1, W2 = N / sqrt(C_in); b1, b2 uniform in +-0.3 [C_out]; float32, read-only.  The
    biases keep every pre-activation of a row without entries (P = b exactly) decided: |b| is far above its bound."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, C_in)).astype(np.float32)
    g = rng.standard_normal((n, C_out)).astype(np.float32)
    W1 = (rng.standard_normal((C_in, C_out)) / np.sqrt(C_in)).astype(np.float32)
    W2 = (rng.standard_normal((C_in, C_out)) / np.sqrt(C_in)).astype(np.float32)
    b1 = rng.uniform(-0.3, 0.3, size=C_out).astype(np.float32)
    b2 = rng.uniform(-0.3, 0.3, size=C_out).astype(np.float32)
    out = dict(X=X, g=g, W1=W1, W2=W2, b1=b1, b2=b2)
    for x in out.values():
        x.setflags(write=False)
    return out


def act64(P, activation):
    return np.where(P > 0, P, float(SLOPE32[activation]) * P)


def forward_ref(A, X, W1, b1, W2, b2, activation, normalize=True, p=0.0, mask=None, L=None, e_A=None):
    """A: scipy CSR of the float32 weights.  float64: dict(agg, e_agg, M, e_M, P1, e_P1, P2, e_P2, x, e_x, r, clamped, out, out_bound) --
    the module docstring has the derivation; ``out`` is y with ``normalize``, else x.  ``e_A`` (a CSR of entrywise bounds, or None):
    where the reference is NOT over the very weights the kernel reads (tests against the oracle, which normalises in float64), the
    weights' own error: e_agg gains e_A |X|, which flows on through |X|, |W1| and |W2| like the rest of e_agg."""
    n, C_in = X.shape
    C_out = W1.shape[1]
    L = plan_threshold(n) if L is None else L
    A = sp.csr_matrix(A, dtype=np.float64)
    t = terms_of(A, L)
    X64 = f64(X)
    agg = A @ X64
    a_abs = abs(A) @ np.abs(X64)
    extra = np.zeros(a_abs.shape) if e_A is None else e_A @ np.abs(X64)
    e_agg = (t + 4) * U32 * a_abs + extra
    M, m_abs = X64 * agg, np.abs(X64) * a_abs
    e_M = (t + 5) * U32 * m_abs + np.abs(X64) * extra
    z = np.zeros(C_out)
    c1, c2 = (z if b1 is None else f64(b1).reshape(-1)), (z if b2 is None else f64(b2).reshape(-1))
    P1 = M @ f64(W1) + c1[None, :]
    P2 = agg @ f64(W2) + c2[None, :]
    e_P1 = (t + C_in + 8) * U32 * (m_abs @ np.abs(f64(W1)) + np.abs(c1)[None, :]) + (np.abs(X64) * extra) @ np.abs(f64(W1))
    e_P2 = (t + C_in + 7) * U32 * (a_abs @ np.abs(f64(W2)) + np.abs(c2)[None, :]) + extra @ np.abs(f64(W2))
    a1, a2 = act64(P1, activation), act64(P2, activation)
    S = a1 + a2
    e_S = e_P1 + e_P2 + 2 * U32 * (np.abs(a1) + np.abs(a2))
    s = float(scale(p))
    m = np.ones(S.shape) if mask is None else f64(mask)
    x = s * m * S
    e_x = s * m * e_S + U32 * np.abs(x)
    ss = (x * x).sum(axis=1, keepdims=True)
    clamped = ss < CLAMP
    r = 1.0 / np.sqrt(np.maximum(ss, CLAMP))
    y = x * r
    e_y = np.where(clamped, 1e6 * e_x + 2 * U32 * np.abs(y),
                   r * (e_x + np.abs(y) * (np.abs(y) * e_x).sum(axis=1, keepdims=True)) + ((C_out + 1) / 2 + 4) * U32 * np.abs(y))
    out = dict(agg=agg, e_agg=e_agg, a_abs=a_abs, M=M, e_M=e_M, P1=P1, e_P1=e_P1, P2=P2, e_P2=e_P2, x=x, e_x=e_x, r=r, clamped=clamped,
               y=y, e_y=e_y, t=t)
    out["out"], out["out_bound"] = (y, e_y) if normalize else (x, e_x)
    return out


def forward_f32(A32, X, W1, b1, W2, b2, activation, normalize, order, L):
    """dict(agg, out, rnorm) of the layer in float32 under ``order`` ("library", "sequential", "chunked"), every operation rounded once."""
    f32 = np.float32
    agg = spmm_f32(A32, X, order, L)
    P1 = matmul_f32((np.asarray(X, dtype=f32) * agg).astype(f32), W1, order)
    P2 = matmul_f32(agg, W2, order)
    if b1 is not None:
        P1 = (P1 + np.asarray(b1, dtype=f32).reshape(1, -1)).astype(f32)
    if b2 is not None:
        P2 = (P2 + np.asarray(b2, dtype=f32).reshape(1, -1)).astype(f32)
    act = lambda P: np.where(P > 0, P, (SLOPE32[activation] * P).astype(f32)).astype(f32)
    x = (act(P1) + act(P2)).astype(f32)
    if not normalize:
        return dict(agg=agg, out=x, rnorm=None)
    ss = np.zeros(len(x), dtype=f32)
    for c in range(x.shape[1]):
        ss = (ss + (x[:, c] * x[:, c]).astype(f32)).astype(f32)
    r = (f32(1.0) / np.sqrt(np.maximum(ss, f32(1e-12)), dtype=f32)).astype(f32)
    return dict(agg=agg, out=(x * r[:, None]).astype(f32), rnorm=r)


def gate_share(want):
    """(decided1, decided2, undecided share): where |P| exceeds its forward bound the float64 sign is the bit a float32 evaluation has."""
    d1, d2 = np.abs(want["P1"]) > want["e_P1"], np.abs(want["P2"]) > want["e_P2"]
    return d1, d2, 1.0 - (d1.sum() + d2.sum()) / (d1.size + d2.size)


def unpack_gate(words, C_out):
    """(bit1, bit2) [n, C_out] bool from the gate words [n, 2 ceil(C_out / 32)] (int32 or uint32): the P1 words, then the P2 words."""
    words = np.ascontiguousarray(words).view(np.uint32)
    W = (C_out + 31) // 32
    assert words.shape[1] == 2 * W
    c = np.arange(C_out)
    take = lambda half: ((half[:, c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)
    return take(words[:, :W]), take(words[:, W:])


def back_gate_ref(f, g, bit1, bit2, activation, normalize=True, p=0.0, mask=None):
    """(G1, e_G1, G2, e_G2) in float64 from a forward_ref result ``f`` (made with the same activation, p and mask; any ``normalize``)."""
    g = f64(g)
    C_out = g.shape[1]
    s = float(scale(p))
    m = np.ones(g.shape) if mask is None else f64(mask)
    slope = float(SLOPE32[activation])
    if normalize:
        y, r, e_y, e_x = f["y"], f["r"], f["e_y"], f["e_x"]
        d = (y * g).sum(axis=1, keepdims=True)
        d_abs = np.abs(y * g).sum(axis=1, keepdims=True)
        g_s = np.where(f["clamped"], r * g, r * (g - y * d))
        rho = r * (np.abs(y) * e_x).sum(axis=1, keepdims=True) + ((C_out + 1) / 2 + 3) * U32
        e_d = (e_y * np.abs(g)).sum(axis=1, keepdims=True) + (C_out + 1) * U32 * d_abs
        e_gs = r * (e_y * d_abs + np.abs(y) * e_d) + (rho + 4 * U32) * r * (np.abs(g) + np.abs(y) * d_abs)
    else:
        g_s, e_gs = g, np.zeros(g.shape)
    g_u = s * m * g_s
    out = []
    for bit in (bit1, bit2):
        G = g_u * np.where(bit, 1.0, slope)
        out += [G, s * m * e_gs + 2 * U32 * np.abs(G)]
    return tuple(out)


def backward_ref(A, f, X, W1, W2, G1, e_G1, G2, e_G2, L=None):
    """dict(dX, dW1, dW2, db1, db2 and each name + "_bound") in float64 from a forward_ref result and the gated gradients with their bounds."""
    n = G1.shape[0]
    C_out = G1.shape[1]
    L = plan_threshold(n) if L is None else L
    At = sp.csr_matrix(sp.csr_matrix(A, dtype=np.float64).T)
    tT = terms_of(At, L)
    X64, agg, M = f64(X), f["agg"], f["M"]
    out = dict()
    for k, G, e_G, T, e_T in (("1", G1, e_G1, M, f["e_M"]), ("2", G2, e_G2, agg, f["e_agg"])):
        out["db" + k] = G.sum(axis=0)
        out["db" + k + "_bound"] = e_G.sum(axis=0) + (n + 2) * U32 * np.abs(G).sum(axis=0)
        out["dW" + k] = T.T @ G
        out["dW" + k + "_bound"] = e_T.T @ np.abs(G) + np.abs(T).T @ e_G + (n + 2) * U32 * (np.abs(T).T @ np.abs(G))
    W1t, W2t = f64(W1).T, f64(W2).T
    Q1, Q2 = G1 @ W1t, G2 @ W2t
    q1_abs, q2_abs = np.abs(G1) @ np.abs(W1t), np.abs(G2) @ np.abs(W2t)
    e_Q1 = e_G1 @ np.abs(W1t) + (C_out + 2) * U32 * q1_abs
    e_Q2 = e_G2 @ np.abs(W2t) + (C_out + 2) * U32 * q2_abs
    dA = Q1 * X64 + Q2
    da_abs = q1_abs * np.abs(X64) + q2_abs
    e_dA = e_Q1 * np.abs(X64) + e_Q2 + 2 * U32 * da_abs
    out["dX"] = Q1 * agg + At @ dA
    gathered = abs(At) @ da_abs
    out["dX_bound"] = (e_Q1 * np.abs(agg) + q1_abs * f["e_agg"] + abs(At) @ e_dA + (tT + 4) * U32 * gathered
                       + 2 * U32 * (q1_abs * f["a_abs"] + gathered))
    return out
