"""Float64 references and derived error bounds for the node signals at width 1 (csrc/gnx_signal.hip: the projection, the width-1 SpMV and
its PPR loop, FastReg's smoothness quotient and its gradient), and the dense float64 restatement of a GCNIIReg training step.  numpy and
scipy only at import: imports without a GPU (the model restatement imports tests/model_step_ref.py, hence CPU torch, when it is asked for).

The references take the very float32 operands the kernels read, in float64.  The bounds are first-order bounds of the same float32
computation with its sums taken IN ANY ORDER, in the manner of tests/gcnii_shapes_ref.py, so nothing in them is tuned to a kernel:
    a sum of t terms in any order: (t - 1 + c) u sum|terms|, u = 2^-24; a row cut into chunks adds one term per chunk; the constant c
    covers the roundings around the sum (products that are not fused, a scaling, the final add) and the second-order remainder;
    a global sum over the n rows: the same with t = n, plus the elementwise bound of every addend propagated through it;
    a quantity computed from inexact quantities: its first-order propagated error plus one u per rounding of its own formula.
The criterion everywhere is  max |got - want| / bound <= 1  (gcnii_shapes_ref.ratio).

The projection: f_i = 1 / (1 + expf(-z_i)), z_i = sum_c X_ic w_c.  |dz_i| <= (C + 1) u sum_c |X_ic w_c| (C terms in any order, products
fused or not); the sigmoid has Lipschitz constant 1/4; and the formula itself -- expf, the add, the divide -- moves f by at most EXPF_K u f:
    bound = u (C + 1) sum_c |X_ic w_c| / 4 + EXPF_K u f_i.
EXPF_K: the maximum ULP error of expf as the HIP math documentation states it, plus 2 for the add and the divide.  No document of the
ROCm installation this was written against states it (a search of its .md / .rst / .txt / .html files for "expf" finds none), so
EXPF_K = 4, the value the issue sets for that case.  It is a condition, not a measurement: a wrong or dropped term moves f by about 1e-2,
and 4 u is 2.4e-7."""
import numpy as np
import scipy.sparse as sp

import gcnii_shapes_ref as shapes

U32 = shapes.U32
EXPF_K = 4
f64 = shapes.f64
ratio = shapes.ratio
PPR_ITERATIONS = 10


def ratio1(got, want, bound, rows=None):
    """gcnii_shapes_ref.ratio for [n] vectors and scalars."""
    got, want, bound = (np.atleast_1d(f64(x)).reshape(-1, 1) for x in (got, want, bound))
    return ratio(got, want, bound, rows)


def reversal(coo, vals, shape):
    """The same entries with rows and columns swapped: the transposed walk of the reversal sees the planted hub rows."""
    return np.ascontiguousarray(coo[:, ::-1]), vals, (shape[1], shape[0])


def csr64(coo, vals, shape):
    return shapes.csr_of(coo, vals, shape, dtype=np.float64)


def row_terms(A, L):
    """Terms of every row's sum: its entries plus one per chunk of a row longer than L."""
    deg = np.diff(A.indptr)
    return deg + shapes.chunk_counts(deg, L)


# ---- the width-1 SpMV and its loop -------------------------------------------------------------------------------------------------------
def spmv_ref(A, x, h0, beta, alpha, L):
    """out = beta (A x) + alpha h0 (h0 None: the constant 1) and its bound (terms + 4) u (beta |A| |x| + alpha |h0|): t - 1 adds of the
    sum, the scaling by beta, the product alpha h0, the final add, one to spare.  beta, alpha: the float32 values the launch takes."""
    A = sp.csr_matrix(A, dtype=np.float64)
    h = np.ones(A.shape[0]) if h0 is None else f64(h0)
    beta, alpha = float(np.float32(beta)), float(np.float32(alpha))
    want = beta * (A @ f64(x)) + alpha * h
    size = abs(beta) * (abs(A) @ np.abs(f64(x))) + abs(alpha) * np.abs(h)
    return want, (row_terms(A, L) + 4) * U32 * size


def ppr_ref(A, h0, a, K, L):
    """K steps x <- beta A x + alpha h0 from x = h0, beta = float32(1 - a), alpha = float32(a); the bound carried through the steps:
    E_0 = 0, E_{k+1} = beta |A| E_k + (the step's own bound at the reference iterate)."""
    A = sp.csr_matrix(A, dtype=np.float64)
    beta, alpha = shapes.mix_constants(a)
    x = np.ones(A.shape[0]) if h0 is None else f64(h0)
    bound = np.zeros(A.shape[0])
    for _ in range(K):
        step, own = spmv_ref(A, x, h0, beta, alpha, L)
        bound = beta * (abs(A) @ bound) + own
        x = step
    return x, bound


def colsum_ref(A):
    """D_j = sum_i A_ij and its bound (entries of the column + 1) u sum_i |A_ij|."""
    A = sp.csr_matrix(A, dtype=np.float64)
    At = sp.csr_matrix(A.T)
    D = np.asarray(At.sum(axis=1)).reshape(-1)
    return D, (np.diff(At.indptr) + 1) * U32 * np.asarray(abs(At).sum(axis=1)).reshape(-1)


# ---- the projection --------------------------------------------------------------------------------------------------------------------
def project_ref(X, w, act=1):
    """(f, bound): the module docstring's bound; act = 0: the dot product z with (C + 1) u sum |X w|."""
    X, w = f64(X), f64(w).reshape(-1)
    z = X @ w
    size = np.abs(X) @ np.abs(w)
    C = X.shape[1]
    if not act:
        return z, (C + 1) * U32 * size
    with np.errstate(over="ignore"):
        f = 1.0 / (1.0 + np.exp(-z))
    return f, U32 * (C + 1) * size / 4 + EXPF_K * U32 * f


# ---- the smoothness quotient -------------------------------------------------------------------------------------------------------------
def smoothness_f64(A, X, w, D, upstream=1.0):
    """The mathematics alone, in float64: lambda = sum (f - A f)^2 / sum D f^2 with f = sigmoid(X w), and the analytic gradient of
    upstream * lambda: gz = upstream (2 / den) ((d - A^T d) - lambda D f) f (1 - f) w.r.t. z = X w, dX = gz w^T, dw = X^T gz."""
    A = sp.csr_matrix(A, dtype=np.float64)
    X, w, D = f64(X), f64(w).reshape(-1), f64(D)
    f = 1.0 / (1.0 + np.exp(-(X @ w)))
    d = f - A @ f
    num, den = float(d @ d), float(D @ (f * f))
    lam = num / den
    gz = upstream * (2.0 / den) * ((d - A.T @ d) - lam * D * f) * f * (1.0 - f)
    return dict(f=f, d=d, num=num, den=den, lam=lam, gz=gz, dX=np.outer(gz, w), dw=X.T @ gz)


def smoothness_ref(A, X, w, D, L, Lt, upstream=1.0):
    """smoothness_f64 over the float32 operands (X, w, the adjacency's values, D, the upstream scalar) with a first-order any-order bound
    per quantity (``*_bound``).  L, Lt: the long-row thresholds of the structure and of its transpose (one extra term per chunk).
    Each line below: the propagated error of the operands, plus u per rounding of the line's own formula.
      f      project_ref
      d      = f - A f:           df + |A| df + (terms + 3) u (|f| + |A| |f|)
      num    = sum d^2:           sum 2 |d| dd + (n + 2) u num
      den    = sum D f^2:         sum 2 D |f| df + (n + 3) u den
      lambda = num / den:         lambda (dnum / num + dden / den + 2 u)
      q      = A^T d:             |A^T| dd + (terms_t + 1) u |A^T| |d|
      inner  = (d - q) - lambda D f:  dd + dq + dlambda D |f| + lambda D df + 8 u (|d| + |q| + lambda D |f|)
               (8: whichever way the three terms are formed and subtracted -- fused here, 2 d / den, A^T (2 d / den) and
               2 (num / den^2) D f under autograd -- each carries at most 6 roundings and meets 2 subtractions)
      s      = f (1 - f):         df + 3 u s
      c      = upstream 2 / den:  |c| (dden / den + 3 u)
      gz     = c inner s:         |inner s| dc + |c s| dinner + |c inner| ds + 4 u |gz|
      dX     = gz w^T:            dgz |w|^T + u |dX|
      dw     = X^T gz:            |X|^T dgz + (n + 1) u |X|^T |gz|"""
    A = sp.csr_matrix(A, dtype=np.float64)
    At = sp.csr_matrix(A.T)
    absA, absAt = abs(A), abs(At)
    X64, w64, D = f64(X), f64(w).reshape(-1), f64(D)
    n = A.shape[0]
    upstream = float(np.float32(upstream))
    r = smoothness_f64(A, X, w, D, upstream)
    f, d, num, den, lam, gz = r["f"], r["d"], r["num"], r["den"], r["lam"], r["gz"]
    df = project_ref(X, w)[1]
    dd = df + absA @ df + (row_terms(A, L) + 3) * U32 * (np.abs(f) + absA @ np.abs(f))
    dnum = float(2 * np.abs(d) @ dd) + (n + 2) * U32 * num
    dden = float(2 * (D * np.abs(f)) @ df) + (n + 3) * U32 * den
    dlam = lam * (dnum / num + dden / den + 2 * U32)
    q = At @ d
    dq = absAt @ dd + (row_terms(At, Lt) + 1) * U32 * (absAt @ np.abs(d))
    inner = (d - q) - lam * D * f
    dinner = dd + dq + dlam * D * np.abs(f) + lam * D * df + 8 * U32 * (np.abs(d) + np.abs(q) + lam * D * np.abs(f))
    s = f * (1.0 - f)
    ds = df + 3 * U32 * s
    c = upstream * 2.0 / den
    dc = abs(c) * (dden / den + 3 * U32)
    dgz = np.abs(inner * s) * dc + np.abs(c * s) * dinner + np.abs(c * inner) * ds + 4 * U32 * np.abs(gz)
    r.update(f_bound=df, d_bound=dd, num_bound=dnum, den_bound=dden, lam_bound=dlam, gz_bound=dgz,
             dX_bound=np.outer(dgz, np.abs(w64)) + U32 * np.abs(r["dX"]),
             dw_bound=np.abs(X64).T @ dgz + (n + 1) * U32 * (np.abs(X64).T @ np.abs(gz)))
    return r


def directed_graph_12(seed=4):
    """A 12-node directed graph for the gradient check: dense float64 adjacency with about a third of the entries, one row and one
    column empty."""
    rng = np.random.default_rng(seed)
    A = (rng.random((12, 12)) < 0.35) * rng.uniform(0.5, 1.5, size=(12, 12))
    A[3, :] = 0.0
    A[:, 7] = 0.0
    return A


# ---- FastReg's projection vector ---------------------------------------------------------------------------------------------------------
def uniform_draw(seed, stream, n, bound=1.0):
    """gnx_signal_uniform: bound * (hash_u24(seed, stream, i, 0, 0) - 2^23) / 2^23 as float32 (exact before the scaling)."""
    from oracle import gnntf_oracle as orc
    zeros = np.zeros(n, dtype=np.int64)
    h = orc.hash_u24(seed, stream, np.arange(n, dtype=np.int64), zeros, zeros).astype(np.int64)
    return np.float32(bound) * ((h - (1 << 23)).astype(np.float32) * np.float32(2.0 ** -23))


# ---- a GCNIIReg training step in dense float64 ---------------------------------------------------------------------------------------------
def gcniireg_layers(num_classes, latent_dims=(64,), iterations=2, dropout=0.6, a=0.1, l=0.5):
    """experimental_gcn.py:21-29 as model_step_ref describes layers: Dropout, Dense(relu, dropout) per latent width -- the last is H0 --,
    FastReg, the GCNII layers, Dense(num_classes, regularize=False).  Feature masks are the host-drawn ones (model_step_ref.FixedMasks)."""
    layers = [dict(kind="dropout", rate=dropout, mask="torch")]
    layers += [dict(kind="dense", outputs=w, act="relu", rate=dropout, regularize=True, mask="torch") for w in latent_dims]
    h0 = len(layers) - 1
    layers.append(dict(kind="fastreg"))
    layers += [dict(kind="gcnii", spectral=False, a=a, l=l, k=k, rate=dropout, graph_dropout=0, h0=h0, regularize=True, mask="torch")
               for k in range(iterations)]
    layers.append(dict(kind="dense", outputs=num_classes, act=None, rate=0, regularize=False, mask="torch", last=True))
    return layers


def gcniireg_reference(layers, coo, vals, shape, X, parameters, task, weight_decay, seed, fixed, projection="uniform"):
    """model_step_ref.Reference with the FastReg layer: in a training-mode forward the layer draws one stream for its projection vector
    W (uniform_draw) and passes its input on; the objective then takes -lambda over the adjacency dropped at 0.5 under the NEXT stream
    (drawn when the loss is formed, after the whole forward), un-normalised, D its column sums.  ``.fastreg`` holds what the last
    training forward used: w_stream, W, g_stream.
    ``projection``: "uniform" is this project's FastReg, a NAMED DEVIATION from the reference; "zeros" is the reference's own text:
    its FastReg creates W inside the forward (experimental_filter.py:31), after train()'s only reset() (trainable.py:53), and a new
    variable holds zeros (variables.py:6) -- so W = 0 in every forward, f = sigmoid(0) = 1/2 everywhere, -lambda is a constant of the
    dropped adjacency with no gradient, and no stream is drawn for W (the dropped adjacency takes the forward's next one).
    tests/test_reference_golden_cpu.py holds "zeros" to the reference's recorded steps at 1e-9 and asserts what "uniform" changes."""
    if projection not in ("uniform", "zeros"):
        raise Exception("projection is \"uniform\" or \"zeros\"")
    import torch

    import model_step_ref as ref
    from oracle import gnntf_oracle as orc

    class Reference(ref.Reference):
        def _layer_streams(self, layer, training):
            if layer["kind"] == "fastreg":
                if training:
                    self.fastreg = dict(w_stream=self._draw() if projection == "uniform" else None)
                return None, None
            return super()._layer_streams(layer, training)

        def forward(self, training):
            out, penalty = super().forward(training)
            at = next((i for i, layer in enumerate(self.layers) if layer["kind"] == "fastreg"), None)
            if not training or at is None:
                return out, penalty
            feats = self.values[at]
            info = self.fastreg
            info["g_stream"] = self._draw()
            info["W"] = uniform_draw(self.seed, info["w_stream"], feats.shape[1]) if projection == "uniform" else np.zeros(feats.shape[1], dtype=np.float32)
            ai, av = orc.get_adjacency(self.coo, self.vals, self.shape, graph_dropout=0.5, normalized="none", training=True, seed=self.seed,
                                       stream=info["g_stream"], dtype=np.float64)
            G = self._dense(ai, av)
            f = torch.sigmoid(feats @ torch.from_numpy(info["W"].astype(np.float64)).to(self.dtype).reshape(-1, 1))
            diffs = f - G @ f
            lam = (diffs * diffs).sum() / (G.sum(dim=0).reshape(-1, 1) * f * f).sum()
            info["lam"] = float(lam.detach())
            return out, penalty - lam

    return Reference(layers, coo, vals, shape, X, parameters, task, weight_decay, seed, fixed=fixed)
