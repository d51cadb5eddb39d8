"""Structures, float64 references and a derived error bound for the GCNII layer family at every long-row regime of build_long_plan
(csrc/gnx_internal.h).  numpy and scipy only: imports without a GPU.

planted_graph plants rows at the lengths where the two deciders of the long-row split (d > long_row in the plan, end - beg <= long_row
in the fused kernels) could disagree, and enough hub rows that the row-list passes behind them see more than one MFMA tile (regime T)
or more than one 128-row block of the dense kernel (regime S).  The references take the very float32 weights the kernels read, in
float64.  The bound is the first-order bound of a float32 sum of the same terms IN ANY ORDER, so nothing in it is tuned to a kernel:
    recursive summation of t terms: (t - 1) u sum|terms|; a row cut into chunks adds one term per chunk; the C x C product adds C
    terms; the constant covers the weight product, the two scalings, the final add and the second-order remainder (deg u < 1e-4).
The criterion everywhere is  max |got - want| / bound <= 1."""
import numpy as np
import scipy.sparse as sp

U32 = 2.0 ** -24                                       # float32 unit roundoff
TINY_ROWS, SMALL_ROWS = 1 << 15, 1 << 20               # gnx_internal.h
LONG_ROW, SMALL_LONG_ROW = 512, 128
EMPTY_RUN = (16, 32)                                   # ids 16 .. 31: a whole 16-row tile without entries (row 0 itself is a hub row)
N_NO_IN = 3                                            # columns nothing points at (the longest planted row leaves n - 3L - 7 >= 4 free)

REGIMES = {                                            # name -> (n, L, n_hub)
    "T": (1547, LONG_ROW, 19),                         # n < TINY_ROWS: 97 tiles = 13 blocks, one live wave in the last; n % 16 = 11
    "S": (TINY_ROWS + 11, SMALL_LONG_ROW, 150),        # TINY_ROWS <= n < SMALL_ROWS: 154 hub rows, two blocks of the dense kernel
}
BOUNDARY_NS = (TINY_ROWS - 1, TINY_ROWS)               # the same graph either side of the regime boundary
BOUNDARY_ROW, BOUNDARY_LEN = 1234, 300


def plan_threshold(n):
    """long_row = long_chunk of a structure of n rows (build_long_plan)."""
    return SMALL_LONG_ROW if TINY_ROWS <= n < SMALL_ROWS else LONG_ROW


def planted_lengths(L):
    return (0, 1, 3, 4, 5, L - 1, L, L + 1, 2 * L, 2 * L + 1, 3 * L + 7)


def no_in_columns(n):
    return np.array([7, n // 2 + 3, n - 5])


def _finish(rows, cols, n, rng):
    key = rows.astype(np.int64) * n + cols
    assert len(np.unique(key)) == len(key)                                          # no duplicates: nothing to coalesce
    perm = rng.permutation(len(key))
    coo = np.stack([rows[perm], cols[perm]], axis=1).astype(np.int64)
    vals = rng.uniform(0.5, 1.5, size=len(coo)).astype(np.float32)
    return coo, vals, (n, n)


def planted_graph(n, L, n_hub, seed):
    """(coo, vals, shape, info): a directed COO without duplicates, values uniform in [0.5, 1.5) as float32, shuffled.
    Planted rows (distinct columns each): one of every length in planted_lengths(L) -- 3, 4, 5 straddle the gather loop's U = 4 tail --
    and ``n_hub`` more of lengths drawn from L + 1 .. 2 L; rows 0 and n - 1 are hub rows, so one lies in the ragged last tile when
    n % 16 != 0; ids 16 .. 31 are a run of 16 rows without entries (a whole tile of the natural order), row n // 2 is the planted empty
    row.  About 6 n background entries sit in the other rows.  Three columns (no_in_columns) receive nothing; every planted row id
    receives at least one entry, so that symmetric normalisation leaves its weights nonzero.  No column holds more than L entries:
    the transpose is hub-free.
    ``info``: rows_of[length] -> row ids, hub (ascending ids of the rows longer than L), planted, empty, no_in, ragged."""
    assert L == plan_threshold(n) and n >= 3 * L + 7 + N_NO_IN and n > 64
    rng = np.random.default_rng(seed)
    no_in = no_in_columns(n)
    columns = np.setdiff1d(np.arange(n), no_in)
    lengths = list(planted_lengths(L)) + [int(x) for x in rng.integers(L + 1, 2 * L + 1, size=n_hub)]
    reserved = np.concatenate([np.arange(*EMPTY_RUN), [n // 2, 0, n - 1], no_in])
    free = np.setdiff1d(np.arange(n), reserved)
    ids = rng.choice(free, size=len(lengths) - 3, replace=False)
    # the planted empty row at n // 2, two of the extra hub rows at 0 and n - 1, everything else at drawn ids
    at = [n // 2] + list(ids[:len(planted_lengths(L)) - 1]) + [0, n - 1] + list(ids[len(planted_lengths(L)) - 1:])
    assert len(at) == len(lengths) == len(set(at))
    rows, cols = [], []
    for r, d in zip(at, lengths):
        rows.append(np.full(d, r))
        cols.append(rng.choice(columns, size=d, replace=False))
    planted = np.array(sorted(at))
    background_rows = np.setdiff1d(np.arange(n), np.concatenate([planted, np.arange(*EMPTY_RUN)]))
    key = np.unique(rng.choice(background_rows, size=6 * n) * n + rng.choice(columns, size=6 * n))
    # every planted row id is pointed at by one background row
    feeders = rng.choice(background_rows, size=len(planted)) * n + planted
    key = np.unique(np.concatenate([key, feeders]))
    rows.append(key // n)
    cols.append(key % n)
    coo, vals, shape = _finish(np.concatenate(rows), np.concatenate(cols), n, rng)
    # ---- what the builder promises
    deg = np.bincount(coo[:, 0], minlength=n)
    in_deg = np.bincount(coo[:, 1], minlength=n)
    for r, d in zip(at, lengths):
        assert deg[r] == d, (r, d, deg[r])
    n_long = sum(d > L for d in lengths)
    assert (deg > L).sum() == n_long == 4 + n_hub
    assert in_deg.max() <= L                                                         # the transpose is hub-free
    assert (deg[EMPTY_RUN[0]:EMPTY_RUN[1]] == 0).all() and deg[n // 2] == 0 and deg[0] > L and deg[n - 1] > L
    assert (in_deg[no_in] == 0).all() and (in_deg[planted] > 0).all()
    assert abs(len(coo) - sum(lengths) - 6 * n) < n // 4
    rows_of = {}
    for r, d in zip(at, lengths):
        rows_of.setdefault(d, []).append(r)
    ragged = np.arange(n - n % 16, n)
    assert n % 16 == 0 or (deg[ragged] > L).any()
    info = dict(rows_of=rows_of, hub=np.flatnonzero(deg > L), planted=planted, empty=np.flatnonzero(deg == 0), no_in=no_in, ragged=ragged,
                deg=deg, in_deg=in_deg, L=L)
    return coo, vals, shape, info


def regime_graph(name, seed=0):
    n, L, n_hub = REGIMES[name]
    return planted_graph(n, L, n_hub, seed)


def boundary_graph(n, seed=5):
    """The SAME entries for n = 2^15 - 1 and n = 2^15 (every id is below 2^15 - 1): about 6 n background entries in rows of a few entries
    and row BOUNDARY_ROW with exactly 300: short under the threshold of 512 on the one side, a hub row of three chunks under the
    threshold of 128 on the other.  Returns (coo, vals, shape)."""
    assert n in BOUNDARY_NS
    m = BOUNDARY_NS[0]
    rng = np.random.default_rng(seed)
    others = np.setdiff1d(np.arange(m), [BOUNDARY_ROW])
    key = np.unique(rng.choice(others, size=6 * m) * n + rng.integers(0, m, size=6 * m))
    rows = np.concatenate([key // n, np.full(BOUNDARY_LEN, BOUNDARY_ROW)])
    cols = np.concatenate([key % n, rng.choice(m, size=BOUNDARY_LEN, replace=False)])
    order = np.lexsort((cols, rows))                                                 # the shuffle below must not depend on n through the keys
    coo, vals, shape = _finish(rows[order], cols[order], n, rng)
    deg = np.bincount(coo[:, 0], minlength=n)
    assert deg[BOUNDARY_ROW] == BOUNDARY_LEN and np.delete(deg, BOUNDARY_ROW).max() < SMALL_LONG_ROW
    assert np.bincount(coo[:, 1], minlength=n).max() < SMALL_LONG_ROW
    return coo, vals, shape


# ---- operands: the recipe of the existing GCNII test files ----------------------------------------------------------------------------
def operands(n, C, seed):
    """H, H0, G, S_in seeded normal [n, C]; M = 0.6 I + 0.4 N / sqrt(C); all float32, read-only."""
    rng = np.random.default_rng(seed)
    H, H0, G, S_in = (rng.standard_normal((n, C)).astype(np.float32) for _ in range(4))
    M = (0.6 * np.eye(C) + 0.4 * rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
    out = dict(H=H, H0=H0, G=G, S_in=S_in, M=M, Mt=np.ascontiguousarray(M.T))
    for x in out.values():
        x.setflags(write=False)
    return out


# ---- float64 references and their bounds ----------------------------------------------------------------------------------------------
def mix_constants(a):
    """(beta, alpha) as the host path forms them: float32(1 - a), float32(a); returned as Python floats."""
    return float(np.float32(1.0 - float(a))), float(np.float32(a))


def chunk_counts(deg, L):
    return np.where(deg > L, -(-deg // L), 0)


def f64(x):
    return np.asarray(x, dtype=np.float64)


def forward_ref(A, H, H0, M, a, relu, L=None):
    """A: scipy CSR of the float32 weights as float64.  Returns dict(T, out, T_bound, out_bound): T = beta A H + alpha H0,
    out = act(T M); T_bound = (deg + chunks + 4) u |T|, out_bound = (deg + chunks + C + 6) u (|T| |M|) with |T| = beta |A| |H| + alpha |H0|
    (relu changes nothing: |relu x - relu y| <= |x - y|)."""
    n, C = H.shape
    L = plan_threshold(n) if L is None else L
    beta, alpha = mix_constants(a)
    A = sp.csr_matrix(A, dtype=np.float64)
    deg = np.diff(A.indptr)
    terms = (deg + chunk_counts(deg, L))[:, None]
    T = beta * (A @ f64(H)) + alpha * f64(H0)
    absT = beta * (abs(A) @ np.abs(f64(H))) + alpha * np.abs(f64(H0))
    out = T @ f64(M)
    if relu:
        out = np.maximum(out, 0.0)
    return dict(T=T, out=out, T_bound=(terms + 4) * U32 * absT, out_bound=(terms + C + 6) * U32 * (absT @ np.abs(f64(M))))


def backward_ref(A, G, Mt, a, S_in=None, s_alpha=1.0, L=None):
    """dH = (beta A^T G) Mt, S = s_alpha S_in + (alpha G) Mt and their bounds: dH_bound = (deg^T + chunks^T + C + 6) u ((beta |A^T| |G|) |Mt|),
    S_bound = (C + 6) u (alpha |G| |Mt| + |s_alpha| |S_in|)."""
    n, C = G.shape
    L = plan_threshold(n) if L is None else L
    beta, alpha = mix_constants(a)
    At = sp.csr_matrix(sp.csr_matrix(A, dtype=np.float64).T)
    deg = np.diff(At.indptr)
    terms = (deg + chunk_counts(deg, L))[:, None]
    absMt = np.abs(f64(Mt))
    dH = (beta * (At @ f64(G))) @ f64(Mt)
    dH_bound = (terms + C + 6) * U32 * ((beta * (abs(At) @ np.abs(f64(G)))) @ absMt)
    S = (alpha * f64(G)) @ f64(Mt)
    S_size = (alpha * np.abs(f64(G))) @ absMt
    if S_in is not None:
        S = S + float(np.float32(s_alpha)) * f64(S_in)
        S_size = S_size + abs(float(np.float32(s_alpha))) * np.abs(f64(S_in))
    return dict(dH=dH, S=S, dH_bound=dH_bound, S_bound=(C + 6) * U32 * S_size)


def ratio_rows(got, want, bound):
    """Per row: max over the columns of |got - want| / bound; 0 where both are 0, infinite where the bound is 0 and the error is not, or
    where ``got`` is not finite."""
    got = f64(got)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(got), r, np.inf)
    return r.max(axis=1) if r.shape[1] else np.zeros(len(r))


def ratio(got, want, bound, rows=None):
    """The criterion: max |got - want| / bound (over ``rows`` when given)."""
    r = ratio_rows(got, want, bound)
    r = r if rows is None else r[np.asarray(rows, dtype=np.int64)]
    return float(r.max()) if len(r) else 0.0


# ---- float32 emulations (CPU): what the bound must admit ----------------------------------------------------------------------------------
def seq_segment_sums(indptr, indices, w, X):
    """out[s] = sum over the entries e of segment s, in order, of w[e] * X[indices[e]] -- strictly sequential float32 (one rounded
    product and one rounded add per entry), all segments advanced together."""
    indptr = np.asarray(indptr, dtype=np.int64)
    deg = np.diff(indptr)
    acc = np.zeros((len(deg), X.shape[1]), dtype=np.float32)
    order = np.argsort(-deg, kind="stable")
    sorted_deg = deg[order]
    for k in range(int(deg.max()) if len(deg) else 0):
        rows = order[:np.searchsorted(-sorted_deg, -k, side="left")]                 # the segments with more than k entries
        e = indptr[rows] + k
        acc[rows] = acc[rows] + w[e].astype(np.float32)[:, None] * X[indices[e]]
    return acc


def spmm_f32(A32, X, order, L):
    """A . X in float32 over the CSR A32 (float32 values).  ``order``: "library" (scipy's own product), "sequential" (entry by entry),
    "chunked" (rows longer than L: chunks of L entries summed separately, then added in chunk order -- the long-row path's order)."""
    X = np.asarray(X, dtype=np.float32)
    if order == "library":
        return np.asarray(A32 @ X, dtype=np.float32)
    indptr, indices, w = A32.indptr.astype(np.int64), A32.indices, A32.data
    if order == "sequential":
        return seq_segment_sums(indptr, indices, w, X)
    assert order == "chunked"
    deg = np.diff(indptr)
    pieces = np.where(deg > L, -(-deg // L), 1)                                      # segments per row (short and empty rows: one)
    seg_row = np.repeat(np.arange(len(deg)), pieces)
    first = np.concatenate([[0], np.cumsum(pieces)])
    within = np.arange(len(seg_row)) - first[seg_row]
    seg_beg = indptr[seg_row] + within * L
    seg_end = np.minimum(seg_beg + L, indptr[seg_row + 1])
    assert (seg_end[:-1] <= seg_beg[1:]).all()
    # segments are contiguous and ordered: their boundaries form an indptr of their own
    partial = seq_segment_sums(np.concatenate([seg_beg, [indptr[-1]]]), indices, w, X)
    return seq_segment_sums(first, np.arange(len(seg_row)), np.ones(len(seg_row), dtype=np.float32), partial)


def matmul_f32(T, M, order):
    T, M = np.asarray(T, dtype=np.float32), np.asarray(M, dtype=np.float32)
    if order == "library":
        return T @ M
    out = np.zeros((T.shape[0], M.shape[1]), dtype=np.float32)
    for k in range(T.shape[1]):
        out = out + T[:, k:k + 1] * M[k]
    return out


def forward_f32(A32, H, H0, M, a, relu, order, L):
    """(T, out) of the forward in float32 under ``order``."""
    beta, alpha = np.float32(1.0 - float(a)), np.float32(a)
    T = spmm_f32(A32, H, order, L) * beta + np.asarray(H0, dtype=np.float32) * alpha
    out = matmul_f32(T, M, order)
    return T, np.maximum(out, np.float32(0)) if relu else out


def backward_f32(A32, G, Mt, a, S_in, s_alpha, order, L):
    """(dH, S) of the backward in float32 under ``order``."""
    beta, alpha = np.float32(1.0 - float(a)), np.float32(a)
    At32 = sp.csr_matrix(A32.T)
    At32.sort_indices()
    dH = matmul_f32(spmm_f32(At32, G, order, L) * beta, Mt, order)
    S = matmul_f32(np.asarray(G, dtype=np.float32) * alpha, Mt, order)
    if S_in is not None:
        S = np.float32(s_alpha) * np.asarray(S_in, dtype=np.float32) + S
    return dH, S


def csr_of(coo, vals, shape, dtype=np.float64):
    """The coalesced CSR of a COO without duplicates, columns ascending within a row (the handle's order)."""
    A = sp.csr_matrix((vals.astype(dtype), (coo[:, 0], coo[:, 1])), shape=shape)
    A.sort_indices()
    return A


def degree_order(deg, L, window=0):
    """row_order of build_long_plan: a stable sort by descending min(deg, L) -- inside windows of ``window`` consecutive ids when
    given, the rows without entries trailing the whole order."""
    deg = np.asarray(deg, dtype=np.int64)
    key = L - np.minimum(deg, L)
    if window > 0:
        n_windows = -(-len(deg) // window)
        key = np.where(deg == 0, n_windows, np.arange(len(deg)) // window) * (L + 1) + key
    return np.argsort(key, kind="stable")
