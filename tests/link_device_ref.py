"""numpy reference of the device link task (csrc/gnx_link.hip), restating include/gnx.h line by line over oracle.gnntf_oracle.hash_u24:
the draws of gnx_sample_negatives, the plan of gnx_edge_plan and the float32 summation order of gnx_edge_scores_backward_sorted.
Nothing here imports the package under test."""
import numpy as np

from oracle import gnntf_oracle as orc

U = 2.0 ** -24                       # unit roundoff of float32
CHUNK = 256                          # positions of one node that are added up sequentially


# ---- the pattern -----------------------------------------------------------------------------------------------------------------------
def csr_pattern(coo, n_rows):
    """(rowptr int64 [n_rows + 1], colidx int64 [nnz]) of the coalesced pattern of int64 [nnz, 2] (row, col) pairs: rows ascending,
    columns ascending inside a row, duplicates once."""
    coo = np.asarray(coo, dtype=np.int64).reshape(-1, 2)
    pairs = np.unique(coo, axis=0) if len(coo) else coo
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(pairs[:, 0], minlength=n_rows), out=rowptr[1:])
    return rowptr, pairs[:, 1].copy()


def stored(rowptr, colidx, row, col):
    """Whether (row, col) is a stored entry: a binary search among the ascending columns of the row."""
    b, e = int(rowptr[row]), int(rowptr[row + 1])
    at = b + int(np.searchsorted(colidx[b:e], col, side="left"))
    return at < e and int(colidx[at]) == col


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------
def draw(seed, stream, e, t, K):
    """Candidate index of try ``t`` of slot ``e``: two 24-bit hashes make 48 bits x, j = floor(x K / 2^48)."""
    hi = int(orc.hash_u24(seed, stream, e, 2 * t, 0))
    lo = int(orc.hash_u24(seed, stream, e, 2 * t + 1, 0))
    return ((hi << 24 | lo) * K) >> 48


def sample_negatives(rowptr, colidx, n_rows, positives, samples, candidates, max_tries, seed, stream, linked=None):
    """(edges int64 [m (1 + samples), 2], fallbacks, tries [m samples]): group i is (u_i, v_i), then ``samples`` rows (u_i, w).  Slot
    e = i samples + s takes the first w of its tries that is neither u, v nor linked to u in either direction; after ``max_tries``
    rejected tries it keeps the last w and counts as a fallback.  A positive row with an endpoint outside [0, n_rows) is copied and
    its negatives are -1 (tries 0).  ``linked(u, w)``: another lookup than the binary search (the brute-force check of the host test)."""
    positives = np.asarray(positives, dtype=np.int64).reshape(-1, 2)
    m, K = len(positives), n_rows if candidates is None else len(candidates)
    if linked is None:
        linked = lambda u, w: stored(rowptr, colidx, u, w) or (0 <= w < n_rows and stored(rowptr, colidx, w, u))
    edges = np.empty((m * (1 + samples), 2), dtype=np.int64)
    tries = np.zeros(m * samples, dtype=np.int64)
    fallbacks = 0
    for i, (u, v) in enumerate(positives.tolist()):
        base = i * (1 + samples)
        edges[base] = (u, v)
        for s in range(samples):
            e = i * samples + s
            edges[base + 1 + s, 0] = u
            if not (0 <= u < n_rows and 0 <= v < n_rows):
                edges[base + 1 + s, 1] = -1
                continue
            accepted = False
            for t in range(max_tries):
                j = draw(seed, stream, e, t, K)
                w = j if candidates is None else int(candidates[j])
                tries[e] = t + 1
                if w != u and w != v and not linked(u, w):
                    accepted = True
                    break
            fallbacks += not accepted
            edges[base + 1 + s, 1] = w
    return edges, fallbacks, tries


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
def in_range(edges, n):
    return ((edges >= 0) & (edges < n)).all(axis=1)


def edge_plan(edges, n_rows):
    """(keys [2 m], pos [2 m], chunks): the positions q = 2 i + side stably sorted by the node edges[q] they name, both positions of an
    edge with an endpoint out of range keyed n_rows; chunks = the sorted indices whose distance to the first index of their key is a
    multiple of CHUNK, the trailing bucket left out."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    keys = np.where(np.repeat(in_range(edges, n_rows), 2), edges.reshape(-1), n_rows)
    pos = np.argsort(keys, kind="stable")
    keys = keys[pos]
    first = np.searchsorted(keys, keys, side="left")
    p = np.arange(len(keys))
    return keys, pos, p[((p - first) % CHUNK == 0) & (keys < n_rows)]


# ---- the backward ----------------------------------------------------------------------------------------------------------------------
def sorted_sums_f32(F, edges, r, g):
    """(S float32 [n, C], named bool [n]): what gnx_edge_scores_backward_sorted adds into every named row of dF, in float32 with the
    stated order: t_q = fl(fl(g_i r) F[other_q]) (g_i without r); the positions of a node ascending, in chunks of CHUNK from the node's
    first; a chunk's sum sequential from its first term; a node of several chunks adds its chunk sums in chunk order."""
    F, g = np.asarray(F, dtype=np.float32), np.asarray(g, dtype=np.float32)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(F.shape, dtype=np.float32)
    named = np.zeros(F.shape[0], dtype=bool)
    n = F.shape[0]
    keys, pos, _ = edge_plan(edges, n)
    flat = edges.reshape(-1)
    stop = int(np.searchsorted(keys, n, side="left"))                    # the trailing bucket is skipped
    w = g[pos[:stop] >> 1][:, None] * np.asarray(r, dtype=np.float32)[None, :] if r is not None else g[pos[:stop] >> 1][:, None]
    terms = (w.astype(np.float32) * F[flat[pos[:stop] ^ 1]]).astype(np.float32)
    b = 0
    while b < stop:
        e = int(np.searchsorted(keys, keys[b], side="right"))
        total = None
        for c in range(b, e, CHUNK):
            s = terms[c].copy()
            for p in range(c + 1, min(c + CHUNK, e)):
                s = (s + terms[p]).astype(np.float32)
            total = s if total is None else (total + s).astype(np.float32)
        out[keys[b]], named[keys[b]] = total, True
        b = e
    return out, named


def sorted_backward_f32(sums, dF):
    """dF after the call: every named row is fl(dF + S) once, the others keep their bits."""
    S, named = sums
    out = np.array(dF, dtype=np.float32, copy=True)
    out[named] = (out[named] + S[named]).astype(np.float32)
    return out


def edge_grad_f64(F, edges, r, g, prefill=None):
    """(want, bound) of d_grad_F in float64: dF[u] += g r F[v] and dF[v] += g r F[u] over the edges in range; bound = 1e-4 |want| +
    (k + 4) u sum |term| over the k terms of an element, a pre-filled value being one more term: the bound of a float32 sum of k terms
    in ANY order plus the terms' own roundings (the criterion of tests/test_gpu_heads.py for the atomic form)."""
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    n, C = F.shape
    ok = in_range(edges, n)
    u, v = edges[ok, 0], edges[ok, 1]
    w = f64(g)[ok, None] * (1.0 if r is None else f64(r))
    want, mag = np.zeros((n, C)), np.zeros((n, C))
    for rows, terms in ((u, w * f64(F)[v]), (v, w * f64(F)[u])):
        np.add.at(want, rows, terms)
        np.add.at(mag, rows, np.abs(terms))
    k = f64(np.bincount(u, minlength=n) + np.bincount(v, minlength=n))[:, None]
    if prefill is not None:
        want, mag, k = want + f64(prefill), mag + np.abs(f64(prefill)), k + 1
    return want, 1e-4 * np.abs(want) + (k + 4) * U * mag
