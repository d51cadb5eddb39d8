"""numpy reference of gnx_rank_candidates (include/gnx.h; MeanLinkPrediction.evaluate, reference graph_predictor.py:154-203), written from
the specification and sharing no code with the library: the list of every source, float64 scores with their first-order bound, the
counts, the stable-argsort top-k, and the metrics of the task.  Linkage is a Python set of stored pairs, not a CSR search."""
import numpy as np


def scores64(F, r, sources, nodes):
    """(score, bound), float64 [len(sources), len(nodes)]: score = sum_c F[s, c] r[c] F[v, c]; bound = (C + 4) 2^-24 sum_c |F[s, c] r[c]
    F[v, c]|, the any-order first-order bound of C products, one scaling and C - 1 sums in f32.  NaN where an id is not a row of F."""
    F64 = np.asarray(F, dtype=np.float64)
    n, C = F64.shape
    w = np.ones(C) if r is None else np.asarray(r, dtype=np.float64).reshape(-1)
    sources, nodes = np.asarray(sources, dtype=np.int64), np.asarray(nodes, dtype=np.int64)
    s_ok, v_ok = (sources >= 0) & (sources < n), (nodes >= 0) & (nodes < n)
    A = F64[np.where(s_ok, sources, 0)] * w
    B = F64[np.where(v_ok, nodes, 0)]
    score, bound = A @ B.T, (C + 4) * 2.0 ** -24 * (np.abs(A) @ np.abs(B).T)
    bad = ~(s_ok[:, None] & v_ok[None, :])
    score[bad], bound[bad] = np.nan, np.nan
    return score, bound


def pos_scores64(F, r, sources, pos_ptr, pos_ids):
    """(score, bound) [P] of every held-out pair in CSR order (NaN where an id is out of range or the pointers are)."""
    P = len(pos_ids)
    score, bound = np.full(P, np.nan), np.full(P, np.nan)
    for i, s in enumerate(sources):
        lo, hi = int(pos_ptr[i]), int(pos_ptr[i + 1])
        if 0 <= lo <= hi <= P and hi > lo:
            x, b = scores64(F, r, [s], pos_ids[lo:hi])
            score[lo:hi], bound[lo:hi] = x[0], b[0]
    return score, bound


def linked_set(coo):
    return set(map(tuple, np.asarray(coo, dtype=np.int64).reshape(-1, 2).tolist()))


def rank(linked, n_rows_F, sources, pos_ptr, pos_ids, candidates, k, cand_scores, pos_scores):
    """The outputs of the call for given scores (``cand_scores`` [S, K] of every (source, candidate) pair, ``pos_scores`` [P] of the
    held-out pairs): a dict of arrays n_pos, n_neg, less, equal [S], top_ids, top_scores, top_is_pos [S, k], and ``lists``: per source
    None (out of range) or (ids, labels, scores) of its list, positives first."""
    S, P = len(sources), len(pos_ids)
    out = dict(n_pos=np.zeros(S, dtype=np.int64), n_neg=np.zeros(S, dtype=np.int64), less=np.zeros(S, dtype=np.int64),
               equal=np.zeros(S, dtype=np.int64), top_ids=np.full((S, k), -1, dtype=np.int64), top_scores=np.full((S, k), -np.inf),
               top_is_pos=np.zeros((S, k), dtype=np.uint8), lists=[None] * S)
    for i, s in enumerate(int(x) for x in sources):
        lo, hi = int(pos_ptr[i]), int(pos_ptr[i + 1])
        pointers_ok = 0 <= lo <= hi <= P
        held = [int(v) for v in pos_ids[lo:hi]] if pointers_ok else []
        out["n_pos"][i] = len(held)
        if not pointers_ok or not 0 <= s < n_rows_F or any(not 0 <= v < n_rows_F for v in held):
            out["n_neg"][i] = -1
            continue
        strangers = [(j, int(v)) for j, v in enumerate(candidates)
                     if 0 <= v < n_rows_F and v != s and (s, int(v)) not in linked and (int(v), s) not in linked]
        ids = np.array(held + [v for _, v in strangers], dtype=np.int64)
        labels = np.array([1.0] * len(held) + [0.0] * len(strangers))
        x = np.concatenate([np.asarray(pos_scores[lo:hi], dtype=np.float64), np.asarray(cand_scores[i], dtype=np.float64)[[j for j, _ in strangers]]])
        xp, xn = x[:len(held)], x[len(held):]
        out["n_neg"][i] = len(strangers)
        out["less"][i] = sum(int((xn < p).sum()) for p in xp)
        out["equal"][i] = sum(int((xn == p).sum()) for p in xp)
        best = np.argsort(x, kind="stable")[-k:][::-1]                   # higher first; among equals the LATER entry first
        out["top_ids"][i, :len(best)] = ids[best]
        out["top_scores"][i, :len(best)] = x[best]
        out["top_is_pos"][i, :len(best)] = labels[best] == 1
        out["lists"][i] = (ids, labels, x)
    return out


def metrics(result, k, n_candidates):
    """({auc, avprec, prec, rec, f1: [S]}, coverage) of rank()'s result: measures.py:17-45 over every source's (labels, scores), the
    top-k by the stable order above."""
    names = ("auc", "avprec", "prec", "rec", "f1")
    per = {name: [] for name in names}
    recommended = set()
    for entry in result["lists"]:
        ids, labels, x = entry
        n_pos, n_neg = int(labels.sum()), int((labels == 0).sum())
        if n_pos == 0 or n_neg == 0:
            per["auc"].append(float("nan"))
        else:
            wins = sum(float((x[labels == 0] < p).sum()) + 0.5 * float((x[labels == 0] == p).sum()) for p in x[labels == 1])
            per["auc"].append(wins / (n_pos * n_neg))
        best = np.argsort(x, kind="stable")[-k:][::-1]
        hits = float(labels[best].sum())
        gain = 0.0
        for position, e in enumerate(best):
            gain += labels[e] / (position + 1)
        precision, recall = hits / len(best), hits / n_pos
        per["avprec"].append(0.0 if gain == 0 else gain / hits)
        per["prec"].append(precision)
        per["rec"].append(recall)
        per["f1"].append(0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall))
        recommended.update(int(v) for v in ids[best])
    return {name: np.array(v, dtype=np.float64) for name, v in per.items()}, len(recommended) / n_candidates


# ---- the data sets of the tests ----------------------------------------------------------------------------------------------------------
GRAPH_ROWS, GRAPH_COLS, F_ROWS = 280, 300, 300       # the handle has fewer rows than the embeddings: ids 280 .. 299 are rows of F only
FULL_NODE, MANY_POS_SOURCE = 7, 11                   # node 7 is linked to every other id; source 11 holds out more than one pass


def problem(seed, S, K, pos_pass):
    """The graph (directed pairs, stored one way only, degrees around 10), S sources, their held-out CSR and K ascending candidates of
    data sets 1 and 3.  Among the first sources: one that is a candidate itself, one with ``pos_pass + 8`` held-out neighbours, one
    linked to every candidate, one out of range, one with an out-of-range held-out id, one beyond the handle's rows, one without
    held-out neighbours.  The candidates of K = 300 begin and end with an id out of range."""
    rng = np.random.default_rng(seed)
    coo = np.stack([rng.integers(0, GRAPH_ROWS, 2800), rng.integers(0, GRAPH_COLS, 2800)], axis=1)
    coo = np.concatenate([coo, [(FULL_NODE, v) for v in range(GRAPH_COLS) if v != FULL_NODE], [(20, 20), (5, 290)]])      # a loop; an entry whose column is no row
    universe = np.concatenate([[-3], np.sort(rng.choice(F_ROWS, 298, replace=False)), [400]])
    sources = np.concatenate([[universe[120], MANY_POS_SOURCE, FULL_NODE, F_ROWS, 33, 285, 64], rng.choice(F_ROWS, 30, replace=False)])[:S]
    lists = []
    for i, s in enumerate(sources):
        n = pos_pass + 8 if s == MANY_POS_SOURCE else 0 if i == 6 else int(rng.integers(1, 9))
        held = rng.choice(universe[1:-1], n, replace=False)
        if i == 4:
            held[-1] = F_ROWS + 5
        lists.append(held)
    pos_ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    pos_ids = np.concatenate(lists).astype(np.int64)
    candidates = universe if K == 300 else universe[100:100 + K]
    assert len(candidates) == K and (np.diff(candidates) > 0).all()
    return coo.astype(np.int64), sources.astype(np.int64), pos_ptr, pos_ids, candidates.astype(np.int64)


def exact_embeddings(seed, C):
    """Small integers times powers of two: every product and every sum of a score is exact in f32 in any order, and scores tie often."""
    rng = np.random.default_rng(seed)
    F = (rng.integers(-2, 3, size=(F_ROWS, C)) * 0.5).astype(np.float32)
    r = np.array([0.5, 1.0, 2.0], dtype=np.float32)[rng.integers(0, 3, size=C)]
    return F, r


def bipartite(seed, n_users=12, n_items=200, C=4):
    """Data set 2: users 0 .. n_users - 1 are the sources, items the candidates.  C columns are multiples of 2^-2 in [-1/2, 1/2], so
    their part of a score is a multiple of 2^-4.  One extra column is 1 for users and index 2^-13 for items, indices 80 .. 80 + n_items
    < 512: below 2^-4 and at least 80 2^-13.  The default candidates of the task are every endpoint of a held-out edge, users included,
    and that column alone would tie two users; so a second extra column is (u + 1) 2^-7 for users and 0 for items: user against user
    adds (u + 1)(u' + 1) 2^-14 <= 144 2^-14 < 80 2^-13.  Every score of a user is then exact in f32 in any order, distinct from every
    other by at least 2^-14, and below 2.2, where the f32 sigmoid of the host path still separates 2^-14 by thousands of ulps.
    The graph holds the held-out edges too, as the reference's demos pass the whole graph: a held-out item is then linked, and not its
    own stranger twin with the same score.  Returns (networkx graph, held-out edges, users, items, F)."""
    import networkx as nx
    assert 80 + n_items < 512 and n_users ** 2 < 2 * 80
    rng = np.random.default_rng(seed)
    n = n_users + n_items
    F = np.zeros((n, C + 2), dtype=np.float32)
    F[:, :C] = rng.integers(-2, 3, size=(n, C)) * 0.25
    F[:n_users, C] = 1.0
    F[n_users:, C] = (80 + np.arange(n_items)) * 2.0 ** -13
    F[:n_users, C + 1] = (1 + np.arange(n_users)) * 2.0 ** -7
    G = nx.Graph()
    G.add_nodes_from(range(n))
    held = []
    for u in range(n_users):
        items = n_users + rng.choice(n_items, 12, replace=False)
        G.add_edges_from((u, int(v)) for v in items[:8])
        held += [(u, int(v)) for v in items[8:8 + 1 + u % 4]]
    G.add_edges_from(map(tuple, held))
    return G, np.array(held, dtype=np.int64), list(range(n_users)), list(range(n_users, n)), F
