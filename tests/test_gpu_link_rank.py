"""gnx_rank_candidates on the device against tests/link_rank_ref.py: exact scores with many ties (the tie rule and every count, bit for
bit), the tie-free bipartite task end to end against the host MeanLinkPrediction.evaluate, random embeddings against float64 and against
the reference's ranking of the kernel's own scores, independence of the candidate parts, and recommend.

The C entry is called directly so that every output lies in a buffer of sentinels with 8 rows beyond it, which must stay untouched; the
embeddings are dense, a 4-byte-offset column slice of odd pitch, or a 16-byte-aligned slice, the slices embedded in NaN."""
import functools

import numpy as np
import pytest
import torch

import link_rank_ref as ref
from test_link_rank_cpu import HOST_CASES, NAMES, host_per_source, same

pytestmark = pytest.mark.gpu

SEED = 11
SENTINEL_INT, SENTINEL_FLOAT, SENTINEL_BYTE = -77, 123.5, 9
SIZES_S, SIZES_K, WIDTHS, PITCHES = (1, 17, 37), (1, 15, 16, 17, 300), (1, 5, 16, 64, 100), ("dense", "odd", "quad")
K_MODES = (1, 5, 32, "short")        # "short": one more than the shortest list of the case


def pos_pass():
    from gnntf import sparse
    return sparse.RANK_POS_PASS


@functools.lru_cache(maxsize=None)
def problem(S, K):
    coo, sources, pos_ptr, pos_ids, candidates = ref.problem(SEED, S, K, pos_pass())
    return coo, sources, pos_ptr, pos_ids, candidates, ref.linked_set(coo)


@pytest.fixture(scope="module")
def graph():
    import gnntf
    coo = problem(37, 300)[0]
    return gnntf.DeviceGraph(gnntf.SparseCOO(coo, np.ones(len(coo), dtype=np.float32), (ref.GRAPH_ROWS, ref.GRAPH_COLS)), device="cuda")


def place(F, pitch):
    """F on the device as a dense matrix or as a column slice of a NaN matrix: nothing outside the slice may reach a score."""
    n, C = F.shape
    if pitch == "dense":
        return torch.from_numpy(F).cuda()
    offset, ld = (1, C + 2 + (C + 1) % 2) if pitch == "odd" else (4, (C + 3) // 4 * 4 + 8)       # odd pitch, 4-byte offset / 16-byte aligned
    big = torch.full((n, ld), float("nan"), dtype=torch.float32, device="cuda")
    big[:, offset:offset + C] = torch.from_numpy(F).cuda()
    view = big[:, offset:offset + C]
    assert view.stride(0) == ld and (pitch == "odd") == (ld % 2 == 1) and (view.data_ptr() % 16 == 0) == (pitch == "quad")
    return view


def launch(graph, F, r, sources, pos_ptr, pos_ids, candidates, k, splits, scores=True):
    """One call of the C entry; returns the outputs of the S sources as numpy arrays after checking the 8 rows beyond them."""
    from gnntf import _native as nat
    S, K, P, extra = len(sources), len(candidates), len(pos_ids), 8
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()
    d_sources, d_ptr, d_ids, d_cand = up(sources), up(pos_ptr), up(pos_ids), up(candidates)
    d_r = None if r is None else torch.from_numpy(r).cuda()
    counts = torch.full((4, S + extra), SENTINEL_INT, dtype=torch.int64, device="cuda")
    top_ids = torch.full((S + extra, k), SENTINEL_INT, dtype=torch.int64, device="cuda")
    top_scores = torch.full((S + extra, k), SENTINEL_FLOAT, dtype=torch.float32, device="cuda")
    top_is_pos = torch.full((S + extra, k), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    raw = torch.full((S + extra, K), SENTINEL_FLOAT, dtype=torch.float32, device="cuda") if scores else None
    nbytes = int(nat.lib().gnx_rank_candidates_bytes(S, P, K, k, splits))
    assert nbytes >= 0
    workspace = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    with nat.on_device(F.device):
        nat.check(nat.lib().gnx_rank_candidates(
            graph.handle, nat.ptr(F), F.stride(0), F.shape[0], F.shape[1], nat.ptr(d_r), nat.ptr(d_sources), S, nat.ptr(d_ptr), nat.ptr(d_ids), P,
            nat.ptr(d_cand), K, k, splits, nat.ptr(counts[0]), nat.ptr(counts[1]), nat.ptr(counts[2]), nat.ptr(counts[3]), nat.ptr(top_ids),
            nat.ptr(top_scores), nat.ptr(top_is_pos), nat.ptr(raw), nat.ptr(workspace), nbytes, nat.current_stream()))
    torch.cuda.synchronize()
    assert (counts[:, S:] == SENTINEL_INT).all() and (top_ids[S:] == SENTINEL_INT).all() and (top_scores[S:] == SENTINEL_FLOAT).all()
    assert (top_is_pos[S:] == SENTINEL_BYTE).all() and (raw is None or (raw[S:] == SENTINEL_FLOAT).all())
    names = ("n_pos", "n_neg", "less", "equal")
    out = {name: counts[i, :S].cpu().numpy() for i, name in enumerate(names)}
    out.update(top_ids=top_ids[:S].cpu().numpy(), top_scores=top_scores[:S].cpu().numpy(), top_is_pos=top_is_pos[:S].cpu().numpy(),
               scores=None if raw is None else raw[:S].cpu().numpy())
    return out


OUTPUTS = ("n_pos", "n_neg", "less", "equal", "top_ids", "top_scores", "top_is_pos")


def assert_outputs(got, want):
    for name in OUTPUTS:
        assert np.array_equal(got[name], want[name].astype(got[name].dtype)), name


def short_k(linked, sources, pos_ptr, pos_ids, candidates):
    lengths = [int(pos_ptr[i + 1] - pos_ptr[i]) + sum(1 for v in candidates if 0 <= v < ref.F_ROWS and v != s and (s, v) not in linked
                                                       and (v, s) not in linked)
               for i, s in enumerate(int(x) for x in sources) if 0 <= s < ref.F_ROWS and (pos_ids[pos_ptr[i]:pos_ptr[i + 1]] < ref.F_ROWS).all()]
    return min(min(lengths) + 1, 32)


def cases():
    """Every S with every K; every width with every pitch; every k with every number of parts; the remaining operands of a case cycle
    through their values.  Widths 200 and 260 reach the widest register-resident A operand and the path that streams it."""
    out = []
    for i, (S, K) in enumerate((S, K) for S in SIZES_S for K in SIZES_K):
        out.append((S, K, WIDTHS[i % 5], K_MODES[i % 4], (1, 3)[i % 2], PITCHES[i % 3]))
    out += [(37, 300, C, 5, 3, pitch) for C in WIDTHS for pitch in PITCHES]
    out += [(37, 300, 16, k, splits, "dense") for k in K_MODES for splits in (1, 3)]
    out += [(17, 300, 200, 5, 3, "quad"), (17, 300, 260, 5, 3, "odd")]
    return out


def own_positive_scores(graph, F, r, sources, pos_ptr, pos_ids):
    """The kernel's own scores of the held-out pairs: the score matrix of a call whose candidates are the held-out ids."""
    valid = np.unique(pos_ids[(pos_ids >= 0) & (pos_ids < ref.F_ROWS)])
    if len(valid) == 0:
        return np.zeros(len(pos_ids))
    matrix = launch(graph, F, r, sources, np.zeros(len(sources) + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), valid, 1, 0)["scores"]
    out = np.full(len(pos_ids), np.nan)
    for i in range(len(sources)):
        for p in range(int(pos_ptr[i]), int(pos_ptr[i + 1])):
            at = np.searchsorted(valid, pos_ids[p])
            if at < len(valid) and valid[at] == pos_ids[p]:
                out[p] = matrix[i, at]
    return out


# ---- 1: exact scores with many ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,K,C,k,splits,pitch", cases())
def test_exact_scores_with_ties(graph, S, K, C, k, splits, pitch):
    coo, sources, pos_ptr, pos_ids, candidates, linked = problem(S, K)
    k = short_k(linked, sources, pos_ptr, pos_ids, candidates) if k == "short" else k
    F, r = ref.exact_embeddings(SEED + C, C)
    for weights in (r, None):
        got = launch(graph, place(F, pitch), weights, sources, pos_ptr, pos_ids, candidates, k, splits)
        cand_scores, _ = ref.scores64(F, weights, sources, candidates)
        pos_scores, _ = ref.pos_scores64(F, weights, sources, pos_ptr, pos_ids)
        valid = ~np.isnan(cand_scores)
        assert (got["scores"][valid] == cand_scores[valid]).all() and (got["scores"][~valid] == SENTINEL_FLOAT).all()
        want = ref.rank(linked, ref.F_ROWS, sources, pos_ptr, pos_ids, candidates, k, cand_scores, pos_scores)
        assert_outputs(got, want)


def test_the_exact_case_holds_what_it_claims(graph):
    """The edge cases of data set 1 are present in the full case, and the kernel meets each."""
    coo, sources, pos_ptr, pos_ids, candidates, linked = problem(37, 300)
    F, r = ref.exact_embeddings(SEED, 16)
    got = launch(graph, place(F, "dense"), r, sources, pos_ptr, pos_ids, candidates, 5, 3)
    assert sources[0] in candidates                                      # a source that is a candidate itself
    assert sources[1] == ref.MANY_POS_SOURCE and got["n_pos"][1] > pos_pass()                # more held-out neighbours than one pass holds
    assert sources[2] == ref.FULL_NODE and got["n_neg"][2] == 0 and got["n_pos"][2] > 0      # linked to every candidate: AUC is NaN
    assert sources[3] == ref.F_ROWS and got["n_neg"][3] == -1 and (got["top_ids"][3] == -1).all()          # a source out of range
    assert pos_ids[pos_ptr[5] - 1] >= ref.F_ROWS and got["n_neg"][4] == -1                   # a held-out id out of range
    assert sources[5] >= ref.GRAPH_ROWS and got["n_neg"][5] > 0                              # a source beyond the handle's rows
    assert got["n_pos"][6] == 0 and got["less"][6] == 0 and got["top_is_pos"][6].sum() == 0
    assert candidates[0] < 0 and candidates[-1] >= ref.F_ROWS            # candidates out of range: skipped
    assert (got["n_neg"][got["n_neg"] >= 0] <= 298).all()
    one_way = [(u, v) for u, v in linked if (v, u) not in linked and u in sources and v in candidates and u != ref.FULL_NODE]
    other_way = [(u, v) for u, v in linked if (v, u) not in linked and v in sources and u in candidates and u != ref.FULL_NODE]
    assert one_way and other_way                                         # pairs stored one way only, met from both ends
    twice = [i for i in range(37) if got["n_neg"][i] > 0 and any(v in candidates and (int(sources[i]), int(v)) not in linked
             and (int(v), int(sources[i])) not in linked and v != sources[i] for v in pos_ids[pos_ptr[i]:pos_ptr[i + 1]])]
    assert twice                                                         # a held-out neighbour that is a non-linked candidate too
    assert (got["equal"] > 0).any()


# ---- 2: the tie-free task, end to end -------------------------------------------------------------------------------------------------------
def task_against_host(monkeypatch, capsys, negatives, k, weights, device_graph):
    import gnntf
    G, held, users, items, F = ref.bipartite(1)
    negative_nodes = None if negatives is None else items if negatives == "items" else items[:negatives]
    features = torch.from_numpy(F).cuda()
    gnn = gnntf.Layered(F.shape) if weights else None
    common = dict(k=k, positive_nodes=users, negative_nodes=negative_nodes, gnn=gnn, similarity="dot")
    host = gnntf.MeanLinkPrediction(held, graph=G, **common)
    on_device = gnntf.DeviceGraph(gnntf.graph2adj(G), device="cuda") if device_graph else G
    device = gnntf.MeanLinkPrediction(held, graph=on_device, ranking="device", **common)
    if weights:
        gnn.reset()
        host.r.data.copy_(torch.tensor([0.5, 1.0, 2.0, 1.0, 1.0, 1.0], device=host.r.device).reshape(-1, 1))
        assert device.r is host.r
    host_value, host_per, host_line = host_per_source(monkeypatch, capsys, host, features)
    kept = []
    original = gnntf.link_tasks.ranking_metrics
    monkeypatch.setattr(gnntf.link_tasks, "ranking_metrics", lambda *a: kept.append(original(*a)) or kept[-1])
    value = device.evaluate(features)
    line = capsys.readouterr().out
    for name in NAMES:
        assert same(kept[0][0][name], host_per[name]), name
    assert abs(value - host_value) <= 1e-12 and line == host_line and line.startswith("per-node ranking: AUC")
    if k == 12:
        assert min(len(host.parsed_edges[u]) for u in users) + 6 < k      # the shortest list is shorter than k


@pytest.mark.parametrize("negatives,k", HOST_CASES)
@pytest.mark.parametrize("weights", (False, True))
def test_task_equals_the_host_path(monkeypatch, capsys, negatives, k, weights):
    task_against_host(monkeypatch, capsys, negatives, k, weights, device_graph=False)


def test_task_takes_a_device_graph(monkeypatch, capsys):
    task_against_host(monkeypatch, capsys, "items", 5, True, device_graph=True)


def test_device_ranking_refuses_cpu_embeddings_and_keeps_the_other_paths():
    import gnntf
    G, held, users, items, F = ref.bipartite(1)
    task = gnntf.MeanLinkPrediction(held, graph=G, positive_nodes=users, ranking="device")
    with pytest.raises(Exception, match="GPU only"):
        task.evaluate(torch.from_numpy(F))
    features = torch.from_numpy(F).cuda()
    plain = gnntf.LinkPrediction(held)
    assert torch.equal(task.predict(features, to_logits=True), plain.predict(features, to_logits=True))
    assert float(task.loss(features)) == float(plain.loss(features))


# ---- 3: random normal embeddings ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,K,C,k,splits,pitch", cases())
def test_random_embeddings(graph, S, K, C, k, splits, pitch):
    coo, sources, pos_ptr, pos_ids, candidates, linked = problem(S, K)
    k = short_k(linked, sources, pos_ptr, pos_ids, candidates) if k == "short" else k
    rng = np.random.default_rng(SEED + C)
    F = rng.standard_normal((ref.F_ROWS, C)).astype(np.float32)
    r = (rng.random(C) + 0.5).astype(np.float32)
    device_F = place(F, pitch)
    got = launch(graph, device_F, r, sources, pos_ptr, pos_ids, candidates, k, splits)
    cand_scores, bound = ref.scores64(F, r, sources, candidates)
    valid = ~np.isnan(cand_scores)
    assert (np.abs(got["scores"][valid] - cand_scores[valid]) <= bound[valid]).all() and (got["scores"][~valid] == SENTINEL_FLOAT).all()
    own_pos = own_positive_scores(graph, device_F, r, sources, pos_ptr, pos_ids)
    pos_scores, pos_bound = ref.pos_scores64(F, r, sources, pos_ptr, pos_ids)
    ok = ~np.isnan(pos_scores) & ~np.isnan(own_pos)
    assert (np.abs(own_pos[ok] - pos_scores[ok]) <= pos_bound[ok]).all()
    want = ref.rank(linked, ref.F_ROWS, sources, pos_ptr, pos_ids, candidates, k, got["scores"], own_pos)
    assert_outputs(got, want)


def test_cosine_similarity_equals_prenormalised_rows(capsys):
    import gnntf
    G, held, users, items, _ = ref.bipartite(1)
    F = torch.from_numpy(np.random.default_rng(5).standard_normal((len(G), 20)).astype(np.float32)).cuda()
    cos = gnntf.MeanLinkPrediction(held, graph=G, positive_nodes=users, ranking="device", similarity="cos")
    dot = gnntf.MeanLinkPrediction(held, graph=G, positive_nodes=users, ranking="device", similarity="dot")
    capsys.readouterr()
    a = cos.evaluate(F)
    line_a = capsys.readouterr().out
    b = dot.evaluate(torch.nn.functional.normalize(F, dim=1, eps=1e-12))
    assert a == b and line_a == capsys.readouterr().out and 0 < a <= 1


# ---- 4: independence of the geometry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", (True, False))
@pytest.mark.parametrize("S,K,C,k", ((37, 300, 16, 32), (17, 300, 100, 5), (37, 17, 5, 5)))
def test_outputs_do_not_depend_on_the_parts(graph, exact, S, K, C, k):
    coo, sources, pos_ptr, pos_ids, candidates, linked = problem(S, K)
    if exact:
        F, r = ref.exact_embeddings(SEED + C, C)
    else:
        rng = np.random.default_rng(SEED + C)
        F, r = rng.standard_normal((ref.F_ROWS, C)).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32)
    device_F = place(F, "quad")
    first = launch(graph, device_F, r, sources, pos_ptr, pos_ids, candidates, k, 1, scores=True)
    for splits, scores in ((3, True), (1, False), (3, False), (0, True), (5, False)):
        other = launch(graph, device_F, r, sources, pos_ptr, pos_ids, candidates, k, splits, scores=scores)
        for name in OUTPUTS:
            assert first[name].tobytes() == other[name].tobytes(), (name, splits, scores)
        if scores:
            assert first["scores"].tobytes() == other["scores"].tobytes()


# ---- 5: recommend ---------------------------------------------------------------------------------------------------------------------------
def test_recommend(graph):
    import gnntf
    coo, sources, _, _, candidates, linked = problem(37, 300)
    keep = (sources >= 0) & (sources < ref.F_ROWS)
    nodes = sources[keep]
    F, r = ref.exact_embeddings(SEED, 16)
    empty = np.zeros(len(nodes) + 1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    cand_scores, _ = ref.scores64(F, r, nodes, candidates)
    want = ref.rank(linked, ref.F_ROWS, nodes, *empty, candidates, 7, cand_scores, np.zeros(0))

    class Model:
        pass
    model = Model()
    model.graph = graph
    shuffled = np.concatenate([candidates[::-1], candidates[:5]])         # recommend sorts and de-duplicates
    for where in (graph, model):
        ids, scores = gnntf.recommend(torch.from_numpy(F).cuda(), nodes, 7, where, candidates=shuffled, r=torch.from_numpy(r).cuda())
        ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
        assert np.array_equal(ids, want["top_ids"]) and np.array_equal(scores, want["top_scores"].astype(np.float32))
    for i, s in enumerate(int(x) for x in nodes):
        for v in ids[i][ids[i] >= 0]:
            assert v != s and (s, int(v)) not in linked and (int(v), s) not in linked
    full = list(nodes).index(ref.FULL_NODE)
    assert (ids[full] == -1).all() and np.isneginf(scores[full]).all()   # fewer than k non-linked candidates: padded
    ranked = gnntf.rank_candidates(graph, torch.from_numpy(F).cuda(), nodes, None, candidates, 7, r=torch.from_numpy(r).cuda(), scores=True)
    assert isinstance(ranked, gnntf.RankResult) and np.array_equal(ranked.top_ids.cpu().numpy(), ids)
    assert (ranked.n_pos == 0).all() and torch.isnan(ranked.scores[:, 0]).all() and torch.isnan(ranked.scores[:, -1]).all()
    everyone, _ = gnntf.recommend(torch.from_numpy(F).cuda(), nodes[:3], 4, graph)       # default candidates: every node of the graph
    assert everyone.shape == (3, 4) and int(everyone.max()) < ref.GRAPH_ROWS
