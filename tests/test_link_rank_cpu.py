"""The device ranking evaluation without a GPU: the header declares the entries and the library exports them, their argument checks run
before anything touches a device, the package exports the new names and refuses what it cannot do, and the numpy reference the GPU
tests compare against (tests/link_rank_ref.py) agrees with the host MeanLinkPrediction.evaluate on the tie-free construction -- as
does the metric assembly of the device path when it is fed the reference's counts and lists."""
import ctypes
import re

import numpy as np
import pytest
import torch

import abi_header
import link_rank_ref as ref

ENTRIES = ("gnx_rank_candidates_bytes", "gnx_rank_candidates")
FAKE = ctypes.c_void_p(4096)         # stands for a device pointer: every call below fails a check before anything would read it
NAMES = ("auc", "avprec", "prec", "rec", "f1")


def lib():
    from gnntf import _native
    return _native.lib()


def test_header_declares_and_library_exports_the_entries():
    from gnntf import _native, sparse
    header, declared = abi_header.text(), abi_header.declared()
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and hasattr(handle, name) and name in _native.SIGNATURES
    assert "graph_predictor.py:154-203" in header
    assert handle.gnx_version() == _native.ABI_VERSION == 900            # added within 0.9: callers probe for the symbols
    constants = dict(re.findall(r"#define (GNX_RANK_[A-Z_]+) (\d+)", header))
    assert int(constants["GNX_RANK_MAX_K"]) == sparse.RANK_MAX_K >= 32 and int(constants["GNX_RANK_POS_PASS"]) == sparse.RANK_POS_PASS


def refused(rc, *words):
    message = lib().gnx_last_error()
    assert rc == -1 and all(w.encode() in message for w in words), message


def test_argument_errors():
    call, nbytes = lib().gnx_rank_candidates, lib().gnx_rank_candidates_bytes
    max_k = 32
    assert nbytes(10, 20, 300, 5, 0) >= 20 * 4 + 10 * 5 * 8 and nbytes(0, 0, 0, 1, 0) >= 0
    assert nbytes(10, 20, 300, 5, 3) >= 20 * 4 + 10 * 3 * 5 * 8
    assert nbytes(10, 20, 30, 5, 3) == nbytes(10, 20, 30, 5, 1)           # one tile of candidates: one part
    for bad in ((-1, 0, 10, 5, 0), (10, -1, 10, 5, 0), (10, 0, -1, 5, 0), (10, 0, 2 ** 31, 5, 0), (10, 0, 10, 0, 0), (10, 0, 10, max_k + 1, 0),
                (10, 0, 10, 5, -1), (10, 0, 10, 5, 257)):
        assert nbytes(*bad) == -1 and b"gnx_rank_candidates_bytes" in lib().gnx_last_error()
    good = dict(g=FAKE, F=FAKE, ldf=8, n=50, C=8, r=None, src=FAKE, S=10, ptr=FAKE, ids=FAKE, P=20, cand=FAKE, K=300, k=5, splits=0,
                n_pos=FAKE, n_neg=FAKE, less=FAKE, equal=FAKE, top_ids=FAKE, top_scores=FAKE, top_is_pos=FAKE, scores=None, ws=FAKE,
                bytes=nbytes(10, 20, 300, 5, 0))

    def run(**change):
        a = dict(good, **change)
        return call(a["g"], a["F"], a["ldf"], a["n"], a["C"], a["r"], a["src"], a["S"], a["ptr"], a["ids"], a["P"], a["cand"], a["K"], a["k"],
                    a["splits"], a["n_pos"], a["n_neg"], a["less"], a["equal"], a["top_ids"], a["top_scores"], a["top_is_pos"], a["scores"],
                    a["ws"], a["bytes"], None)

    for change in (dict(S=-1), dict(P=-1), dict(K=-1), dict(K=2 ** 31), dict(S=2 ** 31)):
        refused(run(**change), "gnx_rank_candidates: S, P and K")
    for change in (dict(k=0), dict(k=-3), dict(k=max_k + 1)):
        refused(run(**change), "k must be in [1, 32]")
    for change in (dict(splits=-1), dict(splits=257)):
        refused(run(**change), "splits")
    for change in (dict(C=0), dict(ldf=7), dict(n=-1), dict(n=2 ** 31)):
        refused(run(**change), "bad sizes")
    refused(run(g=None), "NULL handle")
    for change in (dict(F=None), dict(src=None), dict(ptr=None), dict(ids=None), dict(cand=None), dict(n_pos=None), dict(n_neg=None),
                   dict(less=None), dict(equal=None), dict(top_ids=None), dict(top_scores=None), dict(top_is_pos=None), dict(ws=None)):
        refused(run(**change), "NULL pointer")
    refused(run(bytes=good["bytes"] - 1), "gnx_rank_candidates_bytes")
    refused(run(splits=3, bytes=nbytes(10, 20, 300, 5, 3) - 1), "gnx_rank_candidates_bytes")
    refused(run(ws=ctypes.c_void_p(4100)), "16-byte aligned")
    assert run(S=0, F=None, src=None, ptr=None, ws=None, bytes=0, n_pos=None, top_ids=None) == 0      # no sources: nothing to do, nothing read


def test_package_exports_and_refusals():
    import gnntf
    for name in ("recommend", "rank_candidates", "ranking_metrics", "RankResult", "MeanLinkPrediction"):
        assert hasattr(gnntf, name)
    assert gnntf.recommend is gnntf.link_tasks.recommend and gnntf.rank_candidates is gnntf.sparse.rank_candidates
    with pytest.raises(Exception, match="GPU only"):
        gnntf.rank_candidates(None, torch.zeros(4, 4), [0], None, [1, 2], 2)
    G, held, users, items, F = ref.bipartite(0)
    with pytest.raises(Exception, match="ranking"):
        gnntf.MeanLinkPrediction(held, graph=G, ranking="fast")
    assert gnntf.MeanLinkPrediction(held, graph=G).ranking == "host"
    task = gnntf.MeanLinkPrediction(held, graph=G, positive_nodes=users, ranking="device")
    with pytest.raises(Exception, match="GPU only"):
        task.evaluate(torch.from_numpy(F))
    with pytest.raises(Exception, match="Node not found"):               # a source without held-out edges: at construction
        gnntf.MeanLinkPrediction(held, graph=G, positive_nodes=[len(G) + 7], ranking="device")
    with pytest.raises(Exception, match="k in"):
        gnntf.MeanLinkPrediction(held, graph=G, positive_nodes=users, ranking="device", k=33)
    sources, ptr, ids, candidates = task._rank_host                      # laid out once, in parsed_edges order
    assert sources.tolist() == users and (np.diff(candidates) > 0).all()
    for i, u in enumerate(users):
        assert ids[ptr[i]:ptr[i + 1]].tolist() == [int(v) for v in task.parsed_edges[u]]


class Recorder:
    """Wraps the metric functions of gnntf.metrics, which the host evaluate calls per source, and keeps what they return."""

    def __init__(self, monkeypatch):
        from gnntf import metrics
        self.values = {name: [] for name in NAMES}
        for name in NAMES:
            monkeypatch.setattr(metrics, name, self._wrap(name, getattr(metrics, name)))

    def _wrap(self, name, fn):
        def wrapped(*args, **kwargs):
            value = fn(*args, **kwargs)
            self.values[name].append(float(value))
            return value
        return wrapped


def host_per_source(monkeypatch, capsys, task, F):
    """(mean F1, per-source metrics, the printed line) of the host evaluate.  metrics.f1 calls prec and rec again: every second of their
    recorded values is the evaluate's own call."""
    with monkeypatch.context() as patch:
        recorder = Recorder(patch)
        capsys.readouterr()
        value = task.evaluate(F)
    line = capsys.readouterr().out
    per = {name: np.array(v) for name, v in recorder.values.items()}
    per["prec"], per["rec"] = per["prec"][0::2], per["rec"][0::2]
    return value, per, line


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


# (negative_nodes: None = the default candidates, "items", or that many items), k: 12 exceeds the shortest list of the last case
HOST_CASES = ((None, 1), ("items", 5), (6, 12))


@pytest.mark.parametrize("negatives,k", HOST_CASES)
@pytest.mark.parametrize("weights", (False, True))
def test_reference_equals_the_host_evaluate(monkeypatch, capsys, negatives, k, weights):
    import gnntf
    gnntf.set_default_device("cpu")
    try:
        G, held, users, items, F = ref.bipartite(1)
        negative_nodes = None if negatives is None else items if negatives == "items" else items[:negatives]
        gnn = gnntf.Layered(F.shape) if weights else None
        task = gnntf.MeanLinkPrediction(held, graph=G, k=k, positive_nodes=users, negative_nodes=negative_nodes, gnn=gnn)
        if weights:
            gnn.reset()
            with torch.no_grad():
                task.r.copy_(torch.tensor([0.5, 1.0, 2.0, 1.0, 1.0, 1.0]).reshape(-1, 1))      # powers of two: still exact
        value, per, line = host_per_source(monkeypatch, capsys, task, torch.from_numpy(F))
    finally:
        gnntf.set_default_device(None)
    r = task.r.detach().numpy().reshape(-1) if weights else None

    candidates = np.array(sorted(set(v for vs in task.parsed_edges.values() for v in vs) if negative_nodes is None else set(negative_nodes)))
    sources = np.array(users)
    lists = [task.parsed_edges[u] for u in users]
    pos_ptr, pos_ids = np.concatenate([[0], np.cumsum([len(x) for x in lists])]), np.concatenate(lists)
    linked = ref.linked_set(np.array(G.edges()))
    cand_scores, _ = ref.scores64(F, r, sources, candidates)
    pos_scores, _ = ref.pos_scores64(F, r, sources, pos_ptr, pos_ids)
    result = ref.rank(linked, len(F), sources, pos_ptr, pos_ids, candidates, k, cand_scores, pos_scores)
    for _, _, x in result["lists"]:                                       # the construction: no two entries of a list score alike
        assert np.diff(np.sort(x)).min() >= 2.0 ** -14 and np.abs(x).max() < 2.2 and (x.astype(np.float32) == x).all()
    want, coverage = ref.metrics(result, k, len(candidates))
    if k == 12:
        assert (result["n_pos"] + result["n_neg"]).min() < k             # the top-k list of some source is shorter than k
    for name in NAMES:
        assert same(want[name], per[name]), name
    assert abs(np.mean(want["f1"]) - value) <= 1e-12
    mean = {name: float(np.mean(v)) for name, v in want.items()}
    assert line == ("per-node ranking: AUC %.3f  MAP %.3f  precision %.3f  recall %.3f  F1 %.3f  coverage %.3f\n"
                    % (mean["auc"], mean["avprec"], mean["prec"], mean["rec"], mean["f1"], coverage))

    # the metric assembly of the device path, fed the reference's counts and lists
    got, got_coverage = gnntf.ranking_metrics(result["n_pos"], result["n_neg"], result["less"], result["equal"], result["top_ids"],
                                              result["top_is_pos"], k, len(candidates))
    for name in NAMES:
        assert same(got[name], per[name]), name
    assert got_coverage == coverage


def test_reference_ties_positions_and_out_of_range():
    """The tie rule and the edge cases of the specification on a list small enough to read."""
    F = np.array([[1.0], [1.0], [1.0], [2.0], [0.5], [1.0]], dtype=np.float32)
    linked = ref.linked_set([(0, 4), (5, 0)])                            # 4 is linked as stored, 5 the other way round
    sources, pos_ptr, pos_ids = np.array([0, 0, 9]), np.array([0, 2, 3, 4]), np.array([1, 2, 7, 1])
    candidates = np.array([-2, 0, 1, 2, 3, 4, 5, 6])
    cand, _ = ref.scores64(F, None, sources, candidates)
    pos, _ = ref.pos_scores64(F, None, sources, pos_ptr, pos_ids)
    out = ref.rank(linked, len(F), sources, pos_ptr, pos_ids, candidates, 4, cand, pos)
    # source 0: positives 1, 2 (score 1 each), strangers 1, 2, 3 (scores 1, 1, 2): the held-out ids are non-linked candidates too
    assert out["n_pos"].tolist() == [2, 1, 1] and out["n_neg"].tolist() == [3, -1, -1]
    assert out["less"][0] == 0 and out["equal"][0] == 4
    assert out["top_ids"][0].tolist() == [3, 2, 1, 2] and out["top_is_pos"][0].tolist() == [0, 0, 0, 1]
    assert out["top_scores"][0].tolist() == [2.0, 1.0, 1.0, 1.0]
    assert out["top_ids"][1].tolist() == [-1] * 4 and np.isneginf(out["top_scores"][2]).all()
    with pytest.raises(Exception, match="not a row"):
        __import__("gnntf").ranking_metrics(out["n_pos"], out["n_neg"], out["less"], out["equal"], out["top_ids"], out["top_is_pos"], 4, 8)
