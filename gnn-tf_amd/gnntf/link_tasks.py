"""Link-prediction tasks over node embeddings: edge samplers, LinkPrediction and its ranking evaluation.

API and behaviour follow reference gnntf/core/gnn/graph_predictor.py:34-203 (same class names, constructor arguments, label
layout of the samplers -- one positive followed by ``samples`` negatives -- loss definitions and evaluation metrics); the
structure is this build's own.  On device embeddings the edge logits come from ONE launch of the link-head kernel
(gnx_edge_scores: gather of both endpoint rows + product + optional DistMult weights + reduction); CPU embeddings (host-logic
tests of the protocol) use torch ops."""
from __future__ import annotations

import random

import numpy as np
import torch

from . import metrics, sparse
from .training import Predictor


def _linked(graph, u, v):
    return graph.has_edge(u, v) or graph.has_edge(v, u)


def recommend_all(node, graph=None, positive_edges=None, negative_nodes=None):
    """Every candidate edge of ``node`` with its 0/1 label (graph_predictor.py:34-49): the positive edges that touch the node,
    then (node, v) for every candidate v that is not linked to it."""
    if positive_edges is None:
        positive_edges = [[node, neighbor] for neighbor in graph.neighbors(node)]
    candidates = list(graph) if negative_nodes is None else negative_nodes
    touching = [[u, v] for u, v in positive_edges if node in (u, v)]
    strangers = [[node, v] for v in candidates if v != node and (graph is None or not _linked(graph, node, v))]
    return np.array(touching + strangers), [1] * len(touching) + [0] * len(strangers)


class negative_sampling:
    """Callable edge sampler (graph_predictor.py:52-98): each call returns (edges, labels) where every positive edge (u, v) is
    followed by ``samples`` freshly drawn corrupted edges (u, v') with v' neither u, v nor a neighbour of u; labels are
    1, 0, ..., 0 per group.  ``pool``: draw the negatives of a source node from a fixed pre-sampled pool of that size."""

    def __init__(self, positive_edges, graph, samples=1, negative_nodes=None, pool=None):
        self.positive_edges, self.graph, self.samples, self.pool = positive_edges, graph, samples, pool
        self.negative_nodes = list(graph) if negative_nodes is None else negative_nodes
        group = 1 + samples
        self.labels = np.tile(np.array([1.] + [0.] * samples), len(positive_edges))
        self.edges = np.full((group * len(positive_edges), 2), -1, dtype=int)
        for i, (u, v) in enumerate(positive_edges):
            self.edges[i * group:(i + 1) * group, 0] = u
            self.edges[i * group, 1] = v
        self._negative_pool = None
        if pool is not None:
            self._negative_pool = {u: [self._draw(u, None, self.negative_nodes) for _ in range(pool)]
                                   for u in set(u for u, _ in positive_edges)}

    def _draw(self, u, v, candidates):
        while True:
            w = random.choice(candidates)
            if w != u and w != v and not _linked(self.graph, u, w):
                return w

    def __call__(self):
        group = 1 + self.samples
        for i, (u, v) in enumerate(self.positive_edges):
            candidates = self.negative_nodes if self._negative_pool is None else self._negative_pool[u]
            for s in range(1, group):
                self.edges[i * group + s, 1] = self._draw(u, v, candidates)
        return self.edges, self.labels


class device_negative_sampling:
    """negative_sampling on the device (graph_predictor.py:52-98; the layout and the acceptance rule are the reference's, the draws are
    this build's counter RNG): the positive pairs, the candidates, the labels and ONE [m (1 + samples), 2] edge buffer live on the
    device of ``model``; each call takes the model's next mask stream and fills the buffer with one launch of gnx_sample_negatives
    over ``model.graph`` -- no host loop, no upload, and a call records into a device graph (train(capture=True)).  A slot whose
    ``max_tries`` draws were all rejected keeps its last draw; ``fallbacks()`` counts those (it synchronises: not for the loop).
    ``negative_nodes``: the candidate ids (default: every node).  The reference's ``pool`` stays with the host sampler."""

    def __init__(self, positive_edges, model, samples=1, negative_nodes=None, max_tries=32):
        graph = model.graph
        if int(samples) < 1 or int(max_tries) < 1:
            raise Exception("device_negative_sampling: samples and max_tries must be at least 1")
        self.model, self.graph, self.samples, self.max_tries = model, graph, int(samples), int(max_tries)
        self.positive_edges = sparse.DeviceIndex(positive_edges, graph.device, graph.n_rows, "edge endpoint").tensor.reshape(-1, 2)
        self.negative_nodes = None if negative_nodes is None else \
            sparse.DeviceIndex(negative_nodes, graph.device, graph.n_rows, "candidate node").tensor.reshape(-1)
        m = self.positive_edges.shape[0]
        self.labels = torch.tensor([1.] + [0.] * self.samples, dtype=torch.float32, device=graph.device).repeat(m)
        # no upper bound on the index: the embedding rows it is scored against may outnumber the graph's (NGCF stacks its layers' rows)
        self.edges = sparse.DeviceIndex(torch.full((m * (1 + self.samples), 2), -1, dtype=torch.int64, device=graph.device), graph.device,
                                        fixed=False)
        self._fallbacks = torch.zeros(1, dtype=torch.int64, device=graph.device)
        self()

    def __call__(self):
        seed, stream = self.model._next_mask_stream()
        sparse.sample_negatives(self.graph, self.positive_edges, self.samples, self.negative_nodes, seed, stream, out=self.edges.tensor,
                                max_tries=self.max_tries, fallbacks=self._fallbacks)
        return self.edges, self.labels

    def fallbacks(self) -> int:
        return int(self._fallbacks.item())


def _on_device(edges) -> bool:
    return isinstance(edges, sparse.DeviceIndex) or (isinstance(edges, torch.Tensor) and edges.is_cuda)


def _edge_logits(features, edges, r, backward="atomic"):
    if features.is_cuda:
        return sparse.edge_scores(features, edges, r, backward=backward)
    e = torch.as_tensor(np.asarray(edges), dtype=torch.int64)
    prod = features[e[:, 0]] * features[e[:, 1]]
    return prod.sum(dim=1) if r is None else (prod @ r).reshape(-1)


def _as_labels(labels):
    if labels is None:
        return None
    if isinstance(labels, torch.Tensor) and labels.is_cuda:             # a device sampler's labels stay where they are
        return labels.to(torch.float32).reshape(-1, 1)
    return np.asarray(labels, dtype=np.float32).reshape(-1, 1)


class LinkPrediction(Predictor):
    """graph_predictor.py:101-151.  ``edges`` is an [m, 2] array or a sampler (called again before every use);
    ``similarity`` "dot" or "cos"; ``loss`` "diff" (pairwise: -mean log sigmoid(logit_even - logit_odd), for samplers with one
    negative per positive) or anything else for binary cross entropy on the labels; ``gnn``: adds the shared DistMult weights.
    ``edges`` may also live on the device -- a device_negative_sampling, a sparse.DeviceIndex or a device tensor -- and then stays
    there: nothing is uploaded per call, which is what train(capture=True) needs.  ``edge_backward``: how the gradient of the edge
    logits is summed into the embedding rows (sparse.edge_scores): "atomic" or "sorted" (fixed order: a step repeats bit for bit);
    default "sorted" for a device_negative_sampling and "atomic" for everything else."""

    def __init__(self, edges, labels=None, gnn=None, similarity="dot", loss="diff", regularize=0, batch_size=float('inf'),
                 edge_backward=None):
        if edge_backward is None:
            edge_backward = "sorted" if isinstance(edges, device_negative_sampling) else "atomic"
        if edge_backward not in ("atomic", "sorted"):
            raise Exception('LinkPrediction: edge_backward must be "atomic" or "sorted"')
        self.edge_backward = edge_backward
        self.edge_sampler = edges if callable(edges) else None
        if self.edge_sampler is not None:
            edges, labels = self.edge_sampler()
        self.batch_size = batch_size
        if _on_device(edges):
            if batch_size != float('inf'):
                raise Exception("LinkPrediction: batch_size subsamples the edge list with the host's `random`, which edges kept on "
                                "the device (device_negative_sampling, DeviceIndex, device tensor) cannot follow: leave it infinite")
            self.edges = edges if isinstance(edges, sparse.DeviceIndex) else sparse.DeviceIndex(edges.reshape(-1, 2), edges.device, fixed=False)
        else:
            self.edges = np.array(edges)
        self.loss_func = loss
        self.labels = _as_labels(labels)
        self.r = None if gnn is None else gnn.create_var(shape=(gnn.top_shape()[1], 1), regularize=0, shared_name="distmult",
                                                          normalization="ones", trainable=True)
        self.similarity = similarity
        self.regularize = regularize

    def _update_labels(self):
        if self.edge_sampler is not None:
            edges, labels = self.edge_sampler()
            self.edges = edges
            self.labels = _as_labels(labels)

    def _embed(self, features):
        return torch.nn.functional.normalize(features, dim=1, eps=1e-12) if self.similarity == "cos" else features

    def predict(self, features, to_logits=False):
        self._update_labels()
        logits = _edge_logits(self._embed(features), self.edges, self.r, self.edge_backward)
        return logits if to_logits else torch.sigmoid(logits)

    def loss(self, features):
        self._update_labels()
        features = self._embed(features)
        if self.loss_func == "diff":
            edges = self.edges
            take = min(self.batch_size, len(edges))
            if take != len(edges):
                edges = edges[random.sample(range(len(edges)), take), :]
            logits = _edge_logits(features, edges, self.r, self.edge_backward)
            return -torch.nn.functional.logsigmoid(logits[0::2] - logits[1::2]).mean()
        logits = _edge_logits(features, self.edges, self.r, self.edge_backward)
        target = torch.as_tensor(self.labels, dtype=torch.float32, device=logits.device).reshape(-1)
        return torch.nn.functional.binary_cross_entropy_with_logits(logits, target)

    def evaluate(self, features):
        self._update_labels()
        return metrics.auc(self.labels.reshape(-1), self.predict(features))


def recommend(F, nodes, k, graph, candidates=None, r=None):
    """The ``k`` best candidates of every node of ``nodes`` that are neither the node itself nor linked to it in ``graph`` (a
    sparse.DeviceGraph, or a model for its graph), by the link head's score <F[u] * r, F[v]>: (ids [S, k], scores [S, k]) on the device,
    best first, ties to the larger id; a row with fewer than ``k`` such candidates ends in ids of -1 (scores -inf).  ``candidates``:
    node ids (default: every node of the graph).  One call of sparse.rank_candidates without held-out neighbours: no score matrix is
    stored."""
    graph = graph if isinstance(graph, sparse.DeviceGraph) else graph.graph
    if candidates is None:
        candidates = torch.arange(graph.n_rows, dtype=torch.int64, device=graph.device)
    elif isinstance(candidates, torch.Tensor):
        candidates = torch.unique(candidates.to(graph.device, torch.int64).reshape(-1))      # sorted and de-duplicated
    else:
        candidates = torch.from_numpy(np.unique(np.asarray(candidates, dtype=np.int64))).to(graph.device)
    ranked = sparse.rank_candidates(graph, F, nodes, None, candidates, k, r=r)
    return ranked.top_ids, ranked.top_scores


def ranking_metrics(n_pos, n_neg, less, equal, top_ids, top_is_pos, k, n_candidates):
    """The per-source metrics of MeanLinkPrediction.evaluate from what sparse.rank_candidates returns, as host arrays: AUC from the rank
    statistic (NaN without a stranger), and average precision, precision (over min(k, list length) entries), recall and F1 of the top-k
    list -- the definitions of metrics.py, in its order of operations -- plus the coverage: distinct ids in the top-k lists over the
    number of candidates.  Returns ({name: float64 [S]}, coverage)."""
    n_pos, n_neg = np.asarray(n_pos, dtype=np.int64), np.asarray(n_neg, dtype=np.int64)
    less, equal = np.asarray(less, dtype=np.float64), np.asarray(equal, dtype=np.float64)
    top_ids, labels = np.asarray(top_ids).reshape(len(n_pos), -1), np.asarray(top_is_pos, dtype=np.float64).reshape(len(n_pos), -1)
    if (n_neg < 0).any():
        raise Exception("ranking_metrics: a source or one of its held-out nodes is not a row of the embeddings")
    taken = np.minimum(k, n_pos + n_neg)                                 # entries of the top-k list; the columns beyond them are padding
    real = np.arange(labels.shape[1])[None, :] < taken[:, None]
    labels = np.where(real, labels, 0.0)
    hits = labels.sum(axis=1)
    gain = np.zeros(len(n_pos))
    for position in range(labels.shape[1]):                              # best first, added in metrics.avprec's order
        gain = gain + labels[:, position] / (position + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        pairs = (n_pos * n_neg).astype(np.float64)
        auc = np.where(pairs > 0, (less + equal / 2.0) / pairs, np.nan)
        avprec = np.where(gain == 0, 0.0, gain / hits)
        precision, recall = hits / taken, hits / n_pos
        f1 = np.where(precision + recall == 0, 0.0, 2 * precision * recall / (precision + recall))
    scores = {"auc": auc, "avprec": avprec, "prec": precision, "rec": recall, "f1": f1}
    return scores, len(np.unique(top_ids[real])) / n_candidates


class MeanLinkPrediction(LinkPrediction):
    """graph_predictor.py:154-203: per-node ranking quality -- for every positive node, its held-out edges against all
    non-linked candidates; prints mean AUC / MAP / precision / recall / F1 at k and the coverage of the top-k lists,
    returns the mean F1.
    ``ranking``: "host" (default) walks the sources in Python, one launch of the link head per source.  "device" ranks every source in
    ONE call of sparse.rank_candidates on device embeddings and downloads O(sources * k) numbers; the constructor then lays out, once,
    the sources, the CSR list of their held-out neighbours (in ``parsed_edges`` order) and the sorted candidates, and ``graph`` may be a
    networkx graph whose nodes are numbered 0 .. n - 1 in order (graph2adj's numbering) or a sparse.DeviceGraph; a networkx graph
    becomes a pattern-only DeviceGraph at the first evaluation, on the device of the embeddings it is given.  Scores that tie are
    ordered as np.argsort(kind="stable") orders the host list built in ascending candidate order."""

    def __init__(self, *args, graph, positive_nodes=None, negative_nodes=None, k=5, ranking="host", **kwargs):
        super().__init__(*args, **kwargs)
        if ranking not in ("host", "device"):
            raise Exception('MeanLinkPrediction: ranking must be "host" or "device"')
        self.positive_nodes, self.negative_nodes, self.k, self.graph, self.ranking = positive_nodes, negative_nodes, k, graph, ranking
        self.parsed_edges = dict()
        for u, v in self.edges:
            self.parsed_edges.setdefault(u, list())
            self.parsed_edges.setdefault(v, list())
            self.parsed_edges[u].append(v)
            self.parsed_edges[v].append(u)
        if ranking == "device":
            self._lay_out_ranking()

    def _lay_out_ranking(self):
        if not 1 <= int(self.k) <= sparse.RANK_MAX_K:
            raise Exception(f'MeanLinkPrediction: ranking="device" takes k in [1, {sparse.RANK_MAX_K}]')
        sources = list(self.parsed_edges) if self.positive_nodes is None else list(self.positive_nodes)
        for node in sources:
            if node not in self.parsed_edges:
                raise Exception("Node not found")
        lengths = [len(self.parsed_edges[node]) for node in sources]
        candidates = set(v for neighbors in self.parsed_edges.values() for v in neighbors) if self.negative_nodes is None \
            else set(self.negative_nodes)
        self._rank_host = (np.asarray(sources, dtype=np.int64).reshape(-1), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64),
                           np.asarray([v for node in sources for v in self.parsed_edges[node]], dtype=np.int64).reshape(-1),
                           np.asarray(sorted(candidates), dtype=np.int64).reshape(-1))
        self._rank_device = None                                         # (graph, sources, (ptr, ids), candidates) on the device
        if isinstance(self.graph, sparse.DeviceGraph):
            self._upload_ranking(self.graph.device)
        elif list(self.graph) != list(range(len(self.graph))):
            raise Exception('MeanLinkPrediction: ranking="device" needs a graph whose nodes are numbered 0 .. n - 1 in order '
                            '(graph2adj numbers them so), or a DeviceGraph')

    def _upload_ranking(self, device):
        graph = self.graph
        if not isinstance(graph, sparse.DeviceGraph):
            from .graph_io import graph2adj
            graph = sparse.DeviceGraph(graph2adj(graph, directed=True), device=device)      # the pattern: either direction links a pair
        sources, ptr, ids, candidates = (torch.from_numpy(x).to(graph.device) for x in self._rank_host)
        self._rank_device = (graph, sources, (ptr, ids), candidates)

    def _evaluate_on_device(self, features):
        if not features.is_cuda:
            raise Exception('MeanLinkPrediction: ranking="device" runs on the GPU only (embeddings on %s); ranking="host" evaluates '
                            'CPU embeddings' % features.device)
        if self._rank_device is None:
            self._upload_ranking(features.device)
        graph, sources, positives, candidates = self._rank_device
        with torch.no_grad():
            ranked = sparse.rank_candidates(graph, self._embed(features), sources, positives, candidates, self.k, r=self.r)
            counts = torch.stack([ranked.n_pos, ranked.n_neg, ranked.less, ranked.equal]).cpu().numpy()
            top_ids, top_is_pos = ranked.top_ids.cpu().numpy(), ranked.top_is_pos.cpu().numpy()
        scores, coverage = ranking_metrics(*counts, top_ids, top_is_pos, self.k, len(candidates))
        mean = {name: float(np.mean(v)) for name, v in scores.items()}
        print("per-node ranking: AUC %.3f  MAP %.3f  precision %.3f  recall %.3f  F1 %.3f  coverage %.3f"
              % (mean["auc"], mean["avprec"], mean["prec"], mean["rec"], mean["f1"], coverage))
        return np.mean(scores["f1"])

    def evaluate(self, features):
        if self.ranking == "device":
            return self._evaluate_on_device(features)
        k = self.k
        sources = list(self.parsed_edges) if self.positive_nodes is None else self.positive_nodes
        # default candidates: every node that appears in the held-out edges.  (The reference iterates the dict's KEYS here,
        # graph_predictor.py:178, which raises TypeError for integer nodes; the neighbour lists are what was meant.)
        candidates = set(v for neighbors in self.parsed_edges.values() for v in neighbors) if self.negative_nodes is None \
            else set(self.negative_nodes)
        scores = {name: [] for name in ("auc", "avprec", "prec", "rec", "f1")}
        recommended = set()
        for node in sources:
            if node not in self.parsed_edges:
                raise Exception("Node not found")
            held_out = [[node, v] for v in self.parsed_edges[node]]
            strangers = [[node, v] for v in candidates if v != node and not _linked(self.graph, node, v)]
            self.labels = np.array([1.] * len(held_out) + [0] * len(strangers))
            self.edges = np.array(held_out + strangers)
            prediction = metrics._np(self.predict(features))
            scores["auc"].append(metrics.auc(self.labels, prediction))
            for name in ("avprec", "prec", "rec", "f1"):
                scores[name].append(getattr(metrics, name)(self.labels, prediction, k))
            recommended.update(self.edges[i][1] for i in np.argsort(prediction)[-k:])
        mean = {name: float(np.mean(v)) for name, v in scores.items()}
        print("per-node ranking: AUC %.3f  MAP %.3f  precision %.3f  recall %.3f  F1 %.3f  coverage %.3f"
              % (mean["auc"], mean["avprec"], mean["prec"], mean["rec"], mean["f1"], len(recommended) / len(candidates)))
        return np.mean(scores["f1"])
