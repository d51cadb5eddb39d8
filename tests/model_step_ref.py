"""One training step of GCN, GCNII, NGCF and the Dropout + Dense pre-MLP in dense float64 with torch autograd on the CPU: the meaning a
whole step of the HIP models is judged against (tests/test_gpu_model_steps.py), judged on its own in tests/test_model_step_ref_cpu.py.
numpy and CPU torch only: imports without a GPU and without the package.

Written from the behavioural contract -- the reference project's gnntf/core/gnn/architectures/gcn.py (the layers and the three model
constructors), gnntf/core/gnn/gnn.py:36-50 (get_adjacency), gnntf/core/nn/layers.py (Dense, Dropout, Concatenate),
gnntf/core/nn/layered.py (the training-mode switch, dropout, Layer.loss) and gnntf/core/nn/trainable.py:69-79 (the objective) -- and
from the rules this build documents for what the contract leaves open (the counter RNG and the numbering of its streams).  Nothing
here reads a model: an architecture is a list of layer descriptions (gcn / gcnii / ngcf below build them as the class constructors
do), the parameters are a flat list in creation order.

The objective (trainable.py:71-77):  task loss(training-mode forward) + sum over layers output_regularize * sum(value^2) / 2
                                     + regularization * sum over variables var.regularize * sum(var^2) / 2.
  regularize per variable: Dense W, b: the layer's ``regularize`` (False on the last Dense of GCNII); GCN layers W, b: 1;
  GCNII W: ``convolution_regularization``, the spectral layer's bias: 1; NGCFLayer(regularize=0.0): W1, W2: 0, b1, b2: 1.

The layers, training mode (drop = feature dropout: keep mask times 1 / (1 - p)):
  Dropout(p)        drop(X)
  Dense             drop(act(X W + b))
  GCNLayer          drop(relu((A X) W + b))                    A = get_adjacency(graph_dropout), a new one per forward
  GCNSpectral...    2 drop(relu((A X) W + b) - b)
  GCNIILayer        drop(relu(T M)),  T = (1 - a) A H + a H0,  M = (1 - beta) I + beta W,  beta = log1p(l / (k + 1))
  GCNIISpectral...  2 drop(relu(T M + bias) - bias)
  NGCFLayer         l2_normalize(drop(leaky((X * (B X)) W1 + b1) + leaky((B X) W2 + b2)))     B = the bipartite adjacency, taken ONCE when
                    the layer is built (gcn.py:127); output_regularize = 1
  Concatenate       the listed layers' values stacked along axis 0 (layers.py:98-101)
In eval mode every dropout is the identity and A is the constant adjacency.

Mask streams (protocol.Layered._next_mask_stream): a model numbers the masks of the counter RNG 0, 1, 2, ... over its lifetime.  In
training mode a layer draws one stream for its dropped adjacency (graph_dropout != 0) and THEN one for its feature mask where that mask
is the counter RNG's (0 < p < 1); layers draw in layer order; an eval-mode forward draws none; the numbering carries on from one
step to the next.  The reference keeps this count itself (``Reference.streams``).

Feature masks come from one of two providers, per layer (``mask`` of a layer description):
  "torch"    drawn once on the host and handed out in call order (FixedMasks): the GPU test patches the same object into
             ``model.dropout``, so both sides see the same masks;
  "counter"  keep iff hash_u24(seed, stream, i, c, 0) >= int(p 2^24), kept values times the f32 1 / (1 - p) (dense_drop_ref.keep_mask).

``mistake=`` plants one wrong reading of the contract (MISTAKES): what tests/test_model_step_ref_cpu.py measures the bar against."""
import math

import numpy as np
import torch

import dense_drop_ref
import graphs
from oracle import gnntf_oracle as orc

MISTAKES = ("stream_off_by_one", "mask_stream_first", "no_dropout_scale", "no_doubling", "beta_k", "last_dense_decayed",
            "no_output_penalty", "concatenate_axis_1", "bipartite_row_sums")

# the bar of tests/test_gpu_training.py: the loss within LOSS_RTOL, gradients within GRAD_RTOL |want| + GRAD_ATOL max|want|, and
# every compared gradient above NON_TRIVIAL somewhere
LOSS_RTOL, GRAD_RTOL, GRAD_ATOL, NON_TRIVIAL = 1e-5, 1e-3, 2e-5, 1e-4
STEP_SIZE = 0.05
LEAKY_SLOPE = 0.2                                       # tf.nn.leaky_relu's default (gcn.py:117)


class FixedMasks:
    """Feature-dropout masks drawn once on the host, handed out in call order: the same masks drive the HIP model
    (patched into Layered.dropout) and the dense reference, so the two computations are comparable bit for bit."""

    def __init__(self, seed):
        self.rng, self.masks, self.cursor = np.random.default_rng(seed), [], 0

    def mask(self, shape, p):
        if self.cursor == len(self.masks):
            self.masks.append((self.rng.random(shape) >= p).astype(np.float64) / (1.0 - p))
        m = self.masks[self.cursor]
        self.cursor += 1
        return m

    def rewind(self):
        self.cursor = 0


def counter_mask(shape, p, seed, stream):
    """The counter RNG's feature mask times the f32 1 / (1 - p), as float64."""
    keep = dense_drop_ref.keep_mask((p, seed, stream), shape[0], shape[1])
    return keep.astype(np.float64) * np.float64(dense_drop_ref.scale(p))


# ---- architectures as the class constructors build them ------------------------------------------------------------------------------
def gcn(num_classes, latent_dims=(64,), spectral=False, counter=()):
    """gcn.py:108-113: one layer per latent width with graph_dropout = dropout = 0.5, then the output layer with neither (it keeps the
    relu).  ``counter``: the indices of the layers whose feature mask is the counter RNG's."""
    layers = [dict(kind="gcn", outputs=w, spectral=spectral, rate=0.5, graph_dropout=0.5) for w in latent_dims]
    layers.append(dict(kind="gcn", outputs=num_classes, spectral=spectral, rate=0, graph_dropout=0))
    for i, layer in enumerate(layers):
        layer["mask"] = "counter" if i in counter else "torch"
    return layers


def gcnii(num_classes, a=0.1, l=0.5, latent_dims=(64,), iterations=64, dropout=0.6, convolution_regularization=True, spectral=False,
          graph_dropout=0, mask="torch", input_mask="torch"):
    """gcn.py:54-74: Dropout(dropout), Dense(relu) per latent width -- the last one is H0 --, ``iterations`` layers numbered k = 0 ..,
    Dense(num_classes, regularize=False).  The class passes graph_dropout = 0; the layers' own default is 0.5."""
    layers = [dict(kind="dropout", rate=dropout, mask=input_mask)]
    layers += [dict(kind="dense", outputs=w, act="relu", rate=0, regularize=True, mask=input_mask) for w in latent_dims]
    h0 = len(layers) - 1
    layers += [dict(kind="gcnii", spectral=spectral, a=a, l=l, k=k, rate=dropout, graph_dropout=graph_dropout, h0=h0,
                    regularize=convolution_regularization, mask=mask) for k in range(iterations)]
    layers.append(dict(kind="dense", outputs=num_classes, act=None, rate=0, regularize=False, mask=input_mask, last=True))
    return layers


def ngcf(num_classes, latent_dims=None, dropout=0.1, mask="torch"):
    """gcn.py:138-154: NGCFLayer(regularize=0.0, dropout, output_regularize=1) per width, closed by Concatenate over all of them."""
    widths = ([num_classes] * 2 if latent_dims is None else list(latent_dims)) + [num_classes]
    layers = [dict(kind="ngcf", outputs=w, rate=dropout, mask=mask, penalty=1.0) for w in widths]
    layers.append(dict(kind="concatenate", sources=list(range(len(widths)))))
    return layers


def variables(layers, width):
    """[(shape, regularize, role)] of every variable in creation order, for input features of ``width`` columns."""
    out = []
    for layer in layers:
        kind = layer["kind"]
        if kind == "dense":
            out += [((width, layer["outputs"]), float(layer["regularize"]), "W"), ((1, layer["outputs"]), float(layer["regularize"]), "b")]
            width = layer["outputs"]
        elif kind == "gcn":
            out += [((width, layer["outputs"]), 1.0, "W"), ((1, layer["outputs"]), 1.0, "b")]
            width = layer["outputs"]
        elif kind == "gcnii":
            out.append(((width, width), float(layer["regularize"]), "M"))
            if layer["spectral"]:
                out.append(((1, width), 1.0, "b"))
        elif kind == "ngcf":
            out += [((width, layer["outputs"]), 0.0, "W"), ((width, layer["outputs"]), 0.0, "W"), ((1, layer["outputs"]), 1.0, "b"),
                    ((1, layer["outputs"]), 1.0, "b")]
            width = layer["outputs"]
    return out


def initial_parameters(layers, width, seed):
    """float32 start values, non-degenerate on purpose: transforms U(+-1/sqrt(fan_out)), GCNII W = N(0, 1) / 6 (the reference's zero
    init makes M a multiple of the identity), every bias U(+-0.1)."""
    rng = np.random.default_rng(seed)
    out = []
    for shape, _, role in variables(layers, width):
        if role == "W":
            out.append(rng.uniform(-1, 1, size=shape) / math.sqrt(shape[1]))
        elif role == "M":
            out.append(rng.standard_normal(shape) / 6)
        else:
            out.append(rng.uniform(-0.1, 0.1, size=shape))
    return [p.astype(np.float32) for p in out]


# ---- the reference -------------------------------------------------------------------------------------------------------------------
class Reference:
    """``task``: ("node", nodes, labels) -- mean cross entropy of log_softmax(out[nodes]) (graph_predictor.py:24-25) -- or
    ("link", edges, labels, "diff" | "bce") over a fixed edge list (orc.link_loss_diff / orc.link_loss_bce state the meaning)."""

    def __init__(self, layers, coo, vals, shape, X, parameters, task, weight_decay, seed, fixed=None, mistake=None, dtype=torch.float64):
        if mistake is not None and mistake not in MISTAKES:
            raise Exception("unknown mistake " + str(mistake))
        self.layers, self.coo, self.vals, self.shape = layers, np.asarray(coo), np.asarray(vals), tuple(shape)
        self.task, self.weight_decay, self.seed, self.fixed, self.mistake, self.dtype = task, weight_decay, int(seed), fixed, mistake, dtype
        self.X = torch.from_numpy(np.asarray(X, dtype=np.float64)).to(dtype)
        self.parameters = [torch.from_numpy(np.asarray(p, dtype=np.float64)).to(dtype).requires_grad_() for p in parameters]
        self.regularize = [r for _, r, _ in variables(layers, self.X.shape[1])]
        assert [tuple(p.shape) for p in self.parameters] == [s for s, _, _ in variables(layers, self.X.shape[1])]
        self.streams = 0                                 # the reference's own count of the mask streams drawn so far
        self._constant = dict()
        self.bipartite = self._bipartite()               # gcn.py:127: once, when the layers are built
        self.seen = dict()                               # what the last forward saw: pre-activations per gated layer, NGCF row norms

    # -- adjacencies ------------------------------------------------------------------------------------------------------------------
    def _dense(self, ai, av):
        return torch.from_numpy(orc.to_dense(ai, av, self.shape, dtype=np.float64)).to(self.dtype)

    def _bipartite(self):
        if self.mistake == "bipartite_row_sums":
            raw = orc.to_dense(self.coo, self.vals, self.shape, dtype=np.float64)
            sums = raw.sum(axis=1)
            D = np.divide(1.0, sums, out=np.zeros_like(sums), where=sums != 0)
            return torch.from_numpy(D[:, None] * raw).to(self.dtype)
        return self._dense(*orc.get_adjacency(self.coo, self.vals, self.shape, normalized="bipartite", training=False, dtype=np.float64))

    def _adjacency(self, graph_dropout, stream):
        """gnn.py:36-50: dropped per stored entry and re-normalised under ``stream``; the constant adjacency where stream is None."""
        if stream is None:
            if "symmetric" not in self._constant:
                self._constant["symmetric"] = self._dense(*orc.get_adjacency(self.coo, self.vals, self.shape, training=False, dtype=np.float64))
            return self._constant["symmetric"]
        return self._dense(*orc.get_adjacency(self.coo, self.vals, self.shape, graph_dropout=graph_dropout, training=True, seed=self.seed,
                                              stream=stream, dtype=np.float64))

    # -- streams and masks ------------------------------------------------------------------------------------------------------------
    def _draw(self):
        stream = self.streams
        self.streams += 1
        if self.mistake == "stream_off_by_one" and not self._shifted:
            self._shifted = True
            return stream + 1
        return stream

    def _layer_streams(self, layer, training):
        """(the adjacency's stream, the feature mask's stream) of a layer, None where it draws none: the adjacency's first."""
        rate = layer.get("rate", 0)
        wants_adjacency = training and layer.get("graph_dropout", 0) != 0
        wants_mask = training and layer.get("mask") == "counter" and 0 < rate < 1
        if self.mistake == "mask_stream_first":
            mask = self._draw() if wants_mask else None
            return (self._draw() if wants_adjacency else None), mask
        adjacency = self._draw() if wants_adjacency else None
        return adjacency, (self._draw() if wants_mask else None)

    def _drop(self, H, layer, training, stream):
        rate = layer.get("rate", 0)
        if not training or rate == 0:
            return H
        if layer["mask"] == "counter":
            mask = counter_mask(tuple(H.shape), rate, self.seed, stream)
            if self.mistake == "no_dropout_scale":
                mask = (mask != 0).astype(np.float64)
        else:
            mask = self.fixed.mask(tuple(H.shape), rate)
            if self.mistake == "no_dropout_scale":
                mask = mask * (1.0 - rate)
        return H * torch.from_numpy(mask).to(self.dtype)

    # -- the forward ------------------------------------------------------------------------------------------------------------------
    def forward(self, training):
        """The model's output and the sum of the layers' output penalties; ``self.values`` holds every layer's value."""
        self._shifted = False
        self.seen = dict(gates=[], norms=[])
        double = 1.0 if self.mistake == "no_doubling" else 2.0
        params = iter(self.parameters)
        H, values, penalty = self.X, [], 0.0
        for layer in self.layers:
            kind = layer["kind"]
            adjacency_stream, mask_stream = self._layer_streams(layer, training)
            if kind == "dropout":
                H = self._drop(H, layer, training, mask_stream)
            elif kind == "dense":
                W, b = next(params), next(params)
                pre = H @ W + b
                if layer["act"] == "relu":
                    self.seen["gates"].append(pre.detach())
                    pre = torch.relu(pre)
                H = self._drop(pre, layer, training, mask_stream)
            elif kind == "gcn":
                W, b = next(params), next(params)
                A = self._adjacency(layer["graph_dropout"], adjacency_stream)
                pre = (A @ H) @ W + b
                self.seen["gates"].append(pre.detach())
                if layer["spectral"]:
                    H = double * self._drop(torch.relu(pre) - b, layer, training, mask_stream)
                else:
                    H = self._drop(torch.relu(pre), layer, training, mask_stream)
            elif kind == "gcnii":
                W = next(params)
                bias = next(params) if layer["spectral"] else None
                A = self._adjacency(layer["graph_dropout"], adjacency_stream)
                k = layer["k"]
                beta = math.log1p(layer["l"] / (k if self.mistake == "beta_k" and k > 0 else k + 1))    # (planted from k = 1 on: l / 0)
                M =(1 - beta) * torch.eye(W.shape[1], dtype=self.dtype) + beta * W
                T = (1 - layer["a"]) * (A @ H) + layer["a"] * values[layer["h0"]]
                if layer["spectral"]:
                    pre = T @ M + bias
                    self.seen["gates"].append(pre.detach())
                    H = double * self._drop(torch.relu(pre) - bias, layer, training, mask_stream)
                else:
                    pre = T @ M
                    self.seen["gates"].append(pre.detach())
                    H = self._drop(torch.relu(pre), layer, training, mask_stream)
            elif kind == "ngcf":
                W1, W2, b1, b2 = next(params), next(params), next(params), next(params)
                aggregated = self.bipartite @ H
                pre1, pre2 = (H * aggregated) @ W1 + b1, aggregated @ W2 + b2
                self.seen["gates"] += [pre1.detach(), pre2.detach()]
                summed = torch.nn.functional.leaky_relu(pre1, LEAKY_SLOPE) + torch.nn.functional.leaky_relu(pre2, LEAKY_SLOPE)
                dropped = self._drop(summed, layer, training, mask_stream)
                squares = (dropped * dropped).sum(dim=1, keepdim=True)
                self.seen["norms"].append(squares.detach())
                H = dropped / torch.sqrt(torch.clamp(squares, min=1e-12))            # tf.math.l2_normalize
                if self.mistake != "no_output_penalty":
                    penalty = penalty + layer["penalty"] * (H * H).sum() / 2            # layered.py:83-86
            elif kind == "concatenate":
                H = torch.cat([values[i] for i in layer["sources"]], dim=1 if self.mistake == "concatenate_axis_1" else 0)
            values.append(H)
        self.values = values
        return H, penalty

    def task_loss(self, out):
        if self.task[0] == "node":
            _, nodes, labels = self.task
            logp = torch.log_softmax(out[torch.from_numpy(np.asarray(nodes))], dim=1)
            return -logp[torch.arange(len(nodes)), torch.from_numpy(np.asarray(labels))].mean()
        _, edges, labels, form = self.task
        edges = torch.from_numpy(np.asarray(edges, dtype=np.int64))
        if self.mistake == "concatenate_axis_1":          # an [n, 3 C] output has no row 3 n - 1: the ids wrap (the only reading there is)
            edges = edges % out.shape[0]
        z = (out[edges[:, 0]] * out[edges[:, 1]]).sum(dim=1)
        if form == "diff":                                 # graph_predictor.py:138-141
            return -torch.nn.functional.logsigmoid(z[0::2] - z[1::2]).mean()
        y = torch.from_numpy(np.asarray(labels, dtype=np.float64)).to(self.dtype)      # graph_predictor.py:142-146
        return (torch.clamp(z, min=0) - z * y + torch.log1p(torch.exp(-z.abs()))).mean()

    def step(self):
        """One training-mode evaluation of the objective and its gradients: (loss, [gradient per variable]) as float64 numpy."""
        for p in self.parameters:
            p.grad = None
        out, total = self.forward(training=True)
        total = total + self.task_loss(out)
        for p, regularize, layer_last in zip(self.parameters, self.regularize, self._of_last_dense()):
            if self.mistake == "last_dense_decayed" and layer_last:
                regularize = 1.0
            if regularize != 0:
                total = total + self.weight_decay * regularize * (p * p).sum() / 2
        total.backward()
        self.loss = float(total.detach())
        return self.loss, [p.grad.detach().numpy().astype(np.float64) for p in self.parameters]

    def _of_last_dense(self):
        flags = []
        for layer in self.layers:
            count = {"dense": 2, "gcn": 2, "ngcf": 4, "gcnii": 2 if layer.get("spectral") else 1}.get(layer["kind"], 0)
            flags += [bool(layer.get("last"))] * count
        return flags

    def evaluate(self):
        """An eval-mode forward: draws no stream."""
        with torch.no_grad():
            return self.forward(training=False)[0].numpy().astype(np.float64)

    def update(self, step_size=STEP_SIZE):
        with torch.no_grad():
            for p in self.parameters:
                p -= step_size * p.grad

    def run(self):
        """A case: a training step, an eval forward, a training step, with a plain gradient step after each training step.
        Returns [(loss, gradients)] of the two steps and the stream count after each of the three phases."""
        results, counts = [], []
        for phase in ("step", "eval", "step"):
            if phase == "eval":
                self.evaluate()
            else:
                results.append(self.step())
                self.update()
            counts.append(self.streams)
        return results, counts

    # -- the input conditions -----------------------------------------------------------------------------------------------------------
    def gate_shares(self):
        """Per relu / leaky-relu pre-activation of the last forward: the share of elements with |x| <= 1e-5 max|x|."""
        return [float((g.abs() <= 1e-5 * g.abs().max()).double().mean()) for g in self.seen["gates"]]

    def smallest_squared_norm(self):
        return min((float(s.min()) for s in self.seen["norms"]), default=float("inf"))


def ratio_to_bar(got, want):
    """max |got - want| / (GRAD_RTOL |want| + GRAD_ATOL max|want|): at most 1 where np.testing.assert_allclose(rtol, atol) passes.
    (In units of the bar every case but NGCF's is held to; a case's own bar is ``case["bar"]`` of these units.)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / (GRAD_RTOL * np.abs(want) + GRAD_ATOL * np.abs(want).max())).max())


def loss_ratio_to_bar(got, want):
    return abs(got - want) / (LOSS_RTOL * abs(want))


# ---- the inputs of tests/test_gpu_model_steps.py ---------------------------------------------------------------------------------------
N, HUB, EMPTY_TILE, CLASSES, WEIGHT_DECAY, SEED = 800, 7, (320, 336), 5, 5e-3, 17


def graph():
    """One graph for all cases: a symmetrised R-MAT body, one hub vertex with more than 512 neighbours (both directions), the 16 vertices
    of one row tile without entries, and 300 entries stored twice with another value on the second copy (dropout acts per stored
    entry; the copies also make row sums and column sums differ)."""
    coo, vals, shape = graphs.rmat_symmetric_coo(N, 5000, seed=3)
    rng = np.random.default_rng(8)
    others = rng.permutation(np.setdiff1d(np.arange(N), [HUB]))[:600]
    spokes = np.stack([np.full(600, HUB), others], axis=1)
    key = np.unique(np.concatenate([coo[:, 0] * N + coo[:, 1], spokes[:, 0] * N + spokes[:, 1], spokes[:, 1] * N + spokes[:, 0]]))
    coo = np.stack([key // N, key % N], axis=1).astype(np.int64)
    inside = lambda v: (v >= EMPTY_TILE[0]) & (v < EMPTY_TILE[1])
    coo = coo[~inside(coo[:, 0]) & ~inside(coo[:, 1])]
    coo = coo[rng.permutation(len(coo))]
    twice = coo[:300]
    coo = np.concatenate([coo, twice])
    vals = np.concatenate([np.ones(len(coo) - 300, dtype=np.float32), np.full(300, 0.5, dtype=np.float32)])
    return coo, vals, (N, N)


def features(width, seed=5):
    return np.random.default_rng(seed + width).standard_normal((N, width)).astype(np.float32)


def node_task():
    rng = np.random.default_rng(6)
    nodes = np.concatenate([[HUB], np.arange(EMPTY_TILE[0], EMPTY_TILE[0] + 4), rng.permutation(N)[:300]])
    return ("node", nodes, rng.integers(0, CLASSES, size=len(nodes)))


def link_task(form, blocks=3):
    """200 (positive, negative) pairs of edges over the rows of all ``blocks`` stacked layer outputs, so that every layer's variables
    get a gradient from the task (the output penalty of a normalised row is a constant)."""
    rng = np.random.default_rng(9)
    edges = rng.integers(0, blocks * N, size=(400, 2))
    edges[1::2, 0] = edges[0::2, 0]                         # a pair shares its source, as negative_sampling lays it out
    return ("link", edges, np.tile([1, 0], 200), form)


# ---- the cases: a model as its constructor builds it, the switches on it, and what the switches change in the meaning ------------------
def _case(model, layers, width, task, options=None, build=None, entries=(), absent=()):
    """``model``: the class; ``build``: further constructor arguments (``layer_type`` by name); ``options``: the GNN switches;
    ``entries`` / ``absent``: library entries a case must / must not call (a switch that fell back would pass as the composed path)."""
    return dict(model=model, layers=layers, width=width, task=task, options=dict(options or {}), build=dict(build or {}),
                entries=tuple(entries), absent=tuple(absent))


def cases():
    node = node_task()
    GCN = dict(latent_dims=[64, 64])
    GCNII = dict(latent_dims=[32], iterations=4)
    gcn_plain = lambda **kw: gcn(CLASSES, (64, 64), **kw)
    gcn_spec = lambda **kw: gcn(CLASSES, (64, 64), spectral=True, **kw)
    gcnii_of = lambda **kw: gcnii(CLASSES, latent_dims=(32,), iterations=4, **kw)
    spectral = dict(layer_type="GCNSpectralPreservingLayer")
    # (a rate of 0.4: at the class's 0.6 the doubled survivors spread the pre-activations so far that 1.05e-3 of them lie within 1e-5 of
    # their layer's largest -- above what the gate condition of tests/test_model_step_ref_cpu.py admits)
    spectral_ii = dict(layer_type="GCNIISpectralPreservingLayer", dropout=0.4)
    gcn_backs, spectral_step = ("gnx_gcn_step_back", "gnx_gcn_step_back_dropped"), ("gnx_step_spectral_gcn", "gnx_gcnii_spectral_back")
    fd = dict(feature_dropout="fused")
    out = {
        # GCN: the 40 -> 64 layer gathers at the feature width and stays composed (torch's mask); 64 -> 64 and 64 -> classes fuse
        "gcn": _case("GCN", gcn_plain(), 40, node, build=GCN, absent=("gnx_gcn_step",)),
        "gcn-transform_first": _case("GCN", gcn_plain(), 40, node, build=dict(GCN, transform_first=True)),
        "gcn-fused": _case("GCN", gcn_plain(counter=(1,)), 40, node, dict(fd, gcn_layer="fused", gcn_backward="composed"), GCN,
                           entries=("gnx_gcn_step",), absent=gcn_backs),
        "gcn-fused-back": _case("GCN", gcn_plain(counter=(1,)), 40, node, dict(fd, gcn_layer="fused", gcn_backward="fused"), GCN,
                                entries=("gnx_gcn_step",) + gcn_backs),
        "gcn-spectral": _case("GCN", gcn_spec(), 40, node, build=dict(GCN, **spectral)),
        "gcn-spectral-fused": _case("GCN", gcn_spec(counter=(1,)), 40, node, dict(gcn_spectral="fused", gcn_backward="composed"),
                                    dict(GCN, **spectral), entries=spectral_step, absent=gcn_backs),
        "gcn-spectral-fused-back": _case("GCN", gcn_spec(counter=(1,)), 40, node, dict(gcn_spectral="fused", gcn_backward="fused"),
                                         dict(GCN, **spectral), entries=spectral_step + gcn_backs),
        # GCNII
        "gcnii": _case("GCNII", gcnii_of(), 40, node, build=GCNII, absent=("gnx_gcnii_step_drop", "gnx_gcnii_step_back", "gnx_dense_drop")),
        "gcnii-drop": _case("GCNII", gcnii_of(mask="counter"), 40, node, dict(fd, gcnii_backward="composed"), GCNII,
                            entries=("gnx_gcnii_step_drop",), absent=("gnx_gcnii_step_back",)),
        "gcnii-drop-back": _case("GCNII", gcnii_of(mask="counter"), 40, node, dict(fd, gcnii_backward="fused"), GCNII,
                                 entries=("gnx_gcnii_step_drop", "gnx_gcnii_step_back"), absent=("gnx_gcnii_wgrad",)),
        "gcnii-drop-back-recomputed": _case("GCNII", gcnii_of(mask="counter"), 40, node,
                                            dict(fd, gcnii_backward="fused", gcnii_weight_gradient="recomputed"), GCNII,
                                            entries=("gnx_gcnii_step_drop", "gnx_gcnii_step_back", "gnx_gcnii_wgrad"), absent=("gnx_dense_drop",)),
        "gcnii-drop-back-recomputed-dense": _case("GCNII", gcnii_of(mask="counter", input_mask="counter"), 40, node,
                                                  dict(fd, gcnii_backward="fused", gcnii_weight_gradient="recomputed", dense_dropout="fused"),
                                                  GCNII, entries=("gnx_gcnii_step_drop", "gnx_gcnii_step_back", "gnx_gcnii_wgrad",
                                                                  "gnx_dense_drop", "gnx_dense_wgrad_drop")),
        "gcnii-spectral": _case("GCNII", gcnii_of(spectral=True, dropout=0.4), 40, node, build=dict(GCNII, **spectral_ii)),
        "gcnii-spectral-fused": _case("GCNII", gcnii_of(spectral=True, dropout=0.4, mask="counter"), 40, node, dict(gcnii_spectral="fused"),
                                      dict(GCNII, **spectral_ii), entries=("gnx_gcnii_step_spectral", "gnx_gcnii_spectral_back")),
        # GCNIILayer(..., graph_dropout=0.5), the layer's own default: a stack added by hand, as the GCNII constructor lays it out
        "gcnii-edge": _case("stack", gcnii_of(graph_dropout=0.5), 40, node, build=GCNII,
                            absent=("gnx_gcnii_step_dropped", "gnx_gcnii_step_back_dropped")),
        "gcnii-edge-fused": _case("stack", gcnii_of(graph_dropout=0.5, mask="counter"), 40, node,
                                  dict(fd, gcnii_edge_dropout="fused", gcnii_backward="fused"), GCNII,
                                  entries=("gnx_gcnii_step_dropped", "gnx_gcnii_step_back_dropped")),
        # NGCF
        "ngcf": _case("NGCF", ngcf(16, dropout=0.25), 16, link_task("diff"), build=dict(dropout=0.25), absent=("gnx_ngcf_step",)),
        "ngcf-fused": _case("NGCF", ngcf(16, dropout=0.25), 16, link_task("bce"), dict(ngcf_layer="fused"), dict(dropout=0.25),
                            entries=("gnx_ngcf_step", "gnx_ngcf_back_gate"), absent=("gnx_step_back_ngcf",)),
        "ngcf-fused-drop": _case("NGCF", ngcf(16, dropout=0.25, mask="counter"), 16, link_task("diff"),
                                 dict(fd, ngcf_layer="fused", ngcf_backward="composed"), dict(dropout=0.25),
                                 entries=("gnx_ngcf_step", "gnx_ngcf_back_gate"), absent=("gnx_step_back_ngcf",)),
        "ngcf-fused-drop-back": _case("NGCF", ngcf(16, dropout=0.25, mask="counter"), 16, link_task("diff"),
                                      dict(fd, ngcf_layer="fused", ngcf_backward="fused"), dict(dropout=0.25),
                                      entries=("gnx_ngcf_step", "gnx_step_back_ngcf")),
        "ngcf-wide": _case("NGCF", ngcf(128, dropout=0.25), 128, link_task("diff"),
                           dict(ngcf_layer="fused", ngcf_wide="fused", ngcf_wide_backward="fused"), dict(dropout=0.25),
                           entries=("gnx_step_wide_ngcf", "gnx_step_back_wide_ngcf")),
        "ngcf-wide-drop": _case("NGCF", ngcf(128, dropout=0.25, mask="counter"), 128, link_task("bce"),
                                dict(fd, ngcf_layer="fused", ngcf_wide="fused", ngcf_wide_backward="fused"), dict(dropout=0.25),
                                entries=("gnx_step_wide_ngcf", "gnx_step_back_wide_ngcf")),
    }
    for name, case in out.items():
        case["bar"] = 4 * FLOAT32_YARDSTICK[name] if name in FLOAT32_YARDSTICK else 1.0
    return out


# The composed default of NGCF misses the gradient bar, and so does this reference evaluated in float32 on the CPU against itself in
# float64: NGCF(output_regularize=1) adds sum(value^2) / 2 of l2-normalised rows to the objective -- a constant, whose gradient is
# exactly zero -- and in float32 the backward of the normalisation leaves a cancellation residue of about 2^-24 / |row| per element in
# its place, summed over 2 400 rows into gradients of 1e-3 ... 1e-2.  Without the penalty the same float32 evaluation is within 0.01 x
# the bar.  So the yardstick for NGCF is that float32 evaluation: its worst gradient error over the two steps in units of the bar
# (GRAD_RTOL, GRAD_ATOL), measured on the CPU per meaning (cases that differ in a switch alone share it) and written here; a case's
# gradient bar is four times it.  The loss bar stays LOSS_RTOL.  tests/test_model_step_ref_cpu.py measures it again.
FLOAT32_YARDSTICK = {"ngcf": 2.857, "ngcf-fused": 18.453, "ngcf-fused-drop": 4.294, "ngcf-fused-drop-back": 4.294, "ngcf-wide": 5.348,
                     "ngcf-wide-drop": 22.504}


def reference_for(case, mistake=None, dtype=torch.float64, fixed_seed=23, parameters=None):
    """The Reference of a case over the shared inputs (what the GPU test builds its model from as well)."""
    coo, vals, shape = graph()
    X = features(case["width"])
    if parameters is None:
        parameters = initial_parameters(case["layers"], case["width"], seed=31)
    return Reference(case["layers"], coo, vals, shape, X, parameters, case["task"], WEIGHT_DECAY, SEED, fixed=FixedMasks(fixed_seed),
                     mistake=mistake, dtype=dtype)
