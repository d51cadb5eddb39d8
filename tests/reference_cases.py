"""The inputs of the reference fixtures (tests/golden/reference_*.npz), written once: tests/golden/make_reference_golden.py feeds them to
the reference project's own classes, tests/test_reference_golden_cpu.py to this project's restatements and
tests/test_gpu_reference_golden.py to the HIP path.  numpy (and through tests/model_step_ref.py CPU torch) only: imports without a GPU,
without the package and without the reference.  Every fixture stores its inputs, or a digest of those that the three sides make with
the same code here, so a drift of a generator shows as a failed digest and not as a wrong figure."""
import glob
import math
import os

import numpy as np

import graphs
import model_step_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LARGEST_FIXTURE = 821622                                  # bytes: arxiv_mini_gcn.npz, the largest fixture before these


def f16(x):
    """Rounded to float16-representable values (stored compactly and exactly), as float32."""
    return np.asarray(x, dtype=np.float16).astype(np.float32)


def digest(*arrays):
    """float64 [sum, sum of squares, size] per array: what a fixture keeps of inputs that both sides generate."""
    return np.array([[float(np.asarray(a, dtype=np.float64).sum()), float((np.asarray(a, dtype=np.float64) ** 2).sum()), np.asarray(a).size]
                     for a in arrays], dtype=np.float64)


def load(name):
    """All arrays of fixture ``name``: reference_<name>.npz and, where one file would pass the size limit, its .partK.npz siblings."""
    paths = sorted(glob.glob(os.path.join(GOLDEN, f"reference_{name}.npz")) + glob.glob(os.path.join(GOLDEN, f"reference_{name}.part*.npz")))
    if not paths:
        raise FileNotFoundError(f"no fixture reference_{name}")
    out = dict()
    for path in paths:
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


# ---- adjacency -------------------------------------------------------------------------------------------------------------------------
NORMALIZED, ADD_EYE, ADJ_RATE, ADJ_SEED, EMPTIED_COLUMN = ("symmetric", "bipartite", "none"), ("none", "before", "after"), 0.3, 1234, 17


def adjacency_graphs():
    """The graph of dropout_masks.npz (96 vertices, 700 weighted entries, 30 % stored more than once, unordered), and the same with
    every entry of one column taken out: a column sum of 0, which divide_no_nan turns into a scale of 0."""
    coo, vals, shape = graphs.random_coo(96, 96, 700, seed=3, weighted=True, dup_frac=0.3)
    vals = f16(vals)
    stay = coo[:, 1] != EMPTIED_COLUMN
    return {"full": (coo, vals, shape), "emptied": (coo[stay], vals[stay], shape)}


# ---- graph container ---------------------------------------------------------------------------------------------------------------------
def container_graphs():
    """name -> (nodes in iteration order, edges in insertion order, weights or None, the graph is a DiGraph, graph2adj's ``directed``).
    Node names are not their positions; the DiGraph stores two arcs in both directions, so its symmetrised form holds entries twice."""
    nodes = [10, 3, 7, 42, 5, 8, 0]
    undirected = [(10, 3), (3, 7), (7, 42), (5, 10), (42, 42), (8, 3)]
    arcs = [(10, 3), (3, 10), (3, 7), (42, 7), (7, 42), (5, 8), (0, 0)]
    w_u, w_a = [0.5, 2.0, 1.25, 3.0, 0.75, 1.5], [0.5, 2.0, 1.25, 3.0, 0.75, 1.5, 4.0]
    return {"undirected": (nodes, undirected, None, False, False), "undirected-weighted": (nodes, undirected, w_u, False, False),
            "directed": (nodes, arcs, None, True, True), "directed-weighted": (nodes, arcs, w_a, True, True),
            "directed-symmetrised": (nodes, arcs, w_a, True, False)}


# ---- eval forwards -----------------------------------------------------------------------------------------------------------------------
EVAL_WIDTH, EVAL_LATENT, EVAL_ITERATIONS, APPNP_ITERATIONS = 40, 32, 4, 10
EVAL_MODELS = ("appnp", "appnpreg", "gcn", "gcn-spectral", "gcnii", "gcnii-spectral", "gcniireg", "ngcf", "pprsweep", "structural",
               "structural-l2")


def eval_layers(name):
    """The layer description (model_step_ref's) of an eval model, None where model_step_ref has none."""
    if name in ("gcn", "gcn-spectral"):
        return ref.gcn(ref.CLASSES, (64, 64), spectral=name.endswith("spectral"))
    if name in ("gcnii", "gcnii-spectral", "gcniireg"):
        return ref.gcnii(ref.CLASSES, latent_dims=(EVAL_LATENT,), iterations=EVAL_ITERATIONS, spectral=name.endswith("spectral"))
    if name == "ngcf":
        return ref.ngcf(16, dropout=0.25)
    return None


def eval_inputs(name):
    """(X, parameters in creation order), float16-exact float32.  appnp / appnpreg: Dense(40 -> 32, relu), Dense(32 -> classes);
    pprsweep: 7 feature columns, no parameter; structural: zero-width features, embeddings of 100 and 700 rows, 16 wide."""
    if name in ("appnp", "appnpreg"):
        layers = [dict(kind="dense", outputs=EVAL_LATENT, regularize=True), dict(kind="dense", outputs=ref.CLASSES, regularize=False)]
        return f16(ref.features(EVAL_WIDTH)), [f16(p) for p in ref.initial_parameters(layers, EVAL_WIDTH, seed=31)]
    if name == "pprsweep":
        return f16(ref.features(7)), []
    if name.startswith("structural"):
        rng = np.random.default_rng(12)
        return np.zeros((ref.N, 0), dtype=np.float32), [f16(rng.standard_normal((100, 16))), f16(rng.standard_normal((ref.N - 100, 16)))]
    width = 16 if name == "ngcf" else EVAL_WIDTH
    return f16(ref.features(width)), [f16(p) for p in ref.initial_parameters(eval_layers(name), width, seed=31)]


# ---- training steps ------------------------------------------------------------------------------------------------------------------------
def step_meanings():
    """One case name per distinct meaning of model_step_ref.cases() (test_gpu_model_steps.key_of), the first in sorted order."""
    from test_gpu_model_steps import key_of
    cases, seen, out = ref.cases(), set(), []
    for name in sorted(cases):
        if key_of(cases[name]) not in seen:
            seen.add(key_of(cases[name]))
            out.append(name)
    return out


def feature_mask_kinds(layers):
    """Per feature-dropout call of one training forward, in layer order: whose mask it is ("torch": host-drawn, "counter")."""
    return [layer["mask"] for layer in layers if layer.get("rate", 0) != 0]


APPNP_STEP = dict(n=600, F=40, hidden=16, classes=5, K=10, a=0.1, weight_decay=5e-4, seed=17, mask_seed=23)


def appnp_step_inputs():
    """The inputs of tests/test_gpu_training.py's whole-model step, with seeded parameters in place of the model's own draw."""
    c = APPNP_STEP
    coo, vals, shape = graphs.rmat_symmetric_coo(c["n"], 4000, seed=3)
    coo = np.concatenate([coo, coo[:300]])
    vals = np.concatenate([vals, np.full(300, 0.5, dtype=np.float32)])
    rng = np.random.default_rng(5)
    X = rng.standard_normal((c["n"], c["F"])).astype(np.float32)
    labels = rng.integers(0, c["classes"], size=c["n"])
    train = np.arange(0, 200)
    parameters = [(rng.uniform(-1, 1, size=(c["F"], c["hidden"])) / math.sqrt(c["hidden"])).astype(np.float32),
                  rng.uniform(-0.1, 0.1, size=(1, c["hidden"])).astype(np.float32),
                  (rng.uniform(-1, 1, size=(c["hidden"], c["classes"])) / math.sqrt(c["classes"])).astype(np.float32),
                  rng.uniform(-0.1, 0.1, size=(1, c["classes"])).astype(np.float32)]
    return coo, vals, shape, X, train, labels[train], parameters


# GCNIIReg(latent_dims=[64], iterations=2) on the graph, features and node task of the other steps (tests/signal_ref.py describes it)
GCNIIREG_STEP = dict(width=40, latent_dims=(64,), iterations=2)

APPNP_STEP_KINDS = {"appnp": ["torch", "torch"], "appnp-counter": ["counter", "counter"]}


# ---- heads ---------------------------------------------------------------------------------------------------------------------------------
NODE_WIDTHS, LINK_WIDTHS = (1, 7, 16, 40, 129), (1, 5, 16, 40, 128)


def node_head_inputs(C):
    """Logits [800, C] and 700 listed nodes with repeats, as test_gpu_dense.test_node_head draws them; one row holds its maximum twice."""
    rng = np.random.default_rng(8 + C)
    logits = f16(rng.standard_normal((ref.N, C)) * 3)
    nodes = rng.integers(0, ref.N, size=700)
    if C > 2:
        logits[nodes[0], :] = 0
        logits[nodes[0], [1, C - 1]] = 2.0
    return logits, nodes, rng.integers(0, C, size=700)


def link_head_inputs(C):
    """Features [800, C] scaled by 0.1, 1000 edges in (positive, negative) pairs, 0/1 labels, DistMult weights in [0.5, 1.5)."""
    rng = np.random.default_rng(14 + C)
    F = f16(rng.standard_normal((ref.N, C)) * 0.1)
    edges = rng.integers(0, ref.N, size=(1000, 2))
    r = f16(rng.random((C, 1)) + 0.5)
    labels = rng.integers(0, 2, size=1000).astype(np.float32)
    labels[:2] = [0, 1]
    return F, edges, labels, r


# ---- measures ------------------------------------------------------------------------------------------------------------------------------
def measure_inputs():
    """(labels, scores) pairs: random with distinct scores, with tied scores across the classes (the area under the curve sees them), a
    perfect and an inverted ranking, no positive among the best five.  The best five scores are distinct wherever the top-k measures
    read them: which of two equal scores an unstable sort puts first is no property of the measures."""
    rng = np.random.default_rng(3)
    out = []
    labels = (rng.random(60) < 0.3).astype(np.float64)
    out.append((labels, rng.random(60)))
    tied = np.round(rng.random(60) * 8) / 8
    tied[np.argsort(tied)[-6:]] += np.arange(6) * 1e-3
    out.append((labels, tied))
    out.append((labels, labels + 0.1 * rng.random(60)))
    out.append((labels, -labels + 0.1 * rng.random(60)))
    few = np.zeros(40)
    few[[3, 9]] = 1
    scores = rng.random(40)
    scores[[3, 9]] = -1 - np.arange(2)
    out.append((few, scores))
    return out
