"""Runs the reference project's own classes on the TensorFlow stand-in (oracle/tf_standin) and writes what they compute as fixtures:

    python tests/golden/make_reference_golden.py [OUTPUT DIRECTORY, default: this one]

The reference tree is read from GNX_REFERENCE_DIR (default /root/reference) and imported UNMODIFIED in a child process: its package
is called ``gnntf`` as this project's is, so the child's sys.path holds the stand-in, the reference, the repository root and tests/
(for ``oracle`` and the *_ref helpers that the mask provider needs) and never ``gnn-tf_amd``.  Nothing of the reference's text is
written anywhere: the fixtures (reference_<case>.npz, split into .partK.npz where one file would pass the size of the largest fixture
committed before them) hold arrays and scalars only -- inputs or their digests (tests/reference_cases.py makes the inputs on every
side), float64 outputs, and the recorded dropout calls.

What the reference decides here: composition, call order, constants, axes, regularisation.  What stays our reading: the meaning of
each TensorFlow op (documented per op in the stand-in), TensorFlow's RNG streams and initialisers (every case assigns its parameters;
masks come from this project's contract through the provider below), TensorFlow's own float32 roundings.

A training case runs the reference's ``train()`` itself for two epochs: its objective (trainable.py:70-78) is formed by its own text
inside the stand-in's tape.  ``train()`` takes the optimizer as an argument; the one handed in records the gradients and applies
``v -= 0.05 * grad``, and the validation predictor handed in records the eval forward between the two steps.

Dropout calls are recorded as rows (ordinal, kind, rows, columns, rate * 1e6, stream): kind 0 an edge mask (a 1-D call of length nnz:
orc.keep_mask under the next stream), 1 a counter-RNG feature mask (dense_drop_ref's, under the next stream), 2 a host-drawn feature
mask (model_step_ref.FixedMasks in call order, stream -1)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("GNX_REFERENCE_DIR", "/root/reference")


def main(argv):
    """The parent: one child process per run, with the search path spelled out."""
    out = os.path.abspath(argv[1]) if len(argv) > 1 else HERE
    if not os.path.isdir(os.path.join(REFERENCE, "gnntf")):
        raise SystemExit(f"no reference tree at {REFERENCE} (GNX_REFERENCE_DIR)")
    os.makedirs(out, exist_ok=True)
    # one thread and torch's processor-independent kernels: the same sums in the same order wherever this runs, so that a regeneration
    # can be compared with the committed files array for array (the stand-in itself keeps away from the vector math library and
    # the BLAS, whose code paths follow the processor whatever is set here; MKL_CBWR is kept for whatever else might reach them)
    env = dict(os.environ, GNX_REFERENCE_CHILD="1", PYTHONDONTWRITEBYTECODE="1", OMP_NUM_THREADS="1", MKL_NUM_THREADS="1",
               MKL_CBWR="COMPATIBLE", ATEN_CPU_CAPABILITY="default")
    env.pop("PYTHONPATH", None)
    return subprocess.run([sys.executable, "-s", "-B", os.path.abspath(__file__), out], env=env, cwd=ROOT).returncode     # -s: no user site-packages


# ======================================================================================================================================
# the child
# ======================================================================================================================================
def child(out):
    global np, torch, tf, rg, orc, ref, cases
    sys.path[:] = [os.path.join(ROOT, "oracle", "tf_standin"), REFERENCE, ROOT, os.path.join(ROOT, "tests")] + \
                  [p for p in sys.path if "gnn-tf_amd" not in p and os.path.abspath(p or ".") != HERE]
    import numpy as np
    import torch
    torch.set_num_threads(1)                                 # one thread: the same sums in the same order on every machine
    import tensorflow as tf
    import gnntf as rg                                       # the reference's package
    assert os.path.abspath(rg.__file__).startswith(os.path.abspath(REFERENCE)) and tf.__file__.startswith(ROOT), (rg.__file__, tf.__file__)
    from oracle import gnntf_oracle as orc
    import model_step_ref as ref
    import reference_cases as cases
    for stale in os.listdir(out):
        if stale.startswith("reference_") and stale.endswith(".npz"):
            os.remove(os.path.join(out, stale))
    adjacency(out)
    container(out)
    eval_forwards(out)
    for name in cases.step_meanings():
        training_steps(out, name)
    for name in sorted(cases.APPNP_STEP_KINDS):
        appnp_steps(out, name)
    gcniireg_steps(out)
    heads(out)
    measures(out)
    for name in sorted(os.listdir(out)):
        if name.startswith("reference_"):
            print(name, os.path.getsize(os.path.join(out, name)), "bytes")


def save(out, name, arrays):
    """reference_<name>.npz; where that would pass the size limit, the arrays go into .partK.npz files, each within it."""
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    path = os.path.join(out, f"reference_{name}.npz")
    np.savez_compressed(path, **arrays)
    if os.path.getsize(path) <= cases.LARGEST_FIXTURE:
        return
    os.remove(path)
    parts, current = [], dict()
    for key in sorted(arrays):
        trial = dict(current, **{key: arrays[key]})
        np.savez_compressed(path, **trial)
        if os.path.getsize(path) > cases.LARGEST_FIXTURE and current:
            parts.append(current)
            trial = {key: arrays[key]}
        current = trial
    os.remove(path)
    parts.append(current)
    for k, part in enumerate(parts):
        part_path = os.path.join(out, f"reference_{name}.part{k}.npz")
        np.savez_compressed(part_path, **part)
        assert os.path.getsize(part_path) <= cases.LARGEST_FIXTURE, (part_path, sorted(part))


class MaskProvider:
    """What tf.nn.dropout asks (the module docstring).  ``kinds``: per feature-dropout call of one training forward, whose mask it is."""

    def __init__(self, coo, seed, kinds=(), fixed=None):
        self.coo, self.seed, self.kinds, self.fixed = np.asarray(coo), int(seed), list(kinds), fixed
        self.streams, self.feature_calls, self.calls = 0, 0, []

    def __call__(self, ordinal, shape, rate):
        if len(shape) == 1:
            assert shape[0] == len(self.coo), (shape, len(self.coo))
            kind, stream = 0, self._draw()
            mask = orc.keep_mask(self.coo, rate, self.seed, stream).astype(np.float64) / (1.0 - rate)
        else:
            whose = self.kinds[self.feature_calls % len(self.kinds)]
            self.feature_calls += 1
            if whose == "counter":
                kind, stream = 1, self._draw()
                mask = ref.counter_mask(tuple(shape), rate, self.seed, stream)
            else:
                kind, stream = 2, -1
                mask = self.fixed.mask(tuple(shape), rate)
        self.calls.append((ordinal, kind, shape[0], shape[1] if len(shape) > 1 else 0, int(round(rate * 1e6)), stream))
        return mask

    def _draw(self):
        self.streams += 1
        return self.streams - 1

    def recorded(self):
        return np.asarray(self.calls, dtype=np.int64).reshape(-1, 6)


def sparse_graph(coo, vals, shape):
    return tf.SparseTensor(np.asarray(coo, dtype=np.int64), np.asarray(vals, dtype=np.float64), shape)


def assign(model, parameters):
    """The stated parameters, now and at every reset(): ``train()`` begins with one."""
    variables = model.vars()
    assert [tuple(v.var.shape) for v in variables] == [tuple(p.shape) for p in parameters], [tuple(v.var.shape) for v in variables]
    for v, p in zip(variables, parameters):
        v.reset = lambda v=v, p=p: v.assign(np.asarray(p, dtype=np.float64))
        v.reset()


def value(t):
    return t.numpy().astype(np.float64) if hasattr(t, "numpy") else np.asarray(t, dtype=np.float64)


# ---- adjacency ---------------------------------------------------------------------------------------------------------------------------
def adjacency(out):
    arrays = dict(rate=cases.ADJ_RATE, seed=cases.ADJ_SEED, emptied_column=cases.EMPTIED_COLUMN)
    for gname, (coo, vals, shape) in cases.adjacency_graphs().items():
        arrays[f"{gname}.coo"], arrays[f"{gname}.vals"], arrays[f"{gname}.n"] = coo.astype(np.int32), vals.astype(np.float16), shape[0]
        provider = MaskProvider(coo, cases.ADJ_SEED)
        tf.standin_configure(dtype="float64", provider=provider)
        model = rg.GNN(sparse_graph(coo, vals, shape), tf.zeros((shape[0], 1)))
        for mode in ("eval", "train"):
            model.training_mode(mode == "train")
            for normalized in cases.NORMALIZED:
                for add_eye in cases.ADD_EYE:
                    before = provider.streams
                    A = model.get_adjacency(graph_dropout=cases.ADJ_RATE, normalized=normalized, add_eye=add_eye)
                    key = f"{gname}.{mode}.{normalized}.{add_eye}"
                    arrays[key + ".indices"], arrays[key + ".values"] = A.indices.numpy().astype(np.int32), value(A.values)
                    arrays[key + ".stream"] = before if provider.streams > before else -1
        arrays[f"{gname}.calls"] = provider.recorded()
    save(out, "adjacency", arrays)


# ---- graph container -----------------------------------------------------------------------------------------------------------------------
def container(out):
    import networkx as nx
    tf.standin_configure(dtype="float64")
    arrays = dict()
    for name, (nodes, edges, weights, is_digraph, directed) in cases.container_graphs().items():
        G = nx.DiGraph() if is_digraph else nx.Graph()
        G.add_nodes_from(nodes)
        for k, (u, v) in enumerate(edges):
            G.add_edge(u, v, **({} if weights is None else {"weight": weights[k]}))
        A = rg.graph2adj(G, directed=directed)
        arrays[name + ".nodes"], arrays[name + ".edges"] = np.asarray(list(G), dtype=np.int32), np.asarray(list(G.edges()), dtype=np.int32)
        arrays[name + ".weights"] = np.asarray([d.get("weight", 1.0) for _, _, d in G.edges(data=True)], dtype=np.float16)
        arrays[name + ".directed"] = directed
        arrays[name + ".indices"], arrays[name + ".values"] = A.indices.numpy().astype(np.int32), value(A.values)
        arrays[name + ".n"] = A.dense_shape[0]
    save(out, "container", arrays)


# ---- models --------------------------------------------------------------------------------------------------------------------------------
def build_eval_model(name, G, X):
    layer = dict(layer_type=rg.GCNSpectralPreservingLayer) if name == "gcn-spectral" else \
        dict(layer_type=rg.GCNIISpectralPreservingLayer) if name == "gcnii-spectral" else dict()
    if name in ("appnp", "appnpreg"):
        cls = rg.APPNP if name == "appnp" else rg.APPNPReg
        return cls(G, X, ref.CLASSES, latent_dims=[cases.EVAL_LATENT], iterations=cases.APPNP_ITERATIONS)
    if name.startswith("gcnii-") or name == "gcnii":
        return rg.GCNII(G, X, ref.CLASSES, latent_dims=[cases.EVAL_LATENT], iterations=cases.EVAL_ITERATIONS, **layer)
    if name == "gcniireg":
        return rg.GCNIIReg(G, X, ref.CLASSES, latent_dims=[cases.EVAL_LATENT], iterations=cases.EVAL_ITERATIONS)
    if name.startswith("gcn"):
        return rg.GCN(G, X, ref.CLASSES, latent_dims=[64, 64], **layer)
    if name == "ngcf":
        return rg.NGCF(G, X, num_classes=16, dropout=0.25)
    if name == "pprsweep":
        model = rg.GNN(G, X)
        model.add(rg.PPRSweep())
        return model
    return rg.GNN(G, X, preprocessor=rg.Structural(dims=16, regularize=0, bipartite=100, l2_contraint=name.endswith("l2")))


def eval_forwards(out):
    coo, vals, shape = ref.graph()
    arrays = dict(graph=cases.digest(coo, vals))
    for name in cases.EVAL_MODELS:
        provider = MaskProvider(coo, ref.SEED)              # an eval forward asks for no mask: the record must stay empty
        tf.standin_configure(dtype="float64", provider=provider)
        X, parameters = cases.eval_inputs(name)
        model = build_eval_model(name, sparse_graph(coo, vals, shape), tf.constant(X.astype(np.float64)))
        assign(model, parameters)
        model.training_mode(False)
        arrays[name + ".out"] = value(model(model.features))
        arrays[name + ".X"] = X.astype(np.float16)
        for k, p in enumerate(parameters):
            arrays[f"{name}.p{k}"] = p.astype(np.float16)
        arrays[name + ".calls"] = provider.recorded()
        if name == "ngcf":                                   # the first layer's value: what orc.ngcf_layer_eval restates
            arrays[name + ".layer0"] = value(model.layers()[0].value)
    save(out, "eval", arrays)


class Recorder:
    """The optimizer handed to the reference's train(): keeps the gradients it is given and applies the plain step."""

    def __init__(self, provider):
        self.provider, self.gradients, self.marks = provider, [], []

    def apply_gradients(self, pairs):
        pairs = list(pairs)
        self.gradients.append([np.zeros(tuple(v.shape)) if g is None else value(g) for g, v in pairs])      # None: the objective does not reach v
        for g, v in pairs:
            if g is not None:
                v.assign(v - ref.STEP_SIZE * g)
        self.mark()

    def mark(self):
        self.marks.append((self.provider.streams, len(self.provider.calls)))


def two_steps(model, task, provider, weight_decay, prefix, keep_eval=True):
    """The reference's train() for two epochs -- a step, the update, an eval forward, a step (then an update and an eval forward that
    nothing reads) -- and what it went through: losses, gradients, the eval output, stream and call counts after the three phases."""
    recorder, seen = Recorder(provider), []

    class Validation(rg.Predictor):
        def loss(self, features):
            seen.append(value(features))
            recorder.mark()
            return task.loss(features)

    model.train(train=task, valid=Validation(), regularization=weight_decay, epochs=2, patience=10, optimizer=recorder)
    losses = tf.standin_tape_targets()
    assert len(losses) == 2 and len(recorder.gradients) == 2 and len(seen) == 2 and len(recorder.marks) == 4
    arrays = {prefix + "losses": np.asarray(losses, dtype=np.float64), prefix + "streams_after": np.asarray([m[0] for m in recorder.marks[:3]]),
              prefix + "calls_after": np.asarray([m[1] for m in recorder.marks[:3]]), prefix + "calls": provider.recorded()[:recorder.marks[2][1]]}
    for step, gradients in enumerate(recorder.gradients):
        for k, g in enumerate(gradients):
            arrays[f"{prefix}step{step}.g{k}"] = g
    if keep_eval:
        arrays[prefix + "eval"] = seen[0]
    return arrays


def build_step_model(case, G, X):
    build = {k: v for k, v in case["build"].items() if k in ("latent_dims", "iterations", "dropout", "layer_type")}
    if "layer_type" in build:
        build["layer_type"] = getattr(rg, build["layer_type"])
    if case["model"] == "GCN":
        return rg.GCN(G, X, ref.CLASSES, **build)
    if case["model"] == "GCNII":
        return rg.GCNII(G, X, ref.CLASSES, **build)
    if case["model"] == "NGCF":
        return rg.NGCF(G, X, num_classes=case["width"], **build)
    model = rg.GNN(G, X)                                    # "stack": the GCNII constructor's layout with the layers' own graph_dropout
    model.add(rg.Dropout(0.6))
    for width in build["latent_dims"]:
        model.add(rg.Dense(width, dropout=0, activation=tf.nn.relu))
    H0 = model.top_layer()
    for k in range(build["iterations"]):
        model.add(rg.GCNIILayer(H0, 0.1, 0.5, k, activation=tf.nn.relu, dropout=0.6, graph_dropout=0.5))
    model.add(rg.Dense(ref.CLASSES, dropout=0, regularize=False))
    return model


def task_of(task):
    if task[0] == "node":
        return rg.NodeClassification(task[1], task[2])
    return rg.LinkPrediction(task[1], np.asarray(task[2], dtype=np.float64), loss=task[3])


def both_precisions(make_model, make_task, make_provider, weight_decay, keep_eval=True, keep_float32=True):
    """The two steps in float64 and again in float32 (stored as float32; where ``keep_float32`` is off -- the 128-wide cases, whose
    gradients alone pass the size of a fixture -- as each gradient's error against the float64 run in units of the bar,
    model_step_ref.ratio_to_bar).  Both runs must have asked for the same dropout calls: one record serves both."""
    arrays, records = dict(), []
    for dtype, prefix in (("float64", ""), ("float32", "f32.")):
        provider = make_provider()
        tf.standin_configure(dtype=dtype, provider=provider)
        model = make_model()
        got = two_steps(model, make_task(), provider, weight_decay, prefix, keep_eval=keep_eval and dtype == "float64")
        records.append([got[prefix + k] for k in ("calls", "calls_after", "streams_after")])
        if dtype == "float32":
            got = {k: v for k, v in got.items() if not k.endswith(("calls", "calls_after", "streams_after"))}
            if not keep_float32:
                grads = sorted(k for k in got if ".g" in k)
                for step in (0, 1):
                    mine = sorted((k for k in grads if k.startswith(f"f32.step{step}.g")), key=lambda k: int(k.rsplit("g", 1)[1]))
                    got[f"f32.step{step}.ratio"] = np.asarray([ref.ratio_to_bar(got[k], arrays[k[4:]]) for k in mine], dtype=np.float64)
                got = {k: v for k, v in got.items() if k not in grads}
            got = {k: (v.astype(np.float32) if v.dtype == np.float64 and not k.endswith("ratio") else v) for k, v in got.items()}
        arrays.update(got)
    assert all(np.array_equal(a, b) for a, b in zip(*records)), "the float32 run asked for other dropout calls than the float64 run"
    return arrays


def training_steps(out, name):
    case = ref.cases()[name]
    coo, vals, shape = ref.graph()
    X, parameters = ref.features(case["width"]), ref.initial_parameters(case["layers"], case["width"], seed=31)

    def make_model():
        model = build_step_model(case, sparse_graph(coo, vals, shape), tf.constant(X.astype(np.float64)))
        assign(model, parameters)
        return model

    arrays = both_precisions(make_model, lambda: task_of(case["task"]),
                             lambda: MaskProvider(coo, ref.SEED, cases.feature_mask_kinds(case["layers"]), ref.FixedMasks(23)),
                             ref.WEIGHT_DECAY, keep_eval=case["width"] <= 64, keep_float32=case["width"] <= 64)
    arrays["inputs"] = cases.digest(coo, vals, X, *parameters)
    save(out, "step_" + name, arrays)


def gcniireg_steps(out):
    """GCNIIReg: FastReg creates its projection vector inside every forward, so the reference's variable list grows (the second
    step's gradients end with those of the two vectors the first step's and the eval forward made) and the vector is the zeros a new
    variable holds."""
    import signal_ref
    g = cases.GCNIIREG_STEP
    coo, vals, shape = ref.graph()
    layers = signal_ref.gcniireg_layers(ref.CLASSES, g["latent_dims"], g["iterations"])
    X, parameters = ref.features(g["width"]), ref.initial_parameters(layers, g["width"], seed=31)
    made = []

    def make_model():
        model = rg.GCNIIReg(sparse_graph(coo, vals, shape), tf.constant(X.astype(np.float64)), ref.CLASSES, latent_dims=list(g["latent_dims"]),
                            iterations=g["iterations"])
        assign(model, parameters)
        made.append(model)
        return model

    arrays = both_precisions(make_model, lambda: task_of(ref.node_task()),
                             lambda: MaskProvider(coo, ref.SEED, cases.feature_mask_kinds(layers), ref.FixedMasks(23)), ref.WEIGHT_DECAY)
    arrays["inputs"] = cases.digest(coo, vals, X, *parameters)
    arrays["variables_after"] = len(made[0].vars())
    arrays["projections"] = np.stack([value(v.var).reshape(-1) for v in made[0].vars()[len(parameters):]])
    save(out, "step_gcniireg", arrays)


def appnp_steps(out, name):
    c = cases.APPNP_STEP
    coo, vals, shape, X, nodes, labels, parameters = cases.appnp_step_inputs()

    def make_model():
        model = rg.APPNP(sparse_graph(coo, vals, shape), tf.constant(X.astype(np.float64)), num_classes=c["classes"], a=c["a"],
                         latent_dims=[c["hidden"]], iterations=c["K"])
        assign(model, parameters)
        return model

    arrays = both_precisions(make_model, lambda: rg.NodeClassification(nodes, labels),
                             lambda: MaskProvider(coo, c["seed"], cases.APPNP_STEP_KINDS[name], ref.FixedMasks(c["mask_seed"])), c["weight_decay"])
    arrays["inputs"] = cases.digest(coo, vals, X, nodes, labels, *parameters)
    save(out, "step_" + name, arrays)


# ---- heads ---------------------------------------------------------------------------------------------------------------------------------
def heads(out):
    tf.standin_configure(dtype="float64")
    arrays = dict()
    for C in cases.NODE_WIDTHS:
        logits, nodes, labels = cases.node_head_inputs(C)
        task, L = rg.NodeClassification(nodes, labels), tf.constant(logits.astype(np.float64))
        key = f"node{C}."
        arrays[key + "logits"], arrays[key + "nodes"], arrays[key + "labels"] = logits.astype(np.float16), nodes.astype(np.int32), labels.astype(np.int32)
        arrays[key + "loss"], arrays[key + "predict"], arrays[key + "evaluate"] = value(task.loss(L)), task.predict(L).numpy(), float(task.evaluate(L))
    for C in cases.LINK_WIDTHS:
        F, edges, labels, r = cases.link_head_inputs(C)
        Ft = tf.constant(F.astype(np.float64))
        key = f"link{C}."
        arrays[key + "F"], arrays[key + "edges"], arrays[key + "labels"], arrays[key + "r"] = F.astype(np.float16), edges.astype(np.int32), labels, r.astype(np.float16)
        for similarity in ("dot", "cos"):
            for form in ("diff", "bce"):
                for weighted in (False, True):
                    holder = None
                    if weighted:                             # the DistMult weights: a variable of the architecture the task is given
                        holder = rg.Layered((cases.ref.N, C))
                    task = rg.LinkPrediction(edges, labels.astype(np.float64), gnn=holder, similarity=similarity, loss=form)
                    if weighted:
                        holder.vars()[-1].assign(r.astype(np.float64))
                    tag = f"{key}{similarity}.{form}.{'r' if weighted else 'plain'}."
                    arrays[tag + "loss"] = value(task.loss(Ft))
                    if form == "diff":
                        arrays[tag + "predict"] = value(task.predict(Ft)).reshape(-1)
                        arrays[tag + "logits"] = value(task.predict(Ft, to_logits=True)).reshape(-1)
    save(out, "heads", arrays)


# ---- measures ------------------------------------------------------------------------------------------------------------------------------
def measures(out):
    tf.standin_configure(dtype="float64")
    arrays = dict()
    for k, (labels, scores) in enumerate(cases.measure_inputs()):
        arrays[f"m{k}.labels"], arrays[f"m{k}.scores"] = labels, scores
        arrays[f"m{k}.auc"] = float(rg.auc(labels, scores))
        for name in ("avprec", "rec", "prec", "f1"):
            arrays[f"m{k}.{name}"] = np.asarray([float(getattr(rg, name)(labels, scores, top)) for top in (1, 5, 10)], dtype=np.float64)
    rng = np.random.default_rng(2)
    predictions, labels = rng.integers(0, 4, size=50), rng.integers(0, 4, size=50)
    arrays["acc.predictions"], arrays["acc.labels"] = predictions, labels
    arrays["acc"] = float(rg.acc(tf.constant(predictions), labels))
    save(out, "measures", arrays)


if __name__ == "__main__":
    if os.environ.get("GNX_REFERENCE_CHILD") == "1":
        child(sys.argv[1])
    else:
        raise SystemExit(main(sys.argv))
