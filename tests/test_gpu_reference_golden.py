"""The HIP path against what the reference project's OWN program text computes (tests/golden/reference_*.npz, recorded by
tests/golden/make_reference_golden.py on the TensorFlow stand-in; tests/test_reference_golden_cpu.py shows where they come from and
that this project's restatements agree with them to 1e-9).  Reads tests/golden/ only: neither the reference nor the stand-in is needed.

Bars: eval logits rtol 1e-4 (BASELINE.json) with the atol of the existing eval tests (1e-5; 1e-4 for the spectral-preserving layers,
as tests/test_gpu_dense.py holds them); normalised adjacency values rtol 1e-6; the two training steps at the bars of
tests/test_gpu_model_steps.py (LOSS_RTOL, GRAD_RTOL, GRAD_ATOL, NON_TRIVIAL, four times the float32 yardstick for NGCF) with the
``_mask_calls`` counts; the heads at the bars of tests/test_gpu_dense.py's test_node_head and test_link_head_edge_scores."""
import numpy as np
import pytest
import torch

import model_step_ref as ref
import reference_cases as cases
import test_gpu_model_steps as steps

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def assign(model, parameters):
    assert [tuple(v.var.shape) for v in model.vars()] == [tuple(p.shape) for p in parameters]
    for v, p in zip(model.vars(), parameters):
        v.assign(torch.from_numpy(np.asarray(p, dtype=np.float32)))


def worst(got, want, rtol, atol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, bar = np.abs(got - want), rtol * np.abs(want) + atol
    return float(np.where(err == 0, 0.0, err / np.where(bar == 0, np.finfo(np.float64).tiny, bar)).max())


# ---- eval logits -----------------------------------------------------------------------------------------------------------------------------
def build_eval_model(gnntf, name, graph, X):
    if name in ("appnp", "appnpreg"):
        cls = gnntf.APPNP if name == "appnp" else gnntf.APPNPReg
        return cls(graph, X, ref.CLASSES, latent_dims=[cases.EVAL_LATENT], iterations=cases.APPNP_ITERATIONS)
    if name in ("gcnii", "gcnii-spectral"):
        layer = dict(layer_type=gnntf.GCNIISpectralPreservingLayer) if name.endswith("spectral") else dict()
        return gnntf.GCNII(graph, X, ref.CLASSES, latent_dims=[cases.EVAL_LATENT], iterations=cases.EVAL_ITERATIONS, **layer)
    if name == "gcniireg":
        return gnntf.GCNIIReg(graph, X, ref.CLASSES, latent_dims=[cases.EVAL_LATENT], iterations=cases.EVAL_ITERATIONS)
    if name in ("gcn", "gcn-spectral"):
        layer = dict(layer_type=gnntf.GCNSpectralPreservingLayer) if name.endswith("spectral") else dict()
        return gnntf.GCN(graph, X, ref.CLASSES, latent_dims=[64, 64], **layer)
    if name == "ngcf":
        return gnntf.NGCF(graph, X, num_classes=16, dropout=0.25)
    if name == "pprsweep":
        model = gnntf.GNN(graph, X)
        model.add(gnntf.PPRSweep())
        return model
    return gnntf.GNN(graph, X, preprocessor=gnntf.Structural(dims=16, regularize=0, bipartite=100, l2_contraint=name.endswith("l2")))


@pytest.mark.parametrize("name", cases.EVAL_MODELS)
def test_eval_logits(gnntf, name):
    z = cases.load("eval")
    coo, vals, shape = ref.graph()
    assert np.array_equal(z["graph"], cases.digest(coo, vals))
    parameters = [z[f"{name}.p{k}"].astype(np.float32) for k in range(len(cases.eval_inputs(name)[1]))]
    gnntf.set_seed(ref.SEED)
    model = build_eval_model(gnntf, name, gnntf.SparseCOO(coo, vals, shape), z[name + ".X"].astype(np.float32))
    assign(model, parameters)
    model.training_mode(False)
    with torch.no_grad():
        got = model(model.features).cpu().numpy()
    want = z[name + ".out"]
    atol = 1e-4 if name.endswith("spectral") else ATOL
    print(f"eval logits of {name}: {worst(got, want, RTOL, atol):.3g} x the bar (rtol {RTOL}, atol {atol})")
    assert got.shape == want.shape and model._mask_calls == 0
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=atol)


# ---- the normalised adjacency -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["full", "emptied"])
def test_normalized_adjacency(gnntf, gname):
    """gnntf.normalize against GNN.get_adjacency of the reference for every normalisation, add_eye and mode, as matrices (equal indices
    added up on both sides: the handle stores the coalesced structure and keeps the added identity apart in ``diag``)."""
    z = cases.load("adjacency")
    coo, vals, n = z[gname + ".coo"].astype(np.int64), z[gname + ".vals"].astype(np.float32), int(z[gname + ".n"])
    graph = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, (n, n)), device="cuda:0")
    rowptr, colidx, _ = (x.cpu().numpy() for x in graph.csr_arrays())
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    seen = 0.0
    for mode in ("eval", "train"):
        for normalized in cases.NORMALIZED:
            for add_eye in cases.ADD_EYE:
                key = f"{gname}.{mode}.{normalized}.{add_eye}"
                adj = gnntf.normalize(graph, normalized, add_eye, dropout=float(z["rate"]) if mode == "train" else 0.0, seed=int(z["seed"]),
                                      stream_id=max(int(z[key + ".stream"]), 0))
                got = np.zeros((n, n))
                np.add.at(got, (rows, colidx), adj.vals.cpu().numpy().astype(np.float64))
                if add_eye != "none":
                    got[np.arange(n), np.arange(n)] += adj.diag.cpu().numpy().astype(np.float64)
                want = np.zeros((n, n))
                np.add.at(want, (z[key + ".indices"][:, 0], z[key + ".indices"][:, 1]), z[key + ".values"])
                assert np.array_equal(got == 0, want == 0), key                                        # the same entries dropped, the same D = 0
                seen = max(seen, worst(got, want, 1e-6, 0.0) if want.any() else 0.0)
                np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=key)
    print(f"normalised adjacency, {gname} graph: {seen:.3g} x the bar (rtol 1e-6)")


def test_dropped_adjacency_skips_where_the_reference_multiplies_a_stored_zero(gnntf):
    """NAMED EXPECTED DIFFERENCE, on an input where it shows.  The reference keeps a dropped entry in the index list with the value 0
    (tf.nn.dropout on G.values, layered.py:50; the adjacency fixtures hold those zeros), so a non-finite feature row reaches every row
    that stores an entry to it: 0 * inf = NaN.  sparse.DroppedAdjacency never gathers a dropped entry's row (it saves about half of
    the gathers; finite features are its documented precondition), so such a row gets the sum of its kept entries alone."""
    import graphs
    from gnntf import sparse
    from oracle import gnntf_oracle as orc
    coo, vals, shape = graphs.rmat_symmetric_coo(800, 5000, seed=3)
    graph = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    seed, stream, poisoned = 77, 5, int(np.bincount(coo[:, 1]).argmax())                         # the column most rows store an entry to
    adj = sparse.dropped_adjacency(graph, 0.5, seed, stream)
    assert isinstance(adj, sparse.DroppedAdjacency)
    X = np.random.default_rng(2).standard_normal((800, 16)).astype(np.float32)
    X[poisoned] = np.inf
    got = gnntf.spmm(adj, dev(X)).cpu().numpy()
    ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=0.5, training=True, seed=seed, stream=stream, dtype=np.float64)
    kept = orc.keep_mask(coo, 0.5, seed, stream)
    assert np.array_equal(ai, coo) and not av[~kept].any()
    # (a row all of whose column's entries were dropped has the degree scale 0: its kept entries are zeros on both sides -- left out)
    dead = np.zeros(800, dtype=bool)
    dead[ai[kept & (av == 0), 0]] = True
    with np.errstate(invalid="ignore"):
        reference = orc.sparse_dense_matmul(ai, av, shape, X.astype(np.float64))                   # the stored zeros multiplied: 0 * inf
        skipped = orc.sparse_dense_matmul(ai[kept], av[kept], shape, X.astype(np.float64))
    to_poisoned = np.zeros(800, dtype=bool)
    to_poisoned[ai[ai[:, 1] == poisoned, 0]] = True
    kept_to_poisoned = np.zeros(800, dtype=bool)
    kept_to_poisoned[ai[kept & (ai[:, 1] == poisoned), 0]] = True
    only_dropped = to_poisoned & ~kept_to_poisoned & ~dead
    kept_to_poisoned &= ~dead
    assert only_dropped.sum() >= 10 and kept_to_poisoned.sum() >= 10
    assert np.isnan(reference[only_dropped]).all() and np.isfinite(skipped[only_dropped]).all()     # where the difference shows
    assert np.isfinite(got[only_dropped]).all() and np.isinf(got[kept_to_poisoned]).all() and np.isinf(skipped[kept_to_poisoned]).all()
    finite = ~kept_to_poisoned & ~dead
    np.testing.assert_allclose(got[finite], skipped[finite], rtol=RTOL, atol=ATOL)
    assert np.array_equal(np.isnan(reference[~dead]), np.repeat(only_dropped[~dead, None], 16, axis=1))      # and nowhere else


# ---- two training steps ------------------------------------------------------------------------------------------------------------------------
def two_steps(model, objective):
    """The protocol of tests/test_gpu_model_steps.py: a step, ``v -= 0.05 grad``, an eval forward, a step."""
    got, counts, out = [], [], None
    for phase in ("step", "eval", "step"):
        if phase == "eval":
            assert not model.is_training()
            with torch.no_grad():
                out = model(model.features).cpu().numpy()
        else:
            with model:
                for v in model.vars():
                    v.var.grad = None
                loss = objective()
                loss.backward()
            assert all(v.var.grad is not None for v in model.vars())
            got.append((float(loss.detach()), [v.var.grad.detach().cpu().numpy().astype(np.float64) for v in model.vars()]))
            with torch.no_grad():
                for v in model.vars():
                    v.var -= ref.STEP_SIZE * v.var.grad
        counts.append(model._mask_calls)
    return got, counts, out


def judge_steps(name, z, got, counts, out, bar=1.0, eval_atol=ATOL):
    for step, (loss, grads) in enumerate(got):
        want_loss = float(z["losses"][step])
        ratios = [ref.ratio_to_bar(g, z[f"step{step}.g{k}"]) for k, g in enumerate(grads)]
        print(f"{name} step {step}: loss {loss:.9g} against the reference's {want_loss:.9g} = {ref.loss_ratio_to_bar(loss, want_loss):.3g} x the bar; "
              f"worst gradient {max(ratios):.3g} x the bar (variable {int(np.argmax(ratios))} of {len(ratios)}); the case's bar is {bar:.3g} x")
    assert counts == z["streams_after"].tolist(), (counts, z["streams_after"].tolist())
    for step, (loss, grads) in enumerate(got):
        want_loss = float(z["losses"][step])
        assert abs(loss - want_loss) <= ref.LOSS_RTOL * abs(want_loss), (step, loss, want_loss)
        assert f"step{step}.g{len(grads)}" not in z
        for k, g in enumerate(grads):
            w = z[f"step{step}.g{k}"]
            scale = np.abs(w).max()
            assert scale > ref.NON_TRIVIAL, (step, k)
            np.testing.assert_allclose(g, w, rtol=bar * ref.GRAD_RTOL, atol=bar * ref.GRAD_ATOL * scale, err_msg=f"step {step}, variable {k}")
    if "eval" in z:                                     # the eval forward between the steps: after one update, at the eval bar
        np.testing.assert_allclose(out, z["eval"], rtol=RTOL, atol=eval_atol)


@pytest.mark.parametrize("name", cases.step_meanings())
def test_two_training_steps_match_the_reference(gnntf, monkeypatch, name):
    from gnntf.training import _Objective
    case, z = steps.CASES[name], cases.load("step_" + name)
    coo, vals, shape = ref.graph()
    assert np.array_equal(z["inputs"], cases.digest(coo, vals, ref.features(case["width"]), *ref.initial_parameters(case["layers"], case["width"], seed=31)))
    nat = gnntf.sparse.nat
    counting = steps.CountingLibrary(nat.lib())
    monkeypatch.setattr(nat, "lib", lambda: counting)
    model = steps.build_model(gnntf, case)
    assert model._mask_calls == 0
    fixed = ref.FixedMasks(steps.MASK_SEED)
    model.dropout = lambda feats, p=0.5: feats if (not model.is_training() or p == 0) else \
        feats * torch.from_numpy(fixed.mask(tuple(feats.shape), p)).to(feats.device, feats.dtype)
    got, counts, out = two_steps(model, _Objective(model, steps.task_of(gnntf, case), ref.WEIGHT_DECAY))
    judge_steps(name, z, got, counts, out, bar=case["bar"], eval_atol=1e-4 if "spectral" in name else ATOL)    # as test_eval_logits holds them
    missing = [e for e in case["entries"] if e not in counting.calls]
    unexpected = [e for e in case["absent"] if e in counting.calls]
    assert not missing and not unexpected, (missing, unexpected, sorted(counting.calls))


@pytest.mark.parametrize("name", sorted(cases.APPNP_STEP_KINDS))
def test_two_appnp_training_steps_match_the_reference(gnntf, name):
    from gnntf.training import _Objective
    c, z = cases.APPNP_STEP, cases.load("step_" + name)
    coo, vals, shape, X, nodes, labels, parameters = cases.appnp_step_inputs()
    assert np.array_equal(z["inputs"], cases.digest(coo, vals, X, nodes, labels, *parameters))
    gnntf.set_seed(c["seed"])
    counter = cases.APPNP_STEP_KINDS[name][0] == "counter"
    model = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=c["classes"], latent_dims=[c["hidden"]], iterations=c["K"], a=c["a"],
                        fused=False, dense_dropout="fused" if counter else "torch")
    assign(model, parameters)
    fixed = ref.FixedMasks(c["mask_seed"])
    model.dropout = lambda feats, p=0.5: feats if (not model.is_training() or p == 0) else \
        feats * torch.from_numpy(fixed.mask(tuple(feats.shape), p)).to(feats.device, feats.dtype)
    got, counts, out = two_steps(model, _Objective(model, gnntf.NodeClassification(nodes, labels), c["weight_decay"]))
    assert (len(fixed.masks) == 0) == counter               # the counter RNG's masks leave the dense launch; the host-drawn ones were used
    judge_steps(name, z, got, counts, out)


# ---- the heads ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", cases.NODE_WIDTHS)
def test_node_head(gnntf, C):
    z = cases.load("heads")
    key = f"node{C}."
    logits, nodes, labels = z[key + "logits"].astype(np.float32), z[key + "nodes"].astype(np.int64), z[key + "labels"].astype(np.int64)
    want = float(z[key + "loss"])
    loss = float(gnntf.node_ce(dev(logits), nodes, labels))
    print(f"node head C={C}: loss {loss:.9g} against the reference's {want:.9g}")
    assert abs(loss - want) <= 1e-5 * max(abs(want), 1.0)
    np.testing.assert_array_equal(gnntf.node_argmax(dev(logits), nodes).cpu().numpy(), z[key + "predict"])
    task = gnntf.NodeClassification(nodes, labels)
    assert abs(float(task.loss(dev(logits))) - want) <= 1e-5 * max(abs(want), 1.0)
    np.testing.assert_array_equal(task.predict(dev(logits)).cpu().numpy(), z[key + "predict"])
    assert abs(task.evaluate(dev(logits)) - float(z[key + "evaluate"])) < 1e-12


@pytest.mark.parametrize("C", cases.LINK_WIDTHS)
def test_link_head(gnntf, C):
    z = cases.load("heads")
    key = f"link{C}."
    F, edges, labels, r = z[key + "F"].astype(np.float32), z[key + "edges"].astype(np.int64), z[key + "labels"], z[key + "r"].astype(np.float32)
    for weights, tag in ((None, "plain"), (r, "r")):
        got = gnntf.edge_scores(dev(F), edges, None if weights is None else dev(weights)).cpu().numpy()
        want = z[f"{key}dot.diff.{tag}.logits"]
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=1e-4)
        # the features are scaled by 0.1, so the logits are about 1e-2 and the bar's absolute term would carry them alone: the same
        # bar once more with the absolute term in units of the largest logit
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=1e-4 * np.abs(want).max())
    seen = 0.0
    for similarity in ("dot", "cos"):
        for tag in ("plain", "r"):                          # "r": the DistMult weights, a variable of the architecture the task is given
            heads = dict()
            for form in ("diff", "bce"):
                holder = gnntf.Layered((ref.N, C)) if tag == "r" else None
                heads[form] = gnntf.LinkPrediction(edges, labels, gnn=holder, similarity=similarity, loss=form)
                if holder is not None:
                    assert len(holder.vars()) == 1 and tuple(holder.vars()[0].var.shape) == (C, 1)
                    holder.vars()[0].assign(torch.from_numpy(r))
                want = float(z[f"{key}{similarity}.{form}.{tag}.loss"])
                got = float(heads[form].loss(dev(F)).detach())
                seen = max(seen, abs(got - want))
                assert abs(got - want) < 1e-4, (similarity, form, tag, got, want)
            want = z[f"{key}{similarity}.diff.{tag}.predict"]
            np.testing.assert_allclose(heads["diff"].predict(dev(F)).detach().cpu().numpy().reshape(-1), want, rtol=RTOL, atol=1e-4)
    print(f"link head C={C}: worst loss difference {seen:.3g} (bar 1e-4)")
