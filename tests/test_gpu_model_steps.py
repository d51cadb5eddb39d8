"""Two consecutive training steps of GCN, GCNII and NGCF on the HIP path -- as built by default and under every switch that reroutes
their layers -- against tests/model_step_ref.py: the same steps in dense float64 with torch autograd on the CPU, written from the
reference's meaning and not from graph_model.py (tests/test_model_step_ref_cpu.py judges that reference on its own and shows that the
bar below sees a wrong stream id, order, scale, doubling, beta, decay, penalty, axis or normalisation at 10 x and more).

A case: a training step, a plain ``v -= 0.05 * grad``, an eval forward, a second training step -- on both sides, each with its own
gradients.  Compared: the loss and every parameter gradient of each step, at the bar of tests/test_gpu_training.py (loss 1e-5
relative, gradients rtol 1e-3 and atol 2e-5 max|want|, every gradient above 1e-4 somewhere; for NGCF, whose composed default misses
the gradient bar as the float32 evaluation of the reference itself does, four times that float32 evaluation's error:
model_step_ref.FLOAT32_YARDSTICK holds the measured values, 2.9 ... 22.5 x the bar, and the reason); the model's ``_mask_calls`` after each of
the three phases against the reference's own count; and, through the library entries the case called, that a switch ran its launch
and did not fall back to the composed path.

One graph for all cases (model_step_ref.graph): 800 vertices -- so the long-row threshold is 512 --, an R-MAT body, a hub vertex of 614
entries (the hub-row path of the fused layers), a 16-row tile without entries, 300 entries stored twice.  Torch's feature masks are
replaced on both sides by the same host-drawn masks (FixedMasks patched into ``model.dropout``); the counter RNG's masks and the
dropped adjacencies follow from (seed, stream) on both sides."""
import functools

import numpy as np
import pytest
import torch

import model_step_ref as ref

pytestmark = pytest.mark.gpu

CASES = ref.cases()
MASK_SEED = 23


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


class CountingLibrary:
    """The loaded library with every entry that is asked for recorded by name."""

    def __init__(self, real):
        self.real, self.calls = real, set()

    def __getattr__(self, name):
        if name.startswith("gnx_"):
            self.calls.add(name)
        return getattr(self.real, name)


@functools.lru_cache(maxsize=None)
def wanted(meaning):
    """The reference's two steps and stream counts, once per meaning (cases that differ in a switch alone share it)."""
    case = next(c for c in CASES.values() if key_of(c) == meaning)
    return ref.reference_for(case, fixed_seed=MASK_SEED).run()


def key_of(case):
    return repr((case["layers"], case["width"], case["task"][0], case["task"][-1]))


def build_model(gnntf, case):
    gnntf.set_seed(ref.SEED)
    coo, vals, shape = ref.graph()
    graph, X = gnntf.SparseCOO(coo, vals, shape), ref.features(case["width"])
    build, options = dict(case["build"]), case["options"]
    if "layer_type" in build:
        build["layer_type"] = getattr(gnntf, build["layer_type"])
    if case["model"] == "GCN":
        model = gnntf.GCN(graph, X, ref.CLASSES, **build, **options)
    elif case["model"] == "GCNII":
        model = gnntf.GCNII(graph, X, ref.CLASSES, **build, **options)
    elif case["model"] == "NGCF":
        model = gnntf.NGCF(graph, X, num_classes=case["width"], **build, **options)
    else:                                               # the GCNII constructor's layout with the layers' own graph_dropout = 0.5
        model = gnntf.GNN(graph, X, **options)
        model.add(gnntf.Dropout(0.6))
        for width in build["latent_dims"]:
            model.add(gnntf.Dense(width, dropout=0, activation=gnntf.relu))
        H0 = model.top_layer()
        for k in range(build["iterations"]):
            model.add(gnntf.GCNIILayer(H0, 0.1, 0.5, k, activation=gnntf.relu, dropout=0.6, graph_dropout=0.5))
        model.add(gnntf.Dense(ref.CLASSES, dropout=0, regularize=False))
    start = ref.initial_parameters(case["layers"], case["width"], seed=31)
    assert [tuple(v.var.shape) for v in model.vars()] == [p.shape for p in start]
    for v, p in zip(model.vars(), start):
        v.assign(torch.from_numpy(p))
    return model


def task_of(gnntf, case):
    if case["task"][0] == "node":
        _, nodes, labels = case["task"]
        return gnntf.NodeClassification(nodes, labels)
    _, edges, labels, form = case["task"]
    return gnntf.LinkPrediction(edges, labels, loss=form)


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_training_steps_match_dense_float64(gnntf, monkeypatch, name):
    from gnntf.training import _Objective
    case = CASES[name]
    nat = gnntf.sparse.nat
    counting = CountingLibrary(nat.lib())
    monkeypatch.setattr(nat, "lib", lambda: counting)
    model = build_model(gnntf, case)
    assert model.graph.long_row_threshold == 512 and model.graph.n_hub_rows >= 1 and model._mask_calls == 0
    fixed = ref.FixedMasks(MASK_SEED)
    model.dropout = lambda feats, p=0.5: feats if (not model.is_training() or p == 0) else \
        feats * torch.from_numpy(fixed.mask(tuple(feats.shape), p)).to(feats.device, feats.dtype)
    objective = _Objective(model, task_of(gnntf, case), ref.WEIGHT_DECAY)

    got, counts = [], []
    for phase in ("step", "eval", "step"):
        if phase == "eval":
            assert not model.is_training()
            with torch.no_grad():
                model(model.features)
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

    want, want_counts = wanted(key_of(case))
    # the figures first: the worst ratio to the bar per step
    for step, ((got_loss, got_grads), (want_loss, want_grads)) in enumerate(zip(got, want)):
        ratios = [ref.ratio_to_bar(g, w) for g, w in zip(got_grads, want_grads)]
        print(f"{name} step {step}: loss {got_loss:.9g} against {want_loss:.9g} = {ref.loss_ratio_to_bar(got_loss, want_loss):.3g} x the bar; "
              f"worst gradient {max(ratios):.3g} x the bar (variable {int(np.argmax(ratios))} of {len(ratios)}); the case's bar is {case['bar']:.3g} x")
    assert counts == want_counts, (counts, want_counts)
    for step, ((got_loss, got_grads), (want_loss, want_grads)) in enumerate(zip(got, want)):
        assert abs(got_loss - want_loss) <= ref.LOSS_RTOL * abs(want_loss), (step, got_loss, want_loss)
        assert len(got_grads) == len(want_grads)
        for i, (g, w) in enumerate(zip(got_grads, want_grads)):
            scale = np.abs(w).max()
            assert scale > ref.NON_TRIVIAL, (step, i)
            np.testing.assert_allclose(g, w, rtol=case["bar"] * ref.GRAD_RTOL, atol=case["bar"] * ref.GRAD_ATOL * scale,
                                       err_msg=f"step {step}, variable {i}")
    # a switch that fell back would have passed as the composed path
    missing = [e for e in case["entries"] if e not in counting.calls]
    unexpected = [e for e in case["absent"] if e in counting.calls]
    assert not missing and not unexpected, (missing, unexpected, sorted(counting.calls))
