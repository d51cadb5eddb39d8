"""tests/model_step_ref.py judged on its own, without a GPU: its forwards against the oracle's eval forwards, the bar of
tests/test_gpu_model_steps.py against wrong readings of the contract planted in the reference, its stream count against the documented
rule, and the two conditions the GPU comparison needs of its inputs."""
import functools

import numpy as np
import pytest
import torch

import model_step_ref as ref
from oracle import gnntf_oracle as orc

CASES = ref.cases()


def without_rates(layers):
    """The same architecture with every dropout rate 0."""
    return [dict(layer, rate=0, graph_dropout=0) if "rate" in layer else dict(layer) for layer in layers]


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_the_graph_holds_every_row_regime():
    coo, vals, shape = ref.graph()
    rows, columns = np.bincount(coo[:, 0], minlength=ref.N), np.bincount(coo[:, 1], minlength=ref.N)
    assert shape == (ref.N, ref.N) and ref.N < 1 << 15                           # few enough rows for a long-row threshold of 512
    assert rows[ref.HUB] > 512 and columns[ref.HUB] > 512 and np.sort(rows)[-2] < 512
    tile = slice(*ref.EMPTY_TILE)
    assert ref.EMPTY_TILE[0] % 16 == 0 and ref.EMPTY_TILE[1] - ref.EMPTY_TILE[0] == 16 and not rows[tile].any() and not columns[tile].any()
    copies = orc.duplicate_rank(coo)
    assert (copies == 1).sum() == 300 and copies.max() == 1 and (vals[copies == 1] == 0.5).all() and (vals[copies == 0] == 1).all()
    raw = orc.to_dense(coo, vals, shape)
    assert (raw.sum(axis=0) != raw.sum(axis=1)).sum() > 100                      # row sums are not column sums: the bipartite form shows


# ---- 1. rate 0 and eval adjacencies: the oracle's eval forwards, layer by layer ---------------------------------------------------------
@pytest.mark.parametrize("training", [False, True])
def test_gcn_forward_is_the_oracles(training):
    """(training mode with every rate 0 is the same function: no mask, the constant adjacency, no stream)"""
    case = CASES["gcn"]
    coo, vals, shape = ref.graph()
    X = ref.features(40)
    params = ref.initial_parameters(case["layers"], 40, seed=31)
    r = ref.Reference(without_rates(case["layers"]), coo, vals, shape, X, params, case["task"], 0.0, ref.SEED)
    with torch.no_grad():
        r.forward(training=training)
    assert r.streams == 0
    weights = [(params[2 * k].astype(np.float64), params[2 * k + 1].astype(np.float64)) for k in range(3)]
    for k in range(3):
        want = orc.gcn_forward_eval(coo, vals, shape, X, weights[:k + 1], dtype=np.float64)
        assert np.abs(want).max() > 0.1
        close(r.values[k].numpy(), want)


def test_gcnii_forward_is_the_oracles():
    """Every depth 1 .. 4 of the stack (the oracle returns the logits alone: the depth-k model shows the k-th layer)."""
    coo, vals, shape = ref.graph()
    X = ref.features(40)
    full = ref.initial_parameters(CASES["gcnii"]["layers"], 40, seed=31)         # W, b of the Dense, 4 x W, W, b of the output Dense
    for depth in range(1, 5):
        layers = without_rates(ref.gcnii(ref.CLASSES, latent_dims=(32,), iterations=depth))
        params = full[:2 + depth] + full[-2:]
        r = ref.Reference(layers, coo, vals, shape, X, params, CASES["gcnii"]["task"], 0.0, ref.SEED)
        got = r.evaluate()
        p64 = [p.astype(np.float64) for p in params]
        want = orc.gcnii_forward_eval(coo, vals, shape, X, (p64[0], p64[1]), p64[2:2 + depth], (p64[-2], p64[-1]), a=0.1, l=0.5, dtype=np.float64)
        assert np.abs(want).max() > 0.1 and r.streams == 0
        close(got, want)


@pytest.mark.parametrize("name", ["ngcf", "ngcf-wide"])
def test_ngcf_forward_is_the_oracles(name):
    case = CASES[name]
    coo, vals, shape = ref.graph()
    X = ref.features(case["width"])
    params = ref.initial_parameters(case["layers"], case["width"], seed=31)
    r = ref.Reference(without_rates(case["layers"]), coo, vals, shape, X, params, case["task"], 0.0, ref.SEED)
    out = r.evaluate()
    H = X.astype(np.float64)
    for k in range(3):
        W1, W2, b1, b2 = (p.astype(np.float64) for p in params[4 * k:4 * k + 4])
        want = orc.ngcf_layer_eval(coo, vals, shape, H, W1, b1, W2, b2, dtype=np.float64)
        close(r.values[k].numpy(), want)
        close(out[k * ref.N:(k + 1) * ref.N], want)                              # Concatenate: block k of axis 0 is layer k
        H = want
    assert out.shape == (3 * ref.N, case["width"])


# ---- 2. the reference's own stream count ---------------------------------------------------------------------------------------------
# per training step: one per dropped adjacency, then one per counter-RNG feature mask, in layer order; an eval forward draws none
STREAMS_PER_STEP = {
    "gcn": 2, "gcn-transform_first": 2, "gcn-fused": 3, "gcn-fused-back": 3, "gcn-spectral": 2, "gcn-spectral-fused": 3,
    "gcn-spectral-fused-back": 3, "gcnii": 0, "gcnii-drop": 4, "gcnii-drop-back": 4, "gcnii-drop-back-recomputed": 4,
    "gcnii-drop-back-recomputed-dense": 5, "gcnii-spectral": 0, "gcnii-spectral-fused": 4, "gcnii-edge": 4, "gcnii-edge-fused": 8,
    "ngcf": 0, "ngcf-fused": 0, "ngcf-fused-drop": 3, "ngcf-fused-drop-back": 3, "ngcf-wide": 0, "ngcf-wide-drop": 3,
}


@functools.lru_cache(maxsize=None)
def right(name):
    """The case's two steps by the unmistaken reference, once: ((results, counts), gate shares per phase, smallest squared norm)."""
    r = ref.reference_for(CASES[name])
    shares, norms, results, counts = [], [], [], []
    for phase in ("step", "eval", "step"):
        if phase == "eval":
            r.evaluate()
        else:
            results.append(r.step())
            r.update()
        counts.append(r.streams)
        shares.append(r.gate_shares())
        norms.append(r.smallest_squared_norm())
    return results, counts, shares, min(norms)


@pytest.mark.parametrize("name", sorted(CASES))
def test_stream_count_and_input_conditions(name):
    results, counts, shares, smallest = right(name)
    per_step = STREAMS_PER_STEP[name]
    assert counts == [per_step, per_step, 2 * per_step]
    # the gate condition: float32 may decide the gate of an element with |x| <= 1e-5 max|x| the other way
    worst = max(max(phase) for phase in shares)
    print(f"{name}: worst share of near-zero pre-activations {worst:.2e}, smallest squared row norm {smallest:.3g}")
    assert worst <= 1e-3
    assert smallest > 1e-6                                                      # far from the 1e-12 clamp of l2_normalize
    for loss, grads in results:
        assert np.isfinite(loss) and all(np.abs(g).max() > ref.NON_TRIVIAL for g in grads)


def test_every_case_is_listed():
    assert sorted(STREAMS_PER_STEP) == sorted(CASES)


def test_spectral_gcnii_layers_take_edge_dropout():
    """GCNIISpectralPreservingLayer(..., graph_dropout=0.5), the layer's own default: an adjacency stream per layer and step."""
    case = dict(CASES["gcnii-spectral"], layers=ref.gcnii(ref.CLASSES, latent_dims=(32,), iterations=4, spectral=True, dropout=0.4, graph_dropout=0.5))
    r = ref.reference_for(case)
    results, counts = r.run()
    assert counts == [4, 4, 8] and all(np.isfinite(loss) for loss, _ in results)
    assert abs(results[0][0] - right("gcnii-spectral")[0][0][0]) > 1e-3


# ---- 3. the bar sees every planted mistake ----------------------------------------------------------------------------------------------
PLANTED = [
    ("stream_off_by_one", "gcn"), ("stream_off_by_one", "gcnii-drop"), ("stream_off_by_one", "ngcf-fused-drop"),
    ("mask_stream_first", "gcn-fused"), ("mask_stream_first", "gcn-spectral-fused"), ("mask_stream_first", "gcnii-edge-fused"),
    ("no_dropout_scale", "gcn"), ("no_dropout_scale", "gcnii"), ("no_dropout_scale", "gcnii-drop"),
    # (not in NGCF: its dropout is followed by l2_normalize, which takes a uniform scale back out -- the model's meaning has no 1 / (1 - p))
    ("no_doubling", "gcn-spectral"), ("no_doubling", "gcnii-spectral"),
    ("beta_k", "gcnii"), ("beta_k", "gcnii-spectral"),
    ("last_dense_decayed", "gcnii"),
    ("no_output_penalty", "ngcf"), ("concatenate_axis_1", "ngcf"), ("bipartite_row_sums", "ngcf"), ("bipartite_row_sums", "ngcf-wide"),
]


def test_every_mistake_is_planted():
    assert sorted({m for m, _ in PLANTED}) == sorted(ref.MISTAKES)


@pytest.mark.parametrize("mistake,name", PLANTED)
def test_the_bar_sees_the_mistake(mistake, name):
    """The first step of the mistaken reference against the right one: some compared quantity is off by at least 10 x the bar."""
    want_loss, want_grads = right(name)[0][0]
    got_loss, got_grads = ref.reference_for(CASES[name], mistake=mistake).step()
    ratios = [ref.loss_ratio_to_bar(got_loss, want_loss)] + [ref.ratio_to_bar(g, w) for g, w in zip(got_grads, want_grads)]
    print(f"{mistake} in {name}: loss {ratios[0]:.3g} x the bar, worst gradient {max(ratios[1:]):.3g} x the bar; the case's gradient "
          f"bar is {CASES[name]['bar']:.3g} x")
    assert max([ratios[0]] + [r / CASES[name]["bar"] for r in ratios[1:]]) >= 10


# ---- 4. the float32 yardstick of NGCF ---------------------------------------------------------------------------------------------------
def test_only_ngcf_has_a_bar_of_its_own():
    assert sorted(ref.FLOAT32_YARDSTICK) == sorted(n for n in CASES if n.startswith("ngcf"))
    assert all(case["bar"] == (4 * ref.FLOAT32_YARDSTICK[name] if name.startswith("ngcf") else 1.0) for name, case in CASES.items())


def float32_error(name, mistake=None):
    """The worst gradient error, in units of the bar, of the reference evaluated in float32 against itself in float64, over both steps."""
    want, _ = ref.reference_for(CASES[name], mistake=mistake).run() if mistake else (right(name)[0], None)
    got, _ = ref.reference_for(CASES[name], mistake=mistake, dtype=torch.float32).run()
    assert all(ref.loss_ratio_to_bar(g[0], w[0]) <= 0.1 for g, w in zip(got, want))            # the loss bar stays as it is
    return max(ref.ratio_to_bar(g, w) for (_, gs), (_, ws) in zip(got, want) for g, w in zip(gs, ws))


@pytest.mark.parametrize("name", sorted(ref.FLOAT32_YARDSTICK))
def test_float32_yardstick_of_ngcf(name):
    """The value written in model_step_ref.FLOAT32_YARDSTICK is what the float32 evaluation gives (within the factor of 4 the bar allows
    it: float32 sums differ with the BLAS at hand), it is above the bar -- the reason NGCF has a bar of its own -- and it is the output
    penalty's: without it the same evaluation is far inside the bar."""
    measured = float32_error(name)
    print(f"{name}: float32 against float64 {measured:.3f} x the bar (written: {ref.FLOAT32_YARDSTICK[name]})")
    assert ref.FLOAT32_YARDSTICK[name] / 4 <= measured <= 4 * ref.FLOAT32_YARDSTICK[name] and measured > 1
    assert float32_error(name, mistake="no_output_penalty") <= 0.1


@pytest.mark.parametrize("name", ["gcn", "gcn-spectral", "gcnii", "gcnii-spectral", "gcnii-edge"])
def test_float32_meets_the_bar_elsewhere(name):
    assert float32_error(name) <= 0.1
