"""GNN(gcnii_weight_gradient="recomputed") on the MI355X: a 4-layer GCNII stack on the graph of regime T (tests/gcnii_shapes_ref.py:
n = 1547, hub rows, a ragged last tile, rows and a tile without entries) at C = 16 and 64 with the fused feature dropout, in f32 and with
bf16 rows (whose width and row gates are patched down, as tests/test_gpu_gcnii_bf16_training.py does).

Between "stored" and "recomputed" everything but the layers' dW is bit for bit equal: the logits, the loss, the gradient that arrives at H0
(dH0 plus the gradient of the run's input: the same tensor) and every other variable's gradient.  Every dW is judged against float64 by the
criterion of tests/test_gpu_gcnii_wgrad.py -- want = f64(T)^T f64(G), bound = gamma (|T|^T |G|) + T_bound^T |G|, gamma of an f32 sum of
n + 4 terms in any order, over the very rows and gated gradient the launch read -- propagated through M = (1 - b) I + b W: dW = b dM, which
torch forms with two more roundings (b to float32, the product), so  |dW - b want| <= b bound + 2 u b |want|.
The memory saving is asserted as a condition: the bytes of the distinct storages autograd saves in one forward."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcnii_shapes_ref as ref

pytestmark = pytest.mark.gpu

LAYERS, CLASSES, FEATURES = 4, 5, 100
WIDTHS = (16, 64)
DTYPES = (torch.float32, torch.bfloat16)


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


@pytest.fixture(scope="module")
def case():
    coo, vals, shape, info = ref.regime_graph("T", 0)
    n = shape[0]
    rng = np.random.default_rng(21)
    # mostly zeros: the model holds such input features as sparse rows, whose dropout draws from the counter RNG -- nothing in a
    # "fused" model then asks torch's generator, which a captured run and an eager run do not advance alike
    X = (rng.standard_normal((n, FEATURES)) * (rng.random((n, FEATURES)) < 0.02)).astype(np.float32)
    X[np.arange(n), rng.integers(FEATURES, size=n)] = 1.0       # no empty rows; about 3 % of the elements are not zero
    labels = rng.integers(0, CLASSES, size=n)
    weights = {C: [(np.random.default_rng(40 + k).standard_normal((C, C)) / math.sqrt(4 * C)).astype(np.float32) for k in range(LAYERS)]
               for C in WIDTHS}
    return dict(coo=coo, vals=vals, shape=shape, n=n, info=info, X=X, labels=labels, weights=weights, train=np.arange(0, 300),
                valid=np.arange(300, 600))


@pytest.fixture
def bf16_gates_down(gnntf, monkeypatch):
    monkeypatch.setattr(gnntf.sparse, "GCNII_BF16_TRAIN_MIN_ROWS", 0)
    monkeypatch.setattr(gnntf.sparse, "GCNII_BF16_TRAIN_MIN_WIDTH", 16)


def make_model(gnntf, case, C, seeded_weights=True, **option):
    gnntf.set_seed(11)
    torch.manual_seed(3)
    model = gnntf.GCNII(gnntf.SparseCOO(case["coo"], case["vals"], case["shape"]), case["X"], CLASSES, latent_dims=[C], iterations=LAYERS,
                        **option)
    model.reset()
    convs = [layer for layer in model.layers() if isinstance(layer, gnntf.GCNIILayer)]
    assert len(convs) == LAYERS
    if seeded_weights:                                  # the reference initialises W to zero: M would be a multiple of the identity
        for layer, W in zip(convs, case["weights"][C]):
            layer.W.data.copy_(torch.from_numpy(W).cuda())
    return model


def options(dtype, weight_gradient, feature_dropout="fused"):
    return dict(feature_dropout=feature_dropout, gcnii_backward="fused", gcnii_training_dtype=dtype, gcnii_weight_gradient=weight_gradient)


class Record:
    """What one training step of a model did: its logits, loss and gradients, the gradient at H0, the kernels, what autograd saved, and
    every call of the recomputed weight gradient (rows, H0, a, G, dM)."""


def one_step(gnntf, case, model, monkeypatch):
    rec = Record()
    rec.wgrads, saved = [], []
    inner = gnntf.sparse.gcnii_wgrad

    def recording(adj, H, H0, a, G, hub_rows=None):
        dM = inner(adj, H, H0, a, G, hub_rows=hub_rows)
        rec.wgrads.append((H.detach().clone(), H0.detach().clone(), float(a), G.detach().clone(), dM.detach().clone()))
        return dM

    monkeypatch.setattr(gnntf.sparse, "gcnii_wgrad", recording)
    task = gnntf.NodeClassification(case["train"], case["labels"][case["train"]])
    torch.manual_seed(17)                               # torch's own dropout (the input features; every layer under "torch")
    with model:
        assert isinstance(model._input_features(), gnntf.SparseRows)
        for v in model.vars():
            v.var.grad = None
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
            logits = model(model.features)
        rec.forward_kernel = model.graph.last_kernel()
        convs = [layer for layer in model.layers() if isinstance(layer, gnntf.GCNIILayer)]
        H0 = convs[0].H0.value
        H0.retain_grad()
        loss = task.loss(logits)
        loss.backward()
    monkeypatch.setattr(gnntf.sparse, "gcnii_wgrad", inner)
    rec.logits, rec.loss, rec.dH0 = logits.detach().clone(), float(loss.detach()), H0.grad.clone()
    rec.conv_W = [id(layer.W) for layer in convs]
    rec.grads = {id(v.var): v.var.grad.clone() for v in model.vars()}
    rec.dW = [layer.W.grad.clone() for layer in convs]
    rec.b = [layer.beta_transformer(layer.l / (layer.k + 1)) for layer in convs]
    rec.order = [id(v.var) for v in model.vars()]
    storages = {}
    for t in saved:
        storages[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
    rec.saved_bytes, rec.saved = sum(storages.values()), saved
    # the layers' values as they stand (a GCNIILayer keeps its own in _value, None while an inner layer of a bf16 run has not been read)
    values = [layer.__dict__["_value"] if "_value" in layer.__dict__ else layer.__dict__.get("value") for layer in model.layers()]
    rec.values = {v.data_ptr() for v in values + [model.features] if isinstance(v, torch.Tensor)}
    rec.adj = model.get_adjacency(0)
    rec.graph = model.graph
    return rec


def adjacency_f64(rec, n):
    rowptr, colidx, _ = (x.cpu().numpy() for x in rec.graph.csr_arrays())
    return sp.csr_matrix((rec.adj.vals.cpu().numpy().astype(np.float64), colidx, rowptr), shape=(n, n))


def judge_dW(case, rec, C, what):
    """Every recorded call against float64, and the layer's dW = b dM through the bound of the module's docstring.  The backward runs the
    last layer first."""
    n = case["n"]
    A = adjacency_f64(rec, n)
    assert len(rec.wgrads) == LAYERS
    terms = (n + 4) * ref.U32
    gamma = terms / (1.0 - terms)
    for k, (H, H0, a, G, dM) in zip(range(LAYERS - 1, -1, -1), rec.wgrads):
        H, H0, G = (x.float().cpu().numpy() for x in (H, H0, G))
        fwd = ref.forward_ref(A, H, H0, np.eye(C, dtype=np.float32), a, False)
        beta, alpha = ref.mix_constants(a)
        absT = beta * (abs(A) @ np.abs(ref.f64(H))) + alpha * np.abs(ref.f64(H0))
        want = fwd["T"].T @ ref.f64(G)
        bound = gamma * (absT.T @ np.abs(ref.f64(G))) + fwd["T_bound"].T @ np.abs(ref.f64(G))
        r_M = ref.ratio(dM.cpu().numpy(), want, bound)
        b = rec.b[k]
        r_W = ref.ratio(rec.dW[k].cpu().numpy(), b * want, b * bound + 2 * ref.U32 * b * np.abs(want))
        print(f"{what}, C = {C}, layer {k}: dM error / bound = {r_M:.4f}, dW error / bound = {r_W:.4f}")
        assert float(np.abs(want).max()) > 0 and r_M <= 1.0 and r_W <= 1.0, (what, C, k, r_M, r_W)


def equal_but_dW(stored, recomputed):
    assert torch.equal(stored.logits, recomputed.logits) and stored.loss == recomputed.loss
    assert torch.equal(stored.dH0, recomputed.dH0) and float(stored.dH0.abs().max()) > 0
    others = 0
    for (ks, gs), (kr, gr) in zip(((k, stored.grads[k]) for k in stored.order), ((k, recomputed.grads[k]) for k in recomputed.order)):
        if ks in stored.conv_W:
            assert kr in recomputed.conv_W
            continue
        others += 1
        assert torch.equal(gs, gr)
    assert others >= 2                                  # the two Dense layers' variables


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("C", WIDTHS)
def test_recomputed_against_stored(gnntf, case, bf16_gates_down, monkeypatch, C, dtype):
    n = case["n"]
    stored = one_step(gnntf, case, make_model(gnntf, case, C, **options(dtype, "stored")), monkeypatch)
    recomputed = one_step(gnntf, case, make_model(gnntf, case, C, **options(dtype, "recomputed")), monkeypatch)
    bf16 = dtype is torch.bfloat16
    assert stored.forward_kernel == ("spmm_gcnii_mfma_train_bf16" if bf16 else "spmm_gcnii_mfma_drop")
    assert recomputed.forward_kernel == ("spmm_gcnii_mfma_drop_bf16" if bf16 else "spmm_gcnii_mfma_drop")
    assert not stored.wgrads and len(recomputed.wgrads) == LAYERS
    assert all(H.dtype == dtype for H, *_ in recomputed.wgrads)
    equal_but_dW(stored, recomputed)
    judge_dW(case, recomputed, C, "recomputed, " + ("bf16" if bf16 else "f32") + " rows")
    # the two weight gradients differ in their summation order alone: close, and (at these sizes) not the same bits everywhere
    assert any(not torch.equal(s, r) for s, r in zip(stored.dW, recomputed.dW))
    # memory, as a condition: T, 4 n C bytes per layer, is what is no longer saved -- the layer's input and H0 are saved by their makers
    print(f"C = {C}, {dtype}: saved bytes stored / recomputed = {stored.saved_bytes} / {recomputed.saved_bytes}")
    assert stored.saved_bytes - recomputed.saved_bytes == LAYERS * 4 * n * C
    # no saved tensor of T's shape and dtype that is not an input or output of a layer
    strays = [t for t in recomputed.saved if tuple(t.shape) == (n, C) and t.dtype == torch.float32 and t.data_ptr() not in recomputed.values]
    assert not strays
    assert sum(tuple(t.shape) == (n, C) and t.dtype == torch.float32 and t.data_ptr() not in stored.values for t in stored.saved) == LAYERS


@pytest.mark.parametrize("C,dtype", [(64, torch.float32), (64, torch.bfloat16), (16, torch.float32)], ids=("64-f32", "64-bf16", "16-f32"))
def test_captured_training_equals_eager(gnntf, case, bf16_gates_down, C, dtype):
    """train(capture=True) for 3 epochs with "recomputed", bit for bit the eager run (the pattern of tests/test_gpu_gcnii_drop.py)."""
    results = []
    for capture in (False, True):
        model = make_model(gnntf, case, C, seeded_weights=False, **options(dtype, "recomputed"))
        gnntf.set_seed(11)
        torch.manual_seed(5)
        valid = gnntf.NodeClassification(case["valid"], case["labels"][case["valid"]])
        model.train(train=gnntf.NodeClassification(case["train"], case["labels"][case["train"]]), valid=valid, epochs=3, patience=50,
                    capture=capture, optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
        results.append(([v.var.detach().clone() for v in model.vars()], float(model.loss(valid)), model._mask_calls))
    (eager, eager_loss, eager_masks), (captured, captured_loss, captured_masks) = results
    print("captured vs eager, max |difference| per variable:", [float((e - c).abs().max()) for e, c in zip(eager, captured)])
    assert all(torch.equal(e, c) for e, c in zip(eager, captured))
    assert eager_loss == captured_loss and eager_masks == captured_masks
    convs_moved = [float(v.abs().max()) > 0 for v in eager if tuple(v.shape) == (C, C)]
    assert len(convs_moved) >= LAYERS and all(convs_moved)                  # the weight gradients arrived: W started at zero


@pytest.mark.parametrize("C", WIDTHS)
def test_with_torch_dropout_the_switch_still_trains(gnntf, case, monkeypatch, C):
    """feature_dropout="torch": the layer's input is the dropout's own tensor, so nothing is saved less, but the path is the same: all
    but dW keeps its bits, every dW passes the bound.  Either gcnii_backward."""
    stored = one_step(gnntf, case, make_model(gnntf, case, C, **options(torch.float32, "stored", "torch")), monkeypatch)
    recomputed = one_step(gnntf, case, make_model(gnntf, case, C, **options(torch.float32, "recomputed", "torch")), monkeypatch)
    assert stored.forward_kernel == recomputed.forward_kernel == "spmm_gcnii_mfma"
    equal_but_dW(stored, recomputed)
    judge_dW(case, recomputed, C, "recomputed, torch dropout")
    assert recomputed.saved_bytes <= stored.saved_bytes
    composed = dict(options(torch.float32, "recomputed", "torch"), gcnii_backward="composed")
    other = one_step(gnntf, case, make_model(gnntf, case, C, **composed), monkeypatch)
    assert torch.equal(other.logits, stored.logits) and len(other.wgrads) == LAYERS
    # the last layer's gated gradient does not depend on the backward's form, so its dW has the same bits; below it the two backwards
    # hand down gradients that agree to rounding only, and every dW is judged against float64 over the gradient its launch read
    assert torch.equal(other.dW[-1], recomputed.dW[-1])
    judge_dW(case, other, C, "recomputed, torch dropout, composed backward")
