"""The fused dropout around Dense on the MI355X (gnx_dense_drop, gnx_dense_wgrad_drop, sparse.dense_step, GNN(dense_dropout="fused")).
The masks are functions of (seed, stream + counter, row, column) alone and the kernels add the k terms in gnx_dense's order, so the
forward and the weight gradient are compared BIT FOR BIT with the composition feature_dropout -> dense -> feature_dropout over a
materialised dropped X, at shapes that reach every kernel of the dispatch and their ragged ends; out, dW, db and dX are also held against
float64 inside the bounds of tests/dense_drop_ref.py.  Then the counter, the autograd node (what it saves, what it allocates) and the
models: the layer list, eval mode, seeds, capture against eager, the Dropout layer's pending value, fuse_runs = False."""
import numpy as np
import pytest
import torch

import dense_drop_ref as dref
import graphs

pytestmark = pytest.mark.gpu

TALL = 16384 + 37
SEED = 7
IN, OUT = (0.5, SEED, 2), (0.6, SEED, 3)
BOTH = (IN, OUT)
# (n, F, O, columns of padding behind a row of X, (input triple, output triple)) -- which kernel carries the shape: dense_kernel_for
CASES = [
    (TALL, 256, 64, 0, BOTH), (TALL, 256, 32, 0, BOTH), (TALL, 128, 64, 0, BOTH), (TALL, 128, 128, 0, BOTH),      # k_dense_wreg's rules
    (TALL, 64, 64, 0, BOTH), (TALL, 192, 64, 0, BOTH),                                                           # k_dense_ring's rules
    (TALL, 100, 7, 0, BOTH), (TALL, 200, 40, 0, BOTH),                                                           # k_dense_mfma's rules
    (300, 64, 64, 0, BOTH), (1, 64, 64, 0, BOTH), (300, 33, 5, 0, BOTH), (1, 33, 5, 0, BOTH),                     # short inputs
    (TALL, 128, 64, 4, BOTH), (300, 33, 5, 3, BOTH), (TALL, 64, 64, 64, BOTH),                                   # ldx > F
    (TALL, 64, 300, 0, BOTH), (300, 36, 300, 0, BOTH),                                                           # a second column panel
    (TALL, 256, 64, 0, (IN, None)), (TALL, 256, 64, 0, (None, OUT)), (TALL, 256, 64, 0, ((0.1, SEED, 0), (0.9, SEED, 1))),
    (TALL, 64, 64, 0, (IN, None)), (TALL, 100, 7, 0, (None, OUT)), (300, 33, 5, 0, ((0.1, SEED, 0), (0.9, SEED, 1))),
    (TALL, 128, 32, 0, ((0.1, SEED, 0), (0.9, SEED, 1))),
]


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


@pytest.fixture(scope="module")
def graph(gnntf):
    """A handle: the entries read its dropout counter and nothing else."""
    coo = np.array([[0, 1], [1, 0], [1, 2], [2, 1]], dtype=np.int64)
    return gnntf.DeviceGraph(gnntf.SparseCOO(coo, np.ones(4, dtype=np.float32), (3, 3)), device="cuda:0")


def host(t):
    return t.detach().cpu().numpy()


def operands(n, F, O, pad, seed=0):
    rng = np.random.default_rng(seed + 13 * F + O)
    rows = torch.from_numpy(rng.standard_normal((n, F + pad)).astype(np.float32)).cuda()
    X = rows[:, :F]                                                 # ldx = F + pad
    W = torch.from_numpy((rng.standard_normal((F, O)) / np.sqrt(F)).astype(np.float32)).cuda()
    b = torch.from_numpy(rng.uniform(-0.4, 0.6, size=(1, O)).astype(np.float32)).cuda()
    g = torch.from_numpy(rng.standard_normal((n, O)).astype(np.float32)).cuda()
    return X, W, b, g


def composed(gnntf, graph, X, W, b, relu, din, dout):
    """feature_dropout -> dense -> feature_dropout over a materialised dropped X: (out, dropped X)."""
    Xd = gnntf.feature_dropout(graph, X.contiguous(), *din) if din is not None else X
    out = gnntf.dense(Xd, W, b, relu=relu)
    return (gnntf.feature_dropout(graph, out, *dout) if dout is not None else out), Xd


@pytest.mark.parametrize("relu", (True, False))
@pytest.mark.parametrize("n,F,O,pad,rates", CASES)
def test_forward_and_backward(gnntf, graph, n, F, O, pad, rates, relu):
    """dense_step: the forward bit for bit the composition; dW bit for bit _dense_wgrad over the dropped X; out, dW, db and dX inside the
    float64 bounds; the counter-RNG zeros where the mask says so."""
    from gnntf import sparse
    din, dout = rates
    X, W, b, g = operands(n, F, O, pad)
    assert X.stride(0) == F + pad
    with torch.no_grad():
        want_out, Xd = composed(gnntf, graph, X, W, b, relu, din, dout)
        plain = gnntf.dense_step(graph, X, W, b, relu=relu, in_dropout=din, out_dropout=dout)
    assert torch.equal(plain, want_out)
    leaves = [X.detach().clone().requires_grad_(), W.clone().requires_grad_(), b.clone().requires_grad_()]
    out = gnntf.dense_step(graph, leaves[0], leaves[1], leaves[2], relu=relu, in_dropout=din, out_dropout=dout)
    assert torch.equal(out, want_out)
    out.backward(g)
    dX, dW, db = (leaf.grad for leaf in leaves)
    G = torch.from_numpy(dref.gated(host(g), host(want_out), relu, dout)).cuda()
    assert torch.equal(dW, sparse._dense_wgrad(Xd, G))              # the weight gradient with the mask made again: the same bits
    if din is not None:
        assert torch.equal(sparse._dense_wgrad_drop(graph, X, G, din), dW)
    # against float64
    Xh, Wh, bh = host(X), host(W), host(b)
    fwd = dref.forward(Xh, Wh, bh, relu, din, dout)
    back = dref.backward(Xh, Wh, host(G), din)
    ratios = dict(out=dref.ratio(host(out), fwd["out"], fwd["out_bound"]), dW=dref.ratio(host(dW), back["dW"], back["dW_bound"]),
                  db=dref.ratio(host(db).reshape(-1), back["db"], back["db_bound"]), dX=dref.ratio(host(dX), back["dX"], back["dX_bound"]))
    print(f"n={n} {F}->{O} ldx={F + pad} relu={relu} in={din} out={dout}: error / bound " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1 for v in ratios.values()), ratios
    if dout is not None and not relu:
        assert np.array_equal(host(out) == 0, ~dref.keep_mask(dout, n, O) | (fwd["out"] == 0))
    if din is not None:
        assert np.array_equal(host(dX) != 0, dref.keep_mask(din, n, F) & (host(dX) != 0)) and float(dX.abs().max()) > 0


@pytest.mark.parametrize("n,F,O", ((TALL, 256, 64), (TALL, 64, 64), (TALL, 100, 7), (300, 33, 5), (TALL, 64, 300)))
def test_without_masks_it_is_dense(gnntf, graph, n, F, O):
    X, W, b, _ = operands(n, F, O, 0)
    with torch.no_grad():
        want = gnntf.dense(X, W, b, relu=True)
        for rates in ((None, None), ((0.0, 1, 2), (0, 3, 4)), ((0.0, 1, 2), None)):
            assert torch.equal(gnntf.dense_step(graph, X, W, b, relu=True, in_dropout=rates[0], out_dropout=rates[1]), want)
        # the entry itself with rates of 0 (dense_step does not reach it then)
        from gnntf import sparse
        assert torch.equal(sparse._dense_drop_launch(graph, X, W, b, True, None, None), want)


@pytest.mark.parametrize("n,F,O", ((TALL, 256, 64), (TALL, 128, 32), (TALL, 192, 64), (300, 100, 7)))
def test_the_counter(gnntf, n, F, O):
    """Two calls with the same triple and counter give the same bits; moving the handle's dropout counter moves the streams: counter k
    with stream s is stream s + k without a counter, forward and weight gradient alike."""
    from gnntf import sparse
    coo = np.array([[0, 1], [1, 0]], dtype=np.int64)
    counted = gnntf.DeviceGraph(gnntf.SparseCOO(coo, np.ones(2, dtype=np.float32), (2, 2)), device="cuda:0")
    plain = gnntf.DeviceGraph(gnntf.SparseCOO(coo, np.ones(2, dtype=np.float32), (2, 2)), device="cuda:0")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    counted.set_dropout_counter(counter)
    X, W, b, g = operands(n, F, O, 0)
    moved = lambda triple, k: (triple[0], triple[1], triple[2] + k)
    with torch.no_grad():
        first = gnntf.dense_step(counted, X, W, b, relu=True, in_dropout=IN, out_dropout=OUT)
        assert torch.equal(first, gnntf.dense_step(counted, X, W, b, relu=True, in_dropout=IN, out_dropout=OUT))
        assert torch.equal(first, gnntf.dense_step(plain, X, W, b, relu=True, in_dropout=IN, out_dropout=OUT))
        counter.fill_(5)
        second = gnntf.dense_step(counted, X, W, b, relu=True, in_dropout=IN, out_dropout=OUT)
        assert not torch.equal(first, second)
        assert torch.equal(second, gnntf.dense_step(plain, X, W, b, relu=True, in_dropout=moved(IN, 5), out_dropout=moved(OUT, 5)))
        assert torch.equal(second, composed(gnntf, counted, X, W, b, True, IN, OUT)[0])
        fwd = dref.forward(host(X), host(W), host(b), True, IN, OUT, counter=5)
        assert dref.ratio(host(second), fwd["out"], fwd["out_bound"]) <= 1
        assert torch.equal(sparse._dense_wgrad_drop(counted, X, g, IN), sparse._dense_wgrad_drop(plain, X, g, moved(IN, 5)))
        assert torch.equal(sparse._dense_wgrad_drop(counted, X, g, IN), sparse._dense_wgrad(gnntf.feature_dropout(counted, X, *IN), g))
        counter.zero_()
        assert torch.equal(first, gnntf.dense_step(counted, X, W, b, relu=True, in_dropout=IN, out_dropout=OUT))
    counted.set_dropout_counter(None)


def test_the_node_saves_x_itself_and_allocates_no_copy_of_it(gnntf, graph):
    """The node's saved tensors are X itself, W and the result; forward + backward with a constant X never hold n * F * 4 bytes beyond
    the start -- no [n, F] temporary exists -- while torch's dropout around dense does."""
    n, F, O = 65536, 256, 32
    X, W, b, g = operands(n, F, O, 0)
    W.requires_grad_()
    b.requires_grad_()

    def peak_of(step):
        W.grad = b.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        out = step()
        out.backward(g)
        torch.cuda.synchronize()
        del out
        return torch.cuda.max_memory_allocated() - start

    out = gnntf.dense_step(graph, X, W, b, relu=True, in_dropout=IN, out_dropout=OUT)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 3 and saved[0].data_ptr() == X.data_ptr() and tuple(saved[0].shape) == (n, F) and saved[0].stride() == X.stride()
    assert saved[1].data_ptr() == W.data_ptr() and saved[2].data_ptr() == out.data_ptr()
    del out, saved
    fused = peak_of(lambda: gnntf.dense_step(graph, X, W, b, relu=True, in_dropout=IN, out_dropout=OUT))
    torchs = peak_of(lambda: torch.nn.functional.dropout(gnntf.dense(torch.nn.functional.dropout(X, 0.5), W, b, relu=True), 0.6))
    passes = peak_of(lambda: gnntf.feature_dropout(graph, gnntf.dense(gnntf.feature_dropout(graph, X, *IN), W, b, relu=True), *OUT))
    print(f"peak bytes beyond the start, n={n} {F}->{O}: dense_step {fused}, torch dropout {torchs}, counter-RNG passes {passes}; n F 4 = {n * F * 4}")
    assert fused < n * F * 4 <= torchs and n * F * 4 <= passes
    assert W.grad is not None and float(W.grad.abs().max()) > 0


# ---- the models ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cora():
    """The Cora-shaped graph with DENSE features (the graph's own are mostly zeros and would travel as SparseRows)."""
    coo, vals, shape, _ = graphs.cora_shaped(seed=4)
    rng = np.random.default_rng(4)
    X = rng.standard_normal((shape[0], 96)).astype(np.float32)
    labels = rng.integers(0, 7, size=shape[0])
    weights = [(np.random.default_rng(40 + k).standard_normal((32, 32)) / 6).astype(np.float32) for k in range(4)]
    return dict(coo=coo, vals=vals, shape=shape, X=X, labels=labels, weights=weights, train=np.arange(0, 300), valid=np.arange(300, 600))


def make_model(gnntf, cora, kind, **option):
    gnntf.set_seed(11)
    torch.manual_seed(3)
    G = gnntf.SparseCOO(cora["coo"], cora["vals"], cora["shape"])
    if kind == "appnp":
        model = gnntf.APPNP(G, cora["X"], 7, latent_dims=[64], **option)
    else:
        model = gnntf.GCNII(G, cora["X"], 7, latent_dims=[32], iterations=4, **option)
    model.reset()
    for layer, W in zip([layer for layer in model.layers() if isinstance(layer, gnntf.GCNIILayer)], cora["weights"]):
        layer.W.data.copy_(torch.from_numpy(W).cuda())       # (the reference initialises these to zero)
    return model


FUSED = dict(appnp=dict(dense_dropout="fused"), gcnii=dict(dense_dropout="fused", feature_dropout="fused"))
STREAMS = dict(appnp=12, gcnii=5)           # per step -- APPNP: the Dropout, the Dense, ten adjacencies; GCNII: the Dropout, four layers


def one_step(gnntf, cora, model):
    """One training-mode forward and backward: (logits, gradients, mask streams taken)."""
    first = model._mask_calls
    for v in model.vars():
        v.var.grad = None
    with model:
        logits = model(model.features)
        gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]]).loss(logits).backward()
    return logits.detach().clone(), [v.var.grad.clone() for v in model.vars()], model._mask_calls - first


@pytest.mark.parametrize("kind", ("appnp", "gcnii"))
def test_layer_list_eval_mode_and_the_pending_value(gnntf, cora, kind):
    from gnntf import metrics, sparse
    fused, default = make_model(gnntf, cora, kind, **FUSED[kind]), make_model(gnntf, cora, kind)
    assert default.dense_dropout == "torch" and fused.dense_dropout == "fused"
    assert [type(layer) for layer in fused.layers()] == [type(layer) for layer in default.layers()]
    if kind == "appnp":                                  # filter.py:30-35
        assert [type(layer) for layer in fused.layers()] == [gnntf.Dropout, gnntf.Dense, gnntf.Dense] + [gnntf.PPRIteration] * 10
    dropout, dense = fused.layers()[0], fused.layers()[1]
    # a training-mode forward: the pair ran as one launch, the Dropout's value is pending and is feature_dropout of the input
    first = fused._mask_calls
    with fused, torch.no_grad():
        fused(fused.features)
        assert dropout.__dict__.get("_pending_value") is not None and dropout.__dict__.get("_value") is None
        want = sparse.feature_dropout(fused.graph, fused.features, dropout.rate, metrics.current_seed(), first)
        assert torch.equal(dropout.value, want) and dropout.__dict__.get("_pending_value") is None
        assert float((want == 0).float().mean()) > 0.3
        own = kind == "appnp"                            # APPNP's Dense has a rate of its own, GCNII's has none
        redone = sparse.dense_step(fused.graph, fused.features, dense.W, dense.b, relu=True, in_dropout=(dropout.rate, metrics.current_seed(), first),
                                   out_dropout=(dense.dropout, metrics.current_seed(), first + 1) if own else None)
        assert torch.equal(dense.value, redone)
    assert fused._mask_calls - first == STREAMS[kind]
    # eval mode: today's path and bits
    outs = []
    default.training_mode(False)                         # (a fresh container starts in training mode, layered.py:9)
    for model in (fused, default):
        assert not model.is_training()
        with torch.no_grad():
            outs.append(model(model.features))
    assert torch.equal(outs[0], outs[1]) and fused.layers()[0].__dict__.get("_pending_value") is None


@pytest.mark.parametrize("kind", ("appnp", "gcnii"))
def test_reproducible_from_the_seed_and_fuse_runs_off(gnntf, cora, kind):
    # (APPNP with its iterations collapsed into one PPRLoop layer, so that fuse_runs decides about the Dropout / Dense pair alone: the
    # run of PPRIteration layers has a switch-off of its own, whose backward associates differently)
    collapsed = dict(FUSED[kind], fused=True) if kind == "appnp" else FUSED[kind]
    one = one_step(gnntf, cora, make_model(gnntf, cora, kind, **collapsed))
    two = one_step(gnntf, cora, make_model(gnntf, cora, kind, **collapsed))
    assert one[2] == two[2] == STREAMS[kind]
    assert torch.equal(one[0], two[0]) and all(torch.equal(a, b) for a, b in zip(one[1], two[1]))
    assert len(one[1]) >= 4 and all(float(grad.abs().max()) > 0 for grad in one[1][:2])
    apart = make_model(gnntf, cora, kind, **collapsed)
    apart.fuse_runs = False                              # the layers run one by one: the counter RNG's pass, then the Dense with its own mask
    three = one_step(gnntf, cora, apart)
    assert three[2] == STREAMS[kind] and apart.layers()[0].__dict__.get("_pending_value") is None
    assert torch.equal(one[0], three[0]) and all(torch.equal(a, b) for a, b in zip(one[1], three[1]))
    other = make_model(gnntf, cora, kind, **collapsed)
    gnntf.set_seed(12)                                   # the same parameters, other masks
    assert not torch.equal(one_step(gnntf, cora, other)[0], one[0])
    # two training runs from one seed give equal parameters
    finals = []
    for _ in range(2):
        model = make_model(gnntf, cora, kind, **FUSED[kind])
        gnntf.set_seed(11)
        torch.manual_seed(5)
        model.train(train=gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]]),
                    valid=gnntf.NodeClassification(cora["valid"], cora["labels"][cora["valid"]]), epochs=3, patience=50)
        finals.append([v.var.detach().clone() for v in model.vars()])
    assert all(torch.equal(a, b) for a, b in zip(*finals))


@pytest.mark.parametrize("kind", ("appnp", "gcnii"))
def test_captured_training_equals_eager(gnntf, cora, kind):
    """train(capture=True) for 3 epochs, bit for bit the eager run on every parameter (the pattern of tests/test_gpu_gcnii_drop.py)."""
    results = []
    for capture in (False, True):
        model = make_model(gnntf, cora, kind, **FUSED[kind])
        gnntf.set_seed(11)
        torch.manual_seed(5)
        valid = gnntf.NodeClassification(cora["valid"], cora["labels"][cora["valid"]])
        model.train(train=gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]]), valid=valid, epochs=3, patience=50,
                    capture=capture, optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
        results.append(([v.var.detach().clone() for v in model.vars()], float(model.loss(valid)), model._mask_calls))
    (eager, eager_loss, eager_masks), (captured, captured_loss, captured_masks) = results
    assert eager_masks == captured_masks == 3 * STREAMS[kind]
    print("captured vs eager, max |difference| per variable:", [float((e - c).abs().max()) for e, c in zip(eager, captured)])
    assert all(torch.equal(e, c) for e, c in zip(eager, captured)) and eager_loss == captured_loss
