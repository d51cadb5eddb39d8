"""The fused feature dropout of the GCNII training layer on the MI355X (gnx_gcnii_step_drop, gnx_feature_dropout,
gnx_feature_dropout_back, sparse.gcnii_step(dropout=), sparse.feature_dropout, GCNII(feature_dropout="fused")).  The mask is a
function of (seed, stream, row, column) alone, so every comparison is exact: the existing entry times the mask built in numpy from
the oracle's hash, the pass entries against the same mask, the dropout counter, reproducibility, autograd against the composition
with an explicit mask over today's _GCNIIStep, and the model: seeds, capture against eager, the default and eval mode untouched."""
import functools

import numpy as np
import pytest
import torch

import graphs
from oracle import gnntf_oracle as orc

pytestmark = pytest.mark.gpu

A_MIX = 0.1
N, HUB, N_HUB = 3000, 1500, 900
WIDTHS = (16, 32, 64, 40, 7)
RATES = (0.6, 0.25)
SEED, STREAM = 7, 2
PLAIN = {True: "spmm_gcnii_mfma", False: "spmm+dense_mfma"}


def kernel_for(C, dropped=True):
    return PLAIN[C in (16, 32, 64)] + ("_drop" if dropped else "")


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()           # (a copy: the shared operands are read-only)


def host(t):
    return t.detach().cpu().numpy()


def directed_coo():
    """The graph of tests/test_gpu_gcnii_back.py: DIRECTED, 3 000 vertices, about 20 000 entries, no duplicates; sources below 2 900
    and targets from 100 up, so vertices 0 .. 99 have no in-edges; column 1 500 holds 900 entries."""
    rng = np.random.default_rng(11)
    src, dst = rng.integers(0, N - 100, size=19100), rng.integers(100, N, size=19100)
    hub_src = rng.permutation(N - 100)[:N_HUB]
    key = np.unique(np.concatenate([src * N + dst, hub_src * N + HUB]))
    coo = np.stack([key // N, key % N], axis=1).astype(np.int64)
    coo = coo[rng.permutation(len(coo))]
    vals = rng.uniform(0.5, 1.5, size=len(coo)).astype(np.float32)
    return coo, vals, (N, N)


@pytest.fixture(scope="module")
def shared(gnntf):
    """Two handles, made once and never changed: the graph itself (rows of a few entries, 100 rows without entries at the end) and
    its TRANSPOSE, whose forward structure has the hub row (900 entries, above the long-row threshold of 512) and 100 rows without
    entries at the start.  ``t`` is the one most tests use."""
    coo, vals, shape = directed_coo()
    out = dict()
    for name, idx in (("a", coo), ("t", coo[:, ::-1].copy())):
        g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, vals, shape), device="cuda:0")
        rowptr = host(g.csr_arrays()[0])
        deg = np.diff(rowptr)
        out[name] = dict(g=g, adj=gnntf.normalize(g, "symmetric"), deg=deg, hub=np.flatnonzero(deg > 512), empty=np.flatnonzero(deg == 0))
    assert 19000 < len(coo) < 21000 and N % 16 != 0
    assert len(out["t"]["hub"]) >= 1 and HUB in out["t"]["hub"] and out["t"]["deg"][HUB] >= N_HUB     # a hub row in the FORWARD structure
    assert len(out["t"]["empty"]) >= 100 and len(out["a"]["empty"]) >= 100 and len(out["a"]["hub"]) == 0
    return out


@functools.lru_cache(maxsize=None)
def keep_mask(seed, stream, p, n, C):
    """The mask in numpy, from the oracle's integers: kept iff hash_u24(seed, stream, row, col, 0) >= dropout_threshold(p)."""
    rows, cols = np.repeat(np.arange(n), C), np.tile(np.arange(C), n)
    keep = orc.hash_u24(seed, stream, rows, cols, np.zeros(n * C, dtype=np.int64)) >= orc.dropout_threshold(p)
    keep = keep.reshape(n, C)
    keep.setflags(write=False)
    return keep


def scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropped(x, keep, p):
    assert x.dtype == np.float32
    return np.where(keep, x * scale(p), np.float32(0))


@functools.lru_cache(maxsize=None)
def operands(C):
    rng = np.random.default_rng(C)
    H, H0 = rng.standard_normal((N, C)).astype(np.float32), rng.standard_normal((N, C)).astype(np.float32)
    M = (0.6 * np.eye(C) + 0.4 * rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
    up = rng.standard_normal((N, C)).astype(np.float32)
    for x in (H, H0, M, up):
        x.setflags(write=False)
    return H, H0, M, up


# ---- 1. the forward: the existing entry times the mask ----------------------------------------------------------------------------------
@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("C", WIDTHS)
def test_forward_is_the_plain_entry_times_the_mask(gnntf, shared, C, p):
    sparse = gnntf.sparse
    H, H0, M, _ = operands(C)
    Hd, H0d, Md = dev(H), dev(H0), dev(M)
    keep = keep_mask(SEED, STREAM, p, N, C)
    for name in ("t", "a"):
        g, adj, hub, empty = (shared[name][k] for k in ("g", "adj", "hub", "empty"))
        for relu in (True, False):
            plain = gnntf.gcnii_step(adj, Hd, H0d, A_MIX, Md, relu=relu)
            assert g.last_kernel() == kernel_for(C, dropped=False)
            got = gnntf.gcnii_step(adj, Hd, H0d, A_MIX, Md, relu=relu, dropout=(p, SEED, STREAM))
            assert g.last_kernel() == kernel_for(C)
            want = dropped(host(plain), keep, p)
            np.testing.assert_array_equal(host(got), want)
            if not relu:                              # the comparison above is not vacuous on hub rows, rows without entries and the last
                for rows in (hub, empty, np.arange(N - N % 16, N)):      # partial tile: both kept and dropped values, exactly the mask's
                    if len(rows):                     # (the graph itself has no hub row)
                        assert 0 < keep[rows].mean() < 1
                        np.testing.assert_array_equal(host(got)[rows] != 0, keep[rows] & (host(plain)[rows] != 0))
            # the training form: the same out, and T bit for bit the T of gnx_gcnii_step
            out_T, T = sparse._gcnii_launch(adj, Hd, H0d, A_MIX, Md, relu, keep_mixed=True, dropout=(p, SEED, STREAM))
            _, T_plain = sparse._gcnii_launch(adj, Hd, H0d, A_MIX, Md, relu, keep_mixed=True)
            assert torch.equal(T, T_plain)
            np.testing.assert_array_equal(host(out_T), want)


@pytest.mark.parametrize("C", WIDTHS)
def test_rate_zero_is_the_plain_entry(gnntf, shared, C):
    sparse = gnntf.sparse
    H, H0, M, _ = operands(C)
    Hd, H0d, Md = dev(H), dev(H0), dev(M)
    g, adj = shared["t"]["g"], shared["t"]["adj"]
    plain = gnntf.gcnii_step(adj, Hd, H0d, A_MIX, Md)
    assert torch.equal(gnntf.gcnii_step(adj, Hd, H0d, A_MIX, Md, dropout=(0.0, SEED, STREAM)), plain)
    out, _ = sparse._gcnii_launch(adj, Hd, H0d, A_MIX, Md, True, keep_mixed=False, dropout=(0.0, SEED, STREAM))    # the C entry itself
    assert torch.equal(out, plain) and g.last_kernel() == kernel_for(C, dropped=False)
    X = dev(H)
    assert torch.equal(sparse._feature_dropout_launch(g, X, 0.0, SEED, STREAM), X)


def test_entry_refuses_a_bad_rate(gnntf, shared):
    nat = gnntf.sparse.nat
    H, H0, M, _ = operands(16)
    Hd, H0d, Md, out = dev(H), dev(H0), dev(M), torch.empty(N, 16, device="cuda")
    for p in (1.0, -0.1, float("nan")):
        rc = nat.lib().gnx_gcnii_step_drop(shared["t"]["g"].handle, None, nat.ptr(Hd), nat.ptr(H0d), A_MIX, 16, nat.ptr(Md), 16, 1, p, SEED,
                                           STREAM, nat.ptr(out), None, nat.current_stream())
        assert rc == -1 and b"outside [0, 1)" in nat.lib().gnx_last_error()


# ---- 2. the pass entries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("C", WIDTHS)
def test_feature_dropout_pass(gnntf, shared, C, p):
    sparse = gnntf.sparse
    g, hub = shared["t"]["g"], shared["t"]["hub"]
    X = operands(C)[0]
    keep = keep_mask(SEED, STREAM, p, N, C)
    want = dropped(X, keep, p)
    np.testing.assert_array_equal(host(sparse._feature_dropout_launch(g, dev(X), p, SEED, STREAM)), want)          # out of place
    np.testing.assert_array_equal(host(gnntf.feature_dropout(g, dev(X), p, SEED, STREAM)), want)                   # the functional form
    Xd = dev(X)
    assert sparse._feature_dropout_launch(g, Xd, p, SEED, STREAM, out=Xd) is Xd                                     # in place
    np.testing.assert_array_equal(host(Xd), want)
    for rows in (hub, np.random.default_rng(C).permutation(N)[:777]):                                              # row lists
        listed = np.zeros((N, 1), dtype=bool)
        listed[rows] = True
        want_rows = np.where(listed, want, X)
        rows_d = dev(rows.astype(np.int32))
        np.testing.assert_array_equal(host(sparse._feature_dropout_launch(g, dev(X), p, SEED, STREAM, rows=rows_d)), want_rows)
        Xd = dev(X)
        sparse._feature_dropout_launch(g, Xd, p, SEED, STREAM, rows=rows_d, out=Xd)
        np.testing.assert_array_equal(host(Xd), want_rows)
    # rows inside a wider buffer (row stride above C; at C = 7 the rows are not 16-byte aligned either)
    wide = torch.full((N, C + 5), 9.0, device="cuda")
    wide[:, :C] = dev(X)
    out = torch.full((N, C + 8), 9.0, device="cuda")
    sparse._feature_dropout_launch(g, wide[:, :C], p, SEED, STREAM, out=out[:, :C])
    np.testing.assert_array_equal(host(out[:, :C]), want)
    assert bool((out[:, C:] == 9.0).all())


@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("C", WIDTHS)
def test_feature_dropout_back_pass(gnntf, shared, C, p):
    sparse = gnntf.sparse
    nat = sparse.nat
    g = shared["t"]["g"]
    X, _, _, up = operands(C)
    keep = keep_mask(SEED, STREAM, p, N, C)
    y = dropped(np.maximum(X, np.float32(0)), keep, p)                      # the DROPPED forward output of a relu layer
    want_relu = np.where(keep & (y > 0), up * scale(p), np.float32(0))
    want_none = np.where(keep, up * scale(p), np.float32(0))
    np.testing.assert_array_equal(host(sparse._feature_dropout_back(g, dev(up), dev(y), p, SEED, STREAM, relu=True)), want_relu)
    np.testing.assert_array_equal(host(sparse._feature_dropout_back(g, dev(up), None, p, SEED, STREAM, relu=False)), want_none)
    for act, yd, want in ((nat.ACT_RELU, dev(y), want_relu), (nat.ACT_NONE, None, want_none)):       # aliased: G is g
        G = dev(up)
        nat.check(nat.lib().gnx_feature_dropout_back(g.handle, nat.ptr(G), C, nat.ptr(yd), C if yd is not None else 0, N, C, p, SEED, STREAM,
                                                     act, nat.ptr(G), C, nat.current_stream()))
        np.testing.assert_array_equal(host(G), want)


# ---- 3. the dropout counter --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 40])
def test_dropout_counter_shifts_the_stream(gnntf, shared, C):
    sparse = gnntf.sparse
    g, adj = shared["t"]["g"], shared["t"]["adj"]
    H, H0, M, up = operands(C)
    Hd, H0d, Md, upd = dev(H), dev(H0), dev(M), dev(up)
    want = gnntf.gcnii_step(adj, Hd, H0d, A_MIX, Md, dropout=(0.6, SEED, 8))
    want_pass = sparse._feature_dropout_launch(g, Hd, 0.6, SEED, 8)
    want_back = sparse._feature_dropout_back(g, upd, want, 0.6, SEED, 8, relu=True)
    counter = torch.tensor([3], dtype=torch.int64, device="cuda")
    g.set_dropout_counter(counter)
    try:
        got = gnntf.gcnii_step(adj, Hd, H0d, A_MIX, Md, dropout=(0.6, SEED, 5))
        got_pass = sparse._feature_dropout_launch(g, Hd, 0.6, SEED, 5)
        got_back = sparse._feature_dropout_back(g, upd, got, 0.6, SEED, 5, relu=True)
        torch.cuda.synchronize()
    finally:
        g.set_dropout_counter(None)
    assert torch.equal(got, want) and torch.equal(got_pass, want_pass) and torch.equal(got_back, want_back)
    assert torch.equal(gnntf.gcnii_step(adj, Hd, H0d, A_MIX, Md, dropout=(0.6, SEED, 8)), want)        # the counter is gone again


# ---- 4. reproducibility ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 64, 40])
def test_two_calls_give_the_same_bits_and_streams_differ(gnntf, shared, C):
    adj = shared["t"]["adj"]
    H, H0, M, _ = operands(C)
    Hd, H0d, Md = dev(H), dev(H0), dev(M)
    first = gnntf.gcnii_step(adj, Hd, H0d, A_MIX, Md, relu=False, dropout=(0.6, SEED, STREAM))
    second = gnntf.gcnii_step(adj, Hd, H0d, A_MIX, Md, relu=False, dropout=(0.6, SEED, STREAM))
    other = gnntf.gcnii_step(adj, Hd, H0d, A_MIX, Md, relu=False, dropout=(0.6, SEED, STREAM + 1))
    reseeded = gnntf.gcnii_step(adj, Hd, H0d, A_MIX, Md, relu=False, dropout=(0.6, SEED + 1, STREAM))
    assert torch.equal(first, second)
    for different in (other, reseeded):
        assert 0.2 < float(((first != 0) != (different != 0)).float().mean()) < 0.8


# ---- 5. autograd: the fused step against the composition with an explicit mask ------------------------------------------------------------
@pytest.mark.parametrize("backward", ["composed", "fused"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C", [16, 64, 40])
def test_autograd_against_the_explicit_mask(gnntf, shared, C, relu, backward):
    sparse = gnntf.sparse
    p = 0.6
    H, H0, M, up = operands(C)
    upd = dev(up)
    mask_scale = dev(np.where(keep_mask(SEED, STREAM, p, N, C), scale(p), np.float32(0)))
    constant = shared["t"]["adj"]
    edge_dropped = sparse.DroppedAdjacency(shared["t"]["g"], 0.5, 1, 0)
    for adj in (constant, edge_dropped):
        def run(fused_dropout):
            leaves = [dev(x).requires_grad_() for x in (H, H0, M)]
            if fused_dropout:
                out = gnntf.gcnii_step(adj, *leaves[:2], A_MIX, leaves[2], relu=relu, backward=backward, dropout=(p, SEED, STREAM))
            else:
                out = gnntf.gcnii_step(adj, *leaves[:2], A_MIX, leaves[2], relu=relu, backward=backward) * mask_scale
            out.backward(upd)
            return [out.detach()] + [leaf.grad for leaf in leaves]

        got, want = run(True), run(False)
        for name, a_, b_ in zip(("out", "dH", "dH0", "dM"), got, want):
            assert a_ is not None and b_ is not None
            np.testing.assert_array_equal(host(a_), host(b_), err_msg=name)
        assert float(got[1].abs().max()) > 0 and float(got[3].abs().max()) > 0


# ---- 6. the model ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cora():
    coo, vals, shape, X = graphs.cora_shaped(seed=4)
    labels = np.random.default_rng(4).integers(0, 7, size=shape[0])
    weights = [(np.random.default_rng(40 + k).standard_normal((32, 32)) / 6).astype(np.float32) for k in range(4)]
    return dict(coo=coo, vals=vals, shape=shape, X=X, labels=labels, weights=weights, train=np.arange(0, 300), valid=np.arange(300, 600))


def make_model(gnntf, cora, seeded_weights=True, **option):
    gnntf.set_seed(11)
    torch.manual_seed(3)
    model = gnntf.GCNII(gnntf.SparseCOO(cora["coo"], cora["vals"], cora["shape"]), cora["X"], 7, latent_dims=[32], iterations=4, **option)
    model.reset()
    convs = [layer for layer in model.layers() if isinstance(layer, gnntf.GCNIILayer)]
    assert len(convs) == 4
    if seeded_weights:                                  # the reference initialises W to zero: M would be a multiple of the identity
        for layer, W in zip(convs, cora["weights"]):
            layer.W.data.copy_(dev(W))
    return model


def three_steps(gnntf, cora, model):
    """Three plain gradient steps in training mode; (losses, gradients of every step, mask streams taken)."""
    task = gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]])
    losses, grads = [], []
    first = model._mask_calls
    for _ in range(3):
        with model:
            for v in model.vars():
                v.var.grad = None
            loss = task.loss(model(model.features))
            loss.backward()
        losses.append(float(loss.detach()))
        grads.append([v.var.grad.clone() for v in model.vars()])
        with torch.no_grad():
            for v in model.vars():
                v.var -= 0.05 * v.var.grad
    return losses, grads, model._mask_calls - first


def test_model_is_reproducible_from_the_seed(gnntf, cora):
    one = three_steps(gnntf, cora, make_model(gnntf, cora, feature_dropout="fused"))
    two = three_steps(gnntf, cora, make_model(gnntf, cora, feature_dropout="fused"))
    assert one[2] == two[2] == 3 * 5                    # per step: the input features' mask and one per GCNII layer
    assert one[0] == two[0]
    for step_one, step_two in zip(one[1], two[1]):
        assert len(step_one) > 4 and all(torch.equal(a_, b_) for a_, b_ in zip(step_one, step_two))
    model = make_model(gnntf, cora, feature_dropout="fused")
    gnntf.set_seed(12)                                  # the same parameters, other masks
    other = three_steps(gnntf, cora, model)
    assert other[0] != one[0] and not all(torch.equal(a_, b_) for a_, b_ in zip(other[1][0], one[1][0]))


def test_captured_training_equals_eager(gnntf, cora, monkeypatch):
    """train(capture=True) for 3 epochs, bit for bit the eager run: parameters, the held-out loss of every epoch (what train() hands
    its early-stopping bookkeeping, training._BestSoFar.observe) and the one after training (the pattern of
    tests/test_gpu_bf16_training.py: both runs get the capturable Adam the captured run builds for itself)."""
    from gnntf import training
    observed, observe = [], training._BestSoFar.observe
    monkeypatch.setattr(training._BestSoFar, "observe", lambda self, loss: (observed[-1].append(loss), observe(self, loss))[1])
    results = []
    for capture in (False, True):
        observed.append([])
        model = make_model(gnntf, cora, seeded_weights=False, feature_dropout="fused")
        gnntf.set_seed(11)
        torch.manual_seed(5)
        valid = gnntf.NodeClassification(cora["valid"], cora["labels"][cora["valid"]])
        model.train(train=gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]]), valid=valid, epochs=3, patience=50,
                    capture=capture, optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
        results.append(([v.var.detach().clone() for v in model.vars()], float(model.loss(valid)), model._mask_calls))
    (eager, eager_loss, eager_masks), (captured, captured_loss, captured_masks) = results
    assert eager_masks == captured_masks == 3 * 5
    print("captured vs eager, max |difference| per variable:", [float((e - c).abs().max()) for e, c in zip(eager, captured)])
    assert all(torch.equal(e, c) for e, c in zip(eager, captured))
    assert eager_loss == captured_loss
    print("held-out losses per epoch, eager / captured:", observed)
    assert len(observed[0]) == len(observed[1]) == 3 and observed[0] == observed[1] and len(set(observed[0])) == 3


def test_default_keeps_its_kernel_and_eval_mode_is_untouched(gnntf, cora):
    fused, default = make_model(gnntf, cora, feature_dropout="fused"), make_model(gnntf, cora)
    assert default.feature_dropout == "torch" and make_model(gnntf, cora, feature_dropout="torch").feature_dropout == "torch"
    for model, kernel in ((fused, "spmm_gcnii_mfma_drop"), (default, "spmm_gcnii_mfma")):
        with model, torch.no_grad():                    # a training-mode forward
            model(model.features)
        assert model.graph.last_kernel() == kernel
    outs = []
    for model in (fused, default):                      # the same weights: eval-mode forwards agree bit for bit
        assert not model.is_training()
        with torch.no_grad():
            outs.append(model(model.features))
        assert model.graph.last_kernel() == "spmm_gcnii_mfma"
    assert torch.equal(outs[0], outs[1]) and float(outs[0].abs().max()) > 0
