"""Sparse input features (SparseRows, sparse_dense, _SparseDense in gnntf/sparse.py) against float64: the one model-level user of
the rectangular + bias-row + relu + transposed combination of the f32 SpMM.  Forward and backward at shapes with hub rows (a
document with more than 512 features) and hub columns (a feature in more than 512 rows: the weight gradient walks long rows),
under a pending stored-entry dropout with the oracle's keep mask, on a COO with duplicates, at the degenerate shapes; then one
whole training step and captured training with the stored-entry dropout running for real.

The bound is the one of tests/spmm_forms_ref.py, over the structure for the forward and over its transpose for dW."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import graphs
import spmm_forms_ref as R
from gcnii_shapes_ref import U32, plan_threshold
from oracle import gnntf_oracle as orc

pytestmark = pytest.mark.gpu
DEVICE = "cuda:0"
SEED, STREAM = 77, 3


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device(DEVICE)
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEVICE)


def features(name):
    """(idx, vals, shape) of a sparse feature matrix."""
    if name in ("Ta", "Tt", "Sa"):                   # the rectangular long-row structures: hub rows (a), hub columns (t)
        st = R.structure(name[0], name[1], True)
        return st["coo"], st["vals"], st["shape"]
    if name == "1x5":
        return np.array([[0, 0], [0, 3], [0, 4]], dtype=np.int64), np.array([0.5, -1.5, 2.0], dtype=np.float32), (1, 5)
    if name == "5x1":
        return np.array([[0, 0], [2, 0], [4, 0]], dtype=np.int64), np.array([1.25, 0.5, -0.75], dtype=np.float32), (5, 1)
    if name == "empty":
        return np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.float32), (6, 4)
    assert name == "dups"                            # a COO given sparse with a fifth of its entries stored again, other values
    return graphs.random_coo(300, 90, 2500, seed=4, weighted=True, dup_frac=0.2)


CASES = [(name, *rest) for name in ("Ta", "Tt") for rest in
         ((1, True, False, 0.1), (7, False, True, 0.5), (16, True, True, 0.9), (64, True, True, 0.0), (100, False, False, 0.0), (260, True, False, 0.5))]
CASES += [("Sa", 64, True, True, 0.5), ("Sa", 260, False, False, 0.0),
          ("1x5", 7, True, True, 0.5), ("1x5", 1, False, False, 0.0), ("5x1", 16, True, False, 0.5), ("5x1", 1, True, True, 0.0),
          ("empty", 7, True, True, 0.5), ("empty", 16, False, False, 0.0),
          ("dups", 16, True, True, 0.5), ("dups", 100, True, False, 0.9), ("dups", 7, False, True, 0.1), ("dups", 64, True, True, 0.0)]
RATIOS = {}


def contiguous_vec(O):
    return 4 if O % 4 == 0 else 2 if O % 2 == 0 else 1


@pytest.mark.parametrize("name,O,bias,relu,p", CASES, ids=lambda v: str(v))
def test_sparse_dense_forward_and_backward(gnntf, name, O, bias, relu, p):
    idx, vals, shape = features(name)
    n, F = shape
    g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, vals, shape), device=DEVICE)
    rows = gnntf.SparseRows(g)
    if p:
        rows = rows.with_dropout(p, SEED, STREAM)
    # ---- the float32 weights the launches read, against the oracle's keep mask over the stored entries in their given order
    rowptr, colidx, raw = (t.cpu().numpy() for t in g.csr_arrays())
    adj = rows.adjacency()
    w = raw if adj.vals is None else adj.vals.cpu().numpy()
    A = sp.csr_matrix((w.astype(np.float64), colidx, rowptr), shape=shape)
    keep = orc.keep_mask(idx, p, SEED, STREAM) if p else np.ones(len(idx), dtype=bool)
    scale = np.float32(1) / (np.float32(1) - np.float32(p))          # the library's float32 scale (gnx_internal.h: drop_scale)
    kept = sp.coo_matrix((np.where(keep, (vals * scale).astype(np.float64), 0.0), (idx[:, 0], idx[:, 1])), shape=shape).tocsr()
    kept.sort_indices()
    assert np.array_equal(kept.indptr, rowptr) and np.array_equal(kept.indices, colidx)
    np.testing.assert_allclose(A.data, kept.data, rtol=4 * U32 if name == "dups" else 0, atol=0)   # (a slot of duplicates: a float32 sum)
    if p and len(idx) > 100:
        assert abs(keep.mean() - (1 - p)) < 0.05
    At = sp.csr_matrix(A.T)
    At.sort_indices()
    deg, deg_t, L, L_t = np.diff(A.indptr), np.diff(At.indptr), plan_threshold(n), plan_threshold(F)
    # ---- forward
    rng = np.random.default_rng([O, n])
    W, b = rng.standard_normal((F, O)).astype(np.float32), rng.standard_normal((1, O)).astype(np.float32)
    Wt, bt = dev(W).requires_grad_(), dev(b).requires_grad_() if bias else None
    out = gnntf.sparse_dense(rows, Wt, bt, relu=relu)
    fwd_name = g.last_kernel()
    ref = R.reference(A, deg, L, W, np.broadcast_to(b, (n, O)) if bias else None, None, beta=1.0, alpha=1.0, relu=relu)
    got = out.detach().cpu().numpy()
    r_f = R.ratio(got, ref["want"], ref["bound"])
    # ---- backward: dW = Xd^T g' over the transposed structure, db = the column sums of g'
    gout = rng.standard_normal((n, O)).astype(np.float32)
    out.backward(dev(gout))
    bwd_name = g.last_kernel()
    gate = gout * (got > 0) if relu else gout                        # the kernel's own gate: the forward bound judges where it lies
    ref_t = R.reference(At, deg_t, L_t, gate, None, None, beta=1.0, alpha=0.0)
    dW = Wt.grad.cpu().numpy()
    r_w = R.ratio(dW, ref_t["want"], ref_t["bound"])
    unreferenced = np.asarray(abs(At).sum(axis=1)).ravel() == 0       # features that no kept entry references
    assert (dW[unreferenced] == 0).all(), (name, O, p, "a feature without a kept entry got a gradient")
    if p == 0.9 and name in ("Ta", "Tt"):
        assert unreferenced.sum() > 16                                # (features whose every entry was dropped, not only empty columns)
    r_b = 0.0
    if bias:
        db = bt.grad.cpu().numpy()
        assert db.shape == (1, O)
        want_b = gate.astype(np.float64).sum(0, keepdims=True)
        r_b = R.ratio(db, want_b, (n + 4) * U32 * np.abs(gate.astype(np.float64)).sum(0, keepdims=True))
    print(f"{name} O={O} bias={bias} relu={relu} p={p}: {fwd_name} / {bwd_name}; error / bound forward {r_f:.3f} dW {r_w:.3f} db {r_b:.3f}")
    for what, r in (("forward", r_f), ("dW", r_w), ("db", r_b)):
        RATIOS[what, name] = max(RATIOS.get((what, name), 0.0), r)
    assert r_f <= 1.0 and r_w <= 1.0 and r_b <= 1.0, (name, O, bias, relu, p, r_f, r_w, r_b)
    if relu and got.size > 50:
        assert 0.2 < (got > 0).mean() < 0.8
    # ---- the launches are the ones the shapes were chosen for
    if name in ("Ta", "Tt", "Sa"):
        vec = contiguous_vec(O)
        assert fwd_name == R.kernel_name(O, vec, n, int((deg > L).sum())), fwd_name
        assert bwd_name == R.kernel_name(O, vec, F, int((deg_t > L_t).sum())), bwd_name
        assert (deg > L).any() == (name[1] == "a") and (deg_t > L_t).any() == (name[1] == "t")


# ---- one whole training step, the stored-entry input dropout running for real ------------------------------------------------------
class FixedMasks:
    """Dense feature-dropout masks drawn once on the host and handed out in call order (tests/test_gpu_training.py)."""

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


@pytest.mark.parametrize("given", ["dense", "sparse"])
def test_whole_training_step_with_stored_entry_dropout_matches_dense_float64(gnntf, given):
    """APPNP on Cora-shaped features: Dropout(0.5) on the STORED ENTRIES (counter RNG, the model's own stream numbering), Dense(relu,
    dropout 0.6) and Dense with fixed dense masks, K x PPRIteration with edge dropout, CE + L2; loss and all four gradients.  The
    reference reproduces the input mask from (metrics.current_seed(), stream): the first stream the step draws."""
    from gnntf import metrics
    from gnntf.protocol import Layered
    from gnntf.training import _Objective
    hidden, classes, K, a, wd = 16, 5, 10, 0.1, 5e-4
    coo, vals, shape, X = graphs.cora_shaped(seed=6, n=600, m=1500, f=300, density=0.02)
    n, F = X.shape
    xi = np.stack(np.nonzero(X), 1).astype(np.int64)                 # row-major: the order SparseRows.from_dense stores
    rng = np.random.default_rng(5)
    labels = rng.integers(0, classes, size=n)
    train = np.arange(0, 200)
    gnntf.set_seed(17)
    feats = X if given == "dense" else gnntf.SparseCOO(xi, X[xi[:, 0], xi[:, 1]], X.shape)
    model = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), feats, num_classes=classes, latent_dims=[hidden], iterations=K, a=a)
    model.reset()
    assert isinstance(model._input_features(), gnntf.SparseRows)
    dense = [l for l in model.layers() if isinstance(l, gnntf.Dense)]
    params = [dense[0].W, dense[0].b, dense[1].W, dense[1].b]
    with torch.no_grad():
        dense[0].b.copy_(torch.from_numpy(rng.uniform(-0.1, 0.1, size=(1, hidden)).astype(np.float32)))
        dense[1].b.copy_(torch.from_numpy(rng.uniform(-0.1, 0.1, size=(1, classes)).astype(np.float32)))
    masks = FixedMasks(23)

    def dropout(feats, p=0.5):                                        # only the dense hidden-layer masks are fixed
        if isinstance(feats, gnntf.SparseRows) or not model.is_training() or p == 0:
            return Layered.dropout(model, feats, p)
        return feats * torch.from_numpy(masks.mask(tuple(feats.shape), p)).to(feats.device, feats.dtype)
    model.dropout = dropout
    seed, first_stream = metrics.current_seed(), model._mask_calls
    with model:
        loss = _Objective(model, gnntf.NodeClassification(train, labels[train]), wd)()
        loss.backward()
    assert model._mask_calls == first_stream + 1 + K                  # the input mask, then one per iteration
    got = [float(loss.detach())] + [p.grad.cpu().numpy().astype(np.float64) for p in params]

    masks.rewind()
    W1, b1, W2, b2 = [torch.tensor(p.detach().cpu().numpy().astype(np.float64), requires_grad=True) for p in params]
    keep = orc.keep_mask(xi, 0.5, seed, first_stream)
    assert 0.4 < keep.mean() < 0.6
    Xd = np.zeros(X.shape)
    Xd[xi[keep, 0], xi[keep, 1]] = X[xi[keep, 0], xi[keep, 1]].astype(np.float64) * 2.0
    H = torch.relu(torch.from_numpy(Xd) @ W1 + b1)
    H = H * torch.from_numpy(masks.mask((n, hidden), 0.6))
    H0 = H @ W2 + b2
    Hk = H0
    for k in range(K):
        ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=0.5, training=True, seed=seed, stream=first_stream + 1 + k, dtype=np.float64)
        Hk = (torch.from_numpy(orc.to_dense(ai, av, shape, dtype=np.float64)) @ Hk) * (1 - a) + H0 * a
    logp = torch.log_softmax(Hk[torch.from_numpy(train)], dim=1)
    want_loss = torch.nn.functional.cross_entropy(logp, torch.from_numpy(labels[train]))
    want_loss = want_loss + wd * ((W1 ** 2).sum() / 2 + (b1 ** 2).sum() / 2)
    want_loss.backward()
    want = [float(want_loss)] + [t.grad.numpy() for t in (W1, b1, W2, b2)]
    assert abs(got[0] - want[0]) <= 1e-5 * abs(want[0]), (got[0], want[0])
    for name, g_, w_ in zip(("dW1", "db1", "dW2", "db2"), got[1:], want[1:]):
        np.testing.assert_allclose(g_, w_, rtol=1e-3, atol=2e-5 * np.abs(w_).max(), err_msg=name)
    assert np.abs(want[1]).max() > 1e-4 and np.abs(want[3]).max() > 1e-4
    # the step without the input dropout is another step: the mask is not a no-op the comparison could miss
    dead = (np.abs(Xd).sum(0) == 0) & (np.abs(X).sum(0) > 0)
    assert dead.any() and np.allclose(got[1][dead], wd * params[0].detach().cpu().numpy().astype(np.float64)[dead], rtol=1e-5, atol=0)


# ---- captured training ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", ["sparse", "dense"])
def test_captured_training_equals_eager_with_sparse_features(gnntf, given):
    """train(capture=True) with input features given sparse, and with dense ones the model converts: the stored-entry dropout of the
    input draws from the counter RNG, so its handle must carry the device counter that advances the streams per replay -- without it
    every replay would drop the same entries.  Eager and captured runs draw the same 12 x 3 masks and end at the same parameters.
    The runs use no weight decay: what is compared is the masks.  Measured on the MI355X (profiles/NOTES.md): without it the two runs
    agree to 6.6e-7; with the default 5e-4, 4 of the 3200 elements of W1, all of hidden unit 11, differ by up to 1.9e-3 -- the same 4
    by the same amounts whether the features are given sparse or dense, so not the counter: Adam's normalised step (the capturable
    form computes its bias corrections in float32 on the device) magnifies a 1e-7 difference on a unit that is active on next to no
    row.  With the feature graph's counter taken out, 3105 of the 3200 elements leave the tolerance: frozen masks show."""
    coo, vals, shape, X = graphs.cora_shaped(seed=8, n=800, m=2400, f=200, density=0.03)
    xi = np.stack(np.nonzero(X), 1).astype(np.int64)
    labels = np.random.default_rng(4).integers(0, 4, size=shape[0])
    train, valid = np.arange(0, 200), np.arange(200, 400)

    def build():
        gnntf.set_seed(11)
        torch.manual_seed(3)
        feats = X if given == "dense" else gnntf.SparseCOO(xi, X[xi[:, 0], xi[:, 1]], X.shape)
        model = gnntf.GNN(gnntf.SparseCOO(coo, vals, shape), feats)
        model.add(gnntf.Dropout(0.5))                                 # on SparseRows: stored entries, the counter RNG (no torch generator)
        model.add(gnntf.Dense(16, activation=gnntf.relu))
        H0 = model.add(gnntf.Dense(4, regularize=False))
        for _ in range(2):
            model.add(gnntf.PPRIteration(H0, 0.1, graph_dropout=0.5))
        return model

    results = []
    for capture in (False, True):
        model = build()
        torch.manual_seed(5)
        model.train(train=gnntf.NodeClassification(train, labels[train]), valid=gnntf.NodeClassification(valid, labels[valid]),
                    epochs=12, patience=50, capture=capture, regularization=0.0)
        assert isinstance(model._input_features(), gnntf.SparseRows)
        results.append([v.var.detach().cpu().numpy().copy() for v in model.vars()] + [model._mask_calls])
    assert results[0][-1] == results[1][-1] == 12 * 3                # the input mask and 2 edge-dropout masks per step, 12 steps
    for eager, captured in zip(results[0][:-1], results[1][:-1]):
        np.testing.assert_allclose(captured, eager, rtol=2e-3, atol=2e-5)


def test_report_the_worst_ratios(capsys):
    """Not a check of its own: prints what the cases above measured (profiles/NOTES.md records a run)."""
    with capsys.disabled():
        print("\n[sparse features, MI355X] worst error / bound:")
        for (what, name), value in sorted(RATIOS.items()):
            print(f"    {what:8s} {name:6s} {value:.3f}")
    assert all(value <= 1.0 for value in RATIOS.values())
