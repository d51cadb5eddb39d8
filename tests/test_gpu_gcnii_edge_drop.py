"""The fused GCNII layer under edge dropout on the MI355X (gnx_gcnii_step_dropped, gnx_gcnii_step_back_dropped,
sparse.gcnii_step(edge_dropout="fused"), sparse.gcnii_step_back(edge_dropout="fused"), GNN(gcnii_edge_dropout="fused")).

The reference for everything is the EXISTING code over the materialised adjacency ``normalize(g, "symmetric", "none", p, seed,
stream)``, whose values are -- the project's own guarantee -- the weights the dropped kernels make.  The new launches run the gather
loop, the entry order, the mix and the transform of the existing ones, so every comparison is bit for bit: the forward (out and T, relu
and identity, with and without the feature mask), the backward (dH and S, with S_in and without, s_alpha != 1, in place, want_S=False),
the dropout counter, autograd under both ``backward`` values, and the model (seeds, capture against eager, the number of mask streams,
the default keyword and eval mode untouched).

Hub rows in the forward test: should the hub rows ALONE differ from the reference, the test first compares spmm(DroppedAdjacency, H)
with spmm(materialised, H) on them and reports which pair disagrees (the long-row kernels or the layer's host path), and then judges
the hub rows by gcnii_shapes_ref.forward_ref over the float32 weights read back, with ratio <= 1 -- the first-order bound of a float32
sum of the same terms in any order.  Every other row stays bit for bit."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcnii_shapes_ref as ref
import graphs
from oracle import gnntf_oracle as orc
from test_gpu_gcnii_drop import HUB, N, N_HUB, directed_coo

pytestmark = pytest.mark.gpu

A_MIX = 0.1
FUSED_WIDTHS, COMPOSED_WIDTHS = (16, 32, 64), (40, 7)
WIDTHS = FUSED_WIDTHS + COMPOSED_WIDTHS
RATES = (0.6, 0.25)
E_SEED, E_STREAM = 5, 3                                  # the edge dropout's (seed, stream)
F_MASK = (0.6, 7, 2)                                     # the feature mask's (p, seed, stream)
HANDLES = ("t", "a", "T", "dup")


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


def with_duplicates(coo, vals):
    """The COO with every entry stored twice, plus 30 % of the slots a third time with ANOTHER value: slots of two equal entries are
    uniform, the others general (gnx_graph_enable_entry_dropout)."""
    rng = np.random.default_rng(23)
    third = rng.random(len(coo)) < 0.3
    idx = np.concatenate([coo, coo, coo[third]])
    val = np.concatenate([vals, vals, (vals[third] * np.float32(0.5) + np.float32(0.25)).astype(np.float32)])
    perm = rng.permutation(len(idx))
    return idx[perm], val[perm], third


@pytest.fixture(scope="module")
def shared(gnntf):
    """The handles, made once and never changed, with their COO (for the oracle's mask): ``a`` the directed 3 000-vertex graph, ``t`` its
    transpose (the hub row of 900 entries in the forward structure, rows without entries), ``T`` regime "T" of gcnii_shapes_ref
    (n = 1 547; rows at L - 1, L, L + 1, 2 L + 1; 23 hub rows) and ``dup`` the first graph with duplicates after enable_entry_dropout()."""
    coo, vals, shape = directed_coo()
    out = dict()
    t_coo, (T_coo, T_vals, T_shape, T_info) = coo[:, ::-1].copy(), ref.regime_graph("T")
    d_coo, d_vals, third = with_duplicates(coo, vals)
    for name, idx, val, shp in (("a", coo, vals, shape), ("t", t_coo, vals, shape), ("T", T_coo, T_vals, T_shape), ("dup", d_coo, d_vals, shape)):
        g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, val, shp), device="cuda:0")
        if name == "dup":
            assert g.nnz_entries > g.nnz and 0.2 < third.mean() < 0.4
            g.enable_entry_dropout()
        else:
            assert g.nnz_entries == g.nnz
        deg = np.diff(host(g.csr_arrays()[0]))
        out[name] = dict(g=g, coo=idx, n=shp[0], deg=deg, hub=np.flatnonzero(deg > g.long_row_threshold), empty=np.flatnonzero(deg == 0))
    assert N % 16 != 0 and HUB in out["t"]["hub"] and out["t"]["deg"][HUB] >= N_HUB and len(out["t"]["empty"]) >= 100
    assert len(out["a"]["hub"]) == 0 and len(out["T"]["hub"]) == 23 and out["T"]["n"] == 1547
    L = T_info["L"]
    assert all(len(T_info["rows_of"][d]) >= 1 for d in (L - 1, L, L + 1, 2 * L + 1))
    # what the masks leave at p = 0.6: a row WITH entries that loses all of them, and a hub row that stays a hub row's worth of gathers
    for name in ("a", "t"):
        idx, n = out[name]["coo"], out[name]["n"]
        keep = orc.keep_mask(idx, 0.6, E_SEED, E_STREAM)
        kept = np.bincount(idx[keep, 0], minlength=n)
        out[name]["all_dropped"] = np.flatnonzero((out[name]["deg"] > 0) & (kept == 0))
        assert len(out[name]["all_dropped"]) >= 1
        if name == "t":
            assert kept[HUB] > 128
    return out


@functools.lru_cache(maxsize=None)
def operands(n, C):
    return ref.operands(n, C, seed=100 + C)


class Pairs:
    """(DroppedAdjacency, the materialised adjacency of the same (p, seed, stream)) per handle and rate, made once."""

    def __init__(self, gnntf, shared):
        self.gnntf, self.shared, self.made = gnntf, shared, dict()

    def __call__(self, name, p, stream=E_STREAM):
        key = (name, p, stream)
        if key not in self.made:
            g = self.shared[name]["g"]
            sparse = self.gnntf.sparse
            self.made[key] = (sparse.DroppedAdjacency(g, p, E_SEED, stream), sparse.normalize(g, "symmetric", "none", p, E_SEED, stream))
        return self.made[key]


@pytest.fixture(scope="module")
def pairs(gnntf, shared):
    return Pairs(gnntf, shared)


def forward_name(C, mask):
    return ("spmm_gcnii_mfma_edrop" if C in FUSED_WIDTHS else "spmm+dense_mfma_edrop") + ("_drop" if mask else "")


def backward_name(C):
    return "spmm_gcnii_back_mfma_edrop" if C in FUSED_WIDTHS else "dense+spmm_back_edrop"


def weights_csr(g, adj):
    """The float32 weights of the materialised adjacency, read back, as a float64 scipy CSR (the handle's order)."""
    rowptr, colidx, _ = g.csr_arrays()
    return sp.csr_matrix((host(adj.vals).astype(np.float64), host(colidx), host(rowptr)), shape=(g.n_rows, g.n_cols))


def judge_hub_rows(gnntf, g, hub, dropped, mat, ops, relu, mask, got_out, got_T, want_out, want_T, where):
    """Called when hub rows ALONE differ from the reference (module docstring): says which pair disagrees, then holds the hub rows to the
    float64 reference over the float32 weights read back."""
    Hd = dev(ops["H"])
    spmm_equal = torch.equal(gnntf.spmm(dropped, Hd)[hub], gnntf.spmm(mat, Hd)[hub])
    print(f"{where}: hub rows differ from the reference; spmm(DroppedAdjacency, H) vs spmm(materialised, H) on them: "
          f"{'equal -- the layer host paths disagree' if spmm_equal else 'DIFFERENT -- the long-row kernels disagree'}")
    want = ref.forward_ref(weights_csr(g, mat), ops["H"], ops["H0"], ops["M"], A_MIX, relu, L=g.long_row_threshold)
    out, bound = want["out"], want["out_bound"]
    if mask is not None:
        p, seed, stream = mask
        n, C = out.shape
        rows, cols = np.repeat(np.arange(n), C), np.tile(np.arange(C), n)
        keep = (orc.hash_u24(seed, stream, rows, cols, np.zeros(n * C, dtype=np.int64)) >= orc.dropout_threshold(p)).reshape(n, C)
        s = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        out, bound = np.where(keep, out * s, 0.0), np.where(keep, bound * s + ref.U32 * np.abs(out * s), 0.0)
    r_T, r_out = ref.ratio(host(got_T), want["T"], want["T_bound"], hub), ref.ratio(host(got_out), out, bound, hub)
    print(f"{where}: hub rows against float64: T ratio {r_T:.3f}, out ratio {r_out:.3f}")
    assert r_T <= 1 and r_out <= 1, where
    rest = np.setdiff1d(np.arange(g.n_rows), hub)
    assert torch.equal(got_T[rest], want_T[rest]) and torch.equal(got_out[rest], want_out[rest]), where


# ---- 1. the forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("C", WIDTHS)
def test_forward_equals_the_materialised_adjacency(gnntf, shared, pairs, C, p):
    sparse = gnntf.sparse
    for name in HANDLES:
        g, n, hub = shared[name]["g"], shared[name]["n"], shared[name]["hub"]
        dropped, mat = pairs(name, p)
        ops = operands(n, C)
        Hd, H0d, Md = dev(ops["H"]), dev(ops["H0"]), dev(ops["M"])
        for relu in (True, False):
            for mask in (None, F_MASK):
                where = f"{name} C={C} p={p} relu={relu} mask={mask is not None}"
                got_out, got_T = sparse._gcnii_launch(dropped, Hd, H0d, A_MIX, Md, relu, keep_mixed=True, dropout=mask, fused_edge=True)
                assert g.last_kernel() == forward_name(C, mask), where
                assert dropped._vals is None                     # no value array was materialised on the way
                want_out, want_T = sparse._gcnii_launch(mat, Hd, H0d, A_MIX, Md, relu, keep_mixed=True, dropout=mask)
                if torch.equal(got_out, want_out) and torch.equal(got_T, want_T):
                    continue
                assert len(hub) > 0, where
                judge_hub_rows(gnntf, g, hub, dropped, mat, ops, relu, mask, got_out, got_T, want_out, want_T, where)
        if name in ("a", "t") and p == 0.6:                      # a row all of whose entries are dropped: T = a H0, out = (a H0) . M
            rows = shared[name]["all_dropped"]
            out, T = sparse._gcnii_launch(dropped, Hd, H0d, A_MIX, Md, False, keep_mixed=True, fused_edge=True)
            assert torch.equal(T[rows], H0d[rows] * A_MIX)
            aH0 = ops["H0"][rows].astype(np.float64) * float(np.float32(A_MIX))
            bound = (C + 6) * ref.U32 * (np.abs(aH0) @ np.abs(ops["M"].astype(np.float64)))
            assert ref.ratio(host(out[rows]), aH0 @ ops["M"].astype(np.float64), bound) <= 1
        if C in FUSED_WIDTHS and name != "dup":                  # inference form of the entry: d_mixed may be NULL at the fused widths
            out, none = sparse._gcnii_launch(dropped, Hd, H0d, A_MIX, Md, True, keep_mixed=False, fused_edge=True)
            want, _ = sparse._gcnii_launch(mat, Hd, H0d, A_MIX, Md, True, keep_mixed=False)
            assert none is None and torch.equal(out[np.setdiff1d(np.arange(n), hub)], want[np.setdiff1d(np.arange(n), hub)])


# ---- 2. the backward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("C", WIDTHS)
def test_backward_equals_the_materialised_adjacency(gnntf, shared, pairs, C, p):
    sparse = gnntf.sparse
    for name in HANDLES:                                         # ("a": the TRANSPOSED structure the backward walks holds the hub row)
        g, n = shared[name]["g"], shared[name]["n"]
        dropped, mat = pairs(name, p)
        ops = operands(n, C)
        Gd, Mtd, S_in = dev(ops["G"]), dev(ops["Mt"]), dev(ops["S_in"])
        for kwargs in (dict(), dict(S_in=S_in, s_alpha=0.75), dict(want_S=False)):
            where = f"{name} C={C} p={p} {sorted(kwargs)}"
            got = gnntf.gcnii_step_back(dropped, Gd, A_MIX, Mtd, edge_dropout="fused", **kwargs)
            assert g.last_kernel() == backward_name(C), where
            assert dropped.vals_t is None and dropped._vals is None
            want = gnntf.gcnii_step_back(mat, Gd, A_MIX, Mtd, **kwargs)
            assert torch.equal(got[0], want[0]), where
            assert (got[1] is None and want[1] is None) if kwargs.get("want_S") is False else torch.equal(got[1], want[1]), where
        # in place: S_out is S_in
        S_got, S_want = dev(ops["S_in"]), dev(ops["S_in"])
        got = sparse._gcnii_back_launch(False, dropped, Gd, None, A_MIX, Mtd, S_got, 0.75, True, True, fused_edge=True)
        want = sparse._gcnii_back_launch(False, mat, Gd, None, A_MIX, Mtd, S_want, 0.75, True, True)
        assert got[1] is S_got and torch.equal(S_got, S_want) and torch.equal(got[0], want[0])
        assert not torch.equal(S_got, S_in)
        assert float(got[0].abs().max()) > 0


# ---- 3. the dropout counter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 40])
def test_dropout_counter_shifts_both_streams(gnntf, shared, pairs, C):
    sparse = gnntf.sparse
    g, n = shared["t"]["g"], shared["t"]["n"]
    ops = operands(n, C)
    Hd, H0d, Md, Gd, Mtd = (dev(ops[k]) for k in ("H", "H0", "M", "G", "Mt"))
    p, k = 0.6, 3
    shifted, _ = pairs("t", p, E_STREAM + k)
    want = sparse._gcnii_launch(shifted, Hd, H0d, A_MIX, Md, True, keep_mixed=True, dropout=(0.6, 7, 5 + k), fused_edge=True)
    want_back = gnntf.gcnii_step_back(shifted, Gd, A_MIX, Mtd, edge_dropout="fused")
    base = sparse.DroppedAdjacency(g, p, E_SEED, E_STREAM, D=shifted.D)       # stream s; the scales are those of stream s + k
    counter = torch.tensor([k], dtype=torch.int64, device="cuda")
    g.set_dropout_counter(counter)
    try:
        got = sparse._gcnii_launch(base, Hd, H0d, A_MIX, Md, True, keep_mixed=True, dropout=(0.6, 7, 5), fused_edge=True)
        got_back = gnntf.gcnii_step_back(base, Gd, A_MIX, Mtd, edge_dropout="fused")
        torch.cuda.synchronize()
    finally:
        g.set_dropout_counter(None)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got_back[0], want_back[0]) and torch.equal(got_back[1], want_back[1])
    plain = sparse._gcnii_launch(base, Hd, H0d, A_MIX, Md, True, keep_mixed=True, dropout=(0.6, 7, 5), fused_edge=True)   # the counter is gone
    assert not torch.equal(plain[1], want[1])


# ---- 4. autograd ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backward", ["composed", "fused"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C", [16, 64, 40])
def test_autograd_equals_the_materialised_adjacency(gnntf, shared, pairs, C, relu, backward):
    for name in ("t", "dup"):
        g, n = shared[name]["g"], shared[name]["n"]
        dropped, mat = pairs(name, 0.6)
        ops = operands(n, C)
        up = dev(ops["S_in"])
        for mask in (None, F_MASK):
            def run(adj, **option):
                leaves = [dev(ops[k]).requires_grad_() for k in ("H", "H0", "M")]
                out = gnntf.gcnii_step(adj, *leaves[:2], A_MIX, leaves[2], relu=relu, backward=backward, dropout=mask, **option)
                kernel = g.last_kernel()
                out.backward(up)
                return [out.detach()] + [leaf.grad for leaf in leaves], kernel, g.last_kernel()

            got, forward_kernel, backward_kernel = run(dropped, edge_dropout="fused")
            assert forward_kernel == forward_name(C, mask)
            assert backward_kernel == (backward_name(C) if backward == "fused" else g.last_kernel())
            want, _, _ = run(mat)
            for what, a_, b_ in zip(("out", "dH", "dH0", "dM"), got, want):
                assert a_ is not None and b_ is not None
                np.testing.assert_array_equal(host(a_), host(b_), err_msg=f"{name} {what} mask={mask is not None}")
            assert float(got[1].abs().max()) > 0 and float(got[3].abs().max()) > 0
    # the default keyword keeps the generic composition of a DroppedAdjacency
    leaves = [dev(ops[k]).requires_grad_() for k in ("H", "H0", "M")]
    gnntf.gcnii_step(dropped, *leaves[:2], A_MIX, leaves[2], relu=relu, backward=backward)
    assert "edrop" not in g.last_kernel()


# ---- 5. the model --------------------------------------------------------------------------------------------------------------------------
FUSED_MODEL = dict(gcnii_edge_dropout="fused", feature_dropout="fused", gcnii_backward="fused")


@pytest.fixture(scope="module")
def cora():
    coo, vals, shape, X = graphs.cora_shaped(seed=4)
    labels = np.random.default_rng(4).integers(0, 7, size=shape[0])
    weights = [(np.random.default_rng(40 + k).standard_normal((32, 32)) / 6).astype(np.float32) for k in range(3)]
    return dict(coo=coo, vals=vals, shape=shape, X=X, labels=labels, weights=weights, train=np.arange(0, 300), valid=np.arange(300, 600))


def make_model(gnntf, cora, seeded_weights=True, **option):
    """A hand-built stack in the style of the reference's demos/custom_layers.py: three GCNIILayer(graph_dropout=0.5, dropout=0.6)."""
    gnntf.set_seed(11)
    torch.manual_seed(3)
    model = gnntf.GNN(gnntf.SparseCOO(cora["coo"], cora["vals"], cora["shape"]), cora["X"], **option)
    model.add(gnntf.Dense(32, dropout=0, activation=gnntf.relu))
    H0 = model.top_layer()
    for k in range(3):
        model.add(gnntf.GCNIILayer(H0, 0.1, 0.5, k, activation=gnntf.relu, dropout=0.6, graph_dropout=0.5))
    model.add(gnntf.Dense(7, dropout=0, regularize=False))
    model.reset()
    convs = [layer for layer in model.layers() if isinstance(layer, gnntf.GCNIILayer)]
    assert len(convs) == 3
    if seeded_weights:                                  # the reference initialises W to zero: M would be a multiple of the identity
        for layer, W in zip(convs, cora["weights"]):
            layer.W.data.copy_(dev(W))
    return model


def three_steps(gnntf, cora, model):
    """Three plain gradient steps in training mode; (losses, gradients of every step, mask streams taken, kernels seen)."""
    task = gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]])
    losses, grads, kernels = [], [], set()
    first = model._mask_calls
    torch.manual_seed(9)                                # (torch's dropout, where a model uses it, starts every run from the same state)
    for _ in range(3):
        with model:
            for v in model.vars():
                v.var.grad = None
            loss = task.loss(model(model.features))
            kernels.add(model.graph.last_kernel())
            loss.backward()
            kernels.add(model.graph.last_kernel())
        losses.append(float(loss.detach()))
        grads.append([v.var.grad.clone() for v in model.vars()])
        with torch.no_grad():
            for v in model.vars():
                v.var -= 0.05 * v.var.grad
    return losses, grads, model._mask_calls - first, kernels


def test_model_is_reproducible_and_draws_todays_streams(gnntf, cora):
    one = three_steps(gnntf, cora, make_model(gnntf, cora, **FUSED_MODEL))
    two = three_steps(gnntf, cora, make_model(gnntf, cora, **FUSED_MODEL))
    composed = three_steps(gnntf, cora, make_model(gnntf, cora, feature_dropout="fused", gcnii_backward="fused"))
    assert one[2] == two[2] == composed[2] == 3 * 6     # per step and layer: the adjacency's stream, then the feature mask's
    assert one[0] == two[0] and all(np.isfinite(one[0]))
    for step_one, step_two in zip(one[1], two[1]):
        assert len(step_one) > 3 and all(torch.equal(a_, b_) for a_, b_ in zip(step_one, step_two))
    assert one[3] == {"spmm_gcnii_mfma_edrop_drop", "spmm_gcnii_back_mfma_edrop"}
    assert not any("edrop" in kernel for kernel in composed[3])
    # the same masks and values as "composed", another order of the same float32 sums: the losses agree to rounding, not bit for bit
    assert np.allclose(one[0], composed[0], rtol=1e-4)
    torch_mask = three_steps(gnntf, cora, make_model(gnntf, cora, gcnii_edge_dropout="fused"))      # torch's dropout follows the launch
    assert torch_mask[2] == 3 * 3 and "spmm_gcnii_mfma_edrop" in torch_mask[3]


def test_captured_training_equals_eager(gnntf, cora, monkeypatch):
    """train(capture=True) for 3 epochs, bit for bit the eager run (the pattern of tests/test_gpu_gcnii_drop.py)."""
    from gnntf import training
    observed, observe = [], training._BestSoFar.observe
    monkeypatch.setattr(training._BestSoFar, "observe", lambda self, loss: (observed[-1].append(loss), observe(self, loss))[1])
    results = []
    for capture in (False, True):
        observed.append([])
        model = make_model(gnntf, cora, seeded_weights=False, **FUSED_MODEL)
        gnntf.set_seed(11)
        torch.manual_seed(5)
        valid = gnntf.NodeClassification(cora["valid"], cora["labels"][cora["valid"]])
        model.train(train=gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]]), valid=valid, epochs=3, patience=50,
                    capture=capture, optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
        results.append(([v.var.detach().clone() for v in model.vars()], float(model.loss(valid)), model._mask_calls))
    (eager, eager_loss, eager_masks), (captured, captured_loss, captured_masks) = results
    assert eager_masks == captured_masks == 3 * 6
    print("captured vs eager, max |difference| per variable:", [float((e - c).abs().max()) for e, c in zip(eager, captured)])
    assert all(torch.equal(e, c) for e, c in zip(eager, captured))
    assert eager_loss == captured_loss
    assert len(observed[0]) == len(observed[1]) == 3 and observed[0] == observed[1] and len(set(observed[0])) == 3


def test_default_keyword_and_eval_mode_are_todays(gnntf, cora):
    default = make_model(gnntf, cora)
    assert default.gcnii_edge_dropout == "composed"
    named = make_model(gnntf, cora, gcnii_edge_dropout="composed")
    one, two = three_steps(gnntf, cora, default), three_steps(gnntf, cora, named)
    assert one[0] == two[0] and one[2] == two[2] and not any("edrop" in kernel for kernel in one[3] | two[3])
    for step_one, step_two in zip(one[1], two[1]):
        assert all(torch.equal(a_, b_) for a_, b_ in zip(step_one, step_two))
    # eval mode: the keyword changes nothing (the other two options are those of the model it is compared with)
    fused, default = make_model(gnntf, cora, **FUSED_MODEL), make_model(gnntf, cora, feature_dropout="fused", gcnii_backward="fused")
    outs = []
    for model in (fused, default):                      # the same weights: eval-mode forwards agree bit for bit, on today's kernel
        model.training_mode(False)                      # (a fresh model starts in training mode, as the reference's does)
        with torch.no_grad():
            outs.append(model(model.features))
        assert model.graph.last_kernel() == "spmm_gcnii_mfma"
    assert torch.equal(outs[0], outs[1]) and float(outs[0].abs().max()) > 0
    # eval mode under autograd: a constant adjacency, today's node and today's gradients
    grads = []
    for model in (fused, default):
        for v in model.vars():
            v.var.grad = None
        model(model.features).square().sum().backward()
        assert "edrop" not in model.graph.last_kernel()
        grads.append([v.var.grad.clone() for v in model.vars()])
    assert all(torch.equal(a_, b_) for a_, b_ in zip(*grads)) and any(float(a_.abs().max()) > 0 for a_ in grads[0])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(gnntf, shared, pairs):
    sparse = gnntf.sparse
    nat = sparse.nat
    lib = nat.lib()
    g, n, C = shared["t"]["g"], shared["t"]["n"], 16
    dropped, _ = pairs("t", 0.6)
    ops = operands(n, C)
    Hd, H0d, Md, Gd = dev(ops["H"]), dev(ops["H0"]), dev(ops["M"]), dev(ops["G"])
    out, T, dH = (torch.empty(n, C, device="cuda") for _ in range(3))

    def step(handle, D, out_, H0_=H0d, M_=Md, p=0.6):
        return lib.gnx_gcnii_step_dropped(handle, nat.ptr(D), p, E_SEED, E_STREAM, nat.ptr(Hd), nat.ptr(H0_), A_MIX, C, nat.ptr(M_), C, 1,
                                          0.0, 0, 0, nat.ptr(out_), nat.ptr(T), nat.current_stream())

    def back(handle, D, p=0.6):
        return lib.gnx_gcnii_step_back_dropped(handle, nat.ptr(D), p, E_SEED, E_STREAM, nat.ptr(Gd), A_MIX, C, nat.ptr(Md), C, nat.ptr(dH), None,
                                               1.0, None, None, nat.current_stream())

    assert step(g.handle, dropped.D, out) == 0 and back(g.handle, dropped.D) == 0          # the calls themselves are well formed
    # a handle with duplicates and no entry tables
    coo, vals, shape = directed_coo()
    d_coo, d_vals, _ = with_duplicates(coo, vals)
    plain_dups = gnntf.DeviceGraph(gnntf.SparseCOO(d_coo, d_vals, shape), device="cuda:0")
    assert plain_dups.nnz_entries > plain_dups.nnz and not plain_dups.entry_dropout
    for rc in (step(plain_dups.handle, dropped.D, out), back(plain_dups.handle, dropped.D)):
        assert rc != 0 and b"duplicate" in lib.gnx_last_error() and b"gnx_graph_enable_entry_dropout" in lib.gnx_last_error()
    with pytest.raises(Exception, match="duplicate"):
        sparse._gcnii_launch(sparse.DroppedAdjacency(plain_dups, 0.6, E_SEED, E_STREAM, D=dropped.D), Hd, H0d, A_MIX, Md, True, True, fused_edge=True)
    # add_eye
    with_eye = sparse.DroppedAdjacency(g, 0.6, E_SEED, E_STREAM, D=dropped.D)
    with_eye.diag = torch.ones(n, device="cuda")
    with pytest.raises(Exception, match="add_eye"):
        sparse._gcnii_launch(with_eye, Hd, H0d, A_MIX, Md, True, True, fused_edge=True)
    with pytest.raises(Exception, match="add_eye"):
        gnntf.gcnii_step_back(with_eye, Gd, A_MIX, Md, edge_dropout="fused")
    # a non-square graph
    wide = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, (n, n + 5)), device="cuda:0")
    D_wide = torch.ones(n + 5, device="cuda")
    for rc in (step(wide.handle, D_wide, out), back(wide.handle, D_wide)):
        assert rc == -1 and b"square" in lib.gnx_last_error()
    with pytest.raises(Exception, match="shape mismatch"):
        sparse._gcnii_launch(sparse.DroppedAdjacency(wide, 0.6, E_SEED, E_STREAM, D=D_wide), Hd, H0d, A_MIX, Md, True, True, fused_edge=True)
    # out aliasing H0 or M; NULL scales; a bad rate
    assert step(g.handle, dropped.D, H0d) == -1 and b"out must not alias H0 / M" in lib.gnx_last_error()
    square = torch.empty(C, C, device="cuda")
    assert lib.gnx_gcnii_step_dropped(g.handle, nat.ptr(dropped.D), 0.6, E_SEED, E_STREAM, nat.ptr(Hd), nat.ptr(H0d), A_MIX, C, nat.ptr(square), C, 1,
                                      0.0, 0, 0, nat.ptr(square), nat.ptr(T), nat.current_stream()) == -1
    assert b"out must not alias H0 / M" in lib.gnx_last_error()
    assert step(g.handle, None, out) == -1 and b"NULL degree scales" in lib.gnx_last_error()
    assert back(g.handle, None) == -1 and b"NULL degree scales" in lib.gnx_last_error()
    for p in (1.0, -0.1):
        assert step(g.handle, dropped.D, out, p=p) == -1 and b"outside [0, 1)" in lib.gnx_last_error()
        assert back(g.handle, dropped.D, p=p) == -1 and b"outside [0, 1)" in lib.gnx_last_error()
    # a bad keyword value
    with pytest.raises(Exception, match="edge_dropout must be one of"):
        gnntf.gcnii_step(dropped, Hd, H0d, A_MIX, Md, edge_dropout="bogus")
    with pytest.raises(Exception, match="edge_dropout must be one of"):
        gnntf.gcnii_step_back(dropped, Gd, A_MIX, Md, edge_dropout=True)
    with pytest.raises(Exception, match="gcnii_edge_dropout must be one of"):
        gnntf.GNN(g, ops["H"], gcnii_edge_dropout="bogus")
    # without the keyword a DroppedAdjacency is refused by the fused backward, as before
    with pytest.raises(Exception, match="constant adjacency"):
        gnntf.gcnii_step_back(dropped, Gd, A_MIX, Md)
