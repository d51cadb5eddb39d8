"""The fused GCNLayer on the MI355X (gnx_gcn_step, gnx_gcn_step_dropped, sparse.gcn_step, GNN(gcn_layer="fused")).

Forward and gradients are judged against the float64 references of tests/gcn_fused_ref.py over the very float32 weights the kernels read,
with max |got - want| / bound <= 1 -- the first-order bound of a float32 evaluation in any order -- at regime T (n = 1547: a ragged last
tile, hub rows at the threshold of 512, a whole tile of rows without entries) and regime S (n = 2^15 + 11, threshold 128) of
tests/gcnii_shapes_ref.py.  Where existing code is the reference the comparison is bit for bit: the gather and MFMA order against
gnx_gcnii_step with H0 = 0, a = 0 and M = W, the edge-dropout entry against gnx_gcn_step over the materialised adjacency, the mask
against the unmasked result times the scale."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_fused_ref as gref
import graphs
from test_gpu_gcnii_drop import HUB, N, N_HUB, directed_coo, keep_mask, scale
from test_gpu_gcnii_edge_drop import with_duplicates

pytestmark = pytest.mark.gpu

SEED, STREAM = 7, 2                                      # the feature mask's
E_SEED, E_STREAM = 5, 3                                  # the edge dropout's
SENTINEL = 1234.5


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


def bits(t):
    return host(t).view(np.int32)


def weights_csr(g, vals):
    """The float32 weights ``vals`` (the handle's order) as a float64 scipy CSR."""
    rowptr, colidx, _ = g.csr_arrays()
    return sp.csr_matrix((host(vals).astype(np.float64), host(colidx), host(rowptr)), shape=(g.n_rows, g.n_cols))


@pytest.fixture(scope="module")
def world(gnntf):
    """Regimes T and S: the handle, its normalised adjacency and the weights read back, made once and never changed."""
    out = dict()
    for name in ("T", "S"):
        coo, vals, shape, info = gref.regime_graph(name)
        g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
        adj = gnntf.normalize(g, "symmetric")
        assert g.long_row_threshold == info["L"] and g.n_hub_rows == len(info["hub"]) > 0
        out[name] = dict(g=g, adj=adj, A=weights_csr(g, adj.vals), info=info, n=shape[0], L=info["L"], coo=coo)
    return out


@functools.lru_cache(maxsize=None)
def operands(n, C_in, C_out):
    return gref.operands(n, C_in, C_out, 500 + 7 * C_in + C_out)


def row_sets(info):
    return (("all", None), ("hub", info["hub"]), ("empty", info["empty"]), ("ragged", info["ragged"]))


def fused_name(C_in, edge=False, drop=False, hubs=True):
    return f"k_spmm_gcn<{C_in}>" + ("_edrop" if edge else "") + ("_drop" if drop else "") + ("+long" if hubs else "")


def composed_name(edge=False, drop=False):
    return "spmm+dense_mfma_gcn" + ("_edrop" if edge else "") + ("_drop" if drop else "")


# ---- 1. the forward against float64; 4. d_agg does not move out --------------------------------------------------------------------------
FORWARD_CASES = [("T",) + s for s in gref.SHAPES] + [("S", 64, 40)]


@pytest.mark.parametrize("regime, C_in, C_out", FORWARD_CASES)
def test_forward_against_float64(gnntf, world, regime, C_in, C_out):
    sparse = gnntf.sparse
    w = world[regime]
    g, info = w["g"], w["info"]
    op = operands(w["n"], C_in, C_out)
    Xd, Wd, bd = dev(op["X"]), dev(op["W"]), dev(op["bias"])
    for relu in (True, False):
        for bias in (op["bias"], None):
            where = f"{regime} {C_in}->{C_out} relu={relu} bias={bias is not None}"
            want = gref.forward_ref(w["A"], op["X"], op["W"], bias, relu, L=w["L"])
            out, none = sparse._gcn_launch(w["adj"], Xd, Wd, None if bias is None else bd, relu, keep_agg=False)
            assert none is None and g.last_kernel() == fused_name(C_in), (where, g.last_kernel())
            kept, agg = sparse._gcn_launch(w["adj"], Xd, Wd, None if bias is None else bd, relu, keep_agg=True)
            assert g.last_kernel() == fused_name(C_in), (where, g.last_kernel())
            assert out.shape == (w["n"], C_out) and agg.shape == (w["n"], C_in)
            for name, rows in row_sets(info):
                assert rows is None or len(rows) > 0
                r_out = gref.ratio(host(out), want["out"], want["out_bound"], rows)
                r_agg = gref.ratio(host(agg), want["agg"], want["agg_bound"], rows)
                print(f"{where} {name} rows: out error / bound = {r_out:.3f}, agg error / bound = {r_agg:.3f}")
                assert r_out <= 1 and r_agg <= 1, (where, name)
            assert torch.equal(out, kept), where         # d_agg does not move a bit of out
            assert float(out.abs().max()) > 0 and float(agg[info["empty"]].abs().max()) == 0


# ---- 2. the composed forms inside the entry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_in, C_out", [(24, 8), (16, 64)])
def test_composed_forms_inside_the_entry(gnntf, world, C_in, C_out):
    sparse = gnntf.sparse
    w = world["T"]
    g, info = w["g"], w["info"]
    op = operands(w["n"], C_in, C_out)
    Xd, Wd, bd = dev(op["X"]), dev(op["W"]), dev(op["bias"])
    for relu in (True, False):
        want = gref.forward_ref(w["A"], op["X"], op["W"], op["bias"], relu, L=w["L"])
        for keep in (False, True):
            out, agg = sparse._gcn_launch(w["adj"], Xd, Wd, bd, relu, keep_agg=keep)
            assert g.last_kernel() == composed_name(), g.last_kernel()
            for name, rows in row_sets(info):
                assert gref.ratio(host(out), want["out"], want["out_bound"], rows) <= 1, (C_in, C_out, relu, name)
                assert agg is None or gref.ratio(host(agg), want["agg"], want["agg_bound"], rows) <= 1


def raw_step(nat, g, Xd, Wd, bd, out, ldo, agg=None, work=None, act=1, rate=0.0, C_out=None, ldw=None, vals=None):
    """gnx_gcn_step itself (``vals`` None: the handle's raw values)."""
    return nat.lib().gnx_gcn_step(g.handle, nat.ptr(vals), nat.ptr(Xd), Xd.stride(0), Xd.shape[1], nat.ptr(Wd), Wd.stride(0) if ldw is None else ldw,
                                  Wd.shape[1] if C_out is None else C_out, nat.ptr(bd), act, rate, SEED, STREAM, nat.ptr(out), ldo, nat.ptr(agg),
                                  nat.ptr(work), nat.current_stream())


def test_refusal_without_a_place_for_the_rows(gnntf, world):
    nat = gnntf.sparse.nat
    w = world["T"]
    n = w["n"]
    for C_in, C_out, why in ((24, 8, b"C_in is not 16, 32 or 64"), (16, 64, b"C_out > C_in"), (64, 40, b"hub rows")):
        op = operands(n, C_in, C_out)
        Xd, Wd, bd = dev(op["X"]), dev(op["W"]), dev(op["bias"])
        out = torch.full((n, C_out), SENTINEL, device="cuda")
        assert raw_step(nat, w["g"], Xd, Wd, bd, out, C_out) == -1
        message = nat.lib().gnx_last_error()
        assert b"gnx_gcn_step: needs d_agg or d_work" in message and why in message, message
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
        work = torch.empty(n, C_in, device="cuda")
        assert raw_step(nat, w["g"], Xd, Wd, bd, out, C_out, work=work) == 0        # d_work alone is enough
        assert not bool((out == SENTINEL).any())


# ---- 3. the bitwise anchor: the gather order and the MFMA order are those of gnx_gcnii_step ---------------------------------------------------
@pytest.mark.parametrize("regime, C", [("T", 16), ("T", 32), ("T", 64), ("S", 64)])
def test_square_layer_without_bias_is_the_gcnii_launch(gnntf, world, regime, C):
    sparse = gnntf.sparse
    w = world[regime]
    op = operands(w["n"], C, C)
    Xd, Wd = dev(op["X"]), dev(op["W"])
    zeros = torch.zeros_like(Xd)
    for relu in (True, False):
        want_out, want_T = sparse._gcnii_launch(w["adj"], Xd, zeros, 0.0, Wd, relu, keep_mixed=True)
        assert w["g"].last_kernel() == "spmm_gcnii_mfma"
        got_out, got_agg = sparse._gcn_launch(w["adj"], Xd, Wd, None, relu, keep_agg=True)
        assert w["g"].last_kernel() == fused_name(C)
        # (the mix there is fmaf(acc, 1, 0): the two agree except in the sign of a zero, which torch.equal does not see)
        assert torch.equal(got_agg, want_T) and torch.equal(got_out, want_out), (regime, C, relu)
        assert torch.equal(gnntf.gcn_step(w["adj"], Xd, Wd, relu=relu), want_out)


# ---- 5. no stray writes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_in", [64, 16])
def test_seven_columns_write_nothing_else(gnntf, world, C_in):
    """C_out = 7 into rows of stride 8 (a float4 and three single values per row), of stride 7 (single values) and of stride 8 from a
    base that is not 16-byte aligned: the same [n, 7] block each time, every other element of the buffers untouched."""
    nat = gnntf.sparse.nat
    w = world["T"]
    n, g, pad = w["n"], w["g"], 64
    op = operands(n, C_in, 7)
    Xd, Wd, bd = dev(op["X"]), dev(op["W"]), dev(op["bias"])
    work = torch.empty(n, C_in, device="cuda")
    results = []
    for ldo, shift in ((8, 0), (7, 0), (8, 1)):
        whole = torch.full((pad + shift + n * ldo + pad,), SENTINEL, device="cuda")
        out = whole[pad + shift:pad + shift + n * ldo]
        assert out.data_ptr() % 16 == (4 * shift) % 16
        assert raw_step(nat, g, Xd, Wd, bd, out, ldo, work=work, vals=w["adj"].vals) == 0, nat.lib().gnx_last_error()
        assert g.last_kernel() == fused_name(C_in)
        torch.cuda.synchronize()
        block = out.view(n, ldo)
        assert bool((whole[:pad + shift] == SENTINEL).all()) and bool((whole[pad + shift + n * ldo:] == SENTINEL).all()), (ldo, shift)
        assert bool((block[:, 7:] == SENTINEL).all()), (ldo, shift)
        assert not bool((block[:, :7] == SENTINEL).any())
        results.append(block[:, :7].clone())
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])
    want = gref.forward_ref(w["A"], op["X"], op["W"], op["bias"], True, L=w["L"])
    assert gref.ratio(host(results[0]), want["out"], want["out_bound"]) <= 1


# ---- 6. under edge dropout: bit for bit the entry over the materialised adjacency ---------------------------------------------------------------
@pytest.fixture(scope="module")
def dropped_world(gnntf):
    """The handles of tests/test_gpu_gcnii_edge_drop.py: ``a`` the directed 3 000-vertex graph, ``t`` its transpose (a hub row of 900
    entries, rows without entries), ``T`` regime T and ``dup`` the first graph with duplicates after enable_entry_dropout()."""
    coo, vals, shape = directed_coo()
    T_coo, T_vals, T_shape, _ = gref.regime_graph("T")
    d_coo, d_vals, _ = with_duplicates(coo, vals)
    out = dict()
    for name, idx, val, shp in (("a", coo, vals, shape), ("t", coo[:, ::-1].copy(), vals, shape), ("T", T_coo, T_vals, T_shape),
                                ("dup", d_coo, d_vals, shape)):
        g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, val, shp), device="cuda:0")
        if name == "dup":
            assert g.nnz_entries > g.nnz
            g.enable_entry_dropout()
        deg = np.diff(host(g.csr_arrays()[0]))
        out[name] = dict(g=g, coo=idx, n=shp[0], deg=deg, hub=np.flatnonzero(deg > g.long_row_threshold))
    assert HUB in out["t"]["hub"] and out["t"]["deg"][HUB] >= N_HUB and N % 16 != 0 and len(out["T"]["hub"]) == 23
    from oracle import gnntf_oracle as orc
    for name in ("a", "t"):
        idx, n = out[name]["coo"], out[name]["n"]
        kept = np.bincount(idx[orc.keep_mask(idx, 0.6, E_SEED, E_STREAM), 0], minlength=n)
        out[name]["all_dropped"] = np.flatnonzero((out[name]["deg"] > 0) & (kept == 0))
        assert len(out[name]["all_dropped"]) >= 1
    return out


@pytest.mark.parametrize("p", [0.6, 0.25])
@pytest.mark.parametrize("C_in, C_out", [(64, 40), (16, 16), (32, 7), (24, 8)])
def test_edge_dropout_equals_the_materialised_adjacency(gnntf, dropped_world, C_in, C_out, p):
    sparse = gnntf.sparse
    for name in ("t", "a", "T", "dup"):
        d = dropped_world[name]
        g, n = d["g"], d["n"]
        dropped = sparse.DroppedAdjacency(g, p, E_SEED, E_STREAM)
        mat = sparse.normalize(g, "symmetric", "none", p, E_SEED, E_STREAM)
        op = operands(n, C_in, C_out)
        Xd, Wd, bd = dev(op["X"]), dev(op["W"]), dev(op["bias"])
        fused = C_in in (16, 32, 64)
        for relu in (True, False):
            for mask in (None, (0.5, SEED, STREAM)):
                where = f"{name} {C_in}->{C_out} p={p} relu={relu} mask={mask is not None}"
                got_out, got_agg = sparse._gcn_launch(dropped, Xd, Wd, bd, relu, keep_agg=True, dropout=mask, fused_edge=True)
                hubs = len(d["hub"]) > 0
                assert g.last_kernel() == (fused_name(C_in, True, mask is not None, hubs) if fused else composed_name(True, mask is not None)), where
                assert dropped._vals is None                 # no value array was materialised on the way
                want_out, want_agg = sparse._gcn_launch(mat, Xd, Wd, bd, relu, keep_agg=True, dropout=mask)
                assert g.last_kernel() == (fused_name(C_in, False, mask is not None, hubs) if fused else composed_name(False, mask is not None)), where
                differ = np.flatnonzero((bits(got_out) != bits(want_out)).any(axis=1) | (bits(got_agg) != bits(want_agg)).any(axis=1))
                assert len(differ) == 0, (where, differ[:8], np.isin(differ, d["hub"]).all())
        if name in ("a", "t") and p == 0.6:                  # a row all of whose entries are dropped: agg = 0, out = act(bias)
            rows = d["all_dropped"]
            out, agg = sparse._gcn_launch(dropped, Xd, Wd, bd, False, keep_agg=True, fused_edge=True)
            assert float(agg[rows].abs().max()) == 0 and torch.equal(out[rows], bd.reshape(1, -1).expand(len(rows), -1))


# ---- 7. the feature mask -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_in, C_out", [(64, 40), (64, 7), (16, 16), (24, 8)])
def test_feature_mask(gnntf, world, C_in, C_out):
    sparse = gnntf.sparse
    w = world["T"]
    g, n = w["g"], w["n"]
    op = operands(n, C_in, C_out)
    Xd, Wd, bd = dev(op["X"]), dev(op["W"]), dev(op["bias"])
    fused = C_in in (16, 32, 64)
    for p in (0.5, 0.25):
        plain, _ = sparse._gcn_launch(w["adj"], Xd, Wd, bd, False, keep_agg=False)
        masked, agg = sparse._gcn_launch(w["adj"], Xd, Wd, bd, False, keep_agg=True, dropout=(p, SEED, STREAM))
        assert g.last_kernel() == (fused_name(C_in, drop=True) if fused else composed_name(drop=True))
        keep = keep_mask(SEED, STREAM, p, n, C_out)
        want = np.where(keep, host(plain) * scale(p), np.float32(0)).astype(np.float32)
        np.testing.assert_array_equal(bits(masked), want.view(np.int32))         # kept: unmasked x scale; dropped: +0
        assert np.array_equal(host(masked) != 0, keep & (host(plain) != 0))
        _, plain_agg = sparse._gcn_launch(w["adj"], Xd, Wd, bd, False, keep_agg=True)
        assert torch.equal(agg, plain_agg)                   # d_agg stays undropped
    triple = (0.5, SEED, STREAM)
    first = sparse._gcn_launch(w["adj"], Xd, Wd, bd, True, keep_agg=False, dropout=triple)[0]
    assert torch.equal(first, sparse._gcn_launch(w["adj"], Xd, Wd, bd, True, keep_agg=False, dropout=triple)[0])
    other = sparse._gcn_launch(w["adj"], Xd, Wd, bd, False, keep_agg=False, dropout=(0.5, SEED, STREAM + 1))[0]
    mine = sparse._gcn_launch(w["adj"], Xd, Wd, bd, False, keep_agg=False, dropout=triple)[0]
    assert 0.2 < float(((mine != 0) != (other != 0)).float().mean()) < 0.8
    # the handle's dropout counter shifts the mask: stream s under a counter of k is stream s + k
    want = sparse._gcn_launch(w["adj"], Xd, Wd, bd, True, keep_agg=False, dropout=(0.5, SEED, STREAM + 3))[0]
    counter = torch.tensor([3], dtype=torch.int64, device="cuda")
    g.set_dropout_counter(counter)
    try:
        got = sparse._gcn_launch(w["adj"], Xd, Wd, bd, True, keep_agg=False, dropout=triple)[0]
        torch.cuda.synchronize()
    finally:
        g.set_dropout_counter(None)
    assert torch.equal(got, want) and not torch.equal(got, first)


# ---- 8. autograd against float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C_in, C_out", [(64, 40), (24, 8)])
def test_autograd_against_float64(gnntf, world, C_in, C_out, relu, edge):
    sparse = gnntf.sparse
    w = world["T"]
    g, n = w["g"], w["n"]
    op = operands(n, C_in, C_out)
    if edge:
        adj = sparse.DroppedAdjacency(g, 0.5, E_SEED, E_STREAM)
        A = weights_csr(g, sparse.normalize(g, "symmetric", "none", 0.5, E_SEED, E_STREAM).vals)
    else:
        adj, A = w["adj"], w["A"]
    for mask in (None, (0.5, SEED, STREAM)):
        leaves = [dev(op[k]).requires_grad_() for k in ("X", "W", "bias")]
        out = gnntf.gcn_step(adj, *leaves, relu=relu, dropout=mask, edge_dropout="fused")
        fused = C_in in (16, 32, 64)
        assert g.last_kernel() == (fused_name(C_in, edge, mask is not None) if fused else composed_name(edge, mask is not None))
        assert not edge or adj._vals is None
        out.backward(dev(op["G"]))
        p = 0.0 if mask is None else mask[0]
        keep = None if mask is None else keep_mask(SEED, STREAM, p, n, C_out)
        fwd = gref.forward_ref(A, op["X"], op["W"], op["bias"], relu, p, keep, L=w["L"])
        assert gref.ratio(host(out), fwd["out"], fwd["out_bound"]) <= 1
        agg32 = host(sparse._gcn_launch(adj, leaves[0].detach(), leaves[1].detach(), leaves[2].detach(), relu, keep_agg=True, fused_edge=edge)[1])
        G = gref.gate_f32(op["G"], host(out), relu, p, keep)
        want = gref.backward_ref(A, agg32, G, op["W"], L=w["L"])
        for name, leaf in zip(("dX", "dW", "db"), leaves):
            got = host(leaf.grad).reshape(want[name].shape if name != "db" else (1, -1))
            worst = gref.ratio(got, want[name].reshape(got.shape), want[name + "_bound"].reshape(got.shape))
            print(f"{C_in}->{C_out} relu={relu} edge={edge} mask={mask is not None} {name}: error / bound = {worst:.3f}")
            assert worst <= 1 and float(np.abs(got).max()) > 0


# ---- 9. the model ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cora():
    coo, vals, shape, X = graphs.cora_shaped(seed=4)
    labels = np.random.default_rng(4).integers(0, 7, size=shape[0])
    return dict(coo=coo, vals=vals, shape=shape, X=X, labels=labels, train=np.arange(0, 300), valid=np.arange(300, 600))


def make_model(gnntf, cora, **option):
    gnntf.set_seed(11)
    torch.manual_seed(3)
    model = gnntf.GCN(gnntf.SparseCOO(cora["coo"], cora["vals"], cora["shape"]), cora["X"], 7, latent_dims=[64, 64], **option)
    model.reset()
    rng = np.random.default_rng(12)
    for layer in model.layers():                            # (the biases start at zero: give them values)
        layer.b.data.copy_(dev(rng.uniform(-0.3, 0.3, size=tuple(layer.b.shape)).astype(np.float32)))
    return model


def record_kernels(monkeypatch, sparse, graph):
    """Every kernel name the handle reports after a call of sparse.spmm / sparse.dense / sparse._gcn_launch, in order."""
    seen = []
    for fn in ("spmm", "dense", "_gcn_launch"):
        def wrapped(*args, _inner=getattr(sparse, fn), _fn=fn, **kwargs):
            result = _inner(*args, **kwargs)
            seen.append((_fn, graph.last_kernel()))
            return result
        monkeypatch.setattr(sparse, fn, wrapped)
    return seen


def test_model_eval_logits_against_float64(gnntf, cora, monkeypatch):
    fused, default = make_model(gnntf, cora, gcn_layer="fused"), make_model(gnntf, cora)
    assert default.gcn_layer == "composed"
    logits = dict()
    for name, model in (("fused", fused), ("default", default)):
        seen = record_kernels(monkeypatch, gnntf.sparse, model.graph)
        model.training_mode(False)
        with torch.no_grad():
            logits[name] = host(model(model.features))
        monkeypatch.undo()
        if name == "fused":                                 # the first layer gathers at the feature width: today's two launches
            assert [fn for fn, _ in seen] == ["spmm", "dense", "_gcn_launch", "_gcn_launch"]
            assert [k for _, k in seen[2:]] == [fused_name(64, hubs=False)] * 2
        else:                                               # without the keyword: today's calls, layer by layer
            assert [fn for fn, _ in seen] == ["spmm", "dense"] * 3 and not any("gcn" in k for _, k in seen)
            default_seen = seen
    named = make_model(gnntf, cora, gcn_layer="composed")
    seen = record_kernels(monkeypatch, gnntf.sparse, named.graph)
    named.training_mode(False)
    with torch.no_grad():
        assert np.array_equal(host(named(named.features)), logits["default"])
    monkeypatch.undo()
    assert seen == default_seen
    # float64 with the same weights, the bound propagated layer by layer: E_l = (|A| E_(l-1)) |W_l| + the layer's own bound
    g = fused.graph
    A = weights_csr(g, fused.get_adjacency(0).vals)
    H, E = cora["X"].astype(np.float64), np.zeros(cora["X"].shape)
    for layer in [l for l in fused.layers() if isinstance(l, gnntf.GCNLayer)]:
        Wl, bl = host(layer.W), host(layer.b).reshape(-1)
        own = gref.forward_ref(A, H, Wl, bl, True, L=g.long_row_threshold)
        H, E = own["out"], (abs(A) @ E) @ np.abs(Wl.astype(np.float64)) + own["out_bound"]
    for name in ("fused", "default"):
        worst = gref.ratio(logits[name], H, E)
        print(f"{name}: eval logits error / propagated bound = {worst:.3f}")
        assert worst <= 1
    top = np.sort(H, axis=1)
    first, second = H.argmax(axis=1), np.argsort(H, axis=1)[:, -2]
    rows = np.arange(len(H))
    decided = top[:, -1] - top[:, -2] > E[rows, first] + E[rows, second]
    print(f"the bound decides the argmax of {decided.mean():.1%} of the rows")
    assert decided.any() and np.array_equal(logits["fused"].argmax(axis=1)[decided], first[decided])


FUSED_MODEL = dict(gcn_layer="fused", feature_dropout="fused")


def three_steps(gnntf, cora, model):
    task = gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]])
    losses, grads, kernels = [], [], set()
    first = model._mask_calls
    torch.manual_seed(9)
    for _ in range(3):
        with model:
            for v in model.vars():
                v.var.grad = None
            loss = task.loss(model(model.features))
            kernels.add(model.graph.last_kernel())
            loss.backward()
        losses.append(float(loss.detach()))
        grads.append([v.var.grad.clone() for v in model.vars()])
        with torch.no_grad():
            for v in model.vars():
                v.var -= 0.05 * v.var.grad
    return losses, grads, model._mask_calls - first, kernels


def test_model_training_is_reproducible_from_the_seed(gnntf, cora):
    one = three_steps(gnntf, cora, make_model(gnntf, cora, **FUSED_MODEL))
    two = three_steps(gnntf, cora, make_model(gnntf, cora, **FUSED_MODEL))
    # per step: the adjacencies of the two latent layers, and the mask of the second (the first, at the feature width, keeps torch's)
    assert one[2] == two[2] == 3 * 3
    assert one[0] == two[0] and all(np.isfinite(one[0])) and len(set(one[0])) == 3
    for step_one, step_two in zip(one[1], two[1]):
        assert len(step_one) == 6 and all(torch.equal(a_, b_) for a_, b_ in zip(step_one, step_two))
        assert all(float(a_.abs().max()) > 0 for a_ in step_one)
    assert one[3] == {fused_name(64, hubs=False)}           # the last layer: no edge dropout, no mask
    composed = three_steps(gnntf, cora, make_model(gnntf, cora))
    assert composed[2] == 3 * 2 and not any("gcn" in k for k in composed[3])


def test_captured_training_equals_eager(gnntf, cora, monkeypatch):
    """train(capture=True) for 3 epochs, bit for bit the eager run (the pattern of tests/test_gpu_gcnii_drop.py)."""
    from gnntf import training
    observed, observe = [], training._BestSoFar.observe
    monkeypatch.setattr(training._BestSoFar, "observe", lambda self, loss: (observed[-1].append(loss), observe(self, loss))[1])
    results = []
    for capture in (False, True):
        observed.append([])
        model = make_model(gnntf, cora, **FUSED_MODEL)
        # (every layer's dropout from the counter RNG: the first layer's too, so that no mask depends on torch's generator under capture)
        layers = [l for l in model.layers() if isinstance(l, gnntf.GCNLayer)]
        layers[0].dropout = 0
        gnntf.set_seed(11)
        torch.manual_seed(5)
        valid = gnntf.NodeClassification(cora["valid"], cora["labels"][cora["valid"]])
        model.train(train=gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]]), valid=valid, epochs=3, patience=50,
                    capture=capture, optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
        results.append(([v.var.detach().clone() for v in model.vars()], float(model.loss(valid)), model._mask_calls))
    (eager, eager_loss, eager_masks), (captured, captured_loss, captured_masks) = results
    assert eager_masks == captured_masks == 3 * 3
    assert all(torch.equal(e, c) for e, c in zip(eager, captured))
    assert eager_loss == captured_loss
    assert len(observed[0]) == len(observed[1]) == 3 and observed[0] == observed[1] and len(set(observed[0])) == 3


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_write_nothing(gnntf, world):
    nat = gnntf.sparse.nat
    lib = nat.lib()
    w = world["T"]
    g, n = w["g"], w["n"]
    op = operands(n, 64, 40)
    Xd, Wd, bd = dev(op["X"]), dev(op["W"]), dev(op["bias"])
    out, agg, work = (torch.full(shape, SENTINEL, device="cuda") for shape in ((n, 40), (n, 64), (n, 64)))

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in (out, agg, work))

    def refused(rc, *causes):
        message = lib.gnx_last_error()
        assert rc == -1 and b"gnx_gcn_step" in message and all(c in message for c in causes), message
        assert untouched()

    refused(raw_step(nat, g, Xd, Wd, bd, Xd, 64, agg=agg), b"out must not alias an input")                 # out is X
    refused(raw_step(nat, g, Xd, Wd, bd, out, 40, agg=Xd), b"d_agg must be a buffer of its own")          # agg is X
    refused(raw_step(nat, g, Xd, Wd, bd, out, 40, agg=agg, work=Wd), b"d_work must be a buffer of its own")
    refused(raw_step(nat, g, Xd, Wd, bd, out, 40, agg=agg, work=agg), b"d_work must be a buffer of its own")
    refused(raw_step(nat, g, Xd, Wd, bd, out, 40, agg=out), b"d_agg must be a buffer of its own")
    refused(raw_step(nat, g, Xd, Wd, out, out, 40, agg=agg), b"out must not alias an input")              # out is the bias
    refused(raw_step(nat, g, Xd, Wd, bd, out, 39, agg=agg), b"ldo 39 < C_out 40")
    refused(raw_step(nat, g, Xd, Wd, bd, out, 40, agg=agg, ldw=39), b"ldw 39 < C_out 40")
    refused(raw_step(nat, g, Xd, Wd, bd, out, 40, agg=agg, rate=1.0), b"dropout rate 1 outside [0, 1)")
    refused(raw_step(nat, g, Xd, Wd, bd, out, 40, agg=agg, rate=-0.5), b"outside [0, 1)")
    refused(raw_step(nat, g, Xd, Wd, bd, out, 40, agg=agg, act=7), b"invalid activation 7")
    D = torch.ones(n, device="cuda")

    def dropped_step(edge_p=0.5, D_=D, out_=out):
        return lib.gnx_gcn_step_dropped(g.handle, nat.ptr(D_), edge_p, E_SEED, E_STREAM, nat.ptr(Xd), 64, 64, nat.ptr(Wd), 40, 40, nat.ptr(bd), 1, 0.0,
                                        SEED, STREAM, nat.ptr(out_), 40, nat.ptr(agg), None, nat.current_stream())

    refused(dropped_step(edge_p=1.0), b"gnx_gcn_step_dropped", b"outside [0, 1)")
    refused(dropped_step(D_=None), b"gnx_gcn_step_dropped: NULL degree scales")
    refused(dropped_step(out_=D), b"gnx_gcn_step_dropped: out must not alias an input")
    assert raw_step(nat, g, Xd, Wd, bd, out, 40, agg=agg) == 0 and dropped_step() == 0                     # the calls themselves are well formed
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any()) and not bool((agg == SENTINEL).any())
