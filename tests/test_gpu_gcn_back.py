"""The fused GCNLayer backward on the MI355X (gnx_gcn_step_back, gnx_gcn_step_back_dropped, sparse.gcn_step_back,
gcn_step(backward="fused"), GNN(gcn_backward="fused")):  dX = (A^T G') W^T, G' gathered at the OUTPUT width.

dX is judged against the float64 reference of tests/gcn_fused_ref.py over the very float32 weights the kernels read, with
max |got - want| / dX_bound <= 1 -- the first-order bound of a float32 evaluation in any order and either association -- at regime T
(n = 1547: a ragged last tile, hub rows at the threshold of 512, a whole tile of rows without entries) and regime S (threshold 128).
Where existing code is the reference the comparison is bit for bit: gnx_gcnii_step_back with a = 0 at C_out == C_in, gnx_dense followed
by gnx_spmm_tv for the composed order, the entry over the materialised adjacency under edge dropout."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_fused_ref as gref
import test_gpu_layer_tile as tile
from test_gpu_gcn_fused import (E_SEED, E_STREAM, SEED, SENTINEL, STREAM, bits, cora, dev, dropped_world, gnntf, host, make_model,  # noqa: F401
                                operands, weights_csr)
from test_gpu_gcnii_drop import keep_mask

pytestmark = pytest.mark.gpu

PAD = 16                                                 # rows past n in a result buffer


@pytest.fixture(scope="module")
def world(gnntf):
    """Regimes T and S TRANSPOSED (the ``t`` handles of tests/test_gpu_gcnii_shapes.py): the planted rows -- hub rows, the tile of rows
    without entries, the ragged last tile -- are rows of the transposed structure, which the backward walks.  The handle, its normalised
    adjacency and the weights read back, made once and never changed."""
    out = dict()
    for name in ("T", "S"):
        coo, vals, shape, info = gref.regime_graph(name)
        g = gnntf.DeviceGraph(gnntf.SparseCOO(coo[:, ::-1].copy(), vals, shape), device="cuda:0")
        adj = gnntf.normalize(g, "symmetric")
        assert g.long_row_threshold == info["L"] and g.n_hub_rows == 0 and g.n_hub_rows_t == len(info["hub"]) > 0
        out[name] = dict(g=g, adj=adj, A=weights_csr(g, adj.vals), info=info, n=shape[0], L=info["L"])
    return out


def roundup4(c):
    return (c + 3) // 4 * 4


def back_name(C_in, edge=False, hubs=True):
    return f"k_spmm_gcn_back<{C_in}>" + ("_edrop" if edge else "") + ("+long" if hubs else "")


def composed_name(edge=False):
    return "dense+spmm_back_gcn" + ("_edrop" if edge else "")


def padded_rows(G, ldg, fill=0.0):
    """G [n, C_out] on the device in rows of stride ``ldg``, the padding columns holding ``fill``; returns (buffer, view)."""
    buf = torch.full((G.shape[0], ldg), fill, dtype=torch.float32, device="cuda")
    buf[:, :G.shape[1]] = dev(G)
    return buf, buf[:, :G.shape[1]]


def raw_back(nat, g, Gbuf, C_out, Wt, dX, work=None, vals_t=None, ldg=None, work_floats=None, edge=None):
    """gnx_gcn_step_back itself (``vals_t`` None: the handle's raw values), or with ``edge`` = (D, p) gnx_gcn_step_back_dropped."""
    tail = (nat.ptr(Gbuf), Gbuf.stride(0) if ldg is None else ldg, C_out, nat.ptr(Wt), max(Wt.stride(0), Wt.shape[1]), Wt.shape[1], nat.ptr(dX), dX.stride(0),
            nat.ptr(work), (0 if work is None else work.numel()) if work_floats is None else work_floats, nat.current_stream())
    if edge is not None:
        return nat.lib().gnx_gcn_step_back_dropped(g.handle, nat.ptr(edge[0]), edge[1], E_SEED, E_STREAM, *tail)
    return nat.lib().gnx_gcn_step_back(g.handle, nat.ptr(vals_t), *tail)


def transposed_sets(A, L, info):
    """The row sets of the TRANSPOSED structure: its hub rows, its rows without entries, and the ragged last tile."""
    deg_t = np.diff(sp.csr_matrix(A.T).indptr)
    return dict(hub=np.flatnonzero(deg_t > L), empty=np.flatnonzero(deg_t == 0), ragged=info["ragged"], deg=deg_t)


@functools.lru_cache(maxsize=None)
def want_dX(regime, C_in, C_out):
    """(dX, dX_bound) of gref.backward_ref over the regime's float32 weights; made once per case."""
    return WANT[regime](C_in, C_out)


WANT = dict()


@pytest.fixture(scope="module")
def refs(world):
    for name, w in world.items():
        def make(C_in, C_out, w=w):
            op = operands(w["n"], C_in, C_out)
            want = gref.backward_ref(w["A"], np.zeros((w["n"], C_in), dtype=np.float32), op["G"], op["W"], L=w["L"])
            return want["dX"], want["dX_bound"]
        WANT[name] = make
    yield world
    want_dX.cache_clear()
    WANT.clear()


# ---- 1. against float64 ------------------------------------------------------------------------------------------------------------------
FLOAT64_CASES = [("T",) + s for s in gref.SHAPES] + [("S", 64, 40), ("S", 64, 7)]


@pytest.mark.parametrize("regime, C_in, C_out", FLOAT64_CASES)
def test_against_float64(gnntf, refs, regime, C_in, C_out):
    sparse, nat = gnntf.sparse, gnntf.sparse.nat
    w = refs[regime]
    g, n = w["g"], w["n"]
    op = operands(n, C_in, C_out)
    want, bound = want_dX(regime, C_in, C_out)
    sets = transposed_sets(w["A"], w["L"], w["info"])
    assert all(np.array_equal(np.sort(sets[k]), np.sort(w["info"][k])) and len(sets[k]) > 0 for k in ("hub", "empty"))
    got = sparse.gcn_step_back(w["adj"], dev(op["G"]), dev(op["W"]))
    assert g.last_kernel() == back_name(C_in), g.last_kernel()
    Gbuf, _ = padded_rows(op["G"], roundup4(C_out))
    Wt = dev(op["W"]).t().contiguous()
    dX, work = torch.full((n, C_in), SENTINEL, device="cuda"), torch.empty(n, C_out, device="cuda")
    assert raw_back(nat, g, Gbuf, C_out, Wt, dX, work, vals_t=w["adj"].transposed_values()) == 0, nat.lib().gnx_last_error()
    assert g.last_kernel() == back_name(C_in), g.last_kernel()
    assert np.array_equal(bits(got), bits(dX))           # the functional form is the entry; two calls give the same bits
    for name, rows in (("all", None), ("hub", sets["hub"]), ("empty", sets["empty"]), ("ragged", sets["ragged"])):
        r = gref.ratio(host(got), want, bound, rows)
        print(f"{regime} {C_in}->{C_out} {name} rows: dX error / bound = {r:.3f}")
        assert r <= 1, (regime, C_in, C_out, name)
    assert float(got[sets["empty"]].abs().max()) == 0                           # rows without transposed entries: exactly 0, written
    somewhere = np.flatnonzero(np.abs(want).max(axis=1) > 0)                   # (entries into a vertex of scale 0 weigh 0)
    assert len(somewhere) > n // 2 and bool((got[somewhere].abs().amax(dim=1) > 0).all())


# ---- 2. bit for bit against existing code ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["T", "S"])
@pytest.mark.parametrize("C", [16, 32, 64])
def test_square_layer_is_the_gcnii_backward(gnntf, world, regime, C):
    """C_out == C_in: the same gather, the same k order, and beta = 1 of gnx_gcnii_step_back(a = 0) is exact -- hub rows included."""
    sparse = gnntf.sparse
    w = world[regime]
    op = operands(w["n"], C, C)
    Gd, Wd = dev(op["G"]), dev(op["W"])
    want, none = sparse.gcnii_step_back(w["adj"], Gd, 0.0, Wd.t().contiguous(), want_S=False)
    assert none is None and w["g"].last_kernel() == "spmm_gcnii_back_mfma"
    got = sparse.gcn_step_back(w["adj"], Gd, Wd)
    assert w["g"].last_kernel() == back_name(C)
    differ = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert len(differ) == 0, (regime, C, differ[:8])


@pytest.mark.parametrize("C_in, C_out, ldg", [(24, 8, 8), (16, 64, 64), (64, 7, 7), (64, 7, 9), (64, 40, 44)])
def test_composed_order_inside_the_entry(gnntf, world, C_in, C_out, ldg):
    """Other widths, C_out > C_in, rows of G' that are no whole 16-byte pieces (ldg = 7, 9) and a base that is not 16-byte aligned
    (the last case): gnx_dense followed by gnx_spmm_tv, bit for bit, under the composed name."""
    sparse, nat = gnntf.sparse, gnntf.sparse.nat
    w = world["T"]
    g, n = w["g"], w["n"]
    op = operands(n, C_in, C_out)
    shift = 1 if ldg == 44 else 0
    whole = torch.zeros(shift + n * ldg, device="cuda")
    Gv = whole[shift:].view(n, ldg)[:, :C_out]
    Gv.copy_(dev(op["G"]))
    assert shift == 0 or Gv.data_ptr() % 16 != 0
    Wt = dev(op["W"]).t().contiguous()
    gT = sparse._dense_launch(Gv, Wt, None, False)
    want = sparse._launch(w["adj"], gT, None, 1.0, 0.0, nat.ACT_NONE, transposed=True)
    dX, work = torch.full((n, C_in), SENTINEL, device="cuda"), torch.empty(n, C_in, device="cuda")
    assert raw_back(nat, g, Gv, C_out, Wt, dX, work, vals_t=w["adj"].transposed_values()) == 0, nat.lib().gnx_last_error()
    assert g.last_kernel() == composed_name(), g.last_kernel()
    assert np.array_equal(bits(dX), bits(want)) and np.array_equal(bits(work), bits(gT))


# ---- 3. padding and the edges of the output ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_in, C_out, ldg", [(64, 7, 8), (32, 1, 4), (64, 40, 40), (64, 7, 16)])
def test_padding_does_not_matter_and_nothing_else_is_written(gnntf, refs, C_in, C_out, ldg):
    nat = gnntf.sparse.nat
    w = refs["T"]
    g, n = w["g"], w["n"]
    op = operands(n, C_in, C_out)
    sets = transposed_sets(w["A"], w["L"], w["info"])
    Wt = dev(op["W"]).t().contiguous()
    results = []
    for fill in (0.0, float("nan")):
        Gbuf, _ = padded_rows(op["G"], ldg, fill)
        assert ldg == C_out or bool(torch.isnan(Gbuf[:, C_out:]).all()) == (fill != 0.0)
        dX = torch.full((n + PAD, C_in), SENTINEL, device="cuda")
        work = torch.full((n, C_out), SENTINEL, device="cuda")
        assert raw_back(nat, g, Gbuf, C_out, Wt, dX[:n], work, vals_t=w["adj"].transposed_values()) == 0, nat.lib().gnx_last_error()
        assert g.last_kernel() == back_name(C_in)
        torch.cuda.synchronize()
        assert bool((dX[n:] == SENTINEL).all())                                  # nothing past row n
        others = np.setdiff1d(np.arange(n), sets["hub"])
        assert bool((work[others] == SENTINEL).all())                            # d_work holds the hub rows' sums and nothing else
        assert not bool((work[sets["hub"]] == SENTINEL).any())
        results.append(dX[:n].clone())
    assert np.array_equal(bits(results[0]), bits(results[1])) and bool(torch.isfinite(results[1]).all())
    want, bound = want_dX("T", C_in, C_out)
    assert gref.ratio(host(results[1]), want, bound) <= 1


# ---- 4. tile edges -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles(gnntf):
    yield {(n, order): tile.Handle(gnntf, n, order) for n in tile.NS for order in tile.ORDERS}
    torch.cuda.empty_cache()


@pytest.mark.parametrize("order", tile.ORDERS)
@pytest.mark.parametrize("C_in, C_out", [(16, 16), (32, 7), (64, 40), (64, 64), (64, 7)])
@pytest.mark.parametrize("n", tile.NS)
def test_tile_edges(gnntf, handles, n, C_in, C_out, order):
    """n = 1, 15, 16, 17, 129 in both row orders: the one-pass gather (C_out <= 16) under a four-pass store (C_in = 64), four gather
    passes at C_out = 40, and nothing written past row n.  No hub rows: d_work is NULL."""
    nat = gnntf.sparse.nat
    h = handles[n, order]
    op = tile.gcn_operands(n, C_in, C_out)
    A = tile.graph_of(n)
    want = gref.backward_ref(A, np.zeros((n, C_in), dtype=np.float32), op["G"], op["W"])
    dense = A.toarray().T @ (op["G"].astype(np.float64) @ op["W"].astype(np.float64).T)
    assert np.allclose(dense, want["dX"], rtol=1e-12, atol=1e-12)
    Gbuf, _ = padded_rows(op["G"], roundup4(C_out), float("nan"))
    Wt = dev(op["W"]).t().contiguous()
    dX = tile.padded(n, C_in)
    where = f"gnx_gcn_step_back n={n} {C_in}<-{C_out} {order}"
    assert raw_back(nat, h.g, Gbuf, C_out, Wt, dX[:n]) == 0, nat.lib().gnx_last_error()
    assert h.g.last_kernel() == back_name(C_in, hubs=False)
    tile.within(where, tile.written(dX, n, where), dense, want["dX_bound"])


# ---- 5. under edge dropout: bit for bit the entry over the materialised adjacency ------------------------------------------------------------
@pytest.mark.parametrize("p", [0.5, 0.9])
@pytest.mark.parametrize("C_in, C_out", [(64, 40), (64, 7), (16, 16), (24, 8)])
def test_edge_dropout_equals_the_materialised_adjacency(gnntf, dropped_world, C_in, C_out, p):
    from oracle import gnntf_oracle as orc
    sparse = gnntf.sparse
    fused = C_in in (16, 32, 64)
    for name in ("t", "a", "T", "dup"):
        d = dropped_world[name]
        g, n = d["g"], d["n"]
        dropped = sparse.DroppedAdjacency(g, p, E_SEED, E_STREAM)
        mat = sparse.normalize(g, "symmetric", "none", p, E_SEED, E_STREAM)
        op = operands(n, C_in, C_out)
        _, Gv = padded_rows(op["G"], roundup4(C_out), float("nan"))
        Wt = dev(op["W"]).t().contiguous()
        hubs = g.n_hub_rows_t > 0
        assert hubs == (name in ("a", "dup"))                # ("a": a hub COLUMN of 900 entries and no hub row; "t" the other way round)
        got = sparse._gcn_back_launch(dropped, Gv, Wt, fused_edge=True)
        assert g.last_kernel() == (back_name(C_in, True, hubs) if fused else composed_name(True)), (name, g.last_kernel())
        assert dropped._vals is None and dropped.vals_t is None                  # no value array was made on the way
        want = sparse._gcn_back_launch(mat, Gv, Wt)
        assert g.last_kernel() == (back_name(C_in, False, hubs) if fused else composed_name()), (name, g.last_kernel())
        differ = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
        assert len(differ) == 0, (name, C_in, C_out, p, differ[:8])
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        if name in ("a", "t"):                               # a row all of whose transposed entries are dropped: dX = 0, written
            idx = d["coo"]
            into = np.bincount(idx[:, 1], minlength=n)
            kept = np.bincount(idx[orc.keep_mask(idx, p, E_SEED, E_STREAM), 1], minlength=n)
            rows = np.flatnonzero((into > 0) & (kept == 0))
            assert p < 0.9 or len(rows) >= 1
            if len(rows):
                assert float(got[rows].abs().max()) == 0


# ---- 6. autograd -------------------------------------------------------------------------------------------------------------------------
def one_backward(gnntf, adj, op, relu, mask, backward, measure=False):
    """out and the gradients of (X, W, bias) of gcn_step(..., backward=...) under the upstream gradient op["G"]; with ``measure`` also
    the peak of torch's allocator over the backward, above what was allocated when it started."""
    leaves = [dev(op[k]).requires_grad_() for k in ("X", "W", "bias")]
    out = gnntf.gcn_step(adj, *leaves, relu=relu, dropout=mask, edge_dropout="fused", backward=backward)
    kernel = adj.graph.last_kernel()
    upstream = dev(op["G"])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out.backward(upstream)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    return dict(out=out.detach(), grads=[leaf.grad for leaf in leaves], kernel=kernel, last=adj.graph.last_kernel(), peak=peak)


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("mask", [None, (0.5, SEED, STREAM)])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C_in, C_out", [(64, 40), (64, 7), (24, 8)])
def test_autograd(gnntf, world, C_in, C_out, relu, mask, edge):
    sparse = gnntf.sparse
    w = world["T"]
    g, n = w["g"], w["n"]
    op = operands(n, C_in, C_out)
    if edge:
        adj = sparse.DroppedAdjacency(g, 0.5, E_SEED, E_STREAM)
        A = weights_csr(g, sparse.normalize(g, "symmetric", "none", 0.5, E_SEED, E_STREAM).vals)
    else:
        adj, A = w["adj"], w["A"]
    fused, composed = (one_backward(gnntf, adj, op, relu, mask, how) for how in ("fused", "composed"))
    one_launch = C_in in (16, 32, 64)
    assert fused["kernel"] == composed["kernel"]
    assert fused["last"] == (back_name(C_in, edge) if one_launch else composed_name(edge)), fused["last"]
    assert "gcn_back" not in composed["last"]
    assert not edge or (adj._vals is None and adj.vals_t is None)
    # out, dW and db: bit for bit those of the composed backward
    assert np.array_equal(bits(fused["out"]), bits(composed["out"]))
    assert np.array_equal(bits(fused["grads"][1]), bits(composed["grads"][1]))
    assert np.array_equal(bits(fused["grads"][2]), bits(composed["grads"][2]))
    p = 0.0 if mask is None else mask[0]
    keep = None if mask is None else keep_mask(SEED, STREAM, p, n, C_out)
    agg32 = host(sparse._gcn_launch(adj, dev(op["X"]), dev(op["W"]), dev(op["bias"]), relu, keep_agg=True, fused_edge=edge)[1])
    G = gref.gate_f32(op["G"], host(fused["out"]), relu, p, keep)
    want = gref.backward_ref(A, agg32, G, op["W"], L=w["L"])
    for run_name, run in (("fused", fused), ("composed", composed)):
        for name, grad in zip(("dX", "dW", "db"), run["grads"]):
            got = host(grad).reshape(want[name].shape if name != "db" else (1, -1))
            worst = gref.ratio(got, want[name].reshape(got.shape), want[name + "_bound"].reshape(got.shape))
            print(f"{C_in}->{C_out} relu={relu} edge={edge} mask={mask is not None} {run_name} {name}: error / bound = {worst:.3f}")
            assert worst <= 1 and float(np.abs(got).max()) > 0
    apart = gref.ratio(host(fused["grads"][0]), host(composed["grads"][0]).astype(np.float64), 2 * want["dX_bound"])
    print(f"{C_in}->{C_out} relu={relu} edge={edge} mask={mask is not None}: |dX fused - dX composed| / (2 bound) = {apart:.3f}")
    assert apart <= 1


def backward_peaks(gnntf, w):
    """Peak of torch's allocator over the backward of the 64 -> 7 layer at regime T (relu and a mask), above what was allocated when the
    backward started: (composed, fused, n * C_in * 4)."""
    n, C_in, C_out = w["n"], 64, 7
    op = operands(n, C_in, C_out)
    runs = dict()
    for how in ("composed", "fused", "composed", "fused"):      # (the second round: the allocator's pools are warm)
        runs[how] = one_backward(gnntf, w["adj"], op, True, (0.5, SEED, STREAM), how)["peak"]
    wide = n * C_in * 4
    print(f"peak over the backward: composed {runs['composed']} B, fused {runs['fused']} B, difference {runs['composed'] - runs['fused']} B, "
          f"n * C_in * 4 = {wide} B")
    return runs["composed"], runs["fused"], wide


def test_fused_backward_holds_one_wide_matrix(gnntf, world):
    """The composed backward holds G' W^T [n, C_in] beside dX [n, C_in], on top of the saved A . X.  The fused one lets A . X go once dW
    is made and only then allocates dX: above what was allocated when the backward started it holds less than ONE [n, C_in] matrix --
    dX in the place of A . X, G' in padded rows [n, 8], the hub rows' sums [n, 7] and a narrow transient."""
    composed, fused, wide = backward_peaks(gnntf, world["T"])
    assert fused < wide and 2 * wide <= composed
    assert fused <= world["T"]["n"] * (8 + 7 + 7 + 7) * 4 + 16 * 512            # G', the hub rows' sums, narrow transients; block rounding


def test_fused_backward_peak_is_a_wide_matrix_lower(gnntf, world):
    """The peak over the fused backward is at least n * C_in * 4 bytes below the composed backward's (64 -> 7, regime T)."""
    composed, fused, wide = backward_peaks(gnntf, world["T"])
    assert composed - fused >= wide


def test_fused_node_runs_its_backward_once(gnntf, world):
    """The price of letting A . X go early: a retained graph cannot run the fused node's backward again, and says so; the composed
    node can."""
    w = world["T"]
    op = operands(w["n"], 64, 7)
    for how in ("fused", "composed"):
        leaves = [dev(op[k]).requires_grad_() for k in ("X", "W", "bias")]
        out = gnntf.gcn_step(w["adj"], *leaves, relu=True, backward=how)
        out.backward(dev(op["G"]), retain_graph=True)
        first = [leaf.grad.clone() for leaf in leaves]
        if how == "fused":
            with pytest.raises(Exception, match="run the forward again"):
                out.backward(dev(op["G"]))
        else:
            out.backward(dev(op["G"]))
            assert all(torch.equal(leaf.grad, 2 * f) for leaf, f in zip(leaves, first))


# ---- 7. the model ------------------------------------------------------------------------------------------------------------------------
BACK_MODEL = dict(gcn_layer="fused", feature_dropout="fused", gcn_backward="fused")
COMPOSED_MODEL = dict(gcn_layer="fused", feature_dropout="fused")
# |loss_3(fused backward) - loss_3(composed backward)| <= LOSS_TOL * loss_3: the two runs see the same masks and differ in the roundings
# of dX of the 64 -> 7 and 64 -> 64 layers alone.  The yardstick is the difference between two COMPOSED runs of this model that differ in
# their summation order alone -- the same three steps with every dropout off, once as built and once with reorder="degree" (another
# entry order in every row sum, the same sums otherwise).  Measured on the MI355X: both pairs agree in every bit (1.9426522254943848
# twice; fused and composed 1.9505761861801147 twice) -- last-place changes of a gradient times the step of 0.05 stay far below the
# last place of a loss near 1.95.  The tolerance is therefore what the float32 loss itself can move by when an addend of its mean over
# 300 nodes changes in the last place: a few units in the last place of a value in [1, 2), taken as 4 * 2^-23.
LOSS_TOL = 4 * 2.0 ** -23


PHASE = dict(now="forward")


def record_back_kernels(monkeypatch, sparse, graph):
    """Every kernel name the handle reports after a call of the launchers DURING A BACKWARD (three_steps says when), in order."""
    seen = []
    for fn in ("_dense_launch", "_launch", "_gcn_back_launch"):
        def wrapped(*args, _inner=getattr(sparse, fn), _fn=fn, **kwargs):
            result = _inner(*args, **kwargs)
            if PHASE["now"] == "backward":
                seen.append((_fn, graph.last_kernel()))
            return result
        monkeypatch.setattr(sparse, fn, wrapped)
    return seen


def three_steps(gnntf, cora, model):
    task = gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]])
    losses, grads = [], []
    torch.manual_seed(9)
    for _ in range(3):
        with model:
            for v in model.vars():
                v.var.grad = None
            loss = task.loss(model(model.features))
            PHASE["now"] = "backward"
            try:
                loss.backward()
            finally:
                PHASE["now"] = "forward"
        losses.append(float(loss.detach()))
        grads.append([v.var.grad.clone() for v in model.vars()])
        with torch.no_grad():
            for v in model.vars():
                v.var -= 0.05 * v.var.grad
    return losses, grads


def without_dropout(model, gnntf):
    for layer in model.layers():
        if isinstance(layer, gnntf.GCNLayer):
            layer.dropout = layer.graph_dropout = 0
    return model


def test_model_training(gnntf, cora, monkeypatch):
    sparse = gnntf.sparse
    model = make_model(gnntf, cora, **BACK_MODEL)
    assert model.gcn_backward == "fused" and make_model(gnntf, cora).gcn_backward == "composed"
    seen = record_back_kernels(monkeypatch, sparse, model.graph)
    one = three_steps(gnntf, cora, model)
    monkeypatch.undo()
    two = three_steps(gnntf, cora, make_model(gnntf, cora, **BACK_MODEL))
    assert one[0] == two[0] and all(np.isfinite(one[0])) and len(set(one[0])) == 3
    for step_one, step_two in zip(one[1], two[1]):
        assert len(step_one) == 6 and all(torch.equal(a_, b_) for a_, b_ in zip(step_one, step_two))
        assert all(float(a_.abs().max()) > 0 for a_ in step_one)
    # per step, last layer first: the 64 -> 7 layer (constant adjacency) and the 64 -> 64 layer (edge dropout) take the new launch; the first
    # layer, at the feature width, keeps gnx_dense (its input needs no gradient: no transposed SpMM)
    names = [k for _, k in seen]
    per_step = [("_gcn_back_launch", back_name(64, hubs=False)), ("_gcn_back_launch", back_name(64, edge=True, hubs=False))]
    assert [s for s in seen if s[0] == "_gcn_back_launch"] == per_step * 3, seen
    assert not any("dense+spmm_back" in k for k in names) and not any(fn == "_launch" for fn, _ in seen)
    # without the keyword: today's calls and names, and the same ones under gcn_backward="composed"
    recorded = []
    for option in (COMPOSED_MODEL, dict(COMPOSED_MODEL, gcn_backward="composed")):
        other = make_model(gnntf, cora, **option)
        seen = record_back_kernels(monkeypatch, sparse, other.graph)
        recorded.append((three_steps(gnntf, cora, other), list(seen)))
        monkeypatch.undo()
    (composed, composed_seen), (named, named_seen) = recorded
    assert composed_seen == named_seen and composed[0] == named[0]
    assert not any(fn == "_gcn_back_launch" or "gcn_back" in k for fn, k in composed_seen)
    assert [fn for fn, _ in composed_seen] == ["_dense_launch", "_launch"] * 2 * 3, composed_seen
    # the loss after three steps against the composed backward's
    apart = abs(one[0][-1] - composed[0][-1]) / abs(composed[0][-1])
    orders = [three_steps(gnntf, cora, without_dropout(make_model(gnntf, cora, gcn_layer="fused", **option), gnntf))[0][-1]
              for option in (dict(), dict(reorder="degree"))]
    print(f"loss after three steps: fused {one[0][-1]!r}, composed {composed[0][-1]!r}, relative difference {apart:.3g}; two composed "
          f"runs in different summation orders: {orders[0]!r}, {orders[1]!r}, relative difference {abs(orders[0] - orders[1]) / orders[0]:.3g}")
    assert apart <= LOSS_TOL


def test_captured_training_equals_eager(gnntf, cora, monkeypatch):
    """train(capture=True) for 3 epochs, bit for bit the eager run (the pattern of tests/test_gpu_gcn_fused.py)."""
    from gnntf import training
    observed, observe = [], training._BestSoFar.observe
    monkeypatch.setattr(training._BestSoFar, "observe", lambda self, loss: (observed[-1].append(loss), observe(self, loss))[1])
    results = []
    for capture in (False, True):
        observed.append([])
        model = make_model(gnntf, cora, **BACK_MODEL)
        layers = [l for l in model.layers() if isinstance(l, gnntf.GCNLayer)]
        layers[0].dropout = 0                                # (no mask from torch's generator under capture)
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


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_write_nothing(gnntf, world):
    """Every refusal is an argument check before any launch: the result and the work buffer keep their sentinels."""
    nat = gnntf.sparse.nat
    lib = nat.lib()
    w = world["T"]
    g, n = w["g"], w["n"]
    op = operands(n, 64, 40)
    Gbuf, _ = padded_rows(op["G"], 40)
    Wt = dev(op["W"]).t().contiguous()
    vals_t = w["adj"].transposed_values()
    dX, work, wide = (torch.full(shape, SENTINEL, device="cuda") for shape in ((n, 64), (n, 40), (n, 64)))

    def refused(rc, *causes, entry=b"gnx_gcn_step_back: "):
        message = lib.gnx_last_error()
        assert rc == -1 and message.startswith(entry) and all(c in message for c in causes), message
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in (dX, work, wide))

    refused(raw_back(nat, g, Gbuf, 40, Wt, dX, None, vals_t), b"needs d_work of n * C_out", b"hub rows")
    refused(raw_back(nat, g, Gbuf, 40, Wt, dX, work, vals_t, work_floats=n * 40 - 1), b"needs d_work of n * C_out", b"hub rows")
    Gwide, _ = padded_rows(op["G"], 64, SENTINEL)              # G' in rows of stride 64: as dX it passes the stride checks
    refused(raw_back(nat, g, Gwide, 40, Wt, Gwide, work, vals_t), b"dX must not alias an input")
    refused(raw_back(nat, g, Gbuf, 40, Wt, Wt, work, vals_t), b"dX must not alias an input")
    refused(raw_back(nat, g, Gbuf, 40, Wt, dX, dX, vals_t), b"d_work must be a buffer of its own")
    refused(raw_back(nat, g, Gbuf, 40, Wt, dX, Gbuf, vals_t), b"d_work must be a buffer of its own")
    refused(raw_back(nat, g, Gbuf, 40, Wt, dX, work, vals_t, ldg=39), b"ldg 39 < C_out 40")
    # rows of G' that are no whole 16-byte pieces run the composed order, which needs n * C_in floats: [n, 40] is too little, and the
    # message says why
    refused(raw_back(nat, g, Gbuf, 39, Wt[:39], dX, work, vals_t, ldg=39), b"needs d_work of n * C_in", b"ldg % 4 != 0 or ldg < roundup4(C_out)")
    refused(raw_back(nat, g, Gbuf, 40, Wt, dX, None, edge=(None, 0.5)), b"NULL degree scales", entry=b"gnx_gcn_step_back_dropped: ")
    D = torch.ones(n, device="cuda")
    refused(raw_back(nat, g, Gbuf, 40, Wt, dX, work, edge=(D, 1.0)), b"outside [0, 1)", entry=b"gnx_gcn_step_back_dropped: ")
    refused(raw_back(nat, g, Gbuf, 40, Wt, Wt, work, edge=(D, 0.5)), b"dX must not alias an input", entry=b"gnx_gcn_step_back_dropped: ")
    wide_graph = gnntf.DeviceGraph(gnntf.SparseCOO(np.array([[0, 1], [1, 2]], dtype=np.int64), np.ones(2, dtype=np.float32), (n, n + 1)),
                                   device="cuda:0")
    refused(raw_back(nat, wide_graph, Gbuf, 40, Wt, dX, work), b"needs a square graph")
    assert raw_back(nat, g, Gbuf, 40, Wt, dX, work, vals_t) == 0 and raw_back(nat, g, Gbuf, 40, Wt, wide, work, edge=(D, 0.5)) == 0
    torch.cuda.synchronize()                                 # the calls themselves are well formed
    assert not bool((dX == SENTINEL).any()) and not bool((wide == SENTINEL).any())
