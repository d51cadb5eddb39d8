"""Fused training edge dropout on graphs whose COO stores entries more than once (graph2adj of a graph that already holds both
directions: every entry twice).  After DeviceGraph.enable_entry_dropout (gnx_graph_enable_entry_dropout) the fused training kernels
make every slot's weight from its kept entries -- bit for bit what gnx_graph_normalize + gnx_spmm give on the same handle."""
import numpy as np
import pytest
import torch

import graphs
from oracle import gnntf_oracle as orc

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


def make_graph(gnntf, coo, vals, shape):
    return gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")


def both_directions(n, m, seed):
    """(i) orc.graph2adj of a graph whose edge list holds both directions: every slot twice, equal values."""
    coo, _, _ = graphs.rmat_symmetric_coo(n, m, seed=seed)
    return orc.graph2adj(range(n), [tuple(e) for e in coo])


def unequal_duplicates(n, nnz, seed):
    """(ii) duplicates with unequal values, some slots with three or more entries; (iv) one slot holding +v and -v."""
    coo, vals, shape = graphs.random_coo(n, n, nnz, seed=seed, weighted=True, dup_frac=0.3)
    coo = np.concatenate([coo, [[1, 2], [1, 2]]])
    vals = np.concatenate([vals, np.float32([0.75, -0.75])]).astype(np.float32)
    return coo, vals, shape


def hub_graph(seed=7):
    """(iii) the hub construction of test_dropped_adjacency_fused_into_spmm_bitwise, every entry stored twice and a share three
    times with another value: rows and columns of more than 512 entries run the long-row kernels."""
    n = 2500
    coo, _, shape = graphs.rmat_symmetric_coo(n, 30000, seed=seed)
    hub = np.random.default_rng(1).choice(np.arange(1, n), size=1300, replace=False)
    coo = np.unique(np.concatenate([coo, np.stack([np.zeros_like(hub), hub], 1), np.stack([hub, np.zeros_like(hub)], 1)]), axis=0)
    vals = (np.random.default_rng(2).random(len(coo)) + 0.5).astype(np.float32)
    third = np.arange(0, len(coo), 5)
    coo = np.concatenate([coo, coo, coo[third]])
    vals = np.concatenate([vals, vals, vals[third] * np.float32(0.5)])
    return coo, vals, shape


GRAPHS = {"both_directions": lambda: both_directions(1500, 12000, 3), "unequal": lambda: unequal_duplicates(1200, 16000, 5),
          "hub": hub_graph}


@pytest.fixture(scope="module")
def prepared(gnntf):
    out = {}
    for name, build in GRAPHS.items():
        coo, vals, shape = build()
        g = make_graph(gnntf, coo, vals, shape)
        assert g.nnz_entries > g.nnz and not g.entry_dropout
        g.enable_entry_dropout()
        assert g.entry_dropout
        out[name] = (coo, vals, shape, g)
    return out


WIDTHS = [3, 7, 8, 16, 24, 40, 64, 100, 128, 256, 300]


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("C", WIDTHS)
def test_entry_dropout_fused_into_spmm_bitwise(gnntf, prepared, name, C):
    """gnx_spmm_dropped on a prepared handle with duplicates == gnx_graph_normalize + gnx_spmm / gnx_spmm_tv on the same handle, bit
    for bit, forward and transposed, through the _entries instantiations; and the oracle's adjacency in float64."""
    _fused_bitwise(gnntf, prepared, name, C, 0.5)


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("p", [0.1, 0.9])
def test_entry_dropout_fused_into_spmm_bitwise_at_other_rates(gnntf, prepared, name, C, p):
    """The same at p = 0.1 and 0.9 (the same parameters under the same name would rename every case of the test above): 1 / (1 - p)
    is no power of two there, so the kept values' products round."""
    _fused_bitwise(gnntf, prepared, name, C, p)


def _fused_bitwise(gnntf, prepared, name, C, p):
    from gnntf.sparse import DroppedAdjacency, _launch
    coo, vals, shape, g = prepared[name]
    n = shape[0]
    rng = np.random.default_rng(C)
    X, H0 = dev(rng.standard_normal((n, C)).astype(np.float32)), dev(rng.standard_normal((n, C)).astype(np.float32))
    fused = gnntf.sparse.dropped_adjacency(g, p, 21, 6)
    assert isinstance(fused, DroppedAdjacency)
    two_pass = gnntf.normalize(g, "symmetric", "none", dropout=p, seed=21, stream_id=6)
    for transposed in (False, True):
        a = _launch(fused, X, H0, 0.9, 0.1, 0, transposed=transposed)
        kernel = g.last_kernel()
        b = _launch(two_pass, X, H0, 0.9, 0.1, 0, transposed=transposed)
        assert torch.equal(a, b), (name, C, p, transposed, float((a - b).abs().max()))
        assert kernel.endswith("_drop_entries"), kernel
    ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=p, training=True, seed=21, stream=6, dtype=np.float64)
    want = orc.sparse_dense_matmul(ai, av, shape, X.cpu().numpy().astype(np.float64)) * 0.9 + 0.1 * H0.cpu().numpy()
    np.testing.assert_allclose(_launch(fused, X, H0, 0.9, 0.1, 0).cpu().numpy(), want, rtol=RTOL, atol=ATOL)


def test_hub_graph_runs_the_long_row_kernels(gnntf, prepared):
    from gnntf.sparse import _launch
    _, _, shape, g = prepared["hub"]
    rowptr = g.csr_arrays()[0].cpu().numpy()
    assert np.diff(rowptr).max() > 1024                                 # > 2 chunks of 512 slots
    X = torch.rand(shape[0], 8, device="cuda")
    D = gnntf.sparse.dropped_degree_scales(g, 0.5, 3, 4, 1)[0]
    _launch(gnntf.sparse.DroppedAdjacency(g, 0.5, 3, 4, D=D), X, None, 1.0, 0.0, 0)
    assert g.last_kernel() == "spmm_group8_drop_entries"


def dense_loop(coo, vals, shape, H0np, gout, K, a, p, seed, first, relu):
    H0d = torch.tensor(H0np, dtype=torch.float64, requires_grad=True)
    H = H0d
    for k in range(K):
        ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=p, training=True, seed=seed, stream=first + k, dtype=np.float64)
        H = (1 - a) * (torch.tensor(orc.to_dense(ai, av, shape)) @ H) + a * H0d
        if relu:
            H = torch.relu(H)
    H.backward(torch.tensor(gout, dtype=torch.float64))
    return H.detach().numpy(), H0d.grad.numpy()


@pytest.mark.parametrize("name", ["both_directions", "unequal"])
@pytest.mark.parametrize("K,relu", [(4, False), (10, False), (4, True), (10, True)])
def test_training_loop_on_prepared_handle(gnntf, prepared, name, K, relu):
    """ppr_loop forward + dH0 on the prepared handle (weights made inside the SpMM) against a second, never-prepared handle of the
    same COO (materialised per iteration): bit for bit, with and without relu; and against dense float64 with the oracle's
    adjacencies."""
    coo, vals, shape, g = prepared[name]
    plain = make_graph(gnntf, coo, vals, shape)
    a, p, seed, first, C = 0.1, 0.5, 5, 3, 16
    assert gnntf.sparse.can_fuse_dropout(g, p) and not gnntf.sparse.can_fuse_dropout(plain, p)
    rng = np.random.default_rng(K)
    H0np, gout = rng.standard_normal((shape[0], C)).astype(np.float32), rng.standard_normal((shape[0], C)).astype(np.float32)
    scales = gnntf.sparse.dropped_degree_scales(g, p, seed, first, K)
    results = []
    for make in (lambda k, bwd=False: gnntf.sparse.dropped_adjacency(g, p, seed, first + k, D=scales[k]),
                 lambda k, bwd=False: gnntf.normalize(plain, "symmetric", "none", p, seed, first + k, transposed_only=bwd)):
        H0 = dev(H0np).requires_grad_()
        out = gnntf.ppr_loop(make, H0, a, K, relu=relu)
        out.backward(dev(gout))
        results.append((out.detach(), H0.grad))
    (fo, fg), (mo, mg) = results
    assert torch.equal(fo, mo) and torch.equal(fg, mg)
    want, want_grad = dense_loop(coo, vals, shape, H0np, gout, K, a, p, seed, first, relu)
    np.testing.assert_allclose(fo.cpu().numpy(), want, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(fg.cpu().numpy(), want_grad, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_degree_scales_of_k_streams_on_prepared_handle(gnntf, prepared, name):
    """gnx_graph_colsum_streams on a prepared handle (one pass over the structure for up to 16 streams) == K gnx_graph_colsum calls,
    bit for bit, and the oracle's keep masks."""
    from gnntf import _native as nat
    coo, vals, shape, g = prepared[name]
    n = shape[1]
    for K in (1, 3, 10, 13, 20):
        got = torch.empty((K, n), device="cuda")
        nat.check(nat.lib().gnx_graph_colsum_streams(g.handle, 0.5, 99, 7, K, nat.ptr(got), nat.current_stream()))
        for k in range(K):
            one = torch.empty(n, device="cuda")
            nat.check(nat.lib().gnx_graph_colsum(g.handle, 0.5, 99, 7 + k, nat.ptr(one), nat.current_stream()))
            assert torch.equal(got[k], one), (name, K, k)
    for k in (0, 12):
        keep = orc.keep_mask(coo, 0.5, 99, 7 + k)
        want = orc.sparse_reduce_sum_axis0(coo, np.where(keep, vals * np.float32(2), np.float32(0)).astype(np.float64), shape)
        np.testing.assert_allclose(got[k].cpu().numpy(), want, rtol=1e-5, atol=1e-5)


def test_c_abi_of_entry_dropout(gnntf):
    """gnx_graph_enable_entry_dropout: GNX_OK with and without duplicates, -1 on NULL; before it the three fused entries refuse a
    handle with duplicates (-4, the message names the call), after it they run."""
    from gnntf import _native as nat
    lib = nat.lib()
    s = nat.current_stream()
    coo, vals, shape = graphs.rmat_symmetric_coo(300, 2000, seed=2)
    single = make_graph(gnntf, coo, vals, shape)
    dup = make_graph(gnntf, np.concatenate([coo, coo]), np.concatenate([vals, vals]), shape)
    n, C = shape[0], 16
    X, out, S = (torch.rand(n, C, device="cuda") for _ in range(3))
    D = torch.rand(n, device="cuda")
    calls = (lambda h: lib.gnx_spmm_dropped(h, nat.ptr(D), 0.5, 1, 1, 0, nat.ptr(X), C, C, None, 0, 1.0, 0.0, 0, nat.ptr(out), C, s),
             lambda h: lib.gnx_spmm_dropped(h, nat.ptr(D), 0.5, 1, 1, 1, nat.ptr(X), C, C, None, 0, 1.0, 0.0, 0, nat.ptr(out), C, s),
             lambda h: lib.gnx_spmm_dropped_chained(h, nat.ptr(D), 0.5, 1, 1, 0, None, nat.ptr(X), C, C, None, 0, 1.0, 0.0, 0, nat.ptr(out),
                                                    C, s),
             lambda h: lib.gnx_spmm_dropped_back(h, nat.ptr(D), 0.5, 1, 1, 0, None, nat.ptr(X), C, C, nat.ptr(S), C, 1.0, 0.5, nat.ptr(S),
                                                 C, 0.9, None, C, 0, s))
    for call in calls:
        assert call(dup.handle) == -4
        err = lib.gnx_last_error()
        assert b"duplicate" in err and b"gnx_graph_enable_entry_dropout" in err
    assert lib.gnx_graph_enable_entry_dropout(None, s) == -1 and b"NULL handle" in lib.gnx_last_error()
    assert lib.gnx_graph_enable_entry_dropout(single.handle, s) == 0
    assert lib.gnx_graph_enable_entry_dropout(dup.handle, s) == 0
    assert lib.gnx_graph_enable_entry_dropout(dup.handle, s) == 0                    # twice: nothing more to do
    for call in calls:
        assert call(dup.handle) == 0, lib.gnx_last_error()
        assert call(single.handle) == 0, lib.gnx_last_error()
    torch.cuda.synchronize()
    # and the numbers: gnx_spmm_dropped on the prepared handle == gnx_graph_normalize(dropout_p) + gnx_spmm / gnx_spmm_tv on the same
    # handle, same seed and stream, with the degree scales of that stream
    nat.check(lib.gnx_graph_colsum(dup.handle, 0.5, 1, 1, nat.ptr(D), s))
    nat.check(lib.gnx_degree_scale(nat.ptr(D), n, nat.NORM["symmetric"], 0, s))
    nnz = dup.nnz
    for transposed, normalize, spmm in ((0, lib.gnx_graph_normalize, lib.gnx_spmm), (1, lib.gnx_graph_normalize_t, lib.gnx_spmm_tv)):
        fused, two = torch.zeros(n, C, device="cuda"), torch.ones(n, C, device="cuda")
        vals_k = torch.empty(nnz, device="cuda")
        nat.check(lib.gnx_spmm_dropped(dup.handle, nat.ptr(D), 0.5, 1, 1, transposed, nat.ptr(X), C, C, nat.ptr(S), C, 0.9, 0.1, 0,
                                       nat.ptr(fused), C, s))
        assert dup.last_kernel().endswith("_drop_entries")
        nat.check(normalize(dup.handle, nat.NORM["symmetric"], nat.EYE["none"], 0.5, 1, 1, nat.ptr(vals_k), None, s))
        nat.check(spmm(dup.handle, nat.ptr(vals_k), None, nat.ptr(X), C, C, nat.ptr(S), C, 0.9, 0.1, 0, nat.ptr(two), C, s))
        assert torch.equal(fused, two) and float(fused.abs().max()) > 0, transposed


def cora_step(gnntf, fuse, activation):
    coo, vals, shape, X = graphs.cora_shaped(seed=1)
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 7, size=shape[0])
    train = np.arange(0, 140)
    gnntf.set_seed(5)
    model = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7, dropout=0.0, activation=activation)
    model.fuse_entry_dropout = fuse
    torch.manual_seed(2)
    model.reset()
    model.dropout = lambda feats, p=0.5: feats                     # no feature dropout: edge dropout is the only randomness
    from gnntf.training import _Objective
    with model:
        loss = _Objective(model, gnntf.NodeClassification(train, labels[train]), 5e-4)()
        loss.backward()
    grads = [v.var.grad.detach().clone() for v in model.vars()]
    return model, loss.detach(), grads


@pytest.mark.parametrize("relu", [False, True])
def test_cora_shaped_appnp_step_with_and_without_entry_dropout(gnntf, relu):
    """The reference's APPNP layer list on the Cora-shaped graph (every entry stored twice): a training step with the fused entry
    dropout against the same step with GNN.fuse_entry_dropout = False (the materialised form): bit for bit, with the identity and
    with relu between the iterations."""
    act = gnntf.relu if relu else gnntf.linear
    fused, loss_f, grads_f = cora_step(gnntf, True, act)
    plain, loss_p, grads_p = cora_step(gnntf, False, act)
    assert fused.graph.entry_dropout and not plain.graph.entry_dropout
    assert fused.graph.nnz_entries == 2 * fused.graph.nnz
    assert torch.equal(loss_f, loss_p)
    for gf, gp in zip(grads_f, grads_p):
        assert torch.equal(gf, gp)
    assert any(float(gf.abs().max()) > 0 for gf in grads_f)


def test_captured_training_on_graph_with_duplicates(gnntf):
    """train(capture=True) on a graph that stores every entry twice: the eager warm-up enables the entry tables before capture, and
    the captured run follows the eager run (same masks; parameters up to the optimizer's float32 rounding)."""
    coo, vals, shape = both_directions(800, 6000, 4)
    rng = np.random.default_rng(4)
    X = rng.standard_normal((800, 20)).astype(np.float32)
    labels = rng.integers(0, 4, size=800)
    train, valid = np.arange(0, 200), np.arange(200, 400)

    def build():
        gnntf.set_seed(11)
        torch.manual_seed(3)
        model = gnntf.GNN(gnntf.SparseCOO(coo, vals, shape), X)
        model.add(gnntf.Dense(16, activation=gnntf.relu))
        H0 = model.add(gnntf.Dense(4, regularize=False))
        for _ in range(4):
            model.add(gnntf.PPRIteration(H0, 0.1, graph_dropout=0.5))
        return model

    results = []
    for capture in (False, True):
        model = build()
        assert not model.graph.entry_dropout
        torch.manual_seed(5)
        model.train(train=gnntf.NodeClassification(train, labels[train]), valid=gnntf.NodeClassification(valid, labels[valid]),
                    epochs=12, patience=50, capture=capture)
        assert model.graph.entry_dropout
        results.append([v.var.detach().cpu().numpy().copy() for v in model.vars()] + [model._mask_calls])
    assert results[0][-1] == results[1][-1] == 12 * 4
    for eager, captured in zip(results[0][:-1], results[1][:-1]):
        np.testing.assert_allclose(captured, eager, rtol=2e-3, atol=2e-5)


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_edge_dropout_with_duplicates_matches_one_gpu(gnntf, world):
    """ShardedGraph(edge_dropout=True) over a COO that stores every entry twice (each rank's COO a row filter of the whole one, so
    the duplicates keep their relative order): forward and dH0 agree with the one-GPU ppr_loop on the whole prepared graph."""
    _sharded_with_duplicates(gnntf, world, "ones")


def test_sharded_edge_dropout_with_unequal_duplicates_matches_one_gpu(gnntf):
    """The same with a value of its own for every stored entry, so every slot's entry list is walked on the vertex blocks (global
    column ids, first-row offset) as well."""
    _sharded_with_duplicates(gnntf, 2, "random")


def _sharded_with_duplicates(gnntf, world, values):
    from gnntf import sharded, sparse
    from thread_comm import run_ranks
    device = torch.device("cuda:0")
    n, C, K, a, p, seed, first = 30000, 16, 4, 0.1, 0.5, 77, 11
    u, w = sharded.rmat_relabelled_pairs(n, 150000, seed=1, device=device)
    idx = torch.cat([torch.stack([u, w], 1), torch.stack([w, u], 1)])
    idx = torch.cat([idx, idx])                                          # graph2adj of a both-direction edge list
    gen = torch.Generator(device=device).manual_seed(2)
    H0 = torch.rand(n, C, device=device, generator=gen) * 2 - 1
    G = torch.rand(n, C, device=device, generator=gen) * 2 - 1
    all_vals = torch.ones(idx.shape[0], device=device)
    if values == "random":
        all_vals = torch.rand(idx.shape[0], device=device, generator=gen) + 0.5
    bounds = sharded.uniform_bounds(n, world)

    def rank_body(comm):
        lo, hi = bounds[comm.rank], bounds[comm.rank + 1]
        rows = (idx[:, 0] >= lo) & (idx[:, 0] < hi)                       # a row filter of the whole COO
        mine = idx[rows]
        sg = sharded.ShardedGraph(mine, all_vals[rows], bounds, comm=comm, edge_dropout=True)
        assert sg.graph.entry_dropout
        scales = sg.dropped_scales(p, seed, first, K)
        out = sg.propagate_dropped(H0[lo:hi], a, K, p, seed, first, scales)
        grad = sg.propagate_dropped_backward(G[lo:hi], a, K, p, seed, first, scales)
        return out, grad

    parts = run_ranks(world, rank_body)
    got, got_grad = torch.cat([q[0] for q in parts]), torch.cat([q[1] for q in parts])
    whole = gnntf.DeviceGraph(gnntf.SparseCOO(idx, all_vals, (n, n)), device=device)
    assert whole.nnz_entries > whole.nnz
    whole.enable_entry_dropout()
    D = sparse.dropped_degree_scales(whole, p, seed, first, K)
    Hf = H0.clone().requires_grad_(True)
    want = sparse.ppr_loop(lambda k, bwd=False: sparse.dropped_adjacency(whole, p, seed, first + k, D=D[k]), Hf, a, K)
    want.backward(G)
    for x, y in ((got, want.detach()), (got_grad, Hf.grad)):
        scale = y.abs().max(dim=1, keepdim=True).values.clamp_min(1e-3)
        assert ((x - y).abs() / scale).max().item() < 1e-4


# ---- edges of the entry tables and of the structure plan ------------------------------------------------------------------------
MULTIPLICITIES = (1, 2, 253, 254, 255, 256, 300)          # 254 equal entries: the last slot the multiplicity byte describes


def multiplicity_graph():
    """64 vertices; one slot each of 1, 2, 253, 254, 255, 256 and 300 equal entries, a slot of 254 entries one of which differs and a
    slot of 256 entries alternating +v / -v (v small: column 9 holds an entry of weight ~1 in every row, so its kept sum stays
    positive), on a background of unique entries; input order shuffled."""
    n = 64
    rng = np.random.default_rng(12)
    back = np.unique(np.concatenate([rng.integers(0, n, size=(500, 2)), np.stack([np.arange(n), np.full(n, 9)], 1)]), axis=0)
    special = [(i, 20 + i) for i in range(len(MULTIPLICITIES))] + [(40, 41), (7, 9)]
    back = back[~np.isin(back[:, 0] * n + back[:, 1], [r * n + c for r, c in special])]
    coo, vals = [back], [(rng.random(len(back)) + 0.5).astype(np.float32)]
    for (r, c), m in zip(special, MULTIPLICITIES):
        coo.append(np.tile([[r, c]], (m, 1))); vals.append(np.full(m, 0.5 + 0.01 * m, dtype=np.float32))
    odd = np.full(254, 0.75, dtype=np.float32); odd[100] = 0.5
    coo.append(np.tile([[40, 41]], (254, 1))); vals.append(odd)
    coo.append(np.tile([[7, 9]], (256, 1))); vals.append(np.float32(1e-3) * np.where(np.arange(256) % 2 == 0, 1, -1).astype(np.float32))
    coo, vals = np.concatenate(coo).astype(np.int64), np.concatenate(vals)
    order = rng.permutation(len(coo))
    return coo[order], vals[order], (n, n)


@pytest.mark.parametrize("p", [0.5, 0.9])
def test_multiplicity_byte_boundary(gnntf, p):
    from gnntf import _native as nat
    from gnntf.sparse import _launch
    coo, vals, shape = multiplicity_graph()
    counts = np.unique(coo, axis=0, return_counts=True)[1]
    assert set(MULTIPLICITIES) <= set(counts.tolist())
    g = make_graph(gnntf, coo, vals, shape)
    g.enable_entry_dropout()
    n = shape[0]
    for C in (8, 40, 100, 256):                                        # one width per dispatch class
        rng = np.random.default_rng(C)
        X, H0 = dev(rng.standard_normal((n, C)).astype(np.float32)), dev(rng.standard_normal((n, C)).astype(np.float32))
        for stream in (3, 4):
            fused = gnntf.sparse.dropped_adjacency(g, p, 8, stream)
            two_pass = gnntf.normalize(g, "symmetric", "none", dropout=p, seed=8, stream_id=stream)
            for transposed in (False, True):
                a = _launch(fused, X, H0, 0.9, 0.1, 0, transposed=transposed)
                assert g.last_kernel().endswith("_drop_entries")
                b = _launch(two_pass, X, H0, 0.9, 0.1, 0, transposed=transposed)
                assert torch.equal(a, b), (C, stream, transposed, float((a - b).abs().max()))
    K = 5
    got = torch.empty((K, n), device="cuda")
    nat.check(nat.lib().gnx_graph_colsum_streams(g.handle, p, 8, 3, K, nat.ptr(got), nat.current_stream()))
    for k in range(K):
        one = torch.empty(n, device="cuda")
        nat.check(nat.lib().gnx_graph_colsum(g.handle, p, 8, 3 + k, nat.ptr(one), nat.current_stream()))
        assert torch.equal(got[k], one), k
        keep = orc.keep_mask(coo, p, 8, 3 + k)
        scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        want = orc.sparse_reduce_sum_axis0(coo, np.where(keep, vals * scale, np.float32(0)).astype(np.float64), shape)
        np.testing.assert_allclose(got[k].cpu().numpy(), want, rtol=1e-5, atol=1e-5)


def stored_twice_with_hubs(n, m, seed):
    """A both-directions graph with hub rows (and columns) above 128 and above 512 slots, a value per slot, every entry stored twice."""
    coo, _, shape = graphs.rmat_symmetric_coo(n, m, seed=seed)
    rng = np.random.default_rng(seed)
    extra = []
    for hub, deg in ((3, 200), (5, 700), (11, 1500)):
        other = rng.choice(np.arange(16, n), size=deg, replace=False)
        extra += [np.stack([np.full(deg, hub), other], 1), np.stack([other, np.full(deg, hub)], 1)]
    coo = np.concatenate([coo] + extra)
    key = np.unique(coo[:, 0] * n + coo[:, 1])
    coo = np.stack([key // n, key % n], 1)
    vals = (np.random.default_rng(seed + 1).random(len(coo)) + 0.5).astype(np.float32)
    return np.concatenate([coo, coo]), np.concatenate([vals, vals]), shape


@pytest.mark.parametrize("n,m", [(40000, 200000), (1 << 20, 2000000)])
def test_size_regimes_of_the_structure_plan(gnntf, n, m):
    """2^15 <= n < 2^20 (rows cut at 128 entries) and n = 2^20 (slot_beg / slot_cnt instead of rowptr): fused == two-pass, bit for bit."""
    from gnntf.sparse import _launch
    coo, vals, shape = stored_twice_with_hubs(n, m, seed=9)
    g = make_graph(gnntf, coo, vals, shape)
    assert g.nnz_entries == 2 * g.nnz
    g.enable_entry_dropout()
    degrees = np.diff(g.csr_arrays()[0].cpu().numpy())
    assert ((degrees > 128) & (degrees <= 512)).any() and (degrees > 512).any()
    names = {8: "spmm_group8_drop_entries", 40: "spmm_group16_drop_entries", 256: "spmm_wave_drop_entries"}
    for C in (8, 40, 256):
        gen = torch.Generator(device="cuda").manual_seed(C)
        X, H0 = (torch.rand(n, C, device="cuda", generator=gen) * 2 - 1 for _ in range(2))
        fused = gnntf.sparse.dropped_adjacency(g, 0.5, 31, 2)
        two_pass = gnntf.normalize(g, "symmetric", "none", dropout=0.5, seed=31, stream_id=2)
        for transposed in (False, True):
            a = _launch(fused, X, H0, 0.9, 0.1, 0, transposed=transposed)
            assert g.last_kernel() == names[C], g.last_kernel()
            b = _launch(two_pass, X, H0, 0.9, 0.1, 0, transposed=transposed)
            assert torch.equal(a, b), (n, C, transposed, float((a - b).abs().max()))
            assert float(a.abs().max()) > 0


@pytest.mark.parametrize("name", ["unequal", "hub"])
@pytest.mark.parametrize("window", [64, 1000])
def test_row_window_on_prepared_handle(gnntf, name, window):
    """gnx_graph_set_row_window before and after enable_entry_dropout(): another launch order, the same bits."""
    from gnntf.sparse import _launch
    coo, vals, shape = GRAPHS[name]()
    n, C = shape[0], 40
    rng = np.random.default_rng(window)
    X, H0 = dev(rng.standard_normal((n, C)).astype(np.float32)), dev(rng.standard_normal((n, C)).astype(np.float32))

    def results(g):
        D = gnntf.sparse.dropped_degree_scales(g, 0.5, 4, 9, 2)
        out = [D]
        for transposed in (False, True):
            out.append(_launch(gnntf.sparse.dropped_adjacency(g, 0.5, 4, 9, D=D[0]), X, H0, 0.9, 0.1, 0, transposed=transposed))
            assert g.last_kernel().endswith("_drop_entries")
        return out

    plain = make_graph(gnntf, coo, vals, shape)
    plain.enable_entry_dropout()
    want = results(plain)
    before = make_graph(gnntf, coo, vals, shape)
    before.set_row_window(window)
    before.enable_entry_dropout()
    after = make_graph(gnntf, coo, vals, shape)
    after.enable_entry_dropout()
    after.set_row_window(window)
    for g in (before, after):
        for x, y in zip(results(g), want):
            assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["unequal", "hub"])
def test_chained_loops_on_prepared_handle(gnntf, prepared, name):
    """gnx_spmm_dropped_chained / gnx_spmm_dropped_back on a handle with duplicates (ppr_loop never takes them there): K = 4 in the
    loop shape ppr_loop uses on graphs without duplicates, against K un-chained gnx_spmm_dropped launches with the fuzz's
    criteria, and against dense float64."""
    import fuzz_kernels as fz
    from gnntf.sparse import _backward_chained, _launch, _launch_chained
    coo, vals, shape, g = prepared[name]
    K, a, p, seed, first, C = 4, 0.1, 0.5, 5, 3, 16
    rng = np.random.default_rng(K)
    H0np, gout = rng.standard_normal((shape[0], C)).astype(np.float32), rng.standard_normal((shape[0], C)).astype(np.float32)
    H0, up = dev(H0np), dev(gout)
    D = gnntf.sparse.dropped_degree_scales(g, p, seed, first, K)
    adjs = [gnntf.sparse.dropped_adjacency(g, p, seed, first + k, D=D[k]) for k in range(K)]
    f_got = f_want = H0
    for k in range(K):
        f_got = _launch_chained(adjs[k], f_got, H0, 1.0 - a, a, prescaled=k > 0, D_next=D[k + 1] if k + 1 < K else None, skip_empty=k + 1 < K)
        assert g.last_kernel().endswith("_drop_entries")
        f_want = _launch(adjs[k], f_want, H0, 1.0 - a, a, 0)
    b_got = _backward_chained(adjs, up, a)
    assert g.last_kernel().endswith("_drop_entries")
    gk, b_want = up, up * a
    for k in range(K - 1, -1, -1):
        gk = _launch(adjs[k], gk, None, 1.0 - a, 0.0, 0, transposed=True)
        b_want = b_want + gk * (a if k >= 1 else 1.0)
    longest = int(np.bincount(coo[:, 0]).max())
    tol = 2e-5 * (1.0 + np.sqrt(longest) / 10.0)
    assert float(fz.rel_rows(f_got, f_want, floor_share=0.0).max()) < tol
    assert float(fz.rel_rows(b_got, b_want).max()) < tol
    want, want_grad = dense_loop(coo, vals, shape, H0np, gout, K, a, p, seed, first, False)
    np.testing.assert_allclose(f_got.cpu().numpy(), want, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(b_got.cpu().numpy(), want_grad, rtol=1e-3, atol=1e-4)
