"""The gather order of the fused training loops on the MI355X (gnx_graph_gather_order, gnx_spmm_dropped_chained_ord,
gnx_spmm_dropped_back_ord, sparse.ppr_loop(gather_order="relabelled"), GNN(train_gather_order=...)): the matrix a launch gathers --
and the one it hands to the next launch -- stored in the library's hub-adjacent order, everything else the caller's.  Per row the same
fused multiply-adds on the same values in the same order, so EVERY comparison here is torch.equal on float32 bits against the entries
and the loop of the caller's order."""
import numpy as np
import pytest
import torch

import graphs

pytestmark = pytest.mark.gpu

P, SEED, FIRST, A = 0.5, 0x5EED77, 5, 0.1
WIDTHS = (7, 8, 16, 40, 64, 128, 132)
UNSUPPORTED = -4
KERNELS_SEEN = {}                                   # width -> reported name, filled by the forward cases


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def shared_coo():
    """Symmetric R-MAT of 3 000 vertices / 20 000 drawn entries; vertex 17 gets 900 further neighbours (a hub row and a hub column
    above the long-row threshold of 512); 200 isolated vertices follow (rows without entries).  No duplicate entries."""
    coo, _, _ = graphs.rmat_symmetric_coo(3000, 20000, seed=0)
    n = 3200
    rng = np.random.default_rng(1)
    present = set(coo[coo[:, 0] == 17, 1].tolist()) | {17}
    extra = [v for v in rng.permutation(3000).tolist() if v not in present][:900]
    hub = np.array([[17, v] for v in extra] + [[v, 17] for v in extra], dtype=np.int64)
    coo = np.concatenate([coo, hub])
    assert len(np.unique(coo[:, 0] * n + coo[:, 1])) == len(coo)
    vals = rng.uniform(0.5, 1.5, size=len(coo)).astype(np.float32)            # positive: no column sum cancels
    return coo, vals, (n, n)


@pytest.fixture(scope="module")
def shared(gnntf):
    """The shared graph, its handle, the degree scales of 10 dropout streams and the gather order: made once, never changed."""
    coo, vals, shape = shared_coo()
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    assert g.nnz_entries == g.nnz
    D = gnntf.sparse.dropped_degree_scales(g, P, SEED, FIRST, 10)
    order, rank = g.gather_order()
    degree = np.bincount(coo[:, 0], minlength=shape[0])
    assert degree[17] > 512 and (degree == 0).sum() >= 200
    return dict(g=g, D=D, order=order.long(), rank=rank.long(), n=shape[0], coo=coo, vals=vals, shape=shape)


def test_gather_order_is_a_permutation_with_hubs_first(shared):
    order, rank, n = shared["order"], shared["rank"], shared["n"]
    assert order.shape == rank.shape == (n,)
    assert torch.equal(torch.sort(order).values, torch.arange(n, device="cuda"))
    assert torch.equal(rank[order], torch.arange(n, device="cuda"))
    degree = torch.from_numpy(np.bincount(shared["coo"][:, 0], minlength=n)).cuda()
    assert int(degree[order[0]]) > 512 and int(rank[17]) < 8        # the heaviest bin (the long rows) leads
    assert bool((degree[order][-200:] == 0).all())                  # rows without entries trail


def chained(nat, s, X, H0, k, prescaled, D_next, act, order, fill=7.0):
    """gnx_spmm_dropped_chained (order None) or _ord over stream FIRST + k into a buffer pre-filled with ``fill``."""
    g = s["g"]
    out = torch.full((s["n"], X.shape[1]), fill, dtype=torch.float32, device="cuda")
    head = (g.handle, nat.ptr(s["D"][k]), P, SEED, FIRST + k, int(prescaled), nat.ptr(D_next), nat.ptr(X), X.stride(0), X.shape[1],
            nat.ptr(H0), H0.stride(0), 1.0 - A, A, act, nat.ptr(out), out.stride(0))
    if order is None:
        nat.check(nat.lib().gnx_spmm_dropped_chained(*head, nat.current_stream()))
    else:
        nat.check(nat.lib().gnx_spmm_dropped_chained_ord(*head, order, nat.current_stream()))
    return out


@pytest.mark.parametrize("C", WIDTHS)
def test_single_forward_launches(gnntf, shared, C):
    nat = gnntf.sparse.nat
    s, order, rank = shared, shared["order"], shared["rank"]
    rng = np.random.default_rng(C)
    X, H0 = dev(rng.standard_normal((s["n"], C)).astype(np.float32)), dev(rng.standard_normal((s["n"], C)).astype(np.float32))
    Xo = X.index_select(0, order).contiguous()                      # X stored in gather order
    for prescaled in (0, 1):
        # (the prescaled launches also carry the next iteration's scale and leave rows without entries untouched, as in a loop)
        D_next = s["D"][2] if prescaled else None
        act = nat.ACT_SKIP_EMPTY if prescaled else nat.ACT_NONE
        want = chained(nat, s, X, H0, 1, prescaled, D_next, act, None)
        assert "_ord" not in s["g"].last_kernel()
        assert torch.equal(chained(nat, s, X, H0, 1, prescaled, D_next, act, 0), want)                       # order 0 IS the namesake
        assert not s["g"].last_kernel().endswith("_ord")
        got = chained(nat, s, Xo, H0, 1, prescaled, D_next, act, nat.ORD_X)
        assert s["g"].last_kernel().endswith("_ord"), s["g"].last_kernel()
        KERNELS_SEEN[C] = s["g"].last_kernel()
        assert torch.equal(got, want)
        got = chained(nat, s, X, H0, 1, prescaled, D_next, act, nat.ORD_OUT)
        assert s["g"].last_kernel().endswith("_ord")
        assert torch.equal(got.index_select(0, rank), want)                                                   # un-permuted: out[rank[row]] = row
        got = chained(nat, s, Xo, H0, 1, prescaled, D_next, act, nat.ORD_X | nat.ORD_OUT)
        assert torch.equal(got.index_select(0, rank), want)
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0


def test_every_dispatch_class_occurred(gnntf, shared):
    """Over the widths the sub-wave groups, one wave per row and the long-row chunk launches all ran under the gather order."""
    nat = gnntf.sparse.nat
    for C in WIDTHS:                                                # (also when this test runs on its own)
        if C not in KERNELS_SEEN:
            X = torch.ones((shared["n"], C), device="cuda")
            chained(nat, shared, X, X.clone(), 0, 0, None, nat.ACT_NONE, nat.ORD_X)
            KERNELS_SEEN[C] = shared["g"].last_kernel()
    names = set(KERNELS_SEEN.values())
    assert all(name.startswith("spmm_") and name.endswith("_drop_ord") for name in names), names
    assert {"spmm_group8+long_drop_ord", "spmm_group16+long_drop_ord", "spmm_group32+long_drop_ord", "spmm_wave+long_drop_ord"} <= names, names
    assert any("group" in name for name in names) and any("wave" in name for name in names) and all("+long" in name for name in names)


def back(nat, s, X, k, prescaled, D_next, S_in, S_out, Y_out, act, order):
    C = X.shape[1]
    head = (s["g"].handle, nat.ptr(s["D"][k]), P, SEED, FIRST + k, int(prescaled), nat.ptr(D_next), nat.ptr(X), C, C, nat.ptr(S_in), C,
            1.0, A * (1.0 - A), nat.ptr(S_out), C, 1.0 - A, nat.ptr(Y_out), C, act)
    if order is None:
        nat.check(nat.lib().gnx_spmm_dropped_back(*head, nat.current_stream()))
    else:
        nat.check(nat.lib().gnx_spmm_dropped_back_ord(*head, order, nat.current_stream()))


@pytest.mark.parametrize("C", WIDTHS)
def test_single_backward_launches(gnntf, shared, C):
    nat = gnntf.sparse.nat
    s, order, rank = shared, shared["order"], shared["rank"]
    rng = np.random.default_rng(100 + C)
    X, S0 = dev(rng.standard_normal((s["n"], C)).astype(np.float32)), dev(rng.standard_normal((s["n"], C)).astype(np.float32))
    Xo = X.index_select(0, order).contiguous()

    def run(order_flags, in_place, prescaled):
        """(S_out, Y_out); in place = GNX_ACT_SKIP_EMPTY with S_in == S_out, as every call but the first of a loop."""
        S_in = S0.clone()
        S_out = S_in if in_place else torch.full_like(S0, 7.0)
        Y = torch.full_like(S0, 7.0)
        Xin = Xo if order_flags is not None and order_flags & nat.ORD_X else X
        back(nat, s, Xin, 2, prescaled, s["D"][1], S_in, S_out, Y, nat.ACT_SKIP_EMPTY if in_place else nat.ACT_NONE, order_flags)
        if order_flags is not None and order_flags & nat.ORD_OUT:
            Y = Y.index_select(0, rank)                             # Y_out was written in gather order; S_out never is
        return S_out, Y

    for in_place, prescaled in ((False, 0), (True, 1)):
        want_S, want_Y = run(None, in_place, prescaled)
        assert not s["g"].last_kernel().endswith("_ord")
        for flags in (0, nat.ORD_X, nat.ORD_OUT, nat.ORD_X | nat.ORD_OUT):
            got_S, got_Y = run(flags, in_place, prescaled)
            assert s["g"].last_kernel().endswith("_ord") == (flags != 0), (flags, s["g"].last_kernel())
            assert torch.equal(got_S, want_S), (flags, in_place)
            assert torch.equal(got_Y, want_Y), (flags, in_place)
    # the last call of a loop has no second result
    S_a, S_b = torch.empty_like(S0), torch.empty_like(S0)
    back(nat, s, X, 0, 1, None, S0, S_a, None, nat.ACT_NONE, None)
    back(nat, s, Xo, 0, 1, None, S0, S_b, None, nat.ACT_NONE, nat.ORD_X)
    assert torch.equal(S_a, S_b) and torch.isfinite(S_a).all() and float((S_a - S0).abs().max()) > 0


def loop_and_gradient(gnntf, g, H0_host, K, gather_order, upstream, relu=False, storage=torch.float32, seed=SEED, first=FIRST, p=P):
    """(H_K, dH0) of sparse.ppr_loop over the fused adjacencies of K dropout streams."""
    sparse = gnntf.sparse
    scales = sparse.dropped_degree_scales(g, p, seed, first, K)
    make_adj = lambda k, bwd=False: sparse.dropped_adjacency(g, p, seed, first + k, D=scales[k])
    H0 = H0_host.clone().requires_grad_(True)
    out = sparse.ppr_loop(make_adj, H0, A, K, relu=relu, storage=storage, gather_order=gather_order)
    out.backward(upstream)
    return out.detach(), H0.grad.detach()


@pytest.mark.parametrize("K", (3, 10))
@pytest.mark.parametrize("C", (7, 40, 64))
def test_loop_returns_the_bits_of_the_callers_order(gnntf, shared, C, K):
    rng = np.random.default_rng(1000 * K + C)
    H0 = dev(rng.standard_normal((shared["n"], C)).astype(np.float32))
    G = dev(rng.standard_normal((shared["n"], C)).astype(np.float32))
    want = loop_and_gradient(gnntf, shared["g"], H0, K, "caller", G)
    assert not shared["g"].last_kernel().endswith("_ord")
    got = loop_and_gradient(gnntf, shared["g"], H0, K, "relabelled", G)
    assert shared["g"].last_kernel().endswith("_ord")              # the backward's last launch
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.isfinite(want[0]).all() and float(want[1].abs().max()) > 0


def test_appnp_training_step(gnntf, shared):
    """One training step of APPNP(train_gather_order="relabelled"): the loss and every parameter gradient are the bits of "caller"."""
    from gnntf.training import _Objective
    n = shared["n"]
    rng = np.random.default_rng(9)
    X = rng.standard_normal((n, 24)).astype(np.float32)
    labels = rng.integers(0, 7, size=n)
    train = np.arange(0, 400)
    results = {}
    for mode in ("caller", "relabelled"):
        gnntf.set_seed(21)
        torch.manual_seed(21)
        model = gnntf.APPNP(gnntf.SparseCOO(shared["coo"], shared["vals"], shared["shape"]), X, num_classes=7, latent_dims=[16],
                            train_gather_order=mode)
        torch.manual_seed(22)
        model.reset()
        torch.manual_seed(23)                                       # the feature-dropout masks of the step
        with model:
            loss = _Objective(model, gnntf.NodeClassification(train, labels[train]), 5e-4)()
            loss.backward()
        results[mode] = [loss.detach()] + [v.var.grad.detach().clone() for v in model.vars() if v.trainable]
        assert model.graph.last_kernel().endswith("_ord") == (mode == "relabelled"), model.graph.last_kernel()
    assert len(results["caller"]) >= 5
    for a, b in zip(results["caller"], results["relabelled"]):
        assert torch.equal(a, b)
    assert all(float(t.abs().max()) > 0 for t in results["caller"])


def test_large_structure_takes_the_separate_long_row_kernels(gnntf):
    """2^20 + 3 vertices / 4M drawn entries at C = 8: the plan of a big structure (rows cut at 512 entries, slot ranges in slot
    order, chunk launches of their own), forward and dH0 of a K = 3 loop bitwise."""
    n = (1 << 20) + 3
    coo, vals, shape = graphs.rmat_symmetric_coo(n, 4_000_000, seed=2)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    gen = torch.Generator(device="cuda").manual_seed(5)
    H0 = torch.randn((n, 8), device="cuda", generator=gen)
    G = torch.randn((n, 8), device="cuda", generator=gen)
    want = loop_and_gradient(gnntf, g, H0, 3, "caller", G)
    got = loop_and_gradient(gnntf, g, H0, 3, "relabelled", G)
    assert g.last_kernel() == "spmm_group8+long_drop_ord", g.last_kernel()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.isfinite(want[0]).all() and float(want[1].abs().max()) > 0


def test_refusals(gnntf, shared):
    """A handle with duplicate entries, a handle with a row window and a vertex block: GNX_ERR_UNSUPPORTED and a message saying which."""
    nat = gnntf.sparse.nat
    lib = nat.lib()
    coo, vals, shape = graphs.rmat_symmetric_coo(500, 3000, seed=6)
    n = shape[0]
    X, H0 = torch.ones((n, 8), device="cuda"), torch.ones((n, 8), device="cuda")
    out, Y = torch.empty_like(X), torch.empty_like(X)
    D = torch.ones(n, device="cuda")

    def both_entries(g):
        codes = []
        for order in (nat.ORD_X, nat.ORD_OUT, nat.ORD_X | nat.ORD_OUT):
            codes.append((lib.gnx_spmm_dropped_chained_ord(g.handle, nat.ptr(D), P, SEED, 0, 0, None, nat.ptr(X), 8, 8, nat.ptr(H0), 8, 0.9, 0.1, 0,
                                                           nat.ptr(out), 8, order, nat.current_stream()), lib.gnx_last_error().decode()))
            codes.append((lib.gnx_spmm_dropped_back_ord(g.handle, nat.ptr(D), P, SEED, 0, 0, None, nat.ptr(X), 8, 8, nat.ptr(H0), 8, 1.0, 0.9,
                                                        nat.ptr(out), 8, 0.9, nat.ptr(Y), 8, 0, order, nat.current_stream()),
                          lib.gnx_last_error().decode()))
        return codes

    doubled = gnntf.DeviceGraph(gnntf.SparseCOO(np.concatenate([coo, coo[:50]]), np.concatenate([vals, vals[:50]]), shape), device="cuda:0")
    doubled.enable_entry_dropout()
    for code, message in both_entries(doubled):
        assert code == UNSUPPORTED and "duplicate" in message, (code, message)
    with pytest.raises(Exception, match="duplicate"):
        doubled.reserve(8, train_gather=True)

    windowed = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    windowed.reserve(8, train_gather=True)                           # built ... and dropped again by the window
    windowed.set_row_window(128)
    for code, message in both_entries(windowed):
        assert code == UNSUPPORTED and "row window" in message, (code, message)
    assert lib.gnx_graph_gather_order(windowed.handle, None, None) == UNSUPPORTED
    windowed.set_row_window(0)                                       # back to the default order: the entries work again
    assert all(code == 0 for code, _ in both_entries(windowed))

    block = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    gid = torch.arange(n, dtype=torch.int32, device="cuda")
    nat.check(lib.gnx_graph_set_block(block.handle, 0, 0, nat.ptr(gid), nat.current_stream()))
    for code, message in both_entries(block):
        assert code == UNSUPPORTED and "vertex block" in message, (code, message)
    torch.cuda.synchronize()


def test_capture_needs_a_reserve_and_replays_bitwise(gnntf, shared):
    """Under capture without a prior reserve: GNX_ERR_UNSUPPORTED naming gnx_graph_reserve.  After reserve(train_gather=True) a
    captured and replayed training step (forward loop + backward loop) equals the eager step bitwise."""
    sparse = gnntf.sparse
    coo, vals, shape = shared["coo"], shared["vals"], shared["shape"]
    n, C, K = shape[0], 16, 4
    rng = np.random.default_rng(3)
    H0 = dev(rng.standard_normal((n, C)).astype(np.float32))
    G = dev(rng.standard_normal((n, C)).astype(np.float32))
    fresh = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    scales = sparse.dropped_degree_scales(fresh, P, SEED, FIRST, K)
    adjs = [sparse.dropped_adjacency(fresh, P, SEED, FIRST + k, D=scales[k]) for k in range(K)]
    want = loop_and_gradient(gnntf, shared["g"], H0, K, "caller", G)
    torch.cuda.synchronize()
    with pytest.raises(Exception, match="gnx_graph_reserve"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            sparse._launch_chained(adjs[0], H0, H0, 1.0 - A, A, False, scales[1], order=sparse.nat.ORD_OUT)
    torch.cuda.synchronize()
    fresh.reserve(C, train_gather=True)
    make_adj = lambda k, bwd=False: adjs[k]
    side = torch.cuda.Stream()                                      # autograd's own lazy set-up, outside the capture
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = H0.clone().requires_grad_(True)
        torch.autograd.grad(sparse.ppr_loop(make_adj, warm, A, K, gather_order="relabelled"), warm, G)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    recorded = torch.cuda.CUDAGraph()
    H0_in = torch.zeros_like(H0).requires_grad_(True)
    with torch.cuda.graph(recorded):
        out = sparse.ppr_loop(make_adj, H0_in, A, K, gather_order="relabelled")
        (grad,) = torch.autograd.grad(out, H0_in, G)
    with torch.no_grad():
        H0_in.copy_(H0)                                             # replays read the buffers as they are NOW
    recorded.replay()
    torch.cuda.synchronize()
    assert fresh.last_kernel().endswith("_ord")
    assert torch.equal(out.detach(), want[0]) and torch.equal(grad, want[1])


def test_modes_where_the_chained_f32_loop_does_not_apply(gnntf, shared, monkeypatch):
    """relu, bf16 training storage and a duplicate-entry graph: "relabelled" took today's path -- the bits of "caller", no _ord launch."""
    sparse = gnntf.sparse
    n, C, K = shared["n"], 40, 3
    rng = np.random.default_rng(8)
    H0 = dev(rng.standard_normal((n, C)).astype(np.float32))
    G = dev(rng.standard_normal((n, C)).astype(np.float32))
    monkeypatch.setattr(sparse, "BF16_TRAIN_MIN_WIDTH", 1)           # let the bf16 loops run on this small graph
    monkeypatch.setattr(sparse, "BF16_TRAIN_MIN_ROWS", 1)
    doubled_coo, doubled_vals = np.concatenate([shared["coo"], shared["coo"]]), np.concatenate([shared["vals"], shared["vals"]])
    doubled = gnntf.DeviceGraph(gnntf.SparseCOO(doubled_coo, doubled_vals, shared["shape"]), device="cuda:0")
    doubled.enable_entry_dropout()
    for g, kwargs in ((shared["g"], dict(relu=True)), (shared["g"], dict(storage=torch.bfloat16)), (doubled, dict())):
        want = loop_and_gradient(gnntf, g, H0, K, "caller", G, **kwargs)
        got = loop_and_gradient(gnntf, g, H0, K, "relabelled", G, **kwargs)
        assert not g.last_kernel().endswith("_ord"), (kwargs, g.last_kernel())
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), kwargs
    # and "auto" outside the allowance is "caller": no _ord launch on this 3 200-vertex graph
    auto = loop_and_gradient(gnntf, shared["g"], H0, K, "auto", G)
    assert not shared["g"].last_kernel().endswith("_ord")
    want = loop_and_gradient(gnntf, shared["g"], H0, K, "caller", G)
    assert torch.equal(auto[0], want[0]) and torch.equal(auto[1], want[1])
