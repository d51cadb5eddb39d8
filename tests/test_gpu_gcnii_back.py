"""The fused backward of the GCNII layer on the MI355X (gnx_gcnii_step_back, sparse.gcnii_step_back, gcnii_step(backward="fused"),
GCNII(gcnii_backward="fused")): with G the gated upstream gradient and Mt = M^T,
    dH = ((1-a) A^T G) . Mt        S = s_alpha S_in + (a G) . Mt
against float64 algebra over the oracle's adjacency, the edge shapes, reproducibility, the composed order of the other widths bit for
bit, and the autograd / model paths against today's composed backward."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import gnntf_oracle as orc

pytestmark = pytest.mark.gpu

A_MIX = 0.1
N, HUB, N_HUB = 3000, 1500, 900
WIDTHS = (16, 32, 64, 40, 7)
FUSED, FALLBACK = "spmm_gcnii_back_mfma", "dense+spmm_back"


def kernel_for(C):
    return FUSED if C in (16, 32, 64) else FALLBACK


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def directed_coo():
    """A DIRECTED graph of 3 000 vertices and about 20 000 entries, asymmetric pattern and values, no duplicates: sources are drawn
    below 2 900 and targets from 100 up, so vertices 0 .. 99 have no in-edges (empty rows of the transposed structure) and vertices
    2 900 .. 2 999 no out-edges; column 1 500 holds 900 entries (a hub ROW of the transposed structure, above its threshold of 512)."""
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
    """The graph of the parity tests, its handle, its normalised adjacency and the same adjacency in float64: made once, never changed."""
    coo, vals, shape = directed_coo()
    in_deg, out_deg = np.bincount(coo[:, 1], minlength=N), np.bincount(coo[:, 0], minlength=N)
    assert in_deg[HUB] >= N_HUB and (in_deg == 0).sum() >= 100 and (out_deg == 0).sum() >= 100 and 19000 < len(coo) < 21000
    forward = set(map(tuple, coo.tolist()))
    assert sum((c, r) in forward for r, c in forward) < len(coo) // 10                 # the pattern is not symmetric
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    adj = gnntf.normalize(g, "symmetric")
    ai, av = orc.get_adjacency(coo, vals, shape, dtype=np.float64)
    A = sp.csr_matrix((av, (ai[:, 0], ai[:, 1])), shape=shape)
    return dict(g=g, adj=adj, A=A, no_in=np.flatnonzero(in_deg == 0), coo=coo, vals=vals, shape=shape)


def operands(n, C, seed):
    rng = np.random.default_rng(seed)
    G, S_in = rng.standard_normal((n, C)).astype(np.float32), rng.standard_normal((n, C)).astype(np.float32)
    Mt = (0.6 * np.eye(C) + 0.4 * rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
    return G, Mt, S_in


def check_against_float64(A, G, Mt, S_in, s_alpha, dH, S):
    """The tolerances test_gcnii_step_fused uses for the same quantities: dH rtol 1e-3 / atol 1e-3, S (dH0) rtol 1e-3 / atol 1e-4."""
    G64, Mt64 = G.astype(np.float64), Mt.astype(np.float64)
    want_dH = (1 - A_MIX) * (A.T @ G64) @ Mt64
    want_S = A_MIX * G64 @ Mt64 + (0 if S_in is None else s_alpha * S_in.astype(np.float64))
    np.testing.assert_allclose(dH.cpu().numpy(), want_dH, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(S.cpu().numpy(), want_S, rtol=1e-3, atol=1e-4)


# ---- 1. parity against float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s_alpha", [1.0, 0.5])
@pytest.mark.parametrize("C", WIDTHS)
def test_matches_float64(gnntf, shared, C, s_alpha):
    G, Mt, S_in = operands(N, C, seed=C)
    dH, S = gnntf.gcnii_step_back(shared["adj"], dev(G), A_MIX, dev(Mt), S_in=dev(S_in), s_alpha=s_alpha)
    assert shared["g"].last_kernel() == kernel_for(C)
    check_against_float64(shared["A"], G, Mt, S_in, s_alpha, dH, S)
    assert bool((dH[dev(shared["no_in"])] == 0).all())             # rows without in-edges: dH = 0, written
    # walking A instead of A^T would not pass: the two differ by far more than the tolerance
    wrong = (1 - A_MIX) * (shared["A"] @ G.astype(np.float64)) @ Mt.astype(np.float64)
    assert np.abs(dH.cpu().numpy() - wrong).max() > 0.1


# ---- 2. small and edge shapes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 16, 17])
def test_small_graphs(gnntf, n):
    rng = np.random.default_rng(n)
    key = np.unique(rng.integers(0, n, size=3 * n) * n + rng.integers(0, n, size=3 * n))
    coo = np.stack([key // n, key % n], axis=1).astype(np.int64)
    vals = rng.uniform(0.5, 1.5, size=len(coo)).astype(np.float32)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, (n, n)), device="cuda:0")
    adj = gnntf.normalize(g, "symmetric")
    ai, av = orc.get_adjacency(coo, vals, (n, n), dtype=np.float64)
    A = sp.csr_matrix((av, (ai[:, 0], ai[:, 1])), shape=(n, n))
    for C in WIDTHS:
        G, Mt, S_in = operands(n, C, seed=100 + C)
        dH, S = gnntf.gcnii_step_back(adj, dev(G), A_MIX, dev(Mt), S_in=dev(S_in), s_alpha=0.5)
        assert g.last_kernel() == kernel_for(C)
        check_against_float64(A, G, Mt, S_in, 0.5, dH, S)


@pytest.mark.parametrize("C", [16, 64, 40])
def test_graph_without_entries(gnntf, C):
    n = 37
    g = gnntf.DeviceGraph(gnntf.SparseCOO(np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.float32), (n, n)), device="cuda:0")
    adj = gnntf.Adjacency(g)
    G, Mt, S_in = operands(n, C, seed=C)
    dH, S = gnntf.gcnii_step_back(adj, dev(G), A_MIX, dev(Mt), S_in=dev(S_in), s_alpha=1.0)
    assert bool((dH == 0).all())
    check_against_float64(sp.csr_matrix((n, n)), G, Mt, S_in, 1.0, dH, S)


@pytest.mark.parametrize("C", [16, 32, 64, 40])
def test_optional_running_sum(gnntf, shared, C):
    """S_in=None drops the s_alpha term; want_S=False returns no S and the same dH bits; S_in aliased with S_out through the C
    binding gives the bits of the out-of-place call."""
    nat = gnntf.sparse.nat
    adj, g = shared["adj"], shared["g"]
    G, Mt, S_in = operands(N, C, seed=7 * C)
    Gd, Mtd = dev(G), dev(Mt)
    dH, S = gnntf.gcnii_step_back(adj, Gd, A_MIX, Mtd)
    check_against_float64(shared["A"], G, Mt, None, 1.0, dH, S)
    dH_only, none = gnntf.gcnii_step_back(adj, Gd, A_MIX, Mtd, want_S=False)
    assert none is None and torch.equal(dH_only, dH)
    dH2, S2 = gnntf.gcnii_step_back(adj, Gd, A_MIX, Mtd, S_in=dev(S_in), s_alpha=0.5)
    assert torch.equal(dH2, dH)
    running, dH3 = dev(S_in), torch.empty_like(Gd)
    work = torch.empty_like(Gd) if C == 40 else None
    nat.check(nat.lib().gnx_gcnii_step_back(g.handle, nat.ptr(adj.transposed_values()), nat.ptr(Gd), A_MIX, C, nat.ptr(Mtd), C,
                                            nat.ptr(dH3), nat.ptr(running), 0.5, nat.ptr(running), nat.ptr(work), nat.current_stream()))
    assert torch.equal(running, S2) and torch.equal(dH3, dH)
    if C == 40:                                                     # the other widths need d_work, and say so
        rc = nat.lib().gnx_gcnii_step_back(g.handle, nat.ptr(adj.transposed_values()), nat.ptr(Gd), A_MIX, C, nat.ptr(Mtd), C,
                                           nat.ptr(dH3), None, 1.0, None, None, nat.current_stream())
        assert rc == -1 and b"d_work" in nat.lib().gnx_last_error()


def test_python_wrapper_refuses_what_the_step_refuses(gnntf, shared):
    sparse = gnntf.sparse
    G, Mt, _ = operands(N, 16, seed=1)
    with pytest.raises(Exception, match="shape mismatch"):
        gnntf.gcnii_step_back(shared["adj"], dev(G[:-1]), A_MIX, dev(Mt))
    with pytest.raises(Exception, match="shape mismatch"):
        gnntf.gcnii_step_back(shared["adj"], dev(G), A_MIX, dev(Mt[:, :8]))
    with pytest.raises(Exception, match="add_eye"):
        gnntf.gcnii_step_back(gnntf.normalize(shared["g"], "symmetric", "after"), dev(G), A_MIX, dev(Mt))
    dropped = sparse.DroppedAdjacency(shared["g"], 0.5, 1, 0, D=torch.ones(N, device="cuda"))
    with pytest.raises(Exception, match="DroppedAdjacency"):
        gnntf.gcnii_step_back(dropped, dev(G), A_MIX, dev(Mt))
    wide = gnntf.DeviceGraph(gnntf.SparseCOO(np.array([[0, 1]], dtype=np.int64), np.ones(1, dtype=np.float32), (N, N + 1)), device="cuda:0")
    with pytest.raises(Exception, match="shape mismatch"):
        gnntf.gcnii_step_back(gnntf.Adjacency(wide), dev(G), A_MIX, dev(Mt))


# ---- 3. reproducibility ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 64, 40])
def test_two_calls_give_the_same_bits(gnntf, shared, C):
    G, Mt, S_in = operands(N, C, seed=3 * C)
    first = gnntf.gcnii_step_back(shared["adj"], dev(G), A_MIX, dev(Mt), S_in=dev(S_in), s_alpha=0.5)
    second = gnntf.gcnii_step_back(shared["adj"], dev(G), A_MIX, dev(Mt), S_in=dev(S_in), s_alpha=0.5)
    assert shared["g"].last_kernel() == kernel_for(C)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


# ---- 4. the other widths keep today's order ------------------------------------------------------------------------------------
def test_fallback_is_dense_then_transposed_spmm_bitwise(gnntf, shared):
    sparse = gnntf.sparse
    G, Mt, _ = operands(N, 40, seed=40)
    Gd, Mtd = dev(G), dev(Mt)
    dH, S = gnntf.gcnii_step_back(shared["adj"], Gd, A_MIX, Mtd)
    assert shared["g"].last_kernel() == FALLBACK
    with torch.no_grad():
        gT = gnntf.dense(Gd, Mtd)
    want = sparse._launch(shared["adj"], gT, None, 1.0 - A_MIX, 0.0, sparse.nat.ACT_NONE, transposed=True)   # _GCNIIStep.backward's call
    assert torch.equal(dH, want)
    np.testing.assert_allclose(S.cpu().numpy(), (gT * A_MIX).cpu().numpy(), rtol=1e-6, atol=1e-7)


# ---- 5. fused against composed through autograd ----------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C", [16, 64, 40])
def test_autograd_fused_against_composed(gnntf, shared, C, relu):
    rng = np.random.default_rng(C + int(relu))
    H, H0 = rng.standard_normal((N, C)).astype(np.float32), rng.standard_normal((N, C)).astype(np.float32)
    M = (0.6 * np.eye(C) + 0.4 * rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
    up = dev(rng.standard_normal((N, C)).astype(np.float32))

    def run(**option):
        leaves = [dev(x).requires_grad_() for x in (H, H0, M)]
        out = gnntf.gcnii_step(shared["adj"], *leaves[:2], A_MIX, leaves[2], relu=relu, **option)
        out.backward(up)
        return [out.detach()] + [leaf.grad for leaf in leaves], shared["g"].last_kernel()

    (out_f, gH_f, gH0_f, gM_f), kernel = run(backward="fused")
    assert kernel == kernel_for(C)
    (out_c, gH_c, gH0_c, gM_c), _ = run(backward="composed")
    (out_d, gH_d, gH0_d, gM_d), _ = run()
    assert torch.equal(out_f, out_c) and torch.equal(gM_f, gM_c)     # the same forward launch, the same gnx_dense_wgrad call
    for fused, composed in ((gH_f, gH_c), (gH0_f, gH0_c)):
        np.testing.assert_allclose(fused.cpu().numpy(), composed.cpu().numpy(), rtol=1e-4, atol=1e-3)
    for default, composed in ((out_d, out_c), (gH_d, gH_c), (gH0_d, gH0_c), (gM_d, gM_c)):
        assert torch.equal(default, composed)                       # no keyword = "composed", bit for bit
    # each gradient is requested only where autograd asks for it
    Hg = dev(H).requires_grad_()
    gnntf.gcnii_step(shared["adj"], Hg, dev(H0), A_MIX, dev(M), relu=relu, backward="fused").backward(up)
    assert torch.equal(Hg.grad, gH_f)
    H0g = dev(H0).requires_grad_()
    gnntf.gcnii_step(shared["adj"], dev(H), H0g, A_MIX, dev(M), relu=relu, backward="fused").backward(up)
    assert torch.equal(H0g.grad, gH0_f)


# ---- 6. the model ----------------------------------------------------------------------------------------------------------------
def test_model_gradients_fused_against_composed(gnntf):
    n = 300
    rng = np.random.default_rng(6)
    key = np.unique(rng.integers(0, n, size=1500) * n + rng.integers(0, n, size=1500))
    coo = np.stack([key // n, key % n], axis=1).astype(np.int64)
    vals = np.ones(len(coo), dtype=np.float32)
    X = rng.standard_normal((n, 20)).astype(np.float32)
    nodes, labels = np.arange(0, n, 3), rng.integers(0, 5, size=len(np.arange(0, n, 3)))
    weights = [(rng.standard_normal((16, 16)) / 4).astype(np.float32) for _ in range(4)]

    def gradients(**option):
        gnntf.set_seed(3)
        torch.manual_seed(3)
        model = gnntf.GCNII(gnntf.SparseCOO(coo, vals, (n, n)), X, 5, latent_dims=[16], iterations=4, dropout=0, **option)
        model.reset()
        convs = [l for l in model.layers() if isinstance(l, gnntf.GCNIILayer)]
        assert len(convs) == 4
        for layer, W in zip(convs, weights):                        # the reference initialises W to zero: use seeded weights
            layer.W.data.copy_(dev(W))
        with model:
            loss = gnntf.node_ce(model(model.features), nodes, labels)
            loss.backward()
        return [v.var.detach().clone() for v in model.vars()], [v.var.grad for v in model.vars()], model.graph.last_kernel()

    params_f, grads_f, kernel = gradients(gcnii_backward="fused")
    assert kernel == FUSED
    params_c, grads_c, _ = gradients()
    assert len(grads_f) == len(grads_c) > 4
    for a_, b_ in zip(params_f, params_c):
        assert torch.equal(a_, b_)                                  # identical parameters
    for fused, composed in zip(grads_f, grads_c):
        assert fused is not None and composed is not None
        np.testing.assert_allclose(fused.cpu().numpy(), composed.cpu().numpy(), rtol=1e-3, atol=1e-4)


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 40])
def test_capture_needs_a_reserve_and_replays_bitwise(gnntf, shared, C):
    G, Mt, S_in = operands(N, C, seed=9 * C)
    Gd, Mtd, Sd = dev(G), dev(Mt), dev(S_in)
    want = gnntf.gcnii_step_back(shared["adj"], Gd, A_MIX, Mtd, S_in=Sd, s_alpha=0.5)
    fresh = gnntf.DeviceGraph(gnntf.SparseCOO(shared["coo"], shared["vals"], shared["shape"]), device="cuda:0")
    adj = gnntf.Adjacency(fresh, shared["adj"].vals, None, vals_t=shared["adj"].transposed_values())
    torch.cuda.synchronize()
    with pytest.raises(Exception, match="gnx_graph_reserve"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            gnntf.gcnii_step_back(adj, Gd, A_MIX, Mtd, S_in=Sd, s_alpha=0.5)
    torch.cuda.synchronize()
    fresh.reserve(C, transposed=True)
    G_in = torch.zeros_like(Gd)
    recorded = torch.cuda.CUDAGraph()
    with torch.cuda.graph(recorded):
        dH, S = gnntf.gcnii_step_back(adj, G_in, A_MIX, Mtd, S_in=Sd, s_alpha=0.5)
    G_in.copy_(Gd)                                                  # replays read the buffers as they are NOW
    recorded.replay()
    torch.cuda.synchronize()
    assert fresh.last_kernel() == kernel_for(C)
    assert torch.equal(dH, want[0]) and torch.equal(S, want[1])
