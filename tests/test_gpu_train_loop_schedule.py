"""The launch schedule of sparse.ppr_loop's chained training loops, pinned against the C entries themselves: the three forward and the
three backward launches of K = 3 iterations are spelled out here as raw library calls -- coefficients, pre-scaling, next scales,
GNX_ACT_SKIP_EMPTY and the gather-order flags per iteration -- and ppr_loop and its backward must give the same bits, in the caller's
order, in the relabelled gather order and with bf16 storage.

Graph: 700 vertices, symmetric, no duplicate entries; 50 vertices are isolated (so GNX_ACT_SKIP_EMPTY matters) and vertex 0 is joined
to each of the other 649 (more than the 512 entries at which a row counts as long).  The "referenced" variant adds one entry that
points at an isolated vertex, so that the rows without entries are no longer gathered by nobody and the library has to ignore the
flag.  700 vertices are below sparse.PAD_MIN_ROWS: the loops run at the width they are given."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, ISOLATED, K, A, P = 700, 50, 3, 0.1, 0.5
SEED, FIRST = 0xC0FFEE, 21
SKIP_EMPTY = 256
ORD_X, ORD_OUT = 1, 2


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def _entries(referenced):
    rng = np.random.default_rng(9)
    live = N - ISOLATED                                            # vertices 0 .. 649 have entries, 650 .. 699 have none
    pairs = {(0, v) for v in range(1, live)}
    while len(pairs) < live - 1 + 2000:
        u, v = (int(x) for x in rng.integers(1, live, size=2))
        if u != v:
            pairs.add((min(u, v), max(u, v)))
    coo = np.array(sorted(pairs | {(v, u) for u, v in pairs}), dtype=np.int64)
    if referenced:
        coo = np.concatenate([coo, np.array([[5, N - 1]], dtype=np.int64)])     # row 5 gathers the isolated vertex 699
    return coo, rng.uniform(0.5, 1.5, size=len(coo)).astype(np.float32)


@pytest.fixture(scope="module")
def prepared(gnntf):
    """Per variant: the handle and the K fused adjacencies (one pass makes all degree scales)."""
    from gnntf import sparse
    out = {}
    for name in ("symmetric", "referenced"):
        coo, vals = _entries(name == "referenced")
        g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, (N, N)), device="cuda:0")
        assert g.nnz_entries == g.nnz == len(coo)
        D = sparse.dropped_degree_scales(g, P, SEED, FIRST, K)
        out[name] = (g, [sparse.DroppedAdjacency(g, P, SEED, FIRST + k, D=D[k]) for k in range(K)])
    return out


def operands(C):
    gen = torch.Generator(device="cuda").manual_seed(100 + C)
    return (torch.randn((N, C), device="cuda", generator=gen), torch.randn((N, C), device="cuda", generator=gen))


def raw_forward(mode, adjs, H0):
    """The three forward launches.  Per iteration: (pre-scaled operand, next scale, act, order flags, bf16 result)."""
    from gnntf import _native as nat
    from gnntf import sparse
    lib, g, C = nat.lib(), adjs[0].graph, H0.shape[1]
    schedule = [(0, adjs[1].D, SKIP_EMPTY, ORD_OUT, 1),
                (1, adjs[2].D, SKIP_EMPTY, ORD_X | ORD_OUT, 1),
                (1, None, 0, ORD_X, 0)]
    X = sparse.to_bf16(H0) if mode == "bf16" else H0
    for adj, (prescaled, D_next, act, order, out_bf16) in zip(adjs, schedule):
        head = (g.handle, nat.ptr(adj.D), P, SEED, adj.stream_id, prescaled, nat.ptr(D_next), nat.ptr(X), C, C, nat.ptr(H0), C, 1.0 - A, A, act)
        if mode == "bf16":
            out = torch.empty((N, C), device="cuda", dtype=torch.bfloat16 if out_bf16 else torch.float32)
            nat.check(lib.gnx_spmm_dropped_chained_bf16(*head, nat.ptr(out), out_bf16, C, nat.current_stream()))
        else:
            out = torch.empty((N, C), device="cuda")
            if mode == "relabelled":
                nat.check(lib.gnx_spmm_dropped_chained_ord(*head, nat.ptr(out), C, order, nat.current_stream()))
            else:
                nat.check(lib.gnx_spmm_dropped_chained(*head, nat.ptr(out), C, nat.current_stream()))
        X = out
    return X


def raw_backward(mode, adjs, G):
    """The three backward launches, iteration 2 first.  Per launch: (adjacency, pre-scaled operand, next scale, running sum in,
    s_alpha, s_beta, a pre-scaled result is written, act, order flags); y_beta = 1 - a throughout."""
    from gnntf import _native as nat
    from gnntf import sparse
    lib, g, C = nat.lib(), adjs[0].graph, G.shape[1]
    S = torch.empty_like(G)
    schedule = [(adjs[2], 0, adjs[1].D, G, A, A * (1.0 - A), True, 0, ORD_OUT),
                (adjs[1], 1, adjs[0].D, S, 1.0, A * (1.0 - A), True, SKIP_EMPTY, ORD_X | ORD_OUT),
                (adjs[0], 1, None, S, 1.0, 1.0 - A, False, SKIP_EMPTY, ORD_X)]
    X = sparse.to_bf16(G) if mode == "bf16" else G
    for adj, prescaled, D_next, S_in, s_alpha, s_beta, has_y, act, order in schedule:
        Y = torch.empty_like(X) if has_y else None
        args = (g.handle, nat.ptr(adj.D), P, SEED, adj.stream_id, prescaled, nat.ptr(D_next), nat.ptr(X), C, C, nat.ptr(S_in), C, s_alpha, s_beta,
                nat.ptr(S), C, 1.0 - A, nat.ptr(Y), C, act)
        if mode == "bf16":
            nat.check(lib.gnx_spmm_dropped_back_bf16(*args, nat.current_stream()))
        elif mode == "relabelled":
            nat.check(lib.gnx_spmm_dropped_back_ord(*args, order, nat.current_stream()))
        else:
            nat.check(lib.gnx_spmm_dropped_back(*args, nat.current_stream()))
        X = Y
    return S


def loop(sparse, make, H0, G, **kw):
    """ppr_loop and its backward; (H_K, dH0, kernel after the forward, kernel after the backward, make_adj calls fwd / bwd)."""
    calls = {False: 0, True: 0}

    def make_adj(k, for_backward=False):
        calls[bool(for_backward)] += 1
        return make(k)
    H0 = H0.clone().requires_grad_(True)
    H = sparse.ppr_loop(make_adj, H0, A, K, **kw)
    fwd = calls[False], calls[True]
    graph = make(0).graph
    after_forward = graph.last_kernel()
    H.backward(G)
    assert fwd == (K, 0) and (calls[False], calls[True]) == (K, K)          # once per iteration forward, once per iteration backward
    return H.detach(), H0.grad, after_forward, graph.last_kernel()


@pytest.mark.parametrize("mode", ["caller", "relabelled", "bf16"])
@pytest.mark.parametrize("C", [8, 40, 132])
@pytest.mark.parametrize("variant", ["symmetric", "referenced"])
def test_loop_is_the_spelled_out_schedule(gnntf, prepared, monkeypatch, variant, C, mode):
    from gnntf import sparse
    monkeypatch.setattr(sparse, "BF16_TRAIN_MIN_ROWS", 0)
    monkeypatch.setattr(sparse, "BF16_TRAIN_MIN_WIDTH", 1)
    g, adjs = prepared[variant]
    H0, G = operands(C)
    want_H, want_dH0 = raw_forward(mode, adjs, H0), raw_backward(mode, adjs, G)
    kw = dict(storage=torch.bfloat16) if mode == "bf16" else dict(gather_order=mode)
    H, dH0, fwd_kernel, bwd_kernel = loop(sparse, lambda k: adjs[k], H0, G, **kw)
    tail = {"caller": "_drop", "relabelled": "_drop_ord", "bf16": "_drop_bf16"}[mode]
    assert fwd_kernel.endswith(tail) and bwd_kernel.endswith(tail), (fwd_kernel, bwd_kernel)
    assert torch.equal(H, want_H)
    assert torch.equal(dH0, want_dH0)
    assert bool(torch.isfinite(H).all()) and bool(torch.isfinite(dH0).all())


def test_relu_and_materialised_adjacencies_go_layer_by_layer(gnntf, prepared, monkeypatch):
    from gnntf import sparse
    monkeypatch.setattr(sparse, "BF16_TRAIN_MIN_ROWS", 0)
    monkeypatch.setattr(sparse, "BF16_TRAIN_MIN_WIDTH", 1)
    g, adjs = prepared["symmetric"]
    H0, G = operands(40)
    asked = dict(storage=torch.bfloat16, gather_order="relabelled")
    materialised = [sparse.normalize(g, "symmetric", "none", P, SEED, FIRST + k) for k in range(K)]
    for make, kw in ((lambda k: adjs[k], dict(relu=True)), (lambda k: materialised[k], {})):
        H, dH0, fwd_kernel, bwd_kernel = loop(sparse, make, H0, G, **kw, **asked)
        assert "bf16" not in fwd_kernel + bwd_kernel and "_ord" not in fwd_kernel + bwd_kernel, (fwd_kernel, bwd_kernel)
        plain = loop(sparse, make, H0, G, **kw)
        assert torch.equal(H, plain[0]) and torch.equal(dH0, plain[1])
