"""Opt-in bf16 feature storage on the MI355X: gnx_cast_bf16, gnx_spmm_bf16 (f32 and bf16 results), gnx_appnp_propagate_bf16
against float64 emulations (tests/bf16_ref.py) and against the f32 loop through the first-order error bound, dispatch of every
kernel class, determinism, and the model-level inference_dtype switch (eval forwards only; training bit for bit unchanged)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import graphs
from bf16_ref import U, appnp_bf16, bf16_bits, bf16_decode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    return gnntf


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def hub_graph(n_rows, n_cols, seed, hubs=(700, 1300, 2600), empty_share=0.2, symmetric=False):
    """Random entries (weights 0.25 .. 1.25), a share of rows without entries, and hub rows longer than every long-row threshold."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_rows, size=6 * n_rows)
    keep = rng.random(n_rows) >= empty_share
    rows = rows[keep[rows]]
    cols = rng.integers(0, n_cols, size=len(rows))
    hub_r = np.concatenate([np.full(h, i % n_rows, dtype=np.int64) for i, h in enumerate(hubs)])
    hub_c = np.concatenate([rng.choice(n_cols, size=min(h, n_cols), replace=False) for h in hubs])
    r, c = np.concatenate([rows, hub_r]), np.concatenate([cols, hub_c])
    if symmetric:
        r, c = np.concatenate([r, c]), np.concatenate([c, r])
        key = np.unique(r * n_cols + c)
        r, c = key // n_cols, key % n_cols
        vals = np.ones(len(r), dtype=np.float32)
    else:
        key, first = np.unique(r * n_cols + c, return_index=True)
        r, c = key // n_cols, key % n_cols
        vals = (rng.random(len(r)) + 0.25).astype(np.float32)
    return np.stack([r, c], 1).astype(np.int64), vals, (n_rows, n_cols)


def device_graph(gnntf, coo, vals, shape):
    return gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")


def scipy_of(g, values=None):
    rowptr, colidx, raw = g.csr_arrays()
    v = raw if values is None else values
    return sp.csr_matrix((v.double().cpu().numpy(), colidx.cpu().numpy(), rowptr.cpu().numpy()), shape=(g.n_rows, g.n_cols))


# ---- 1. the cast ------------------------------------------------------------------------------------------------------------
def test_cast_is_the_torch_cast(gnntf):
    from gnntf import sparse
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((777, 37)) * 10.0 ** rng.integers(-40, 39, (777, 37))).astype(np.float32)
    bits = np.array([0x3F808000, 0x3F818000, 0x00018000, 0x7F7F8000, 0x7F7FFFFF, 0xFF800000, 0x7F800000, 0x80000000],
                    dtype=np.uint32).view(np.float32)
    x[0, :8] = bits
    x[1, :4] = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    X = dev(x)
    got = sparse.to_bf16(X)
    want = X.to(torch.bfloat16)
    nan = torch.isnan(X)
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
    assert torch.isnan(got.float()[nan]).all() and int(nan.sum()) == 4
    # a strided source (leading dimension > C) and the unvectorised path (C odd)
    Xs = dev(rng.standard_normal((100, 48)).astype(np.float32))[:, :33]
    assert torch.equal(sparse.to_bf16(Xs).view(torch.int16), Xs.to(torch.bfloat16).view(torch.int16))
    Xv = dev(rng.standard_normal((100, 64)).astype(np.float32))
    assert torch.equal(sparse.to_bf16(Xv).view(torch.int16), Xv.to(torch.bfloat16).view(torch.int16))


# ---- 2. + 3. single SpMM ------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 3, 7, 8, 16, 17, 32, 40, 64, 100, 128, 256, 260, 512)


def _spmm_case(gnntf, g, A, C, diag, bias, relu, skip_empty, seed, out_bf16=False):
    from gnntf import sparse, _native as nat
    rng = np.random.default_rng(seed)
    Xb = dev(bf16_bits(rng.uniform(-1, 1, (g.n_cols, C)).astype(np.float32)).view(np.int16)).view(torch.bfloat16)
    x = bf16_decode(Xb.view(torch.int16).cpu().numpy().view(np.uint16)).astype(np.float64)
    beta, alpha = 0.9, 0.35
    h0 = rng.uniform(-1, 1, (1 if bias else g.n_rows, C)).astype(np.float32)
    d = rng.uniform(0.5, 1.5, g.n_rows).astype(np.float32) if diag else None
    adj = sparse.Adjacency(g, None, dev(d) if diag else None)
    act = (nat.ACT_RELU if relu else nat.ACT_NONE) | (nat.ACT_SKIP_EMPTY if skip_empty else 0)
    got = sparse._launch_bf16(adj, Xb, dev(h0), beta, alpha, act, out_bf16=out_bf16)
    S, M = A @ x, abs(A) @ abs(x)
    if diag:
        S, M = S + d[:, None] * x, M + np.abs(d)[:, None] * abs(x)
    ref = np.float32(beta) * S + np.float32(alpha) * h0.astype(np.float64)
    mag = abs(np.float32(beta)) * M + abs(np.float32(alpha) * h0.astype(np.float64))
    if relu:
        ref = np.maximum(ref, 0)
    return got, ref, mag, adj.graph.last_kernel()


def test_spmm_f32_out_against_float64(gnntf):
    names = set()
    gsq = device_graph(gnntf, *hub_graph(3000, 3000, seed=3))
    grect = device_graph(gnntf, *hub_graph(2500, 4000, seed=4))
    Asq, Arect = scipy_of(gsq), scipy_of(grect)
    for i, C in enumerate(WIDTHS):
        cases = [(gsq, Asq, dict(diag=True, bias=False, relu=False, skip_empty=False)),
                 (grect, Arect, dict(diag=False, bias=True, relu=True, skip_empty=False)),
                 (gsq, Asq, dict(diag=False, bias=False, relu=(i % 2 == 0), skip_empty=False))]
        for g, A, kw in cases:
            got, ref, mag, name = _spmm_case(gnntf, g, A, C, seed=100 + i, **kw)
            names.add(name)
            got = got.double().cpu().numpy()
            assert got.dtype == np.float64 and np.isfinite(got).all()
            bad = np.abs(got - ref) > 1e-5 * np.abs(ref) + 1e-5 * mag
            assert not bad.any(), (C, kw, np.argwhere(bad)[:5], float(np.max(np.abs(got - ref))))
        # GNX_ACT_SKIP_EMPTY: rows without entries keep what the buffer held; the others are written
        from gnntf import sparse, _native as nat
        rng = np.random.default_rng(i)
        Xb = sparse.to_bf16(dev(rng.uniform(-1, 1, (gsq.n_cols, C)).astype(np.float32)))
        out = torch.full((gsq.n_rows, C), 7.0, device="cuda:0")
        nat.check(nat.lib().gnx_spmm_bf16(gsq.handle, None, None, nat.ptr(Xb), C, C, None, 0, 1.0, 0.0, nat.ACT_SKIP_EMPTY,
                                          nat.ptr(out), 0, C, nat.current_stream()))
        full = sparse._launch_bf16(sparse.Adjacency(gsq), Xb, None, 1.0, 0.0, nat.ACT_NONE)
        empty = torch.from_numpy(np.diff(Asq.indptr) == 0).cuda()
        assert empty.any() and (out[empty] == 7.0).all() and torch.equal(out[~empty], full[~empty])
        names.add(gsq.last_kernel())
    assert all(n.endswith("_bf16") for n in names), names
    classes = {n.split("+")[0].replace("_bf16", "") for n in names}
    assert {"spmm_wave", "spmm_group32", "spmm_group16", "spmm_group8"} <= classes, names
    assert any("+chunks_bf16" in n for n in names) and any("+long_bf16" in n for n in names), names


def test_spmm_bf16_out_is_rounded_once(gnntf):
    g = device_graph(gnntf, *hub_graph(3000, 3000, seed=5))
    A = scipy_of(g)
    exact = total = 0
    for i, C in enumerate(WIDTHS):
        got, ref, mag, name = _spmm_case(gnntf, g, A, C, diag=(i % 2 == 1), bias=False, relu=(i % 3 == 0), skip_empty=False,
                                         seed=200 + i, out_bf16=True)
        assert got.dtype == torch.bfloat16 and name.endswith("_bf16")
        gb = got.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.int64)
        wb = bf16_bits(ref.astype(np.float32)).astype(np.int64)
        # one bf16 ulp = 1 in the bit pattern (same sign); +0 / -0 are the same number
        signed = lambda b: np.where(b >= 0x8000, -(b - 0x8000), b)
        diff = np.abs(signed(gb) - signed(wb))
        cancelling = np.abs(ref) < 1e-4 * mag                    # sums that cancel to their f32 noise: judged by the f32 test
        assert (diff[~cancelling] <= 1).all(), (C, np.argwhere((diff > 1) & ~cancelling)[:5])
        exact += int((diff == 0).sum())
        total += diff.size
    assert exact >= 0.999 * total, (exact, total)


# ---- 4. the K loop -------------------------------------------------------------------------------------------------------------
def _loop_bf16(sparse, adj, H0, a, K, relu):
    H0 = H0.contiguous()
    return sparse._appnp_propagate_bf16(adj, H0, a, K, relu)        # the bf16 kernels at every width (no f32 allowance)


@pytest.mark.parametrize("C", [7, 8, 40, 64, 128, 256])
def test_k_loop_against_emulation_and_f32(gnntf, C):
    from gnntf import sparse
    a = 0.1
    coo, vals, shape = graphs.rmat_symmetric_coo(4000, 30000, seed=C)
    g = device_graph(gnntf, coo, vals, shape)
    Asym = gnntf.normalize(g, "symmetric")
    Aeye = gnntf.normalize(g, "symmetric", "before")
    H0 = dev(np.random.default_rng(C).uniform(-1, 1, (shape[0], C)).astype(np.float32))
    for K in (0, 1, 2, 10):
        for relu in (False, True):
            for adj in (Asym, Aeye):
                got = _loop_bf16(sparse, adj, H0, a, K, relu)
                again = _loop_bf16(sparse, adj, H0, a, K, relu)
                assert torch.equal(got, again)                                           # deterministic
                assert got.dtype == torch.float32 and got.shape == H0.shape
                if K == 0:
                    assert torch.equal(got, H0)
                    continue
                assert g.last_kernel().endswith("_bf16")
                A = scipy_of(g, adj.vals)
                diag = adj.diag.cpu().numpy() if adj.diag is not None else None
                want = appnp_bf16(A, H0.cpu().numpy(), a, K, relu=relu, diag=diag)
                err = np.linalg.norm(got.double().cpu().numpy() - want) / np.linalg.norm(want)
                assert err <= 1e-3, (C, K, relu, diag is not None, err)
                if adj is Asym:
                    _check_bound(sparse, adj, H0, a, K, relu, got)


def _check_bound(sparse, adj, H0, a, K, relu, got):
    """Per column ||bf16 - f32||_2 <= (u/a) max_k ||H_k||_2 * 1.05 (symmetric normalisation of a symmetric pattern: ||A||_2 <= 1)."""
    ref = sparse.appnp_propagate(adj, H0, a, K, relu=relu)
    norms = torch.stack([sparse.appnp_propagate(adj, H0, a, k, relu=relu).double().norm(dim=0) for k in range(K + 1)])
    bound = (U / a) * norms.max(dim=0).values * 1.05
    delta = (got.double() - ref.double()).norm(dim=0)
    assert (delta <= bound).all(), (K, relu, float((delta / bound).max()))


@pytest.mark.parametrize("C", [8, 128])
def test_k_loop_large_graph(gnntf, C):
    """2^20 vertices: the separate long-row launches and the big-graph row kernels run (and, at C = 8, the f32 loop takes its
    relabelled copy while the bf16 loop does not)."""
    from gnntf import sparse
    coo, vals, shape = graphs.rmat_symmetric_coo(1 << 20, 4_000_000, seed=11)
    g = device_graph(gnntf, coo, vals, shape)
    adj = gnntf.normalize(g, "symmetric")
    H0 = dev(np.random.default_rng(3).uniform(-1, 1, (shape[0], C)).astype(np.float32))
    got = _loop_bf16(sparse, adj, H0, 0.1, 10, False)
    name = g.last_kernel()
    assert name.endswith("+long_bf16"), name
    assert torch.equal(got, _loop_bf16(sparse, adj, H0, 0.1, 10, False))
    _check_bound(sparse, adj, H0, 0.1, 10, False, got)
    # the public entry: bf16 above the allowance, f32 (bit for bit today's result) below it
    pub = sparse.appnp_propagate(adj, H0, 0.1, 10, storage=torch.bfloat16)
    if C >= sparse.BF16_MIN_WIDTH or g.n_rows < sparse.BF16_F32_ROWS:
        assert torch.equal(pub, got)
    else:
        assert torch.equal(pub, sparse.appnp_propagate(adj, H0, 0.1, 10))


def test_k_loop_between_the_size_regimes(gnntf):
    """40000 vertices (2^15 <= n < 2^20: rows cut at 128 entries, chunks and short rows in one launch) with hub rows above 128 and
    above 512 entries: deterministic, and within the first-order bound of the f32 loop."""
    from gnntf import sparse
    n = 40000
    coo, _, shape = graphs.rmat_symmetric_coo(n, 200000, seed=6)
    rng = np.random.default_rng(6)
    extra = []
    for hub, deg in ((3, 200), (5, 700), (11, 1500)):
        other = rng.choice(np.arange(16, n), size=deg, replace=False)
        extra += [np.stack([np.full(deg, hub), other], 1), np.stack([other, np.full(deg, hub)], 1)]
    coo = np.unique(np.concatenate([coo] + extra), axis=0)
    g = device_graph(gnntf, coo, np.ones(len(coo), dtype=np.float32), shape)
    degrees = np.diff(g.csr_arrays()[0].cpu().numpy())
    assert ((degrees > 128) & (degrees <= 512)).any() and (degrees > 512).any()
    adj = gnntf.normalize(g, "symmetric")
    names = set()
    for C in (8, 40, 256):
        H0 = dev(rng.uniform(-1, 1, (n, C)).astype(np.float32))
        for relu in (False, True):
            got = _loop_bf16(sparse, adj, H0, 0.1, 10, relu)
            names.add(g.last_kernel())
            assert torch.equal(got, _loop_bf16(sparse, adj, H0, 0.1, 10, relu))
            _check_bound(sparse, adj, H0, 0.1, 10, relu, got)
            A = scipy_of(g, adj.vals)
            want = appnp_bf16(A, H0.cpu().numpy(), 0.1, 10, relu=relu)
            err = np.linalg.norm(got.double().cpu().numpy() - want) / np.linalg.norm(want)
            assert err <= 1e-3, (C, relu, err)
    assert all(name.endswith("_bf16") for name in names) and any("+chunks_bf16" in name for name in names), names


@pytest.mark.parametrize("window", [64, 1000])
def test_row_window_keeps_the_bits(gnntf, window):
    """gnx_graph_set_row_window: another launch order, the same sums -- a bf16 SpMM (f32 and bf16 result) and the bf16 K loop."""
    from gnntf import sparse, _native as nat
    coo, vals, shape = hub_graph(3000, 3000, seed=9, symmetric=True)
    rng = np.random.default_rng(window)
    for C in (8, 100):
        X = dev(rng.uniform(-1, 1, (shape[1], C)).astype(np.float32))
        H0 = dev(rng.uniform(-1, 1, (shape[0], C)).astype(np.float32))
        results = []
        for w in (0, window):
            g = device_graph(gnntf, coo, vals, shape)
            if w:
                g.set_row_window(w)
            adj = gnntf.normalize(g, "symmetric")
            results.append([sparse._launch_bf16(adj, X, H0, 0.9, 0.35, nat.ACT_RELU, out_bf16=False),
                            sparse._launch_bf16(adj, X, H0, 0.9, 0.35, nat.ACT_NONE, out_bf16=True).view(torch.int16),
                            _loop_bf16(sparse, adj, H0, 0.1, 4, False)])
            assert g.last_kernel().endswith("_bf16")
        for x, y in zip(*results):
            assert torch.equal(x, y), (C, window)


def test_public_spmm_storage(gnntf):
    from gnntf import sparse
    coo, vals, shape = graphs.rmat_symmetric_coo(3000, 20000, seed=2)
    g = device_graph(gnntf, coo, vals, shape)
    adj = gnntf.normalize(g, "symmetric")
    X = dev(np.random.default_rng(0).uniform(-1, 1, (shape[0], 40)).astype(np.float32))
    got = gnntf.spmm(adj, X, storage=torch.bfloat16)
    assert torch.equal(got, gnntf.spmm(adj, X.to(torch.bfloat16), storage=torch.bfloat16))     # f32 X is cast, bf16 X taken as is
    assert g.last_kernel().endswith("_bf16")
    f32 = gnntf.spmm(adj, X)
    M = torch.from_numpy(abs(scipy_of(g, adj.vals)) @ np.abs(X.double().cpu().numpy())).cuda()
    assert ((got.double() - f32.double()).abs() <= (U + 1e-5) * M).all()                         # |A.X~ - A.X| <= u |A| |X|
    # the default storage is today's path: a bf16 X is widened to f32 first
    assert torch.equal(gnntf.spmm(adj, X.to(torch.bfloat16)), gnntf.spmm(adj, X.to(torch.bfloat16).float()))
    Xg = X.clone().requires_grad_(True)
    with pytest.raises(Exception, match="inference only"):
        gnntf.spmm(adj, Xg, storage=torch.bfloat16)
    with torch.no_grad():
        assert torch.equal(gnntf.spmm(adj, Xg, storage=torch.bfloat16), got)


# ---- 5. + 6. the model level -----------------------------------------------------------------------------------------------------
def _cora_models(gnntf, golden_dir, **kw):
    from test_oracle_kat import load_cora
    z, coo, vals, shape, X, weights = load_cora(golden_dir)
    models = []
    for dtype in (torch.float32, torch.bfloat16):
        m = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7, inference_dtype=dtype, **kw)
        dense = [l for l in m.layers() if isinstance(l, gnntf.Dense)]
        for layer, (W, b) in zip(dense, weights):
            layer.W.data.copy_(dev(W)); layer.b.data.copy_(dev(b))
        m.training_mode(False)
        models.append(m)
    return z, models


def _margin_check(ref, got, capsys=None, what=""):
    flipped = ref.argmax(1) != got.argmax(1)
    top2 = np.sort(ref, axis=1)[:, -2:]
    margin = top2[:, 1] - top2[:, 0]
    allowed = 2.0 ** -5 * np.abs(ref).max(axis=1)
    assert (margin[flipped] <= allowed[flipped]).all(), np.argwhere(flipped & (margin > allowed))[:5]
    print(f"{what}: {int(flipped.sum())} of {len(ref)} rows change their argmax under bf16 storage")
    return int(flipped.sum())


@pytest.mark.parametrize("reorder", [None, "degree"])
def test_cora_appnp_bf16_inference(gnntf, golden_dir, reorder):
    z, (m32, m16) = _cora_models(gnntf, golden_dir, reorder=reorder)
    with torch.no_grad():
        ref = m32(m32.features).cpu().numpy()
        got = m16(m16.features)
    assert m16.graph.last_kernel().endswith("_bf16"), m16.graph.last_kernel()
    got = got.cpu().numpy()
    assert np.abs(got - ref).max() > 0                                    # bf16 did run
    _margin_check(ref, got, what=f"cora APPNP (reorder={reorder})")
    pred = m16.predict(gnntf.NodeClassification(list(range(1708, 2708))))
    assert pred.shape[0] == 1000 and m16.graph.last_kernel().endswith("_bf16")


@pytest.mark.parametrize("transform_first", [False, True])
def test_gcn_bf16_eval_forward(gnntf, transform_first):
    coo, vals, shape, X = graphs.cora_shaped(seed=4)
    rng = np.random.default_rng(8)
    weights = [(rng.standard_normal((1433, 32)).astype(np.float32), rng.uniform(0.0, 0.2, (1, 32)).astype(np.float32)),
               (rng.standard_normal((32, 7)).astype(np.float32), rng.uniform(0.0, 0.2, (1, 7)).astype(np.float32))]
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        m = gnntf.GCN(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7, latent_dims=[32], transform_first=transform_first,
                      inference_dtype=dtype)
        for layer, (W, b) in zip(m.layers(), weights):            # outputs well away from the last layer's relu floor
            layer.W.data.copy_(dev(W)); layer.b.data.copy_(dev(b))
        m.training_mode(False)
        with torch.no_grad():
            out.append(m(m.features).cpu().numpy())
        if dtype is torch.bfloat16:
            assert m.graph.last_kernel().endswith("_bf16")
    assert (out[0] > 0).mean() > 0.2 and np.abs(out[0] - out[1]).max() > 0
    _margin_check(out[0], out[1], what=f"GCN transform_first={transform_first}")


@pytest.mark.parametrize("fused", [False, True])
def test_training_step_is_untouched(gnntf, fused):
    from gnntf.training import _Objective
    n, F, classes = 600, 40, 5
    coo, vals, shape = graphs.rmat_symmetric_coo(n, 4000, seed=3)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, F)).astype(np.float32)
    labels = rng.integers(0, classes, size=n)
    task = gnntf.NodeClassification(np.arange(200), labels[:200])
    results = []
    for dtype in (torch.float32, torch.bfloat16):
        gnntf.set_seed(17)
        model = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=classes, latent_dims=[16], fused=fused,
                            inference_dtype=dtype)
        model.reset()
        params = [v.var for v in model.vars() if v.trainable]
        with model:
            loss = _Objective(model, task, 5e-4)()
            loss.backward()
        results.append([loss.detach().clone()] + [p.grad.clone() for p in params])
        assert not model.graph.last_kernel().endswith("_bf16")
    assert len(results[0]) == len(results[1]) > 1
    for a_, b_ in zip(*results):
        assert torch.equal(a_, b_)
