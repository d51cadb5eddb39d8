"""The fused NGCFLayer (gnx_ngcf_step, gnx_ngcf_back_gate, sparse.ngcf_step, GNN(ngcf_layer=)) as far as it goes without a GPU: the header
declares the two entries and GNX_ACT_LEAKY and the binding carries their argument types, the entries refuse bad arguments before they
look at a device, the keyword refuses what it does not know, the layer keeps today's ops on CPU tensors whatever the switch says, every
clause of the layer's predicate says no on its own, the mask streams are drawn in the order of the layers, the backward is composed of
today's calls around the gate pass, and the bounds of tests/ngcf_fused_ref.py admit a float32 emulation, reject a lost bias and leave
at most 0.1 % of the gate bits undecided."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from abi_header import ctypes_of, prototype as header_prototype, text as header_text
import ngcf_fused_ref as nref
from test_gcn_fused_cpu import CpuGraph, OnDevice, tiny_graph


PROTOTYPES = {
    "gnx_ngcf_step": ["gnx_graph_t g", "const float *d_vals", "const float *d_X", "int64_t ldx", "int64_t C_in", "const float *d_W1", "int64_t ldw1",
                      "const float *d_W2", "int64_t ldw2", "int64_t C_out", "const float *d_b1", "const float *d_b2", "int act", "double dropout_p",
                      "uint64_t seed", "uint64_t stream_id", "int normalize", "float *d_out", "int64_t ldo", "float *d_agg", "uint32_t *d_gate",
                      "float *d_rnorm", "float *d_work", "int64_t work_floats", "void *stream"],
    "gnx_ngcf_back_gate": ["gnx_graph_t g", "const float *d_g", "int64_t ldg", "const float *d_y", "int64_t ldy", "const float *d_rnorm",
                           "const uint32_t *d_gate", "int64_t n_rows", "int64_t C_out", "int act", "double dropout_p", "uint64_t seed",
                           "uint64_t stream_id", "float *d_G1", "float *d_G2", "int64_t ldG", "void *stream"],
}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_library_and_binding_agree(name):
    from gnntf import _native
    assert header_prototype(name) == PROTOTYPES[name]
    text = header_text()
    assert "gcn.py:116-135" in text and "enum { GNX_ACT_LEAKY = 2 };" in text and _native.ACT_LEAKY == 2
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), name)
    want = ctypes_of(PROTOTYPES[name])
    restype, argtypes = _native.SIGNATURES[name]
    assert restype is ctypes.c_int and argtypes == want
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION


def test_checks_that_need_no_device():
    """The NULL handle and a rate outside [0, 1) are refused before anything is dereferenced; the gate pass checks its activation, widths,
    pointers and strides before it looks at the handle (the one below is not one).  Every message names the entry and the cause."""
    from gnntf import _native
    lib = _native.lib()
    step = (None, 16, 16, 16, 16, 16, 16, 16, 16, None, None, 2, 0.0, 1, 2, 1, 16, 16, None, None, None, None, 0, None)
    assert lib.gnx_ngcf_step(None, *step) == -1
    assert b"gnx_ngcf_step: NULL handle" in lib.gnx_last_error()
    handle = ctypes.c_void_p(16)
    for rate in (1.0, -0.1):
        assert lib.gnx_ngcf_step(handle, *(step[:12] + (rate,) + step[13:])) == -1
        assert b"gnx_ngcf_step: dropout rate" in lib.gnx_last_error()
    g, y, r, gate, G1, G2 = (ctypes.c_void_p(256 * k) for k in range(1, 7))

    def back(h=handle, g=g, ldg=8, y=y, ldy=8, r=r, gate=gate, n=4, C=7, act=2, rate=0.0, G1=G1, G2=G2, ldG=8):
        return lib.gnx_ngcf_back_gate(h, g, ldg, y, ldy, r, gate, n, C, act, rate, 1, 2, G1, G2, ldG, None)

    for change, cause in ((dict(h=None), "NULL handle"), (dict(act=7), "invalid activation 7"), (dict(C=0), "C_out not in [1, 2^20]"),
                          (dict(n=-1), "negative row count"), (dict(g=None), "NULL g / G1 / G2"), (dict(G2=None), "NULL g / G1 / G2"),
                          (dict(ldg=6), "a row stride below C_out"), (dict(ldG=6), "a row stride below C_out"),
                          (dict(y=None), "d_rnorm needs y"), (dict(ldy=6), "d_rnorm needs y"), (dict(gate=None), "need d_gate"),
                          (dict(G2=G1), "G1 and G2 must be buffers of their own"), (dict(G1=g), "G1 and G2 must be buffers of their own"),
                          (dict(G2=y), "G1 and G2 must be buffers of their own"), (dict(rate=1.0), "dropout rate 1 outside [0, 1)")):
        rc = back(**change)
        message = lib.gnx_last_error().decode()
        assert rc == -1 and message.startswith("gnx_ngcf_back_gate: ") and cause in message, (cause, message)


def test_keyword_is_validated_and_the_function_is_exported():
    import gnntf
    from gnntf import sparse
    assert sparse.NGCF_LAYERS == ("composed", "fused") and sparse.NGCF_FUSED_WIDTHS == (16, 32, 64)
    assert gnntf.ngcf_step is sparse.ngcf_step
    X = np.zeros((3, 4), dtype=np.float32)
    for make in (lambda **k: gnntf.GNN(tiny_graph(), X, **k), lambda **k: gnntf.NGCF(tiny_graph(), X, 2, **k)):
        with pytest.raises(Exception, match="ngcf_layer must be one of"):
            make(ngcf_layer="bogus")
        with pytest.raises(Exception, match="ngcf_layer must be one of"):
            make(ngcf_layer=True)
    with pytest.raises(Exception, match="ngcf_step: activation must be one of"):
        sparse.ngcf_step(None, None, None, None, None, None, activation="tanh")
    assert sparse._ngcf_work_floats(1547, 64, 40, 19, True) == 19 * 104 and sparse._ngcf_work_floats(1547, 64, 40, 0, False) == 0
    assert sparse._ngcf_work_floats(1547, 64, 40, 19, False) == 1547 * 64 + 19 * 104
    assert sparse._ngcf_work_floats(9, 7, 3, 9, False) == 64 + 64 + 27                   # the composed form: every row, shares rounded up to 4


# ---- the layer keeps today's ops where the fused launch does not apply ---------------------------------------------------------------------
def cpu_world(monkeypatch):
    """An NGCF model on CPU tensors over a dense stand-in adjacency (the pattern of tests/test_gcn_fused_cpu.py); every launch of the
    fused layer and every call into the library fails the test."""
    from gnntf import _native, graph_model, params, sparse
    monkeypatch.setattr(params, "_default_device", torch.device("cpu"))
    rng = np.random.default_rng(5)
    dense_adj = torch.from_numpy((rng.random((12, 12)) < 0.3).astype(np.float32) / 4)
    monkeypatch.setattr(sparse, "spmm", lambda adj, X, storage=torch.float32: dense_adj @ X)
    monkeypatch.setattr(graph_model.GNN, "get_adjacency", lambda self, *args, **kwargs: sparse.Adjacency(self.graph))
    monkeypatch.setattr(graph_model.sparse, "DeviceGraph", CpuGraph, raising=True)
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the CPU path called into the library"))
    monkeypatch.setattr(sparse, "_ngcf_launch", lambda *a, **k: pytest.fail("the fused launch ran"))
    return dense_adj


def one_step(**option):
    import gnntf
    rng = np.random.default_rng(6)
    X = rng.standard_normal((12, 16)).astype(np.float32)
    edges = rng.integers(0, 12, size=(10, 2))
    labels = rng.integers(0, 2, size=10)
    gnntf.set_seed(3)
    torch.manual_seed(3)
    model = gnntf.NGCF(CpuGraph(), X, 16, **option)
    model.reset()
    torch.manual_seed(4)
    with model:
        loss = gnntf.LinkPrediction(edges, labels).loss(model(model.features))
        loss.backward()
    return float(loss.detach()), [v.var.grad.clone() for v in model.vars()], model._mask_calls


def test_cpu_tensors_keep_the_composed_ops(monkeypatch):
    cpu_world(monkeypatch)
    fused = one_step(ngcf_layer="fused", feature_dropout="fused")
    default = one_step()
    assert fused[2] == default[2] == 0                  # no counter-RNG stream was taken
    assert fused[0] == default[0] and np.isfinite(fused[0])
    assert all(torch.equal(a, b) for a, b in zip(fused[1], default[1]))
    assert len(fused[1]) == 12 and any(float(g.abs().max()) > 0 for g in fused[1])


def rows_of(width, dtype=torch.float32):
    return torch.Tensor._make_subclass(OnDevice, torch.zeros(12, width, dtype=dtype))


def test_the_layer_predicate(monkeypatch):
    """_fused_ngcf says yes to float32 device rows of width 16 / 32 / 64 that the layer does not widen, under leaky_relu, relu or the
    identity, with both biases or none, in either mode -- and no to each of: the default keyword, CPU tensors, float64 and bf16 rows,
    another input width (128 among them), more outputs than inputs, an adjacency with a diagonal, tanh, one bias without the other, a
    subclass."""
    import gnntf
    from gnntf import graph_model, sparse
    cpu_world(monkeypatch)
    X = np.zeros((12, 16), dtype=np.float32)
    rows = rows_of(16)
    assert rows.is_cuda and not torch.zeros(1).is_cuda
    model = gnntf.NGCF(CpuGraph(), X, 16, ngcf_layer="fused")
    first, second, last = [l for l in model.layers() if isinstance(l, gnntf.NGCFLayer)]
    assert model.is_training() and tuple(first.W1.shape) == (16, 16) and first.activation is graph_model.leaky_relu
    for layer in (first, second, last):
        assert layer._fused_ngcf(model, rows)
    assert first._fused_ngcf(model, rows_of(32)) and first._fused_ngcf(model, rows_of(64))
    wide = gnntf.NGCF(CpuGraph(), np.zeros((12, 64), dtype=np.float32), 16, latent_dims=[64, 32], ngcf_layer="fused")
    l64, l32, l16 = [l for l in wide.layers() if isinstance(l, gnntf.NGCFLayer)]
    assert l64._fused_ngcf(wide, rows_of(64)) and l32._fused_ngcf(wide, rows_of(64)) and l16._fused_ngcf(wide, rows_of(32))
    other = gnntf.NGCF(CpuGraph(), X, 16)
    assert not [l for l in other.layers() if isinstance(l, gnntf.NGCFLayer)][0]._fused_ngcf(other, rows)
    named = gnntf.NGCF(CpuGraph(), X, 16, ngcf_layer="composed")
    assert not [l for l in named.layers() if isinstance(l, gnntf.NGCFLayer)][0]._fused_ngcf(named, rows)
    assert not first._fused_ngcf(model, torch.zeros(12, 16))
    assert not first._fused_ngcf(model, rows_of(16, torch.float64)) and not first._fused_ngcf(model, rows_of(16, torch.bfloat16))
    assert not first._fused_ngcf(model, rows_of(24)) and not first._fused_ngcf(model, rows_of(128)) and not first._fused_ngcf(model, rows_of(8))
    keep = first.W1
    first.W1 = torch.nn.Parameter(torch.zeros(16, 17))
    assert not first._fused_ngcf(model, rows)                                           # outputs > C_in
    first.W1 = keep
    plain, first.adjacency = first.adjacency, sparse.Adjacency(CpuGraph(), None, torch.ones(12))
    assert not first._fused_ngcf(model, rows)                                           # a diagonal
    first.adjacency = plain
    for act, want in ((torch.tanh, False), (gnntf.linear, True), (gnntf.relu, True), (graph_model.leaky_relu, True)):
        first.activation = act
        assert first._fused_ngcf(model, rows) == want
    b1, first.b1 = first.b1, 0
    assert not first._fused_ngcf(model, rows)                                           # one bias without the other
    b2, first.b2 = first.b2, 0
    assert first._fused_ngcf(model, rows)                                               # ... none at all is fine
    first.b1, first.b2 = b1, b2
    model.training_mode(False)
    assert first._fused_ngcf(model, rows)
    with torch.no_grad():
        assert first._fused_ngcf(model, rows)

    class Mine(gnntf.NGCFLayer):
        pass
    first.__class__ = Mine
    assert not first._fused_ngcf(model, rows)


def test_stream_draw_order_and_what_each_mode_launches(monkeypatch):
    """The fused layers of a model draw one mask stream each, in layer order, under feature_dropout="fused" in training with
    0 < dropout < 1 -- and none in eval mode, at a rate of 0, or with torch's dropout, where the launch runs with normalize=False and
    torch's dropout and normalize follow."""
    import gnntf
    from gnntf import graph_model, sparse
    cpu_world(monkeypatch)
    X = np.zeros((12, 16), dtype=np.float32)
    calls = []

    def fake(adj, X, W1, b1, W2, b2, activation="leaky", dropout=None, normalize=True):
        calls.append((activation, dropout, normalize))
        return torch.ones(12, W1.shape[1])

    monkeypatch.setattr(sparse, "ngcf_step", fake)
    monkeypatch.setattr(graph_model.NGCFLayer, "_fused_ngcf", lambda self, gcn, features: True)
    gnntf.set_seed(9)
    model = gnntf.NGCF(CpuGraph(), X, 16, ngcf_layer="fused", feature_dropout="fused", dropout=0.25)
    first = model._mask_calls
    with model:
        model(model.features)
    seed = gnntf.metrics.current_seed()
    assert calls == [("leaky", (0.25, seed, first + k), True) for k in range(3)] and model._mask_calls == first + 3
    del calls[:]
    model.training_mode(False)
    model(model.features)
    assert calls == [("leaky", None, True)] * 3 and model._mask_calls == first + 3
    for layer in model.layers():
        if isinstance(layer, gnntf.NGCFLayer):
            layer.dropout = 0
    del calls[:]
    with model:
        model(model.features)
    assert calls == [("leaky", None, True)] * 3 and model._mask_calls == first + 3
    torch_drop = gnntf.NGCF(CpuGraph(), X, 16, ngcf_layer="fused", dropout=0.25)
    del calls[:]
    before = torch_drop._mask_calls
    torch.manual_seed(1)
    with torch_drop:
        out = torch_drop(torch_drop.features)
    assert calls == [("leaky", None, False)] * 3 and torch_drop._mask_calls == before
    norms = out.norm(dim=1)
    assert torch.allclose(norms[norms > 0], torch.ones_like(norms[norms > 0]), atol=1e-6)      # torch's dropout, then torch's normalize


def test_host_function_keeps_the_composed_ops_and_composes_its_backward(monkeypatch):
    """sparse.ngcf_step: CPU tensors, a DroppedAdjacency and a diagonal are today's ops; on device rows the node's backward is the gate
    pass, the two weight gradients, the two products with W^T and ONE transposed SpMM, in that order, and its gradients are those of
    torch's autograd over the same formula."""
    from gnntf import sparse
    dense_adj = cpu_world(monkeypatch)
    rng = np.random.default_rng(8)
    n, C_in, C_out = 12, 16, 7
    X, W1, W2 = (torch.from_numpy((rng.standard_normal(s) / 2).astype(np.float32)) for s in ((n, C_in), (C_in, C_out), (C_in, C_out)))
    b1, b2 = (torch.from_numpy(rng.uniform(-0.3, 0.3, size=(1, C_out)).astype(np.float32)) for _ in range(2))

    def formula(X, W1, b1, W2, b2, act, normalize=True):
        agg = dense_adj @ X
        u = sparse._ngcf_act((X * agg) @ W1 + b1, act) + sparse._ngcf_act(agg @ W2 + b2, act)
        return torch.nn.functional.normalize(u, dim=1, eps=1e-12) if normalize else u

    for act in ("leaky", "relu", "none"):
        assert torch.equal(sparse.ngcf_step(sparse.Adjacency(CpuGraph()), X, W1, b1, W2, b2, activation=act), formula(X, W1, b1, W2, b2, act))
    assert torch.equal(sparse.ngcf_step(sparse.Adjacency(CpuGraph()), X, W1, None, W2, None, normalize=False), formula(X, W1, 0, W2, 0, "leaky", False))
    rows = [torch.Tensor._make_subclass(OnDevice, t) for t in (X, W1, b1, W2, b2)]
    monkeypatch.setattr(sparse, "dense", lambda T, M, b, relu: T @ M + b)
    want = formula(X, W1, b1, W2, b2, "leaky")
    assert torch.equal(sparse.ngcf_step(sparse.DroppedAdjacency(CpuGraph(), 0.5, 1, 0, D=torch.ones(n)), *rows), want)
    assert torch.equal(sparse.ngcf_step(sparse.Adjacency(CpuGraph(), None, torch.ones(n)), *rows), want)
    # the node, over fakes of the launches
    calls = []

    def recorded(name, fn):
        def wrapped(*args, **kwargs):
            calls.append(name)
            return fn(*args, **kwargs)
        monkeypatch.setattr(sparse, name, wrapped)

    def fake_launch(adj, X, W1, b1, W2, b2, activation, keep, dropout=None, normalize=True):
        agg = dense_adj @ X
        P1, P2 = (X * agg) @ W1 + b1, agg @ W2 + b2
        x = sparse._ngcf_act(P1, activation) + sparse._ngcf_act(P2, activation)
        r = 1 / x.norm(dim=1).clamp_min(1e-6)
        return (x * r[:, None]).detach(), agg.detach(), torch.stack([P1 > 0, P2 > 0]), r.detach()

    def fake_gate(graph, g, y, rnorm, gate, activation, dropout=None):
        gs = rnorm[:, None] * (g - y * (y * g).sum(dim=1, keepdim=True))
        slope = sparse.NGCF_SLOPES[activation]
        return gs * torch.where(gate[0], 1.0, slope), gs * torch.where(gate[1], 1.0, slope)

    recorded("_ngcf_launch", fake_launch)
    recorded("_ngcf_back_gate", fake_gate)
    recorded("_dense_wgrad", lambda T, G: T.t() @ G)
    recorded("_dense_launch", lambda G, Wt, b, relu: G @ Wt)
    recorded("_launch", lambda adj, T, H0, beta, alpha, act, transposed=False: dense_adj.t() @ T)
    upstream = torch.from_numpy(rng.standard_normal((n, C_out)).astype(np.float32))
    leaves = [torch.Tensor._make_subclass(OnDevice, t.clone()).requires_grad_() for t in (X, W1, b1, W2, b2)]
    out = sparse.ngcf_step(sparse.Adjacency(CpuGraph()), *leaves, activation="leaky")
    assert calls == ["_ngcf_launch"]
    out.backward(upstream)
    assert calls == ["_ngcf_launch", "_ngcf_back_gate", "_dense_wgrad", "_dense_wgrad", "_dense_launch", "_dense_launch", "_launch"], calls
    plain = [t.clone().requires_grad_() for t in (X, W1, b1, W2, b2)]
    formula(*plain, "leaky").backward(upstream)
    for name, got, ref in zip(("X", "W1", "b1", "W2", "b2"), leaves, plain):
        assert got.grad.shape == ref.grad.shape and torch.allclose(got.grad, ref.grad, rtol=1e-4, atol=1e-5), name


# ---- the bounds admit a float32 evaluation, reject a lost bias and decide the gate bits ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def structure(regime):
    coo, vals, shape, info = nref.regime_graph(regime)
    A, A32 = nref.bipartite(coo, vals, shape)
    return dict(n=shape[0], A=A, A32=A32, info=info, L=info["L"])


BOUND_CASES = [("T",) + s for s in nref.SHAPES] + [("S", 64, 40)]


@pytest.mark.parametrize("regime, C_in, C_out", BOUND_CASES)
def test_bounds_admit_float32_and_decide_the_gate_bits(regime, C_in, C_out):
    """Measured over these cases with the operands of the GPU tests: the undecided share of the gate bits is at most 0.033 % (the bound: 0.1 %)."""
    c = structure(regime)
    info = c["info"]
    assert len(info["hub"]) > 0 and len(info["empty"]) >= 16
    op = nref.operands(c["n"], C_in, C_out, 900 + 7 * C_in + C_out)
    for act in ("leaky", "relu", "none"):
        for normalize in (True, False):
            want = nref.forward_ref(c["A"], op["X"], op["W1"], op["b1"], op["W2"], op["b2"], act, normalize, L=c["L"])
            assert np.isfinite(want["out_bound"]).all()
            assert nref.ratio(want["out"], want["out"], want["out_bound"]) == 0.0
            for order in ("library", "chunked"):
                got = nref.forward_f32(c["A32"], op["X"], op["W1"], op["b1"], op["W2"], op["b2"], act, normalize, order, c["L"])
                worst = nref.ratio(got["out"], want["out"], want["out_bound"])
                print(f"{regime} {C_in}->{C_out} {act} normalize={normalize} {order}: error / bound = {worst:.3f}")
                assert got["out"].dtype == np.float32 and worst <= 1.0
                assert nref.ratio(got["agg"], want["agg"], want["e_agg"]) <= 1.0
                for rows in (info["hub"], info["empty"], info["ragged"]):
                    assert nref.ratio(got["out"], want["out"], want["out_bound"], rows) <= 1.0
        full = nref.forward_ref(c["A"], op["X"], op["W1"], op["b1"], op["W2"], op["b2"], act, L=c["L"])
        lost = nref.forward_ref(c["A"], op["X"], op["W1"], None, op["W2"], op["b2"], act, L=c["L"])["out"]
        factor = nref.ratio(lost, full["out"], full["out_bound"])
        print(f"{regime} {C_in}->{C_out} {act}: a lost b1 is {factor:.3g} x the bound")
        assert factor > 1e3
        d1, d2, share = nref.gate_share(full)
        print(f"{regime} {C_in}->{C_out} {act}: {share:.5%} of the gate bits are undecided by the float64 reference")
        assert share <= 1e-3 and d1[info["empty"]].all() and d2[info["empty"]].all()


def test_gate_words_round_trip():
    rng = np.random.default_rng(3)
    for C_out in (1, 7, 32, 40, 64):
        b1, b2 = rng.random((9, C_out)) < 0.5, rng.random((9, C_out)) < 0.5
        W = (C_out + 31) // 32
        words = np.zeros((9, 2 * W), dtype=np.uint32)
        for c in range(C_out):
            words[:, c >> 5] |= b1[:, c].astype(np.uint32) << np.uint32(c & 31)
            words[:, W + (c >> 5)] |= b2[:, c].astype(np.uint32) << np.uint32(c & 31)
        got = nref.unpack_gate(words.view(np.int32), C_out)
        assert np.array_equal(got[0], b1) and np.array_equal(got[1], b2)


def test_backward_bounds_admit_a_float32_evaluation():
    """The whole backward in float32 (numpy, library order) from the float32 forward's y, r, agg against backward_ref at 64 -> 7, with
    the mask: inside every bound, and gradients that lost the projection of the norm are outside every one of them."""
    c = structure("T")
    n, C_in, C_out = c["n"], 64, 7
    op = nref.operands(n, C_in, C_out, 77)
    rng = np.random.default_rng(78)
    mask = rng.random((n, C_out)) >= 0.25
    f32 = np.float32
    f = nref.forward_ref(c["A"], op["X"], op["W1"], op["b1"], op["W2"], op["b2"], "leaky", True, 0.25, mask, L=c["L"])
    bit1, bit2 = f["P1"] > 0, f["P2"] > 0
    want = nref.backward_ref(c["A"], f, op["X"], op["W1"], op["W2"], *nref.back_gate_ref(f, op["g"], bit1, bit2, "leaky", True, 0.25, mask), L=c["L"])
    # float32, every operation rounded once
    agg = nref.spmm_f32(c["A32"], op["X"], "library", c["L"])
    M = (op["X"] * agg).astype(f32)
    act = lambda P: np.where(P > 0, P, (f32(0.2) * P).astype(f32)).astype(f32)
    x = ((act((M @ op["W1"] + op["b1"]).astype(f32)) + act((agg @ op["W2"] + op["b2"]).astype(f32))) * nref.scale(0.25) * mask).astype(f32)
    r = (f32(1) / np.sqrt(np.maximum((x * x).sum(axis=1, dtype=f32), f32(1e-12)), dtype=f32)).astype(f32)[:, None]
    y = (x * r).astype(f32)
    d = (y * op["g"]).sum(axis=1, dtype=f32)[:, None]
    gu = np.where(mask, (r * (op["g"] - y * d)).astype(f32) * nref.scale(0.25), f32(0)).astype(f32)
    G1 = np.where(bit1, gu, (gu * f32(0.2)).astype(f32)).astype(f32)
    G2 = np.where(bit2, gu, (gu * f32(0.2)).astype(f32)).astype(f32)
    Q1, Q2 = (G1 @ op["W1"].T).astype(f32), (G2 @ op["W2"].T).astype(f32)
    At32 = c["A32"].T.tocsr()
    At32.sort_indices()
    dA = (Q1 * op["X"] + Q2).astype(f32)
    got = dict(dX=(Q1 * agg + nref.spmm_f32(At32, dA, "library", c["L"])).astype(f32), dW1=M.T @ G1, dW2=agg.T @ G2,
               db1=G1.sum(axis=0, dtype=f32), db2=G2.sum(axis=0, dtype=f32))
    for key, value in got.items():
        shape = (-1, value.shape[-1])
        worst = nref.ratio(value.reshape(shape), want[key].reshape(shape), want[key + "_bound"].reshape(shape))
        print(f"{key}: float32 error / bound = {worst:.3f}")
        assert worst <= 1.0
    unprojected = nref.backward_ref(c["A"], dict(f, y=np.zeros_like(f["y"])), op["X"], op["W1"], op["W2"],
                                    *nref.back_gate_ref(dict(f, y=np.zeros_like(f["y"])), op["g"], bit1, bit2, "leaky", True, 0.25, mask), L=c["L"])
    for key in got:                                        # (the hub rows of the bipartite-normalised regime graph carry weights far above 1:
        shape = (-1, want[key].shape[-1])                  # the worst-case bounds are a few percent of the gradients, and still 25 x too tight)
        assert nref.ratio(unprojected[key].reshape(shape), want[key].reshape(shape), want[key + "_bound"].reshape(shape)) > 10
