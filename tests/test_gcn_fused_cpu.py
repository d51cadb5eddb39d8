"""The fused GCNLayer (gnx_gcn_step, gnx_gcn_step_dropped, sparse.gcn_step, GNN(gcn_layer=)) as far as it goes without a GPU: the header
declares the two entries and the binding carries their argument types, the entries refuse bad arguments before they look at a device,
the keyword refuses what it does not know, the layer keeps today's ops on CPU tensors whatever the switch says, the layer's predicate
says no to every excluded case, and the bound of tests/gcn_fused_ref.py admits the float32 emulations and rejects a lost bias."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from abi_header import ctypes_of, prototype as header_prototype, text as header_text
import gcn_fused_ref as gref

BOUND_CASES = [(64, 64), (64, 40), (64, 7), (16, 16)]

TAIL = ["const float *d_X", "int64_t ldx", "int64_t C_in", "const float *d_W", "int64_t ldw", "int64_t C_out", "const float *d_bias", "int act",
        "double dropout_p", "uint64_t seed", "uint64_t stream_id", "float *d_out", "int64_t ldo", "float *d_agg", "float *d_work", "void *stream"]
PROTOTYPES = {
    "gnx_gcn_step": ["gnx_graph_t g", "const float *d_vals"] + TAIL,
    "gnx_gcn_step_dropped": ["gnx_graph_t g", "const float *d_D", "float edge_p", "uint64_t edge_seed", "uint64_t edge_stream"] + TAIL,
}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_library_and_binding_agree(name):
    from gnntf import _native
    assert header_prototype(name) == PROTOTYPES[name]
    assert "gcn.py:88-89" in header_text()
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), name)
    want = ctypes_of(PROTOTYPES[name])
    restype, argtypes = _native.SIGNATURES[name]
    assert restype is ctypes.c_int and argtypes == want
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION


def test_checks_that_need_no_device():
    """The NULL handle and a rate outside [0, 1) are refused before anything is dereferenced; the message names the entry."""
    from gnntf import _native
    lib = _native.lib()
    tail = (16, 16, 16, 16, 16, 16, None, 1, 0.0, 1, 2, 16, 16, None, None, None)
    assert lib.gnx_gcn_step(None, None, *tail) == -1
    assert b"gnx_gcn_step: NULL handle" in lib.gnx_last_error()
    assert lib.gnx_gcn_step_dropped(None, 16, 0.5, 1, 0, *tail) == -1
    assert b"gnx_gcn_step_dropped: NULL handle" in lib.gnx_last_error()
    handle = ctypes.c_void_p(16)                        # never dereferenced: the rate is checked first
    for rate in (1.0, -0.1):
        bad = tail[:8] + (rate,) + tail[9:]
        assert lib.gnx_gcn_step(handle, None, *bad) == -1
        assert b"gnx_gcn_step: dropout rate" in lib.gnx_last_error()
        assert lib.gnx_gcn_step_dropped(handle, 16, 0.5, 1, 0, *bad) == -1
        assert b"gnx_gcn_step_dropped: dropout rate" in lib.gnx_last_error()


def tiny_graph():
    import gnntf
    coo = np.array([[0, 1], [1, 0], [1, 2], [2, 1]], dtype=np.int64)
    return gnntf.SparseCOO(coo, np.ones(len(coo), dtype=np.float32), (3, 3))


def test_keyword_is_validated_and_the_function_is_exported():
    import gnntf
    from gnntf import sparse
    assert sparse.GCN_LAYERS == ("composed", "fused")
    assert gnntf.gcn_step is sparse.gcn_step
    X = np.zeros((3, 4), dtype=np.float32)
    for make in (lambda **k: gnntf.GNN(tiny_graph(), X, **k), lambda **k: gnntf.GCN(tiny_graph(), X, 2, **k)):
        with pytest.raises(Exception, match="gcn_layer must be one of"):
            make(gcn_layer="bogus")
        with pytest.raises(Exception, match="gcn_layer must be one of"):
            make(gcn_layer=True)
    with pytest.raises(Exception, match="edge_dropout must be one of"):
        sparse.gcn_step(None, None, None, edge_dropout="bogus")


# ---- the layer keeps today's ops where the fused launch does not apply ---------------------------------------------------------------------
class CpuGraph:                                          # what GNN keeps as self.graph; never dereferenced on the CPU path
    n_rows = n_cols = 12


def cpu_world(monkeypatch):
    """A GCN model on CPU tensors over a dense stand-in adjacency (the pattern of tests/test_gcnii_spectral_cpu.py); every launch of the
    fused layer and every call into the library fails the test."""
    from gnntf import _native, graph_model, params, sparse
    monkeypatch.setattr(params, "_default_device", torch.device("cpu"))        # (on a machine with a GPU too)
    rng = np.random.default_rng(5)
    dense_adj = torch.from_numpy((rng.random((12, 12)) < 0.3).astype(np.float32) / 4)
    monkeypatch.setattr(sparse, "spmm", lambda adj, X, storage=torch.float32: dense_adj @ X)
    monkeypatch.setattr(graph_model.GNN, "get_adjacency", lambda self, *args, **kwargs: sparse.Adjacency(self.graph))
    monkeypatch.setattr(graph_model.sparse, "DeviceGraph", CpuGraph, raising=True)
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the CPU path called into the library"))
    monkeypatch.setattr(sparse, "_gcn_launch", lambda *a, **k: pytest.fail("the fused launch ran"))
    return dense_adj


def one_step(**option):
    import gnntf
    rng = np.random.default_rng(6)
    X = rng.standard_normal((12, 16)).astype(np.float32)
    nodes, labels = np.arange(0, 12, 2), rng.integers(0, 3, size=6)
    gnntf.set_seed(3)
    torch.manual_seed(3)
    model = gnntf.GCN(CpuGraph(), X, 3, latent_dims=[16, 8], **option)
    model.reset()
    for layer in model.layers():
        if isinstance(layer, gnntf.GCNLayer):
            layer.b.data.copy_(torch.from_numpy(rng.uniform(-0.3, 0.3, size=tuple(layer.b.shape)).astype(np.float32)))
    torch.manual_seed(4)
    with model:
        loss = gnntf.NodeClassification(nodes, labels).loss(model(model.features))
        loss.backward()
    return float(loss.detach()), [v.var.grad.clone() for v in model.vars()], model._mask_calls


def test_cpu_tensors_keep_the_composed_ops(monkeypatch):
    cpu_world(monkeypatch)
    fused = one_step(gcn_layer="fused", feature_dropout="fused")
    default = one_step()
    assert fused[2] == default[2] == 0                  # no counter-RNG stream was taken
    assert fused[0] == default[0] and np.isfinite(fused[0])
    assert all(torch.equal(a, b) for a, b in zip(fused[1], default[1]))
    assert len(fused[1]) == 6 and any(float(g.abs().max()) > 0 for g in fused[1])


class OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda: what the layer's predicate looks at, without a device."""
    is_cuda = True


def test_the_layer_predicate(monkeypatch):
    """_fused_gcn says yes to float32 device rows of width 16 / 32 / 64 with at most as many outputs under relu / the identity -- over a
    constant or a dropped adjacency, in either mode -- and no to each of: the default keyword, CPU tensors, float64 rows, another input
    width, more outputs than inputs, an adjacency with a diagonal, tanh, transform_first, a subclass, a bf16 inference forward."""
    import gnntf
    from gnntf import sparse
    cpu_world(monkeypatch)
    X = np.zeros((12, 16), dtype=np.float32)

    def rows_of(width, dtype=torch.float32):
        return torch.Tensor._make_subclass(OnDevice, torch.zeros(12, width, dtype=dtype))

    rows = rows_of(16)
    assert rows.is_cuda and not torch.zeros(1).is_cuda

    def layer_of(layer_type=gnntf.GCNLayer, **option):
        model = gnntf.GCN(CpuGraph(), X, 3, latent_dims=[16], layer_type=layer_type, **option)
        return model, [l for l in model.layers() if isinstance(l, gnntf.GCNLayer)]

    constant = sparse.Adjacency(CpuGraph())
    model, (first, last) = layer_of(gcn_layer="fused")
    assert model.is_training() and first.W.shape == (16, 16) and last.W.shape == (16, 3)
    for layer in (first, last):
        assert layer._fused_gcn(model, rows, constant)
        assert layer._fused_gcn(model, rows, sparse.DroppedAdjacency(CpuGraph(), 0.5, 1, 0, D=torch.ones(12)))
    assert first._fused_gcn(model, rows_of(32), constant) and first._fused_gcn(model, rows_of(64), constant)
    other = layer_of()
    assert not other[1][0]._fused_gcn(other[0], rows, constant)
    assert not first._fused_gcn(model, torch.zeros(12, 16), constant)
    assert not first._fused_gcn(model, rows_of(16, torch.float64), constant)
    assert not first._fused_gcn(model, rows_of(24), constant) and not first._fused_gcn(model, rows_of(128), constant)
    wide = torch.nn.Parameter(torch.zeros(16, 17))
    keep, first.W = first.W, wide
    assert not first._fused_gcn(model, rows, constant)                                  # outputs > C_in
    first.W = keep
    assert not first._fused_gcn(model, rows, sparse.Adjacency(CpuGraph(), None, torch.ones(12)))
    first.activation = torch.tanh
    assert not first._fused_gcn(model, rows, constant)
    first.activation = gnntf.linear
    assert first._fused_gcn(model, rows, constant)
    first.transform_first = True
    assert not first._fused_gcn(model, rows, constant)
    first.transform_first = False
    model.training_mode(False)
    assert first._fused_gcn(model, rows, constant)                                      # eval mode under autograd
    with torch.no_grad():
        assert first._fused_gcn(model, rows, constant)
        model.inference_dtype = torch.bfloat16
        assert not first._fused_gcn(model, rows, constant)                              # a bf16 inference forward keeps its path
    assert first._fused_gcn(model, rows, constant)                                      # ... and only that forward
    model.inference_dtype = torch.float32
    spectral = layer_of(gnntf.GCNSpectralPreservingLayer, gcn_layer="fused")
    assert not spectral[1][0]._fused_gcn(spectral[0], rows, constant)

    class Mine(gnntf.GCNLayer):
        pass
    first.__class__ = Mine
    assert not first._fused_gcn(model, rows, constant)


def test_host_function_keeps_the_composed_ops(monkeypatch):
    """sparse.gcn_step itself: CPU tensors, a DroppedAdjacency without edge_dropout="fused" and a diagonal are today's ops."""
    from gnntf import sparse
    dense_adj = cpu_world(monkeypatch)
    rng = np.random.default_rng(8)
    X = torch.from_numpy(rng.standard_normal((12, 16)).astype(np.float32))
    W = torch.from_numpy((rng.standard_normal((16, 7)) / 4).astype(np.float32))
    bias = torch.from_numpy(rng.uniform(-0.3, 0.3, size=(1, 7)).astype(np.float32))
    for relu in (True, False):
        want = (dense_adj @ X) @ W + bias
        want = torch.relu(want) if relu else want
        assert torch.equal(sparse.gcn_step(sparse.Adjacency(CpuGraph()), X, W, bias, relu=relu), want)
    assert torch.equal(sparse.gcn_step(sparse.Adjacency(CpuGraph()), X, W, None, relu=False), (dense_adj @ X) @ W)
    rows = [torch.Tensor._make_subclass(OnDevice, t) for t in (X, W, bias)]
    monkeypatch.setattr(sparse, "dense", lambda T, M, b, relu: torch.relu(T @ M + b) if relu else T @ M + b)
    want = torch.relu((dense_adj @ X) @ W + bias)
    dropped = sparse.DroppedAdjacency(CpuGraph(), 0.5, 1, 0, D=torch.ones(12))
    assert torch.equal(sparse.gcn_step(dropped, *rows), want)
    assert torch.equal(sparse.gcn_step(sparse.Adjacency(CpuGraph(), None, torch.ones(12)), *rows), want)


# ---- the bound admits the float32 emulations and rejects a lost bias ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def structure(regime):
    coo, vals, shape, info = gref.regime_graph(regime)
    A64 = gref.csr_of(coo, vals, shape)
    d = np.asarray(A64.sum(axis=0)).ravel()
    scale = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    A32 = sp.csr_matrix(sp.diags(scale) @ A64 @ sp.diags(scale), dtype=np.float32)       # symmetric normalisation, rounded once
    A32.sort_indices()
    return dict(n=shape[0], A32=A32, A=sp.csr_matrix(A32, dtype=np.float64), info=info, L=info["L"])


@pytest.mark.parametrize("regime", ["T", "S"])
@pytest.mark.parametrize("C_in, C_out", BOUND_CASES)
def test_bound_admits_the_float32_emulations(regime, C_in, C_out):
    c = structure(regime)
    op = gref.operands(c["n"], C_in, C_out, 2000 + C_in + C_out)
    info = c["info"]
    for relu in (True, False):
        want = gref.forward_ref(c["A"], op["X"], op["W"], op["bias"], relu, L=c["L"])
        assert np.isfinite(want["out_bound"]).all() and (want["out_bound"] > 0).all()
        # the reference alone is inside its own bound; a lost bias (uniform in +-0.3) is far outside
        assert gref.ratio(want["out"], want["out"], want["out_bound"]) == 0.0
        if not relu:
            factor = gref.ratio(want["out"] - op["bias"][None, :], want["out"], want["out_bound"])
            print(f"{regime} {C_in}->{C_out}: a lost bias is {factor:.3g} x the bound")
            assert factor > 1e3
        for order in ("library", "sequential", "chunked"):
            agg, out = gref.forward_f32(c["A32"], op["X"], op["W"], op["bias"], relu, order, c["L"])
            assert out.dtype == np.float32 and agg.dtype == np.float32
            worst = gref.ratio(out, want["out"], want["out_bound"])
            print(f"{regime} {C_in}->{C_out} relu={relu} {order}: error / bound = {worst:.3f} (agg {gref.ratio(agg, want['agg'], want['agg_bound']):.3f})")
            assert worst <= 1.0 and gref.ratio(agg, want["agg"], want["agg_bound"]) <= 1.0
            for rows in (info["hub"], info["empty"], info["ragged"]):
                assert len(rows) and gref.ratio(out, want["out"], want["out_bound"], rows) <= 1.0


@pytest.mark.parametrize("C_in, C_out", [(64, 40), (24, 8)])
def test_backward_bound_admits_the_float32_emulations(C_in, C_out):
    c = structure("T")
    op = gref.operands(c["n"], C_in, C_out, 3000 + C_in)
    agg32, out = gref.forward_f32(c["A32"], op["X"], op["W"], op["bias"], True, "sequential", c["L"])
    G = gref.gate_f32(op["G"], out, True)
    want = gref.backward_ref(c["A"], agg32, G, op["W"], c["L"])
    for order in ("library", "sequential", "chunked"):
        dX, dW, db = gref.backward_f32(c["A32"], agg32, G, op["W"], order, c["L"])
        for name, got in (("dX", dX), ("dW", dW), ("db", db.reshape(1, -1))):
            worst = gref.ratio(got, want[name].reshape(got.shape), want[name + "_bound"].reshape(got.shape))
            print(f"{C_in}->{C_out} {order} {name}: error / bound = {worst:.3f}")
            assert worst <= 1.0
