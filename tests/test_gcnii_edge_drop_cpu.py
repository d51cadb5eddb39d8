"""The fused GCNII layer under edge dropout (gnx_gcnii_step_dropped, gnx_gcnii_step_back_dropped, sparse.gcnii_step(edge_dropout=),
GNN(gcnii_edge_dropout=)) as far as it goes without a GPU: the header declares the two entries and the binding carries their argument
types, the keyword refuses what it does not know, a "fused" model on CPU tensors trains through today's torch ops bit for bit, and a
layer hands the keyword on -- and draws its mask streams in today's order and number -- exactly where GNN.__init__ says it applies (the
launch is replaced by a recorder, so no device is needed)."""
import ctypes

import numpy as np
import pytest
import torch

from abi_header import ctypes_of, prototype as header_prototype, text as header_text

A_MIX = 0.1

PROTOTYPES = {
    "gnx_gcnii_step_dropped": [
        "gnx_graph_t g", "const float *d_D", "float edge_p", "uint64_t edge_seed", "uint64_t edge_stream", "const float *d_H",
        "const float *d_H0", "float a", "int64_t C", "const float *d_M", "int64_t ldm", "int act", "double feat_p", "uint64_t feat_seed",
        "uint64_t feat_stream", "float *d_out", "float *d_mixed", "void *stream"],
    "gnx_gcnii_step_back_dropped": [
        "gnx_graph_t g", "const float *d_D", "float edge_p", "uint64_t edge_seed", "uint64_t edge_stream", "const float *d_G", "float a",
        "int64_t C", "const float *d_Mt", "int64_t ldmt", "float *d_dH", "const float *d_S_in", "float s_alpha", "float *d_S_out",
        "float *d_work", "void *stream"],
}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_library_and_binding_agree(name):
    from gnntf import _native
    assert header_prototype(name) == PROTOTYPES[name]
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), name)
    want = ctypes_of(PROTOTYPES[name])
    restype, argtypes = _native.SIGNATURES[name]
    assert restype is ctypes.c_int and argtypes == want
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION          # added within ABI 0.9: the number did not move
    text = header_text()
    for reported in ("spmm_gcnii_mfma_edrop", "spmm_gcnii_mfma_edrop_drop", "spmm_gcnii_back_mfma_edrop", "spmm+dense_mfma_edrop",
                     "dense+spmm_back_edrop"):
        assert '"' + reported + '"' in text                                    # the reported names are documented


def test_checks_that_need_no_device():
    from gnntf import _native
    lib = _native.lib()
    assert lib.gnx_gcnii_step_dropped(None, 16, 0.5, 1, 2, 16, 16, 0.1, 16, 16, 16, 1, 0.5, 1, 2, 16, None, None) == -1
    assert b"gnx_gcnii_step_dropped: NULL handle" in lib.gnx_last_error()
    assert lib.gnx_gcnii_step_dropped(None, 16, 0.5, 1, 2, 16, 16, 0.1, 16, 16, 16, 1, 1.5, 1, 2, 16, None, None) == -1
    assert lib.gnx_gcnii_step_back_dropped(None, 16, 0.5, 1, 2, 16, 0.1, 16, 16, 16, 32, None, 1.0, None, None, None) == -1
    assert b"gnx_gcnii_step_back_dropped: NULL handle" in lib.gnx_last_error()


def tiny_graph():
    import gnntf
    coo = np.array([[0, 1], [1, 0], [1, 2], [2, 1]], dtype=np.int64)
    return gnntf.SparseCOO(coo, np.ones(len(coo), dtype=np.float32), (3, 3))


def test_keyword_is_validated():
    import gnntf
    from gnntf import sparse
    assert sparse.GCNII_EDGE_DROPOUTS == ("composed", "fused")
    X = np.zeros((3, 4), dtype=np.float32)
    for make in (lambda **k: gnntf.GNN(tiny_graph(), X, **k), lambda **k: gnntf.GCNII(tiny_graph(), X, 2, iterations=1, **k)):
        for bad in ("bogus", True, None):
            with pytest.raises(Exception, match="gcnii_edge_dropout must be one of"):
                make(gcnii_edge_dropout=bad)
    for bad in ("bogus", True, None):
        with pytest.raises(Exception, match="gcnii_step: edge_dropout must be one of"):
            sparse.gcnii_step(None, None, None, 0.1, None, edge_dropout=bad)
        with pytest.raises(Exception, match="gcnii_step_back: edge_dropout must be one of"):
            sparse.gcnii_step_back(None, None, 0.1, None, edge_dropout=bad)


# ---- a model on CPU tensors: today's torch ops whatever the keyword says --------------------------------------------------------------------
class CpuGraph:                                          # what GNN keeps as self.graph; never dereferenced on the CPU path
    n_rows = n_cols = 12
    nnz = nnz_entries = 40
    entry_dropout = False


def cpu_world(monkeypatch):
    """A hand-built GCNIILayer(graph_dropout=0.5) stack on CPU tensors over a dense stand-in adjacency (the pattern of
    tests/test_gcnii_spectral_cpu.py): get_adjacency draws its mask stream as the real one does and returns a DroppedAdjacency in
    training mode; every call into the library fails the test."""
    from gnntf import _native, graph_model, sparse
    rng = np.random.default_rng(5)
    dense_adj = torch.from_numpy((rng.random((12, 12)) < 0.3).astype(np.float32) / 4)
    constant = sparse.Adjacency(CpuGraph())

    def get_adjacency(self, graph_dropout=0.5, normalized="symmetric", add_eye="none"):
        if graph_dropout != 0 and self.is_training():
            seed, stream = self._next_mask_stream()
            return sparse.DroppedAdjacency(self.graph, graph_dropout, seed, stream, D=torch.ones(12))
        return constant

    monkeypatch.setattr(sparse, "ppr_step", lambda adj, H, H0, a: (dense_adj @ H) * (1 - a) + H0 * a)
    monkeypatch.setattr(graph_model.GNN, "get_adjacency", get_adjacency)
    monkeypatch.setattr(graph_model.sparse, "DeviceGraph", CpuGraph, raising=True)
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the CPU path called into the library"))
    return dense_adj


def stack(**option):
    import gnntf
    rng = np.random.default_rng(6)
    X = rng.standard_normal((12, 6)).astype(np.float32)
    gnntf.set_seed(3)
    torch.manual_seed(3)
    model = gnntf.GNN(CpuGraph(), X, **option)
    model.add(gnntf.Dense(8, dropout=0, activation=gnntf.relu))
    H0 = model.top_layer()
    for k in range(3):
        model.add(gnntf.GCNIILayer(H0, A_MIX, 0.5, k, activation=gnntf.relu, dropout=0.6, graph_dropout=0.5))
    model.add(gnntf.Dense(3, dropout=0, regularize=False))
    model.reset()
    for layer in model.layers():
        if isinstance(layer, gnntf.GCNIILayer):
            layer.W.data.copy_(torch.from_numpy((rng.standard_normal((8, 8)) / 4).astype(np.float32)))
    return model


def one_step(**option):
    import gnntf
    rng = np.random.default_rng(7)
    nodes, labels = np.arange(0, 12, 2), rng.integers(0, 3, size=6)
    model = stack(**option)
    torch.manual_seed(4)
    with model:
        loss = gnntf.NodeClassification(nodes, labels).loss(model(model.features))
        loss.backward()
    return float(loss.detach()), [v.var.grad.clone() for v in model.vars()], model._mask_calls


def test_cpu_model_keeps_todays_ops(monkeypatch):
    cpu_world(monkeypatch)
    fused, default = one_step(gcnii_edge_dropout="fused"), one_step()
    assert fused[2] == default[2] == 3                  # one stream per layer: the adjacency's (torch's dropout draws none)
    assert fused[0] == default[0] and np.isfinite(fused[0])
    assert all(torch.equal(a, b) for a, b in zip(fused[1], default[1]))
    assert len(fused[1]) > 4 and any(float(g.abs().max()) > 0 for g in fused[1])
    both = one_step(gcnii_edge_dropout="fused", feature_dropout="fused", gcnii_backward="fused")      # CPU tensors: no switch applies
    assert both[0] == default[0] and both[2] == 3


# ---- the layer hands the keyword on where it applies, and draws today's streams ---------------------------------------------------------------
class OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda: what the layer looks at, without a device."""
    is_cuda = True


def on_device(t):
    return torch.Tensor._make_subclass(OnDevice, t)


def test_layer_passes_the_keyword_and_draws_todays_streams(monkeypatch):
    import gnntf
    from gnntf import graph_model, metrics, sparse
    cpu_world(monkeypatch)
    rows = on_device(torch.zeros(12, 8))
    assert rows.is_cuda and not torch.zeros(1).is_cuda
    calls = []

    def recorder(adj, H, H0, a, M, **kwargs):
        calls.append((adj, kwargs))
        return H

    monkeypatch.setattr(sparse, "gcnii_step", recorder)

    def layer_of(**option):
        model = stack(**option)
        layer = [l for l in model.layers() if isinstance(l, gnntf.GCNIILayer)][0]
        layer.H0.value = rows
        return model, layer

    def forward(model, layer, features=rows):
        del calls[:]
        first = model._mask_calls
        layer.__forward__(model, features)
        (adj, kwargs), = calls
        return adj, kwargs, model._mask_calls - first, first

    # "fused" with the fused feature mask: the adjacency's stream first, then the mask's -- two streams, as under "composed"
    model, layer = layer_of(gcnii_edge_dropout="fused", feature_dropout="fused", gcnii_backward="fused")
    assert model.is_training()
    adj, kwargs, drawn, first = forward(model, layer)
    assert isinstance(adj, sparse.DroppedAdjacency) and adj.stream_id == first and drawn == 2
    assert kwargs["edge_dropout"] == "fused" and kwargs["backward"] == "fused" and kwargs["relu"] is True
    assert kwargs["dropout"] == (0.6, metrics.current_seed(), first + 1)
    composed_model, composed_layer = layer_of(feature_dropout="fused", gcnii_backward="fused")
    adj, kwargs, drawn, first = forward(composed_model, composed_layer)
    assert isinstance(adj, sparse.DroppedAdjacency) and adj.stream_id == first and drawn == 2 and "edge_dropout" not in kwargs
    assert kwargs["dropout"] == (0.6, metrics.current_seed(), first + 1)
    # "fused" with torch's dropout: one stream, the keyword, no mask triple
    model, layer = layer_of(gcnii_edge_dropout="fused")
    monkeypatch.setattr(model, "dropout", lambda features, dropout=0.5: features)        # (torch's dropout of a tensor subclass is not the point)
    adj, kwargs, drawn, first = forward(model, layer)
    assert kwargs["edge_dropout"] == "fused" and "dropout" not in kwargs and drawn == 1 and adj.stream_id == first
    # the identity as activation applies too
    layer.activation = gnntf.linear
    assert forward(model, layer)[1]["edge_dropout"] == "fused"
    # ... and each of these keeps today's call: another activation, double rows, a tensor for ``a``, eval mode (a constant adjacency),
    # graph_dropout 0, the recomputed weight gradient, a subclass, a graph that cannot fuse its dropout (a materialised adjacency)
    layer.activation = torch.tanh
    assert "edge_dropout" not in forward(model, layer)[1]
    layer.activation = gnntf.relu
    assert "edge_dropout" not in forward(model, layer, on_device(torch.zeros(12, 8, dtype=torch.float64)))[1]
    layer.a = torch.tensor(0.1)
    assert "edge_dropout" not in forward(model, layer)[1]
    layer.a = A_MIX
    assert forward(model, layer)[1]["edge_dropout"] == "fused"
    model.training_mode(False)
    adj, kwargs, drawn, _ = forward(model, layer)
    assert not isinstance(adj, sparse.DroppedAdjacency) and "edge_dropout" not in kwargs and drawn == 0
    model.training_mode(True)
    layer.graph_dropout = 0
    assert "edge_dropout" not in forward(model, layer)[1]
    layer.graph_dropout = 0.5
    recomputed_model, recomputed_layer = layer_of(gcnii_edge_dropout="fused", gcnii_weight_gradient="recomputed")
    monkeypatch.setattr(recomputed_model, "dropout", lambda features, dropout=0.5: features)
    kwargs = forward(recomputed_model, recomputed_layer)[1]
    assert kwargs["weight_gradient"] == "recomputed" and "edge_dropout" not in kwargs
    materialised = sparse.Adjacency(CpuGraph(), torch.ones(40))
    monkeypatch.setattr(graph_model.GNN, "get_adjacency", lambda self, *a, **k: materialised)
    assert "edge_dropout" not in forward(model, layer)[1]

    class Mine(gnntf.GCNIILayer):
        pass
    layer.__class__ = Mine
    assert "edge_dropout" not in forward(model, layer)[1]


def test_host_function_keeps_the_composition_where_the_launch_does_not_apply(monkeypatch):
    """sparse.gcnii_step(edge_dropout="fused") itself: CPU tensors behind a DroppedAdjacency, a constant adjacency and
    weight_gradient="recomputed" are today's ops; device tensors behind a DroppedAdjacency go to the one autograd node."""
    from gnntf import sparse
    dense_adj = cpu_world(monkeypatch)
    rng = np.random.default_rng(8)
    H, H0 = (torch.from_numpy(rng.standard_normal((12, 8)).astype(np.float32)).requires_grad_() for _ in range(2))
    M = torch.from_numpy((np.eye(8) * 0.6 + rng.standard_normal((8, 8)) * 0.2).astype(np.float32))
    monkeypatch.setattr(sparse, "dense", lambda T, M, b, relu: torch.relu(T @ M) if relu else T @ M)
    monkeypatch.setattr(sparse._GCNIIStep, "apply", lambda *args: args)
    dropped = sparse.DroppedAdjacency(CpuGraph(), 0.5, 1, 0, D=torch.ones(12))
    want = torch.relu(((dense_adj @ H) * (1 - A_MIX) + H0 * A_MIX) @ M)
    assert torch.equal(sparse.gcnii_step(dropped, H, H0, A_MIX, M, edge_dropout="fused"), want)           # CPU tensors
    rows = [on_device(t).requires_grad_() for t in (H.detach(), H0.detach(), M)]
    assert torch.equal(sparse.gcnii_step(dropped, *rows[:2], A_MIX, rows[2]), want)                      # the default keyword
    assert torch.equal(sparse.gcnii_step(dropped, *rows[:2], A_MIX, rows[2], edge_dropout="fused", weight_gradient="recomputed"), want)
    node = sparse.gcnii_step(dropped, *rows[:2], A_MIX, rows[2], edge_dropout="fused", backward="fused")
    assert node[3] is dropped and node[6:] == ("fused", None, False, True)                                # (..., backward, dropout, recompute, fused_edge)
    node = sparse.gcnii_step(dropped, *rows[:2], A_MIX, rows[2], edge_dropout="fused", dropout=(0.6, 7, 2))
    assert node[3] is dropped and node[6:] == ("composed", (0.6, 7, 2), False, True)
    constant = sparse.Adjacency(CpuGraph())
    node = sparse.gcnii_step(constant, *rows[:2], A_MIX, rows[2], edge_dropout="fused")                   # a constant adjacency: today's node
    assert node[3] is constant and len(node) == 9
