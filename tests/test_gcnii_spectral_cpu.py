"""The fused GCNIISpectralPreservingLayer (gnx_gcnii_step_spectral, gnx_gcnii_spectral_back, sparse.gcnii_step_spectral,
GNN(gcnii_spectral=)) as far as it goes without a GPU: the header declares the two entries and the binding carries their argument types,
the keyword refuses what it does not know, the layer keeps today's ops on CPU tensors, behind a DroppedAdjacency, with another activation
and at a rate of 1 whatever the switch says, a plain GCNIILayer stack does not notice the switch, and the bound of
tests/gcnii_spectral_ref.py admits the float32 emulations and leaves a small enough share of the gate undecided."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from abi_header import ctypes_of, prototype as header_prototype
import gcnii_shapes_ref as ref
import gcnii_spectral_ref as sref

A_MIX = 0.1
SEED, STREAM = 7, 2
CASES = [("T", 16), ("T", 32), ("T", 64), ("S", 64), ("T", 24)]          # the shapes of tests/test_gpu_gcnii_spectral.py

PROTOTYPES = {
    "gnx_gcnii_step_spectral": [
        "gnx_graph_t g", "const float *d_vals", "const float *d_H", "const float *d_H0", "float a", "int64_t C", "const float *d_M",
        "int64_t ldm", "const float *d_bias", "int act", "double dropout_p", "uint64_t seed", "uint64_t stream_id", "float *d_out",
        "float *d_mixed", "uint32_t *d_gate", "void *stream"],
    "gnx_gcnii_spectral_back": [
        "gnx_graph_t g", "const float *d_g", "int64_t ldg", "const uint32_t *d_gate", "int64_t n_rows", "int64_t C", "int act",
        "double dropout_p", "uint64_t seed", "uint64_t stream_id", "float *d_G", "int64_t ldG", "float *d_dbias", "float *d_work",
        "int64_t work_floats", "void *stream"],
}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_library_and_binding_agree(name):
    from gnntf import _native
    assert header_prototype(name) == PROTOTYPES[name]
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), name)
    want = ctypes_of(PROTOTYPES[name])
    restype, argtypes = _native.SIGNATURES[name]
    assert restype is ctypes.c_int and argtypes == want
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION


def test_checks_that_need_no_device():
    from gnntf import _native
    lib = _native.lib()
    assert lib.gnx_gcnii_step_spectral(None, None, 16, 16, 0.1, 16, 16, 16, 16, 1, 0.5, 1, 2, 16, None, None, None) == -1
    assert b"gnx_gcnii_step_spectral: NULL handle" in lib.gnx_last_error()
    assert lib.gnx_gcnii_spectral_back(None, 16, 16, 16, 4, 16, 1, 0.5, 1, 2, 16, 16, 16, 16, 16, None) == -1
    assert b"gnx_gcnii_spectral_back: NULL handle" in lib.gnx_last_error()


def tiny_graph():
    import gnntf
    coo = np.array([[0, 1], [1, 0], [1, 2], [2, 1]], dtype=np.int64)
    return gnntf.SparseCOO(coo, np.ones(len(coo), dtype=np.float32), (3, 3))


def test_keyword_is_validated_and_the_function_is_exported():
    import gnntf
    from gnntf import sparse
    assert sparse.GCNII_SPECTRALS == ("composed", "fused")
    assert gnntf.gcnii_step_spectral is sparse.gcnii_step_spectral
    X = np.zeros((3, 4), dtype=np.float32)
    for make in (lambda **k: gnntf.GNN(tiny_graph(), X, **k), lambda **k: gnntf.GCNII(tiny_graph(), X, 2, iterations=1, **k)):
        with pytest.raises(Exception, match="gcnii_spectral must be one of"):
            make(gcnii_spectral="bogus")
        with pytest.raises(Exception, match="gcnii_spectral must be one of"):
            make(gcnii_spectral=True)
    with pytest.raises(Exception, match="backward must be one of"):
        sparse.gcnii_step_spectral(None, None, None, 0.1, None, None, backward="bogus")


# ---- the layer keeps today's ops where the fused launch does not apply ---------------------------------------------------------------------
class CpuGraph:                                          # what GNN keeps as self.graph; never dereferenced on the CPU path
    n_rows = n_cols = 12


def cpu_world(monkeypatch):
    """A GCNII model on CPU tensors over a dense stand-in adjacency (the pattern of tests/test_gcnii_drop_cpu.py, with the internals it
    names); every launch of the spectral layer and every call into the library fails the test."""
    from gnntf import _native, graph_model, sparse
    rng = np.random.default_rng(5)
    dense_adj = torch.from_numpy((rng.random((12, 12)) < 0.3).astype(np.float32) / 4)
    monkeypatch.setattr(sparse, "ppr_step", lambda adj, H, H0, a: (dense_adj @ H) * (1 - a) + H0 * a)
    monkeypatch.setattr(graph_model.GNN, "get_adjacency", lambda self, *args, **kwargs: sparse.Adjacency(self.graph))
    monkeypatch.setattr(graph_model.sparse, "DeviceGraph", CpuGraph, raising=True)
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the CPU path called into the library"))
    monkeypatch.setattr(sparse, "_gcnii_spectral_launch", lambda *a, **k: pytest.fail("the fused launch ran"))
    return dense_adj


def one_step(layer_type, activation=None, dropout=0.6, **option):
    import gnntf
    rng = np.random.default_rng(6)
    X = rng.standard_normal((12, 6)).astype(np.float32)
    nodes, labels = np.arange(0, 12, 2), rng.integers(0, 3, size=6)
    gnntf.set_seed(3)
    torch.manual_seed(3)
    model = gnntf.GCNII(CpuGraph(), X, 3, latent_dims=[8], iterations=2, layer_type=layer_type, dropout=dropout, **option)
    model.reset()
    for layer in model.layers():
        if isinstance(layer, gnntf.GCNIILayer):
            layer.W.data.copy_(torch.from_numpy((rng.standard_normal((8, 8)) / 4).astype(np.float32)))
            if activation is not None:
                layer.activation = activation
            if hasattr(layer, "bias"):
                layer.bias.data.copy_(torch.from_numpy(rng.uniform(-0.3, 0.3, size=(1, 8)).astype(np.float32)))
    torch.manual_seed(4)
    with model:
        loss = gnntf.NodeClassification(nodes, labels).loss(model(model.features))
        loss.backward()
    return float(loss.detach()), [v.var.grad.clone() for v in model.vars()], model._mask_calls


@pytest.mark.parametrize("activation, dropout", [(None, 0.6), (torch.tanh, 0.6), (None, 1.0)])
def test_cpu_tensors_keep_the_composed_ops(monkeypatch, activation, dropout):
    import gnntf
    cpu_world(monkeypatch)
    fused = one_step(gnntf.GCNIISpectralPreservingLayer, activation, dropout, gcnii_spectral="fused")
    default = one_step(gnntf.GCNIISpectralPreservingLayer, activation, dropout)
    assert fused[2] == default[2] == 0                  # no counter-RNG stream was taken
    assert fused[0] == default[0] and np.isfinite(fused[0])
    assert all(torch.equal(a, b) for a, b in zip(fused[1], default[1]))
    assert len(fused[1]) > 4 and any(float(g.abs().max()) > 0 for g in fused[1])


def test_plain_stack_does_not_notice_the_switch(monkeypatch):
    import gnntf
    cpu_world(monkeypatch)
    fused, default = one_step(gnntf.GCNIILayer, gcnii_spectral="fused"), one_step(gnntf.GCNIILayer)
    assert fused[0] == default[0] and all(torch.equal(a, b) for a, b in zip(fused[1], default[1]))


class OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda: what the layer's predicate looks at, without a device."""
    is_cuda = True


def test_the_layer_predicate(monkeypatch):
    """_fused_spectral says yes to float32 device rows over a constant adjacency under relu / the identity, and no to each of: the
    default keyword, CPU tensors, a DroppedAdjacency, an adjacency with a diagonal, tanh, a rate of 1 in training mode, a subclass."""
    import gnntf
    from gnntf import sparse
    cpu_world(monkeypatch)
    X = np.zeros((12, 6), dtype=np.float32)
    rows = torch.Tensor._make_subclass(OnDevice, torch.zeros(12, 8))
    assert rows.is_cuda and not torch.zeros(1).is_cuda

    def layer_of(**option):
        model = gnntf.GCNII(CpuGraph(), X, 3, latent_dims=[8], iterations=1, layer_type=gnntf.GCNIISpectralPreservingLayer, **option)
        return model, [l for l in model.layers() if isinstance(l, gnntf.GCNIISpectralPreservingLayer)][0]

    constant = sparse.Adjacency(CpuGraph())
    model, layer = layer_of(gcnii_spectral="fused")
    assert model.is_training() and layer.dropout == 0.6
    assert layer._fused_spectral(model, rows, constant)
    assert not layer._fused_spectral(layer_of()[0], rows, constant)
    assert not layer._fused_spectral(model, torch.zeros(12, 8), constant)
    assert not layer._fused_spectral(model, rows.double(), constant)
    dropped = sparse.DroppedAdjacency(CpuGraph(), 0.5, 1, 0, D=torch.ones(12))
    assert not layer._fused_spectral(model, rows, dropped)
    assert not layer._fused_spectral(model, rows, sparse.Adjacency(CpuGraph(), None, torch.ones(12)))
    layer.activation = torch.tanh
    assert not layer._fused_spectral(model, rows, constant)
    layer.activation = gnntf.linear
    assert layer._fused_spectral(model, rows, constant)
    layer.dropout = 1.0
    assert not layer._fused_spectral(model, rows, constant)
    model.training_mode(False)
    assert layer._fused_spectral(model, rows, constant)     # eval mode: the dropout does not act
    layer.dropout = 0.6

    class Mine(gnntf.GCNIISpectralPreservingLayer):
        pass
    layer.__class__ = Mine
    assert not layer._fused_spectral(model, rows, constant)


def test_host_function_keeps_the_composed_ops(monkeypatch):
    """sparse.gcnii_step_spectral itself: CPU tensors, a DroppedAdjacency, a diagonal and a rate outside [0, 1) are today's ops."""
    from gnntf import sparse
    dense_adj = cpu_world(monkeypatch)
    rng = np.random.default_rng(8)
    H, H0 = (torch.from_numpy(rng.standard_normal((12, 8)).astype(np.float32)) for _ in range(2))
    M = torch.from_numpy((np.eye(8) * 0.6 + rng.standard_normal((8, 8)) * 0.2).astype(np.float32))
    bias = torch.from_numpy(rng.uniform(-0.3, 0.3, size=(1, 8)).astype(np.float32))
    T = (dense_adj @ H) * (1 - A_MIX) + H0 * A_MIX
    for relu in (True, False):
        activated = T @ M + bias
        want = 2 * ((torch.relu(activated) if relu else activated) - bias)
        got = sparse.gcnii_step_spectral(sparse.Adjacency(CpuGraph()), H, H0, A_MIX, M, bias, relu=relu)
        assert torch.equal(got, want)
    rows = [torch.Tensor._make_subclass(OnDevice, t) for t in (H, H0, M, bias)]
    monkeypatch.setattr(sparse, "dense", lambda T, M, b, relu: torch.relu(T @ M + b) if relu else T @ M + b)
    dropped = sparse.DroppedAdjacency(CpuGraph(), 0.5, 1, 0, D=torch.ones(12))
    want = 2 * (torch.relu(T @ M + bias) - bias)
    assert torch.equal(sparse.gcnii_step_spectral(dropped, *rows[:2], A_MIX, rows[2], rows[3]), want)
    with_diag = sparse.Adjacency(CpuGraph(), None, torch.ones(12))
    assert torch.equal(sparse.gcnii_step_spectral(with_diag, *rows[:2], A_MIX, rows[2], rows[3]), want)
    out = sparse.gcnii_step_spectral(sparse.Adjacency(CpuGraph()), *rows[:2], A_MIX, rows[2], rows[3], dropout=(1.0, SEED, STREAM))
    assert out.shape == want.shape and not bool((out != 0).any())             # torch's dropout at a rate of 1


# ---- the bound admits the float32 emulations; the gate's undecided share ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(regime, C):
    coo, vals, shape, info = ref.regime_graph(regime)
    n = shape[0]
    A64 = ref.csr_of(coo, vals, shape)
    d = np.asarray(A64.sum(axis=0)).ravel()
    scale = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    A32 = sp.csr_matrix(sp.diags(scale) @ A64 @ sp.diags(scale), dtype=np.float32)       # symmetric normalisation, rounded once
    A32.sort_indices()
    op = sref.operands(n, C, 1000 + C)
    return dict(n=n, A32=A32, A=sp.csr_matrix(A32, dtype=np.float64), op=op, info=info, L=info["L"])


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("regime, C", CASES)
def test_bound_admits_the_float32_emulations(regime, C, p):
    c = case(regime, C)
    op, n = c["op"], c["n"]
    mask = sref.keep(SEED, STREAM, p, n, C)
    info = c["info"]
    for relu in (True, False):
        want = sref.spectral_ref(c["A"], op["H"], op["H0"], op["M"], op["bias"], A_MIX, relu, p, mask, c["L"])
        assert np.isfinite(want["out_bound"]).all() and (want["out_bound"] > 0).all()
        for order in ("library", "sequential", "chunked"):
            if regime == "S" and order != "chunked" and not relu:
                continue                                 # (the large structure: every order once, the long-row order twice)
            T, P, out = sref.spectral_f32(c["A32"], op["H"], op["H0"], op["M"], op["bias"], A_MIX, relu, order, c["L"], p, mask)
            assert out.dtype == np.float32
            worst = ref.ratio(out, want["out"], want["out_bound"])
            print(f"{regime} C={C} p={p} relu={relu} {order}: error / bound = {worst:.3f}")
            assert worst <= 1.0
            for rows in (info["hub"], info["empty"], info["ragged"]):
                assert len(rows) and ref.ratio(out, want["out"], want["out_bound"], rows) <= 1.0
            assert ref.ratio(P, want["P"], want["P_bound"]) <= 1.0
            wrong, _ = sref.gate_check(P > 0, want["P"], want["P_bound"])
            assert wrong == 0                            # a float32 evaluation decides every decided element as float64 does
        # the bound discriminates: one ulp-scale slip per element of the size of a dropped bias rounding is far inside, a lost bias is not
        assert ref.ratio(want["out"] + 2 * float(sref.scale(p)) * op["bias"][None, :] * mask, want["out"], want["out_bound"]) > 1e3


@pytest.mark.parametrize("regime, C", CASES)
def test_undecided_share_of_the_gate(regime, C):
    c = case(regime, C)
    op = c["op"]
    want = sref.spectral_ref(c["A"], op["H"], op["H0"], op["M"], op["bias"], A_MIX, True, L=c["L"])
    _, share = sref.gate_check(want["P"] > 0, want["P"], want["P_bound"])
    print(f"{regime} C={C}: {share * want['P'].size:.0f} of {want['P'].size} elements undecided ({share:.2e})")
    assert share <= sref.AMBIGUOUS_SHARE


def test_gate_words_round_trip():
    rng = np.random.default_rng(3)
    for C in (16, 24, 32, 64, 70):
        bits = rng.random((37, C)) < 0.5
        words = sref.pack_gate(bits)
        assert words.dtype == np.int32 and words.shape == (37, (C + 31) // 32)
        back, pad_clear = sref.unpack_gate(words, C)
        assert pad_clear and np.array_equal(back, bits)
        assert bool(words[0, 0] & 1) == bool(bits[0, 0]) and bool((words.view(np.uint32)[0, 0] >> 5) & 1) == bool(bits[0, 5])
        if C > 32:
            assert bool(words.view(np.uint32)[0, 1] & 1) == bool(bits[0, 32])
