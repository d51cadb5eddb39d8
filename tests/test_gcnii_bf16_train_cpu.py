"""bf16 row storage for GCNII training (gnx_gcnii_step_train_bf16, gnx_feature_dropout_back_bf16, gnx_gcnii_step_back_bf16,
sparse.gcnii_train_run_bf16, GNN(gcnii_training_dtype=)), as far as it goes without a GPU: the keyword refuses what it does not know,
the header declares the three entries, the library exports them and gnntf/_native.py binds them with the declared argument types, the
float64 emulation the GPU tests compare against is -- with its roundings switched off -- torch's float64 autograd of the dense layer
stack, and the model's run-eligibility predicate takes every fallback GNN.__init__ lists."""
import ctypes
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from abi_header import ctypes_of, prototype as header_prototype, text as header_text
import gcnii_bf16_train_ref as ref


PROTOTYPES = {
    "gnx_gcnii_step_train_bf16": [
        "gnx_graph_t g", "const float *d_vals", "const uint16_t *d_H", "const float *d_H0", "float a", "int64_t C", "const float *d_M",
        "int64_t ldm", "int act", "double dropout_p", "uint64_t seed", "uint64_t stream_id", "void *d_out", "int out_bf16",
        "float *d_mixed", "float *d_work", "void *stream"],
    "gnx_feature_dropout_back_bf16": [
        "gnx_graph_t g", "const float *d_g", "int64_t ldg", "const uint16_t *d_y", "int64_t ldy", "int64_t n_rows", "int64_t C",
        "double dropout_p", "uint64_t seed", "uint64_t stream_id", "int act", "float *d_G", "int64_t ldG", "uint16_t *d_Gb",
        "int64_t ldGb", "void *stream"],
    "gnx_gcnii_step_back_bf16": [
        "gnx_graph_t g", "const float *d_vals_t", "const uint16_t *d_Gb", "const float *d_G", "float a", "int64_t C", "const float *d_Mt",
        "int64_t ldmt", "float *d_dH", "const float *d_S_in", "float s_alpha", "float *d_S_out", "float *d_work", "void *stream"],
}


# ---- the keyword ---------------------------------------------------------------------------------------------------------------------
def tiny_graph():
    import gnntf
    coo = np.array([[0, 1], [1, 0], [1, 2], [2, 1]], dtype=np.int64)
    return gnntf.SparseCOO(coo, np.ones(len(coo), dtype=np.float32), (3, 3))


def test_unknown_gcnii_training_dtype_raises():
    import gnntf
    X = np.zeros((3, 4), dtype=np.float32)
    with pytest.raises(Exception, match="gcnii_training_dtype must be torch.float32 or torch.bfloat16"):
        gnntf.GNN(tiny_graph(), X, gcnii_training_dtype=torch.float16)
    with pytest.raises(Exception, match="gcnii_training_dtype"):
        gnntf.GCNII(tiny_graph(), X, 2, iterations=1, gcnii_training_dtype="bf16")


# ---- the three symbols ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_the_entry(name):
    assert header_prototype(name) == PROTOTYPES[name]
    text = header_text()
    assert "spmm_gcnii_mfma_train_bf16" in text and "spmm_gcnii_back_mfma_bf16" in text      # the reported names are documented
    assert re.search(r"#define\s+GNX_ABI_VERSION\s+900\b", text)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_library_exports_and_native_binds_the_entry(name):
    from gnntf import _native
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), name)
    restype, argtypes = _native.SIGNATURES[name]
    want = ctypes_of(header_prototype(name))
    assert restype is ctypes.c_int and argtypes == want
    fn = getattr(_native.lib(), name)
    assert fn.argtypes == want and fn.restype is ctypes.c_int
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION


def test_checks_that_need_no_device():
    """A NULL handle is refused before anything touches a device."""
    from gnntf import _native
    lib = _native.lib()
    assert lib.gnx_gcnii_step_train_bf16(None, None, 16, 16, 0.1, 16, 16, 16, 1, 0.5, 1, 2, 16, 1, 16, None, None) == -1
    assert b"gnx_gcnii_step_train_bf16: NULL handle" in lib.gnx_last_error()
    assert lib.gnx_feature_dropout_back_bf16(None, 16, 16, None, 0, 4, 16, 0.5, 1, 2, 0, 16, 16, 16, 16, None) == -1
    assert b"gnx_feature_dropout_back_bf16: NULL handle" in lib.gnx_last_error()
    assert lib.gnx_gcnii_step_back_bf16(None, None, 16, 16, 0.1, 16, 16, 16, 16, None, 1.0, 16, None, None) == -1
    assert b"gnx_gcnii_step_back_bf16: NULL handle" in lib.gnx_last_error()


def test_functional_layer_refuses_cpu_tensors():
    from gnntf import sparse

    class NoGraph:
        n_rows = n_cols = 4

    adj = sparse.Adjacency(NoGraph())
    H, M = torch.zeros(4, 16), torch.eye(16)
    with pytest.raises(Exception, match="GPU only"):
        sparse.gcnii_train_run_bf16(adj, H, [(H, 0.1, M, True, None)])
    with pytest.raises(Exception, match="no layers"):
        sparse.gcnii_train_run_bf16(adj, H, [])
    with pytest.raises(Exception, match="add_eye"):
        sparse.gcnii_train_run_bf16(sparse.Adjacency(NoGraph(), diag=torch.zeros(4)), H, [(H, 0.1, M, True, None)])


# ---- the emulation without its roundings is the float64 layer stack -------------------------------------------------------------------
def test_emulation_without_rounding_is_float64_autograd():
    """A 40-vertex directed graph, 4 layers of width 16: relu and identity, two layers with a mask, H0 shared by layers 0, 1 and 3 and
    another one at layer 2.  Output, dH, both dH0 sums and every dM to 1e-12."""
    n, C = 40, 16
    rng = np.random.default_rng(40)
    dense_A = (rng.random((n, n)) < 0.15) * rng.uniform(0.1, 0.6, size=(n, n))
    A = sp.csr_matrix(dense_A)
    H, H0a, H0b, up = (rng.standard_normal((n, C)) for _ in range(4))
    Ms = [0.6 * np.eye(C) + 0.4 * rng.standard_normal((C, C)) / np.sqrt(C) for _ in range(4)]
    masks = [ref.mask_scale(7, 3, 0.6, n, C), None, ref.mask_scale(7, 5, 0.25, n, C), None]
    assert 0 < (masks[0] == 0).mean() < 1 and set(np.unique(masks[0])) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(0.6)))}
    relus = [True, False, True, True]
    a = 0.1
    steps = [(key, {"a": H0a, "b": H0b}[key], a, M, relu, mask) for key, M, relu, mask in zip("aaba", Ms, relus, masks)]
    got = ref.run(A, H, steps, up, rnd=ref.identity, coef=np.float64)

    leaves = {name: torch.tensor(x, dtype=torch.float64, requires_grad=True) for name, x in (("H", H), ("a", H0a), ("b", H0b))}
    Mt = [torch.tensor(M, dtype=torch.float64, requires_grad=True) for M in Ms]
    At = torch.tensor(dense_A, dtype=torch.float64)
    X = leaves["H"]
    for (key, _, _, _, relu, mask), M in zip(steps, Mt):
        X = ((1 - a) * (At @ X) + a * leaves[key]) @ M
        X = torch.relu(X) if relu else X
        X = X * torch.tensor(mask) if mask is not None else X
    X.backward(torch.tensor(up))
    close = dict(rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["out"], X.detach().numpy(), **close)
    np.testing.assert_allclose(got["dH"], leaves["H"].grad.numpy(), **close)
    for key in "ab":
        np.testing.assert_allclose(got["dH0"][key], leaves[key].grad.numpy(), **close)
    for k in range(4):
        np.testing.assert_allclose(got["dM"][k], Mt[k].grad.numpy(), **close)
    assert float(np.abs(got["dH"]).max()) > 0 and float(np.abs(got["dH0"]["b"]).max()) > 0
    # and with them switched on it is another function: the roundings are really made
    rounded = ref.run(A, H, steps, up)
    assert 1e-4 < ref.rel_fro(rounded["out"], got["out"]) < 3e-2


# ---- the run-eligibility predicate ----------------------------------------------------------------------------------------------------
@pytest.fixture
def cpu_models(monkeypatch):
    """GCNII models over a stand-in graph handle (a handle cannot exist without a GPU; the predicate looks at the model alone).
    Depends on these internals: GNN.__init__ takes an instance of sparse.DeviceGraph as it is; the predicate asks gcn.get_adjacency()
    for an Adjacency and reads only its ``diag``."""
    import gnntf
    from gnntf import graph_model, sparse
    n = 12

    class CpuGraph:
        n_rows = n_cols = n

    monkeypatch.setattr(graph_model.GNN, "get_adjacency", lambda self, *args, **kwargs: sparse.Adjacency(self.graph))
    monkeypatch.setattr(graph_model.sparse, "DeviceGraph", type(CpuGraph()), raising=True)
    monkeypatch.setattr(sparse, "GCNII_BF16_TRAIN_MIN_ROWS", 0)
    monkeypatch.setattr(sparse, "GCNII_BF16_TRAIN_MIN_WIDTH", 16)
    X = np.zeros((n, 6), dtype=np.float32)

    def make(width=64, iterations=4, **option):
        option.setdefault("gcnii_training_dtype", torch.bfloat16)
        option.setdefault("feature_dropout", "fused")
        model = gnntf.GCNII(CpuGraph(), X, 3, latent_dims=[width], iterations=iterations, **option)
        convs = [layer for layer in model.layers() if isinstance(layer, gnntf.GCNIILayer)]
        convs[0].H0.value = torch.zeros(n, width)                   # what the pre-MLP leaves there in a forward
        return model, convs, model.layers().index(convs[0])

    return make


def run_of(model, convs, at, k=0):
    return convs[k]._bf16_train_run(model, model.layers(), at + k)


def test_eligible_run_and_every_fallback(cpu_models, monkeypatch):
    import gnntf
    from gnntf import graph_model, sparse
    model, convs, at = cpu_models()
    assert model.is_training() and run_of(model, convs, at) == convs                 # the whole stack is one run
    assert run_of(model, convs, at, k=2) == convs[2:] and run_of(model, convs, at, k=3) is None      # at least 2 layers
    for width in (16, 32):
        m, c, i = cpu_models(width=width)
        assert run_of(m, c, i) == c
    # dropout == 0 needs no fused dropout
    m, c, i = cpu_models(dropout=0, feature_dropout="torch")
    assert run_of(m, c, i) == c
    # the default dtype, torch dropout with a rate, eval mode, no grad, fuse_runs = False
    m, c, i = cpu_models(gcnii_training_dtype=torch.float32)
    assert run_of(m, c, i) is None
    m, c, i = cpu_models(training_dtype=torch.bfloat16, gcnii_training_dtype=torch.float32)       # the other keyword does not switch it on
    assert run_of(m, c, i) is None
    m, c, i = cpu_models(feature_dropout="torch")
    assert run_of(m, c, i) is None
    model.training_mode(False)
    assert run_of(model, convs, at) is None
    model.training_mode(True)
    with torch.no_grad():
        assert run_of(model, convs, at) is None
    model.fuse_runs = False
    assert run_of(model, convs, at) is None
    model.fuse_runs = True
    assert run_of(model, convs, at) == convs
    # a spectral-preserving stack, and one such layer inside a plain stack
    m, c, i = cpu_models(layer_type=gnntf.GCNIISpectralPreservingLayer)
    assert run_of(m, c, i) is None
    m, c, i = cpu_models()
    c[2].__class__ = gnntf.GCNIISpectralPreservingLayer
    assert run_of(m, c, i) == c[:2]
    # width 40, and width 16 below the width gate
    m, c, i = cpu_models(width=40)
    assert run_of(m, c, i) is None
    monkeypatch.setattr(sparse, "GCNII_BF16_TRAIN_MIN_WIDTH", 33)
    m, c, i = cpu_models(width=32)
    assert run_of(m, c, i) is None
    assert run_of(model, convs, at) == convs                                          # 64 stays inside
    # too few rows: the shipped gate on a 12-vertex graph
    monkeypatch.setattr(sparse, "GCNII_BF16_TRAIN_MIN_ROWS", sparse.BF16_TRAIN_MIN_ROWS)
    assert run_of(model, convs, at) is None
    monkeypatch.setattr(sparse, "GCNII_BF16_TRAIN_MIN_ROWS", 0)
    # mixed activations: relu and the identity share a run, any other activation ends it
    convs[1].activation = gnntf.linear
    assert run_of(model, convs, at) == convs
    convs[2].activation = graph_model.leaky_relu
    assert run_of(model, convs, at) == convs[:2] and run_of(model, convs, at, k=2) is None
    convs[2].activation = gnntf.relu
    # a layer whose H0 lies inside the run ends it (its H0's value would have to exist first)
    convs[0].value = torch.zeros(12, 64)
    convs[2].H0 = convs[0]
    assert run_of(model, convs, at) == convs[:2]
    convs[2].H0 = convs[1].H0
    # a tensor-valued a, a diagonal, edge dropout, a rate of 1
    convs[3].a = torch.tensor(0.1)
    assert run_of(model, convs, at) == convs[:3]
    convs[3].a = 0.1
    convs[3].graph_dropout = 0.5
    assert run_of(model, convs, at) == convs[:3]
    convs[3].graph_dropout = 0
    convs[1].dropout = 1.0
    assert run_of(model, convs, at) is None
    convs[1].dropout = 0.6
    monkeypatch.setattr(graph_model.GNN, "get_adjacency", lambda self, *a, **k: sparse.Adjacency(self.graph, diag=torch.zeros(12)))
    assert run_of(model, convs, at) is None


def test_no_mask_stream_is_drawn_by_the_predicate(cpu_models):
    model, convs, at = cpu_models()
    before = model._mask_calls
    assert run_of(model, convs, at) == convs and model._mask_calls == before
