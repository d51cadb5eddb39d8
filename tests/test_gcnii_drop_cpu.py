"""The fused feature dropout of the GCNII training layer (gnx_gcnii_step_drop, gnx_feature_dropout, gnx_feature_dropout_back), as far as
it goes without a GPU: the header declares the three entries, the library exports them, gnntf/_native.py binds them with the declared
argument types, the ABI number did not move, the options refuse what they do not know, a "fused" model on CPU tensors trains through
torch's dropout, and the numpy mask the GPU tests compare against keeps the share of elements it should."""
import ctypes
import re

import numpy as np
import pytest
import torch

from abi_header import ctypes_of, prototype as header_prototype, text as header_text
from oracle import gnntf_oracle as orc


PROTOTYPES = {
    "gnx_gcnii_step_drop": [
        "gnx_graph_t g", "const float *d_vals", "const float *d_H", "const float *d_H0", "float a", "int64_t C", "const float *d_M",
        "int64_t ldm", "int act", "double dropout_p", "uint64_t seed", "uint64_t stream_id", "float *d_out", "float *d_mixed",
        "void *stream"],
    "gnx_feature_dropout": [
        "gnx_graph_t g", "const float *d_X", "int64_t ldx", "int64_t n_rows", "int64_t C", "const int32_t *d_rows", "double dropout_p",
        "uint64_t seed", "uint64_t stream_id", "float *d_out", "int64_t ldo", "void *stream"],
    "gnx_feature_dropout_back": [
        "gnx_graph_t g", "const float *d_g", "int64_t ldg", "const float *d_y", "int64_t ldy", "int64_t n_rows", "int64_t C",
        "double dropout_p", "uint64_t seed", "uint64_t stream_id", "int act", "float *d_G", "int64_t ldG", "void *stream"],
}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_the_entry(name):
    assert header_prototype(name) == PROTOTYPES[name]
    text = header_text()
    assert "spmm_gcnii_mfma_drop" in text and "spmm+dense_mfma_drop" in text           # the reported names are documented
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


def test_version_is_still_900():
    from gnntf import _native
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION


def test_checks_that_need_no_device():
    """A NULL handle is refused before anything touches a device."""
    from gnntf import _native
    lib = _native.lib()
    assert lib.gnx_gcnii_step_drop(None, None, 16, 16, 0.1, 16, 16, 16, 1, 0.5, 1, 2, 16, None, None) == -1
    assert b"gnx_gcnii_step_drop: NULL handle" in lib.gnx_last_error()
    assert lib.gnx_feature_dropout(None, 16, 16, 4, 16, None, 0.5, 1, 2, 16, 16, None) == -1
    assert b"gnx_feature_dropout: NULL handle" in lib.gnx_last_error()
    assert lib.gnx_feature_dropout_back(None, 16, 16, None, 0, 4, 16, 0.5, 1, 2, 0, 16, 16, None) == -1
    assert b"gnx_feature_dropout_back: NULL handle" in lib.gnx_last_error()


def tiny_graph():
    import gnntf
    coo = np.array([[0, 1], [1, 0], [1, 2], [2, 1]], dtype=np.int64)
    return gnntf.SparseCOO(coo, np.ones(len(coo), dtype=np.float32), (3, 3))


def test_unknown_feature_dropout_options_raise():
    import gnntf
    from gnntf import graph_model, sparse
    assert graph_model.FEATURE_DROPOUTS == ("torch", "fused")
    assert gnntf.feature_dropout is sparse.feature_dropout
    X = np.zeros((3, 4), dtype=np.float32)
    with pytest.raises(Exception, match="feature_dropout must be one of"):
        gnntf.GNN(tiny_graph(), X, feature_dropout="bogus")
    with pytest.raises(Exception, match="feature_dropout must be one of"):
        gnntf.GCNII(tiny_graph(), X, 2, iterations=1, feature_dropout="bogus")


def test_bf16_storage_with_dropout_raises():
    from gnntf import sparse
    H, H0, M = torch.zeros(4, 16), torch.zeros(4, 16), torch.eye(16)
    with pytest.raises(Exception, match="bf16 storage is inference only"):
        sparse.gcnii_step(None, H, H0, 0.1, M, storage=torch.bfloat16, dropout=(0.6, 7, 2))
    with pytest.raises(Exception, match="bf16 storage is inference only"):
        sparse.gcnii_step(None, H, H0, 0.1, M, storage=torch.bfloat16, dropout=(0.0, 7, 2))
    with pytest.raises(Exception, match=r"outside \[0, 1\)"):
        sparse.gcnii_step(None, H, H0, 0.1, M, dropout=(1.0, 7, 2))
    with pytest.raises(Exception, match="GPU only"):                                      # no CPU form of the pass exists
        sparse.feature_dropout(None, H, 0.6, 7, 2)


def test_fused_model_on_cpu_tensors_trains_through_torch_dropout(monkeypatch):
    """On CPU tensors the layer keeps its CPU composition and torch's dropout whatever the switch says: the same seeds give the bits
    of the "torch" model, no mask stream is taken, and nothing of the library is called (a handle cannot exist without a GPU, so the
    graph handle is a stand-in the CPU path has no use for).
    Depends on these internals, and has to follow them if they move: GNN.__init__ takes an instance of sparse.DeviceGraph as it is;
    GCNIILayer.__forward__ asks gcn.get_adjacency() for an Adjacency and, on CPU tensors, computes sparse.ppr_step + torch.matmul
    and calls gcn.dropout, which goes through torch.nn.functional.dropout; every library call goes through _native.lib()."""
    import gnntf
    from gnntf import _native, graph_model, sparse
    n, classes = 12, 3
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, 6)).astype(np.float32)
    nodes, labels = np.arange(0, n, 2), rng.integers(0, classes, size=n // 2)
    dense_adj = torch.from_numpy((rng.random((n, n)) < 0.3).astype(np.float32) / 4)

    class CpuGraph:                                     # what GNN keeps as self.graph; never dereferenced on this path
        n_rows = n_cols = n

    monkeypatch.setattr(sparse, "ppr_step", lambda adj, H, H0, a: (dense_adj @ H) * (1 - a) + H0 * a)
    monkeypatch.setattr(graph_model.GNN, "get_adjacency", lambda self, *args, **kwargs: sparse.Adjacency(self.graph))
    monkeypatch.setattr(graph_model.sparse, "DeviceGraph", type(CpuGraph()), raising=True)
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the CPU path called into the library"))
    dropout_calls = []
    real_dropout = torch.nn.functional.dropout
    monkeypatch.setattr(torch.nn.functional, "dropout", lambda *a, **k: (dropout_calls.append(1), real_dropout(*a, **k))[1])

    def run(**option):
        gnntf.set_seed(3)
        torch.manual_seed(3)
        model = gnntf.GCNII(CpuGraph(), X, classes, latent_dims=[8], iterations=2, **option)
        model.reset()
        for layer in model.layers():
            if isinstance(layer, gnntf.GCNIILayer):
                layer.W.data.copy_(torch.from_numpy((rng_w.standard_normal((8, 8)) / 4).astype(np.float32)))
        before = len(dropout_calls)
        with model:
            loss = gnntf.NodeClassification(nodes, labels).loss(model(model.features))
            loss.backward()
        return float(loss.detach()), [v.var.grad.clone() for v in model.vars()], model._mask_calls, len(dropout_calls) - before

    rng_w = np.random.default_rng(9)
    loss_f, grads_f, masks_f, calls_f = run(feature_dropout="fused")
    rng_w = np.random.default_rng(9)
    loss_t, grads_t, masks_t, calls_t = run()
    assert calls_f == calls_t == 3                      # the Dropout layer and the two GCNII layers, through torch
    assert masks_f == masks_t == 0                      # no counter-RNG stream was taken
    assert loss_f == loss_t and all(torch.equal(a, b) for a, b in zip(grads_f, grads_t))


def test_numpy_mask_keeps_the_share_it_should():
    """The mask the GPU tests build in numpy, pinned: for (seed 7, stream 2, p 0.6) over [3000, 64] the kept share lies within 4 standard
    deviations of 0.4 (sqrt(0.4 * 0.6 / 192000) = 0.00112: +-0.0045); another stream is another mask; the scale is the f32 one."""
    n, C, p = 3000, 64, 0.6
    rows, cols = np.repeat(np.arange(n), C), np.tile(np.arange(C), n)
    keep = orc.hash_u24(7, 2, rows, cols, np.zeros(n * C, dtype=np.int64)) >= orc.dropout_threshold(p)
    assert orc.dropout_threshold(p) == 10066329
    assert abs(keep.mean() - 0.4) <= 0.0045
    per_column = keep.reshape(n, C).mean(axis=0)
    assert np.abs(per_column - 0.4).max() <= 5 * np.sqrt(0.24 / n)                        # no column is special
    other = orc.hash_u24(7, 3, rows, cols, np.zeros(n * C, dtype=np.int64)) >= orc.dropout_threshold(p)
    assert 0.2 < (keep != other).mean() < 0.8
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert scale.dtype == np.float32 and scale == np.float32(2.5000002)
