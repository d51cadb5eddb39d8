"""The GCNII weight gradient without stored mixed rows (gnx_gcnii_wgrad, gnx_gcnii_wgrad_bf16, gnx_gcnii_step_drop_bf16), as far as it
goes without a GPU: the header declares the three entries with their argument lists, the library exports them and gnntf/_native.py binds
them with the declared types, the options refuse what they do not know, and a "recomputed" model on CPU tensors keeps the CPU composition
and the bits of the "stored" one."""
import ctypes
import re

import numpy as np
import pytest
import torch

from abi_header import ctypes_of, prototype as header_prototype, text as header_text


WGRAD = ["gnx_graph_t g", "const float *d_vals", "const float *d_H", "const float *d_H0", "float a", "int64_t C", "const float *d_G",
         "float *d_dM", "float *d_hub_rows", "float *d_work", "int64_t work_floats", "void *stream"]
PROTOTYPES = {
    "gnx_gcnii_wgrad": WGRAD,
    "gnx_gcnii_wgrad_bf16": [arg if arg != "const float *d_H" else "const uint16_t *d_H" for arg in WGRAD],
    "gnx_gcnii_step_drop_bf16": [
        "gnx_graph_t g", "const float *d_vals", "const uint16_t *d_H", "const float *d_H0", "float a", "int64_t C", "const float *d_M",
        "int64_t ldm", "int act", "double dropout_p", "uint64_t seed", "uint64_t stream_id", "void *d_out", "int out_bf16", "float *d_work",
        "void *stream"],
}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_the_entry(name):
    assert header_prototype(name) == PROTOTYPES[name]
    text = header_text()
    for reported in ("gcnii_wgrad_mfma", "gcnii_wgrad_mfma_bf16", "spmm_gcnii_mfma_drop_bf16"):
        assert '"' + reported + '"' in text                                              # the reported names are documented
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


def test_checks_that_need_no_device():
    """A NULL handle is refused before anything touches a device."""
    from gnntf import _native
    lib = _native.lib()
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION
    assert lib.gnx_gcnii_wgrad(None, None, 16, 16, 0.1, 16, 16, 16, None, 16, 256, None) == -1
    assert b"gnx_gcnii_wgrad: NULL handle" in lib.gnx_last_error()
    assert lib.gnx_gcnii_wgrad_bf16(None, None, 16, 16, 0.1, 16, 16, 16, None, 16, 256, None) == -1
    assert b"gnx_gcnii_wgrad_bf16: NULL handle" in lib.gnx_last_error()
    assert lib.gnx_gcnii_step_drop_bf16(None, None, 16, 16, 0.1, 16, 16, 16, 1, 0.5, 1, 2, 16, 1, None, None) == -1
    assert b"gnx_gcnii_step_drop_bf16: NULL handle" in lib.gnx_last_error()
    assert lib.gnx_graph_hub_rows(None, None, None) == -1
    assert b"gnx_graph_hub_rows: NULL handle" in lib.gnx_last_error()


def tiny_graph():
    import gnntf
    coo = np.array([[0, 1], [1, 0], [1, 2], [2, 1]], dtype=np.int64)
    return gnntf.SparseCOO(coo, np.ones(len(coo), dtype=np.float32), (3, 3))


def test_unknown_weight_gradient_options_raise():
    import gnntf
    from gnntf import sparse
    assert sparse.GCNII_WEIGHT_GRADIENTS == ("stored", "recomputed")
    assert gnntf.gcnii_wgrad is sparse.gcnii_wgrad
    X = np.zeros((3, 4), dtype=np.float32)
    with pytest.raises(Exception, match="gcnii_weight_gradient must be one of"):
        gnntf.GNN(tiny_graph(), X, gcnii_weight_gradient="x")
    with pytest.raises(Exception, match="gcnii_weight_gradient must be one of"):
        gnntf.GCNII(tiny_graph(), X, 2, iterations=1, gcnii_weight_gradient="x")
    H, H0, M = torch.zeros(4, 16), torch.zeros(4, 16), torch.eye(16)
    with pytest.raises(Exception, match="gcnii_step: weight_gradient must be one of"):
        sparse.gcnii_step(None, H, H0, 0.1, M, weight_gradient="x")
    with pytest.raises(Exception, match="gcnii_train_run_bf16: weight_gradient must be one of"):
        sparse.gcnii_train_run_bf16(None, H, [(H0, 0.1, M, True, None)], weight_gradient="x")


def test_recomputed_model_on_cpu_tensors_gives_the_bits_of_stored(monkeypatch):
    """On CPU tensors the layer keeps its CPU composition whatever the switch says: the same seeds give the bits of the "stored" model and
    nothing of the library is called (a handle cannot exist without a GPU, so the graph handle is a stand-in the CPU path has no use for).
    Depends on the internals tests/test_gcnii_drop_cpu.py names: GNN.__init__ takes an instance of sparse.DeviceGraph as it is;
    GCNIILayer.__forward__ asks gcn.get_adjacency() for an Adjacency and, on CPU tensors, computes sparse.ppr_step + torch.matmul; every
    library call goes through _native.lib()."""
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

    def run(**option):
        gnntf.set_seed(3)
        torch.manual_seed(3)
        rng_w = np.random.default_rng(9)
        model = gnntf.GCNII(CpuGraph(), X, classes, latent_dims=[16], iterations=2, **option)
        model.reset()
        for layer in model.layers():
            if isinstance(layer, gnntf.GCNIILayer):
                layer.W.data.copy_(torch.from_numpy((rng_w.standard_normal((16, 16)) / 4).astype(np.float32)))
        with model:
            loss = gnntf.NodeClassification(nodes, labels).loss(model(model.features))
            loss.backward()
        return float(loss.detach()), [v.var.grad.clone() for v in model.vars()]

    loss_r, grads_r = run(gcnii_weight_gradient="recomputed")
    loss_s, grads_s = run()
    assert loss_r == loss_s and len(grads_r) == len(grads_s) > 0
    assert all(torch.equal(a, b) for a, b in zip(grads_r, grads_s))
    loss_b, grads_b = run(gcnii_weight_gradient="recomputed", gcnii_backward="fused", feature_dropout="fused",
                          gcnii_training_dtype=torch.bfloat16)
    assert loss_b == loss_s and all(torch.equal(a, b) for a, b in zip(grads_b, grads_s))
