"""The node signals at width 1 (csrc/gnx_signal.hip; PPRSweep, FastReg, APPNPReg, GCNIIReg) as far as they go without a GPU: the
gradient formula the backward kernel implements against central differences, the header's prototypes against the bindings, the argument
checks that run before anything touches a device, and the layer lists the two models build."""
import ctypes

import numpy as np
import pytest
import torch

from abi_header import ctypes_of, prototype as header_prototype
import signal_ref as ref


PROTOTYPES = {
    "gnx_signal_project": ["const float *d_X", "int64_t ldx", "int64_t n", "int64_t C", "const float *d_w", "int act", "float *d_out",
                           "void *stream"],
    "gnx_signal_spmv": ["gnx_graph_t g", "const float *d_vals", "int transposed", "const float *d_x", "const float *d_h0", "float beta",
                        "float alpha", "float *d_out", "void *stream"],
    "gnx_signal_ppr": ["gnx_graph_t g", "const float *d_vals", "const float *d_h0", "float a", "int K", "float *d_out", "float *d_work",
                       "void *stream"],
    "gnx_signal_smoothness": ["gnx_graph_t g", "const float *d_vals", "const float *d_f", "const float *d_colsum", "float *d_diff_out",
                              "float *d_sums_out", "float *d_work", "void *stream"],
    "gnx_signal_smoothness_back": ["gnx_graph_t g", "const float *d_vals_t", "const float *d_f", "const float *d_diff", "const float *d_colsum",
                                   "const float *d_sums", "const float *d_upstream", "float *d_gz_out", "void *stream"],
    # beyond the five of the feature's plan: FastReg's per-forward draw, from the counter RNG so that a captured step replays it
    "gnx_signal_uniform": ["gnx_graph_t g", "int64_t n", "float bound", "uint64_t seed", "uint64_t stream_id", "float *d_out", "void *stream"],
}


# ---- the gradient formula ------------------------------------------------------------------------------------------------------------------
def test_analytic_gradient_agrees_with_central_differences():
    """On a 12-node directed graph in float64: d lambda / dX and d lambda / dw of signal_ref.smoothness_f64 -- the formula of the BACK
    epilogue -- against central differences, to 1e-6 relative."""
    A = ref.directed_graph_12()
    rng = np.random.default_rng(2)
    X, w = rng.standard_normal((12, 5)), rng.uniform(-1, 1, size=5)
    D = A.sum(axis=0)
    assert (D == 0).any() and (A.sum(axis=1) == 0).any() and not np.allclose(A, A.T)
    for upstream in (1.0, -1.0, 0.37):
        got = ref.smoothness_f64(A, X, w, D, upstream)
        lam = lambda X_, w_: upstream * ref.smoothness_f64(A, X_, w_, D)["lam"]
        h = 1e-6
        dX = np.zeros_like(X)
        for i in range(X.shape[0]):
            for c in range(X.shape[1]):
                E = np.zeros_like(X)
                E[i, c] = h
                dX[i, c] = (lam(X + E, w) - lam(X - E, w)) / (2 * h)
        dw = np.array([(lam(X, w + h * e) - lam(X, w - h * e)) / (2 * h) for e in np.eye(5)])
        assert np.abs(got["dX"]).max() > 1e-3 and np.abs(got["dw"]).max() > 1e-3
        assert np.abs(got["dX"] - dX).max() <= 1e-6 * np.abs(dX).max()
        assert np.abs(got["dw"] - dw).max() <= 1e-6 * np.abs(dw).max()


def test_reference_bounds_admit_float32_and_see_a_dropped_term():
    """The bounds of signal_ref.smoothness_ref admit the same mathematics evaluated in float32 with numpy's own summation order, and a
    gradient with the lambda D f term dropped misses them by orders of magnitude."""
    import gcnii_shapes_ref as shapes
    coo, vals, shape, _ = shapes.regime_graph("T")
    A = ref.csr64(coo, vals, shape)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((shape[0], 7)).astype(np.float32)
    w = rng.uniform(-1, 1, size=7).astype(np.float32)
    D = np.asarray(A.sum(axis=0)).reshape(-1).astype(np.float32)
    want = ref.smoothness_ref(A, X, w, D, 512, 512)
    A32 = A.astype(np.float32)
    f = (np.float32(1) / (np.float32(1) + np.exp(-(X @ w)))).astype(np.float32)
    d = f - A32 @ f
    num, den = np.float32((d * d).sum()), np.float32((D * f * f).sum())
    lam = num / den
    gz = (np.float32(2) / den) * ((d - A32.T @ d) - lam * D * f) * f * (np.float32(1) - f)
    assert ref.ratio1(f, want["f"], want["f_bound"]) <= 1 and ref.ratio1(d, want["d"], want["d_bound"]) <= 1
    assert ref.ratio1(num, want["num"], want["num_bound"]) <= 1 and ref.ratio1(lam, want["lam"], want["lam_bound"]) <= 1
    assert ref.ratio1(gz, want["gz"], want["gz_bound"]) <= 1
    wrong = (np.float32(2) / den) * (d - A32.T @ d) * f * (np.float32(1) - f)
    assert ref.ratio1(wrong, want["gz"], want["gz_bound"]) > 100


def test_uniform_draw_is_the_default_initialiser_range():
    u = ref.uniform_draw(5, 3, 4096)
    assert u.dtype == np.float32 and -1 <= u.min() < -0.99 and 0.99 < u.max() < 1 and abs(float(u.mean())) < 0.05
    assert not np.array_equal(u, ref.uniform_draw(5, 4, 4096))


# ---- bindings --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_library_and_binding_agree(name):
    from gnntf import _native
    assert header_prototype(name) == PROTOTYPES[name]
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), name) and _native.has_symbol(name) and name in _native.PROBED
    restype, argtypes = _native.SIGNATURES[name]
    want = ctypes_of(header_prototype(name))
    assert restype is ctypes.c_int and argtypes == want
    fn = getattr(_native.lib(), name)
    assert fn.argtypes == want and fn.restype is ctypes.c_int
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION


def test_names_are_exported_from_the_package():
    import gnntf
    from gnntf import graph_model, sparse
    for name in ("PPRSweep", "FastReg", "APPNPReg", "GCNIIReg"):
        assert getattr(gnntf, name) is getattr(graph_model, name)
    for name in ("signal_ppr", "signal_spmv", "signal_project", "sweep", "smoothness"):
        assert getattr(gnntf, name) is getattr(sparse, name)


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_run_before_the_device():
    """What can be refused without a handle.  The NULL buffers, aliases and non-square graphs of the entries that look at their handle
    first need a real one: tests/test_gpu_signal.py::test_entries_refuse_null_buffers_and_aliases."""
    from gnntf import _native
    lib = _native.lib()
    p = 4096                                            # a non-NULL address nothing reads: every call below is refused first

    def refused(rc, prefix):
        message = lib.gnx_last_error()
        assert rc == -1 and message.startswith(prefix), (rc, message)

    # NULL handles
    refused(lib.gnx_signal_spmv(None, None, 0, p, None, 1.0, 0.0, p, None), b"gnx_signal_spmv: NULL handle")
    refused(lib.gnx_signal_ppr(None, None, None, 0.1, 10, p, p, None), b"gnx_signal_ppr: NULL handle")
    refused(lib.gnx_signal_smoothness(None, None, p, p, p, p, p, None), b"gnx_signal_smoothness: NULL handle")
    refused(lib.gnx_signal_smoothness_back(None, None, p, p, p, p, p, p, None), b"gnx_signal_smoothness_back: NULL handle")
    refused(lib.gnx_signal_uniform(None, 4, 1.0, 1, 2, p, None), b"gnx_signal_uniform: NULL handle")
    # K < 0
    refused(lib.gnx_signal_ppr(None, None, None, 0.1, -1, p, p, None), b"gnx_signal_ppr: negative iteration count")
    # the projection: C < 1, ldx < C, NULL buffers, an unknown act, a negative row count
    refused(lib.gnx_signal_project(p, 4, 8, 0, p, 1, p, None), b"gnx_signal_project: width")
    refused(lib.gnx_signal_project(p, 4, 8, -3, p, 1, p, None), b"gnx_signal_project: width")
    refused(lib.gnx_signal_project(p, 3, 8, 4, p, 1, p, None), b"gnx_signal_project: ldx")
    for args in ((None, 4, 8, 4, p, 1, p), (p, 4, 8, 4, None, 1, p), (p, 4, 8, 4, p, 1, None)):
        refused(lib.gnx_signal_project(*args, None), b"gnx_signal_project: NULL buffer")
    refused(lib.gnx_signal_project(p, 4, 8, 4, p, 2, p, None), b"gnx_signal_project: act")
    refused(lib.gnx_signal_project(p, 4, -1, 4, p, 1, p, None), b"gnx_signal_project: row count")
    assert lib.gnx_signal_project(None, 4, 0, 4, None, 1, None, None) == 0          # no rows: nothing to read


def test_functional_forms_refuse_cpu_tensors():
    from gnntf import sparse
    with pytest.raises(Exception, match="GPU only"):
        sparse.signal_project(torch.zeros(4, 3), torch.zeros(3))


# ---- model shapes ---------------------------------------------------------------------------------------------------------------------------
class CpuGraph:                                         # what GNN keeps as self.graph; never dereferenced on the paths below
    n_rows = n_cols = 12


@pytest.fixture
def cpu_models(monkeypatch):
    """Models over a stand-in graph handle (a handle cannot exist without a GPU), as tests/test_gcnii_drop_cpu.py builds them: GNN.__init__
    takes an instance of sparse.DeviceGraph as it is; on CPU tensors GCNIILayer / PPRIteration compute through sparse.ppr_step."""
    import gnntf
    from gnntf import graph_model, sparse
    n = CpuGraph.n_rows
    dense_adj = torch.from_numpy((np.random.default_rng(5).random((n, n)) < 0.3).astype(np.float32) / 4)
    monkeypatch.setattr(sparse, "ppr_step", lambda adj, H, H0, a: (dense_adj @ H) * (1 - a) + H0 * a)
    monkeypatch.setattr(graph_model.GNN, "get_adjacency", lambda self, *args, **kwargs: sparse.Adjacency(self.graph))
    monkeypatch.setattr(graph_model.sparse, "DeviceGraph", CpuGraph, raising=True)
    X = np.random.default_rng(6).standard_normal((n, 6)).astype(np.float32)
    return gnntf, X


def test_gcniireg_builds_the_reference_layer_list(cpu_models):
    gnntf, X = cpu_models
    model = gnntf.GCNIIReg(CpuGraph(), X, 3, latent_dims=[8, 8], iterations=3, dropout=0.4)
    layers = model.layers()
    kinds = [type(layer) for layer in layers]
    assert kinds == [gnntf.Dropout, gnntf.Dense, gnntf.Dense, gnntf.FastReg] + [gnntf.GCNIILayer] * 3 + [gnntf.Dense]
    n = CpuGraph.n_rows
    assert [tuple(layer.output_shape) for layer in layers] == [(n, 6), (n, 8), (n, 8), (n, 8)] + [(n, 8)] * 3 + [(n, 3)]
    fast = layers[3]
    assert fast.output_regularize == 1 and tuple(fast.output_shape) == tuple(layers[2].output_shape) and fast.internal_shape == (8, 1)
    assert all(layer.H0 is layers[2] for layer in layers[4:7]) and [layer.k for layer in layers[4:7]] == [0, 1, 2]
    assert all(layer.dropout == 0.4 and layer.graph_dropout == 0 and layer.activation is gnntf.relu for layer in layers[4:7])
    assert layers[1].dropout == 0.4 and layers[2].dropout == 0.4 and layers[7].dropout == 0
    # Dense W, b regularised except the last; the GCNII transforms follow convolution_regularization; FastReg owns no variable
    flags = [v.regularize for v in model.vars()]
    assert flags == [1.0, 1.0, 1.0, 1.0] + [1.0] * 3 + [0.0, 0.0] and fast.vars == set()
    plain = gnntf.GCNIIReg(CpuGraph(), X, 3, latent_dims=[8], iterations=2, convolution_regularization=False)
    assert [v.regularize for v in plain.vars()] == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    # two forwards: a fresh W each, and the variable list does not grow (the reference's leak is not reproduced)
    model.reset()
    before = len(model.vars())
    out = model(model.features)
    first = fast.W.clone()
    assert fast.value is layers[2].value and tuple(first.shape) == (8, 1) and float(first.abs().max()) <= 1.0
    model(model.features)
    assert tuple(out.shape) == (n, 3) and len(model.vars()) == before and not torch.equal(first, fast.W)
    assert not fast.W.requires_grad
    # an eval-mode forward draws nothing: ahead of any training-mode forward W is the reference's freshly created variable, zeros
    fresh = gnntf.GCNIIReg(CpuGraph(), X, 3, latent_dims=[8], iterations=2)
    fresh.reset()
    fresh.training_mode(False)
    state = torch.get_rng_state()
    fresh(fresh.features)
    assert torch.equal(torch.get_rng_state(), state) and fresh._mask_calls == 0
    assert tuple(fresh.layers()[2].W.shape) == (8, 1) and not fresh.layers()[2].W.any()
    fresh.training_mode(True)
    fresh(fresh.features)
    kept = fresh.layers()[2].W.clone()
    fresh.training_mode(False)
    fresh(fresh.features)
    assert kept.any() and torch.equal(fresh.layers()[2].W, kept)                        # an eval forward keeps the last draw


def test_appnpreg_builds_the_reference_layer_list(cpu_models):
    gnntf, X = cpu_models
    model = gnntf.APPNPReg(CpuGraph(), X, 4, latent_dims=[8], iterations=5, graph_dropout=0.3)
    layers = model.layers()
    assert [type(layer) for layer in layers] == [gnntf.Dense, gnntf.Dense] + [gnntf.PPRIteration] * 5
    assert isinstance(layers[0], gnntf.Dense) and layers[0].dropout == 0.6 and layers[0].activation is gnntf.relu
    n = CpuGraph.n_rows
    assert [tuple(layer.output_shape) for layer in layers] == [(n, 8)] + [(n, 4)] * 6
    assert all(layer.H0 is layers[1] and layer.restart_probability == 0.1 and layer.graph_dropout == 0.3 for layer in layers[2:])
    assert [v.regularize for v in model.vars()] == [1.0, 1.0, 0.0, 0.0]
    reference = gnntf.APPNP(CpuGraph(), X, 4, latent_dims=[8], iterations=5, graph_dropout=0.3)
    assert [type(layer) for layer in reference.layers()[1:]] == [type(layer) for layer in layers]      # APPNP without its leading Dropout
    model.reset()
    assert tuple(model(model.features).shape) == (n, 4)


def test_pprsweep_and_fastreg_layers_bind(cpu_models):
    gnntf, X = cpu_models
    model = gnntf.GNN(CpuGraph(), X)
    sweep = model.add(gnntf.PPRSweep(0.2))
    fast = model.add(gnntf.FastReg())
    assert sweep.restart_probability == 0.2 and tuple(sweep.output_shape) == X.shape and gnntf.PPRSweep.ITERATIONS == 10
    assert fast.output_regularize == 1 and tuple(fast.output_shape) == X.shape and fast.internal_shape == (6, 1)
    assert gnntf.PPRSweep().__dict__["_pending"] == ((), {})                          # the default restart probability is the layer's own
