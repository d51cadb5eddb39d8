"""The fused dropout around Dense (gnx_dense_drop, gnx_dense_wgrad_drop, sparse.dense_step, GNN(dense_dropout=)) as far as it goes
without a GPU: the bounds of tests/dense_drop_ref.py admit the float32 emulation of the stated rounding points and reject three planted
mistakes, the header declares the two entries and the binding carries their argument types, the entries refuse a NULL handle and bad
sizes under their own names without touching a device, the keyword refuses what it does not know, a model without the keyword -- or with
it on CPU tensors -- makes torch's calls, and the layers' predicate says no to every excluded case."""
import ctypes

import numpy as np
import pytest
import torch

from abi_header import ctypes_of, prototype as header_prototype
import dense_drop_ref as dref
from test_gcn_fused_cpu import CpuGraph, OnDevice, cpu_world, tiny_graph


IN, OUT = (0.5, 7, 2), (0.6, 7, 3)
PROTOTYPES = {
    "gnx_dense_drop": ["gnx_graph_t g", "const float *d_X", "int64_t ldx", "int64_t n", "int64_t F", "const float *d_W", "int64_t ldw", "int64_t O",
                       "const float *d_bias", "int act", "double in_p", "uint64_t in_seed", "uint64_t in_stream", "double out_p",
                       "uint64_t out_seed", "uint64_t out_stream", "float *d_out", "int64_t ldo", "void *stream"],
    "gnx_dense_wgrad_drop": ["gnx_graph_t g", "const float *d_X", "int64_t ldx", "const float *d_G", "int64_t ldg", "int64_t n", "int64_t F",
                             "int64_t O", "double in_p", "uint64_t in_seed", "uint64_t in_stream", "float *d_dW", "float *d_work",
                             "int64_t work_floats", "void *stream"],
}


# ---- the bounds ------------------------------------------------------------------------------------------------------------------------
def operands(n, F, O, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, F)).astype(np.float32)
    W = (rng.standard_normal((F, O)) / np.sqrt(F)).astype(np.float32)
    b = rng.uniform(0.2, 0.6, size=O).astype(np.float32)        # positive: a mask ahead of the bias leaves relu(b) != 0 behind
    return X, W, b


@pytest.mark.parametrize("relu", (True, False))
@pytest.mark.parametrize("din,dout", ((IN, OUT), (IN, None), (None, OUT), ((0.1, 3, 0), (0.9, 3, 1))))
def test_the_bound_admits_the_float32_emulation(relu, din, dout):
    X, W, b = operands(67, 100, 40)
    want = dref.forward(X, W, b, relu, din, dout, counter=5)
    got = dref.emulate(X, W, b, relu, din, dout, counter=5)
    worst = dref.ratio(got, want["out"], want["out_bound"])
    print(f"relu={relu} in={din} out={dout}: emulation error / bound = {worst:.3f}")
    assert worst <= 1
    assert np.array_equal(got == 0, want["out"] == 0) or relu          # without relu the zeros are the dropped elements, exactly
    # a second panel of outputs: the global column is the key
    X, W, b = operands(19, 36, 300, seed=1)
    want = dref.forward(X, W, b, relu, din, dout)
    assert dref.ratio(dref.emulate(X, W, b, relu, din, dout), want["out"], want["out_bound"]) <= 1


def test_the_bound_rejects_planted_mistakes():
    X, W, b = operands(19, 36, 300, seed=1)
    want = dref.forward(X, W, b, True, IN, OUT)
    for mistake in ("panel_column", "scale_after", "mask_first"):
        worst = dref.ratio(dref.emulate(X, W, b, True, IN, OUT, mistake=mistake), want["out"], want["out_bound"])
        print(f"{mistake}: error / bound = {worst:.3g}")
        assert worst > 1, mistake
    # the panel-local key is wrong in the second panel alone
    wrong = dref.emulate(X, W, b, True, IN, OUT, mistake="panel_column")
    assert dref.ratio(wrong[:, :256], want["out"][:, :256], want["out_bound"][:, :256]) <= 1
    # a moved counter is another mask
    assert not np.array_equal(dref.keep_mask(IN, 19, 36), dref.keep_mask(IN, 19, 36, counter=1))
    assert np.array_equal(dref.keep_mask(IN, 19, 36, counter=1), dref.keep_mask((IN[0], IN[1], IN[2] + 1), 19, 36))


def test_the_backward_bounds_admit_float32_sums():
    n, F, O = 300, 33, 5
    X, W, b = operands(n, F, O, seed=2)
    g = np.random.default_rng(3).standard_normal((n, O)).astype(np.float32)
    out = dref.emulate(X, W, b, True, IN, OUT)
    G = dref.gated(g, out, True, OUT)
    assert np.array_equal(G != 0, (out > 0) & dref.keep_mask(OUT, n, O) & (g != 0))
    want = dref.backward(X, W, G, IN)
    Xs = np.where(dref.keep_mask(IN, n, F), X * dref.scale(IN[0]), np.float32(0)).astype(np.float32)
    assert dref.ratio(Xs.T @ G, want["dW"], want["dW_bound"]) <= 1
    assert dref.ratio(G.sum(axis=0, dtype=np.float32), want["db"], want["db_bound"]) <= 1
    dX = np.where(dref.keep_mask(IN, n, F), (G @ W.T) * dref.scale(IN[0]), np.float32(0)).astype(np.float32)
    assert dref.ratio(dX, want["dX"], want["dX_bound"]) <= 1
    assert dref.ratio(X.T @ G, want["dW"], want["dW_bound"]) > 1            # the weight gradient over the undropped X is rejected


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_library_and_binding_agree(name):
    from gnntf import _native
    assert header_prototype(name) == PROTOTYPES[name]
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), name) and _native.has_symbol(name) and name in _native.PROBED
    want = ctypes_of(PROTOTYPES[name])
    restype, argtypes = _native.SIGNATURES[name]
    assert restype is ctypes.c_int and argtypes == want
    assert not name.startswith(("gnx_gcnii_", "gnx_gcn_", "gnx_ngcf_", "gnx_feature_dropout"))
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION


def test_argument_errors_need_no_device():
    """NULL handle, a rate outside [0, 1), bad sizes, short strides and NULL buffers are refused before anything is launched."""
    from gnntf import _native
    lib = _native.lib()
    handle = ctypes.c_void_p(16)                        # never dereferenced: the handle is read last, and every call below fails a check before that
    fwd = lambda g=handle, n=4, F=4, O=4, ldx=4, act=0, in_p=0.5, out_p=0.6: lib.gnx_dense_drop(
        g, None, ldx, n, F, None, 4, O, None, act, in_p, 1, 2, out_p, 1, 3, None, 4, None)
    for call, cause in ((lambda: fwd(g=None), b"NULL handle"), (lambda: fwd(in_p=1.0), b"dropout rate"), (lambda: fwd(out_p=-0.1), b"dropout rate"),
                        (lambda: fwd(F=0), b"bad sizes"), (lambda: fwd(n=-1), b"bad sizes"), (lambda: fwd(ldx=3), b"leading dimension"),
                        (lambda: fwd(act=7), b"invalid activation"), (lambda: fwd(), b"NULL pointer")):
        assert call() == -1
        message = lib.gnx_last_error()
        assert message.startswith(b"gnx_dense_drop: ") and cause in message, (cause, message)
    assert fwd(n=0) == 0                                # nothing to do: no pointer is looked at
    back = lambda g=handle, n=4, F=4, O=4, ldx=4, in_p=0.5, dW=None, work=0: lib.gnx_dense_wgrad_drop(
        g, None, ldx, None, 4, n, F, O, in_p, 1, 2, dW, None, work, None)
    out = ctypes.c_void_p(64)
    for call, cause in ((lambda: back(g=None), b"NULL handle"), (lambda: back(in_p=1.5), b"dropout rate"), (lambda: back(O=0), b"bad sizes"),
                        (lambda: back(ldx=2), b"leading dimension"), (lambda: back(), b"NULL output"), (lambda: back(dW=out), b"NULL input")):
        assert call() == -1
        message = lib.gnx_last_error()
        assert message.startswith(b"gnx_dense_wgrad_drop: ") and cause in message, (cause, message)


# ---- the keyword and the layers --------------------------------------------------------------------------------------------------------
def test_keyword_is_validated_and_the_function_is_exported():
    import gnntf
    from gnntf import sparse
    assert sparse.DENSE_DROPOUTS == ("torch", "fused")
    assert gnntf.dense_step is sparse.dense_step
    X = np.zeros((3, 4), dtype=np.float32)
    for make in (lambda **k: gnntf.GNN(tiny_graph(), X, **k), lambda **k: gnntf.APPNP(tiny_graph(), X, 2, **k),
                 lambda **k: gnntf.GCNII(tiny_graph(), X, 2, iterations=2, **k)):
        for bad in ("bogus", True, None, "composed"):
            with pytest.raises(Exception, match="dense_dropout must be one of"):
                make(dense_dropout=bad)
    with pytest.raises(Exception, match="dropout rate"):
        sparse.dense_step(None, None, None, in_dropout=(1.0, 0, 0))


def front_model(**option):
    """Dropout(0.5), Dense(8, relu, dropout=0.6), Dense(3) -- the front of APPNP (filter.py:30-33) -- on CPU tensors."""
    import gnntf
    rng = np.random.default_rng(6)
    X = rng.standard_normal((12, 16)).astype(np.float32)
    gnntf.set_seed(3)
    torch.manual_seed(3)
    model = gnntf.GNN(CpuGraph(), X, **option)
    model.add(gnntf.Dropout(0.5))
    model.add(gnntf.Dense(8, activation=gnntf.relu, dropout=0.6))
    model.add(gnntf.Dense(3, regularize=False))
    model.reset()
    return model, np.arange(0, 12, 2), rng.integers(0, 3, size=6)


def one_step(monkeypatch, **option):
    import gnntf
    model, nodes, labels = front_model(**option)
    calls, torch_dropout = [], torch.nn.functional.dropout
    monkeypatch.setattr(torch.nn.functional, "dropout", lambda x, p=0.5, training=True: (calls.append(float(p)), torch_dropout(x, p=p, training=training))[1])
    torch.manual_seed(4)
    with model:
        loss = gnntf.NodeClassification(nodes, labels).loss(model(model.features))
        loss.backward()
    monkeypatch.setattr(torch.nn.functional, "dropout", torch_dropout)
    return float(loss.detach()), [v.var.grad.clone() for v in model.vars()], model._mask_calls, calls


def test_default_and_cpu_tensors_make_torchs_calls(monkeypatch):
    from gnntf import sparse
    cpu_world(monkeypatch)
    for name in ("dense_step", "feature_dropout", "_dense_drop_launch"):
        monkeypatch.setattr(sparse, name, lambda *a, **k: pytest.fail("the counter-RNG path ran"))
    default = one_step(monkeypatch)
    named = one_step(monkeypatch, dense_dropout="torch")
    fused = one_step(monkeypatch, dense_dropout="fused", feature_dropout="fused")
    for run in (default, named, fused):
        assert run[3] == [0.5, 0.6] and run[2] == 0                 # torch's dropout twice, no counter-RNG stream taken
        assert run[0] == default[0] and np.isfinite(run[0])
        assert all(torch.equal(a, b) for a, b in zip(run[1], default[1]))
    assert len(default[1]) == 4 and all(float(g.abs().max()) > 0 for g in default[1])


def test_the_predicate(monkeypatch):
    """fused_dense_dropout says yes to float32 device rows in training mode at rates in (0, 1) on a GNN with the keyword, and no to each
    of: the default keyword, feature_dropout="fused" alone, eval mode, CPU tensors, float64 rows, SparseRows, rates of 0, 1 and above, a
    container without a graph handle; Dense._fusable says no to a subclass and to tanh."""
    import gnntf
    from gnntf import blocks, sparse
    cpu_world(monkeypatch)
    rows = torch.Tensor._make_subclass(OnDevice, torch.zeros(12, 16))
    fused, _, _ = front_model(dense_dropout="fused")
    assert fused.is_training() and blocks.fused_dense_dropout(fused, rows, 0.5) and blocks.fused_dense_dropout(fused, rows, 0.999)
    for rate in (0, 0.0, 1, 1.0, 1.5, -0.1, True, None):
        assert not blocks.fused_dense_dropout(fused, rows, rate), rate
    assert not blocks.fused_dense_dropout(fused, torch.zeros(12, 16), 0.5)                                        # CPU rows
    assert not blocks.fused_dense_dropout(fused, torch.Tensor._make_subclass(OnDevice, torch.zeros(12, 16, dtype=torch.float64)), 0.5)
    assert not blocks.fused_dense_dropout(fused, object.__new__(sparse.SparseRows), 0.5)
    for other in (front_model()[0], front_model(feature_dropout="fused")[0], front_model(dense_dropout="torch")[0]):
        assert not blocks.fused_dense_dropout(other, rows, 0.5)
    fused.training_mode(False)
    assert not blocks.fused_dense_dropout(fused, rows, 0.5)
    mlp = gnntf.MLP(np.zeros((12, 16), dtype=np.float32), 3)
    mlp.dense_dropout = "fused"                                     # even so: no graph handle, no dropout counter to read
    assert mlp.is_training() and not blocks.fused_dense_dropout(mlp, rows, 0.5)

    class MyDense(gnntf.Dense):
        pass

    holder = gnntf.GNN(CpuGraph(), np.zeros((12, 16), dtype=np.float32))
    assert holder.add(gnntf.Dense(4))._fusable() and holder.add(gnntf.Dense(4, activation=gnntf.relu))._fusable()
    assert not holder.add(MyDense(4))._fusable() and not holder.add(gnntf.Dense(4, activation=torch.tanh))._fusable()
