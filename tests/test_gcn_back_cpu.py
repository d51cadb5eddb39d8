"""The fused GCNLayer backward (gnx_gcn_step_back, gnx_gcn_step_back_dropped, sparse.gcn_step_back, gcn_step(backward=),
GNN(gcn_backward=)) as far as it goes without a GPU: the header declares the two entries and the binding carries their argument types, the
entries refuse bad arguments before they look at a device, the keywords refuse what they do not know, CPU tensors and
``backward="composed"`` make today's calls, and ``dX_bound`` of tests/gcn_fused_ref.py admits the float32 emulations in the FUSED
association, (A^T G') W^T, and rejects a G' that lost its last column."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from abi_header import ctypes_of, prototype as header_prototype
import gcn_fused_ref as gref
from test_gcn_fused_cpu import CpuGraph, OnDevice, cpu_world, one_step, structure, tiny_graph


TAIL = ["const float *d_G", "int64_t ldg", "int64_t C_out", "const float *d_Wt", "int64_t ldwt", "int64_t C_in", "float *d_dX", "int64_t lddx",
        "float *d_work", "int64_t work_floats", "void *stream"]
PROTOTYPES = {
    "gnx_gcn_step_back": ["gnx_graph_t g", "const float *d_vals_t"] + TAIL,
    "gnx_gcn_step_back_dropped": ["gnx_graph_t g", "const float *d_D", "float edge_p", "uint64_t edge_seed", "uint64_t edge_stream"] + TAIL,
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
    """The NULL handle, NULL operands, the widths, the three row strides and work_floats are refused before the handle is dereferenced
    (the handle below is not one), and every message names its cause."""
    from gnntf import _native
    lib = _native.lib()
    handle, buf = ctypes.c_void_p(16), [ctypes.c_void_p(256 * k) for k in range(1, 5)]
    G, Wt, dX, work = buf

    def tail(G=G, ldg=8, C_out=7, Wt=Wt, ldwt=64, C_in=64, dX=dX, lddx=64, work=None, work_floats=0):
        return (G, ldg, C_out, Wt, ldwt, C_in, dX, lddx, work, work_floats, None)

    entries = (("gnx_gcn_step_back", lambda g, t: lib.gnx_gcn_step_back(g, None, *t)),
               ("gnx_gcn_step_back_dropped", lambda g, t: lib.gnx_gcn_step_back_dropped(g, buf[3], 0.5, 1, 0, *t)))
    for name, call in entries:
        for g, t, cause in ((None, tail(), "NULL handle"),
                            (handle, tail(G=None), "NULL G / Wt / dX"),
                            (handle, tail(Wt=None), "NULL G / Wt / dX"),
                            (handle, tail(dX=None), "NULL G / Wt / dX"),
                            (handle, tail(C_out=0), "widths 64 <- 0 not in [1, 2^20]"),
                            (handle, tail(C_in=(1 << 20) + 1, ldwt=1 << 21, lddx=1 << 21), "not in [1, 2^20]"),
                            (handle, tail(ldg=6), "ldg 6 < C_out 7"),
                            (handle, tail(ldwt=63), "ldwt 63 < C_in 64"),
                            (handle, tail(lddx=63), "lddx 63 < C_in 64"),
                            (handle, tail(work_floats=-1), "work_floats -1"),
                            (handle, tail(work_floats=100), "work_floats 100 without d_work"),
                            (handle, tail(dX=G), "dX must not alias an input"),
                            (handle, tail(dX=Wt), "dX must not alias an input"),
                            (handle, tail(work=G, work_floats=100), "d_work must be a buffer of its own"),
                            (handle, tail(work=dX, work_floats=100), "d_work must be a buffer of its own")):
            assert call(g, t) == -1, (name, cause)
            message = lib.gnx_last_error().decode()
            assert message.startswith(name + ": ") and cause in message, (name, cause, message)


def test_keywords_are_validated_and_the_function_is_exported():
    import gnntf
    from gnntf import sparse
    assert sparse.GCN_BACKWARDS == ("composed", "fused")
    assert gnntf.gcn_step_back is sparse.gcn_step_back
    X = np.zeros((3, 4), dtype=np.float32)
    for make in (lambda **k: gnntf.GNN(tiny_graph(), X, **k), lambda **k: gnntf.GCN(tiny_graph(), X, 2, **k)):
        with pytest.raises(Exception, match="gcn_backward must be one of"):
            make(gcn_backward="bogus")
        with pytest.raises(Exception, match="gcn_backward must be one of"):
            make(gcn_backward=True)
    with pytest.raises(Exception, match="gcn_step: backward must be one of"):
        sparse.gcn_step(None, None, None, backward="bogus")
    with pytest.raises(Exception, match="edge_dropout must be one of"):
        sparse.gcn_step_back(None, None, None, edge_dropout="bogus")


def test_cpu_tensors_keep_the_composed_ops(monkeypatch):
    """The model on CPU tensors: whatever gcn_backward says the step is the default's, bit for bit, and nothing reaches the library."""
    from gnntf import sparse
    cpu_world(monkeypatch)
    monkeypatch.setattr(sparse, "_gcn_back_launch", lambda *a, **k: pytest.fail("the fused backward ran"))
    default = one_step()
    for option in (dict(gcn_backward="fused"), dict(gcn_layer="fused", feature_dropout="fused", gcn_backward="fused"), dict(gcn_backward="composed")):
        got = one_step(**option)
        assert got[2] == default[2] == 0
        assert got[0] == default[0] and np.isfinite(got[0])
        assert all(torch.equal(a, b) for a, b in zip(got[1], default[1]))


def test_the_composed_backward_makes_todays_calls(monkeypatch):
    """_GCNStep.backward with backward="composed" (and without the keyword): the gate, gnx_dense_wgrad, gnx_dense over W^T and the
    transposed SpMM, in that order and nothing else; with "fused" the new launch stands where the last two stood."""
    from gnntf import sparse
    rng = np.random.default_rng(21)
    n, C_in, C_out = 12, 16, 7
    A = torch.from_numpy((rng.random((n, n)) < 0.3).astype(np.float32) / 4)
    X, W = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in ((n, C_in), (C_in, C_out)))
    bias = torch.from_numpy(rng.uniform(-0.3, 0.3, size=(1, C_out)).astype(np.float32))
    calls = []

    def recorded(name, fn):
        def wrapped(*args, **kwargs):
            calls.append(name)
            return fn(*args, **kwargs)
        monkeypatch.setattr(sparse, name, wrapped)

    recorded("_gcn_launch", lambda adj, X, W, b, relu, keep_agg, dropout=None, fused_edge=False: (torch.relu((A @ X) @ W + b), A @ X))
    recorded("_dense_wgrad", lambda T, G: T.t() @ G)
    recorded("_dense_launch", lambda G, Wt, b, relu: G @ Wt)
    recorded("_launch", lambda adj, T, H0, beta, alpha, act, transposed=False: A.t() @ T)
    recorded("_gcn_back_launch", lambda adj, G, Wt, fused_edge=False: (A.t() @ G) @ Wt)
    recorded("_feature_dropout_back", lambda *a, **k: pytest.fail("no mask was asked for"))
    adj = sparse.Adjacency(CpuGraph())
    grads = dict()
    for option in (dict(), dict(backward="composed"), dict(backward="fused")):
        leaves = [torch.Tensor._make_subclass(OnDevice, t.clone()).requires_grad_() for t in (X, W, bias)]
        del calls[:]
        out = sparse.gcn_step(adj, *leaves, relu=True, **option)
        out.backward(torch.ones_like(out))
        grads[option.get("backward", "default")] = [leaf.grad for leaf in leaves]
        if option.get("backward") == "fused":
            assert calls == ["_gcn_launch", "_dense_wgrad", "_gcn_back_launch"], calls
        else:
            assert calls == ["_gcn_launch", "_dense_wgrad", "_dense_launch", "_launch"], calls
    for a, b in zip(grads["default"], grads["composed"]):
        assert torch.equal(a, b)
    for name, a, b in zip("XWb", grads["composed"], grads["fused"]):
        assert torch.equal(a, b) if name != "X" else torch.allclose(a, b, rtol=1e-5, atol=1e-6)


# ---- dX_bound admits the float32 emulations in the fused association and rejects a lost column ---------------------------------------------
BOUND_CASES = [("T", 64, 64), ("T", 64, 40), ("T", 64, 7), ("T", 32, 1), ("T", 16, 16), ("S", 64, 40), ("S", 64, 7)]


@pytest.mark.parametrize("regime, C_in, C_out", BOUND_CASES)
def test_bound_admits_the_fused_association(regime, C_in, C_out):
    c = structure(regime)
    info = c["info"]
    op = gref.operands(c["n"], C_in, C_out, 3000 + C_in + C_out)
    agg32 = np.zeros((c["n"], C_in), dtype=np.float32)              # (dW is not judged here)
    G = np.asarray(op["G"], dtype=np.float32)
    want = gref.backward_ref(c["A"], agg32, G, op["W"], c["L"])
    assert np.isfinite(want["dX_bound"]).all()
    At32 = sp.csr_matrix(c["A32"].T)
    At32.sort_indices()
    Wt = np.ascontiguousarray(np.asarray(op["W"], dtype=np.float32).T)
    for order in ("library", "sequential", "chunked"):
        dX = gref.matmul_f32(gref.spmm_f32(At32, G, order, c["L"]), Wt, order)
        assert dX.dtype == np.float32
        worst = gref.ratio(dX, want["dX"], want["dX_bound"])
        print(f"{regime} {C_in}->{C_out} {order}: fused association, error / bound = {worst:.3f}")
        assert worst <= 1.0
        for rows in (info["hub"], info["empty"], info["ragged"]):
            assert len(rows) and gref.ratio(dX, want["dX"], want["dX_bound"], rows) <= 1.0
    lost = G.copy()
    lost[:, -1] = 0
    wrong = gref.backward_ref(c["A"], agg32, lost, op["W"], c["L"])["dX"]
    factor = gref.ratio(wrong, want["dX"], want["dX_bound"])
    print(f"{regime} {C_in}->{C_out}: a G' without its last column is {factor:.3g} x the bound")
    assert factor > 1e3
