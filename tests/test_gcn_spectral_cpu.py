"""The fused GCNSpectralPreservingLayer (gnx_step_spectral_gcn, gnx_step_spectral_gcn_dropped, sparse.gcn_step_spectral,
GNN(gcn_spectral=)) as far as it goes without a GPU: the header declares the two entries and the binding carries their argument types,
the entries refuse a NULL handle under their own names, the keyword refuses what it does not know, the layer keeps today's ops on CPU
tensors whatever the switch says, the layer's predicate says no to every excluded case and to every layer without the keyword, the
gate-word helpers pack and unpack at the widths of the tests, the chosen operands leave at most AMBIGUOUS_SHARE of the gate undecided,
and the bound of tests/gcn_spectral_ref.py admits the float32 emulations of the stated rounding points."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from abi_header import ctypes_of, prototype as header_prototype, text as header_text
import gcn_spectral_ref as sref
from test_gcn_fused_cpu import CpuGraph, OnDevice, cpu_world, structure, tiny_graph


TAIL = ["const float *d_X", "int64_t ldx", "int64_t C_in", "const float *d_W", "int64_t ldw", "int64_t C_out", "const float *d_bias", "int act",
        "double dropout_p", "uint64_t seed", "uint64_t stream_id", "float *d_out", "int64_t ldo", "float *d_agg", "uint32_t *d_gate",
        "float *d_work", "void *stream"]
PROTOTYPES = {
    "gnx_step_spectral_gcn": ["gnx_graph_t g", "const float *d_vals"] + TAIL,
    "gnx_step_spectral_gcn_dropped": ["gnx_graph_t g", "const float *d_D", "float edge_p", "uint64_t edge_seed", "uint64_t edge_stream"] + TAIL,
}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_library_and_binding_agree(name):
    from gnntf import _native
    assert header_prototype(name) == PROTOTYPES[name]
    assert "gcn.py:92-105" in header_text()
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), name) and _native.has_symbol(name) and name in _native.PROBED
    want = ctypes_of(PROTOTYPES[name])
    restype, argtypes = _native.SIGNATURES[name]
    assert restype is ctypes.c_int and argtypes == want
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION


def test_null_handle_is_refused_under_each_entrys_own_name():
    """The NULL handle and a rate outside [0, 1) are refused before anything is dereferenced; the message names the entry."""
    from gnntf import _native
    lib = _native.lib()
    tail = (16, 16, 16, 16, 16, 8, None, 1, 0.5, 7, 3, 16, 8, None, None, None, None)
    assert lib.gnx_step_spectral_gcn(None, None, *tail) == -1
    assert lib.gnx_last_error() == b"gnx_step_spectral_gcn: NULL handle"
    assert lib.gnx_step_spectral_gcn_dropped(None, 16, 0.25, 11, 5, *tail) == -1
    assert lib.gnx_last_error() == b"gnx_step_spectral_gcn_dropped: NULL handle"
    handle = ctypes.c_void_p(16)                        # never dereferenced: the rate is checked first
    for rate in (1.0, -0.1):
        bad = tail[:8] + (rate,) + tail[9:]
        assert lib.gnx_step_spectral_gcn(handle, None, *bad) == -1
        assert b"gnx_step_spectral_gcn: dropout rate" in lib.gnx_last_error()
        assert lib.gnx_step_spectral_gcn_dropped(handle, 16, 0.5, 1, 0, *bad) == -1
        assert b"gnx_step_spectral_gcn_dropped: dropout rate" in lib.gnx_last_error()


def test_keyword_is_validated_and_the_function_is_exported():
    import gnntf
    from gnntf import sparse
    assert sparse.GCN_SPECTRALS == ("composed", "fused")
    assert gnntf.gcn_step_spectral is sparse.gcn_step_spectral
    X = np.zeros((3, 4), dtype=np.float32)
    for make in (lambda **k: gnntf.GNN(tiny_graph(), X, **k),
                 lambda **k: gnntf.GCN(tiny_graph(), X, 2, layer_type=gnntf.GCNSpectralPreservingLayer, **k)):
        with pytest.raises(Exception, match="gcn_spectral must be one of"):
            make(gcn_spectral="bogus")
        with pytest.raises(Exception, match="gcn_spectral must be one of"):
            make(gcn_spectral=True)
    with pytest.raises(Exception, match="edge_dropout must be one of"):
        sparse.gcn_step_spectral(None, None, None, edge_dropout="bogus")
    with pytest.raises(Exception, match="backward must be one of"):
        sparse.gcn_step_spectral(None, None, None, backward="bogus")


# ---- the layer keeps today's ops where the fused launch does not apply ---------------------------------------------------------------------
def one_step(**option):
    import gnntf
    rng = np.random.default_rng(6)
    X = rng.standard_normal((12, 16)).astype(np.float32)
    nodes, labels = np.arange(0, 12, 2), rng.integers(0, 3, size=6)
    gnntf.set_seed(3)
    torch.manual_seed(3)
    model = gnntf.GCN(CpuGraph(), X, 3, latent_dims=[16, 8], layer_type=gnntf.GCNSpectralPreservingLayer, **option)
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
    fused = one_step(gcn_spectral="fused", gcn_backward="fused")
    default = one_step()
    assert fused[2] == default[2] == 0                  # no counter-RNG stream was taken
    assert fused[0] == default[0] and np.isfinite(fused[0])
    assert all(torch.equal(a, b) for a, b in zip(fused[1], default[1]))
    assert len(fused[1]) == 6 and any(float(g.abs().max()) > 0 for g in fused[1])


def test_the_layer_predicate(monkeypatch):
    """_fused_spectral says yes to float32 device rows of width 16 / 32 / 64 with at most as many outputs under relu / the identity -- over
    a constant or a dropped adjacency, in either mode -- and no to each of: the default keyword (every layer), gcn_layer="fused" alone,
    CPU tensors, float64 rows, another input width, more outputs than inputs, an adjacency with a diagonal, tanh, transform_first, a
    rate of 1 in training mode, a subclass, the plain GCNLayer, a bf16 inference forward."""
    import gnntf
    from gnntf import sparse
    cpu_world(monkeypatch)
    X = np.zeros((12, 16), dtype=np.float32)

    def rows_of(width, dtype=torch.float32):
        return torch.Tensor._make_subclass(OnDevice, torch.zeros(12, width, dtype=dtype))

    rows = rows_of(16)

    def layer_of(layer_type=gnntf.GCNSpectralPreservingLayer, **option):
        model = gnntf.GCN(CpuGraph(), X, 3, latent_dims=[16], layer_type=layer_type, **option)
        return model, [l for l in model.layers() if isinstance(l, gnntf.GCNLayer)]

    constant = sparse.Adjacency(CpuGraph())
    dropped = sparse.DroppedAdjacency(CpuGraph(), 0.5, 1, 0, D=torch.ones(12))
    model, (first, last) = layer_of(gcn_spectral="fused")
    assert model.is_training() and first.W.shape == (16, 16) and last.W.shape == (16, 3) and first.dropout == 0.5
    for layer in (first, last):
        assert layer._fused_spectral(model, rows, constant) and layer._fused_spectral(model, rows, dropped)
    assert first._fused_spectral(model, rows_of(32), constant) and first._fused_spectral(model, rows_of(64), constant)
    for option in (dict(), dict(gcn_spectral="composed"), dict(gcn_layer="fused", gcn_backward="fused", feature_dropout="fused")):
        other, layers = layer_of(**option)
        assert other.gcn_spectral == "composed"
        assert not any(l._fused_spectral(other, rows, adj) for l in layers for adj in (constant, dropped))
        assert not any(l._fused_gcn(other, rows, constant) for l in layers)              # gcn_layer="fused" keeps ignoring this class
    assert not first._fused_spectral(model, torch.zeros(12, 16), constant)
    assert not first._fused_spectral(model, rows_of(16, torch.float64), constant)
    assert not first._fused_spectral(model, rows_of(24), constant) and not first._fused_spectral(model, rows_of(128), constant)
    wide = torch.nn.Parameter(torch.zeros(16, 17))
    keep, first.W = first.W, wide
    assert not first._fused_spectral(model, rows, constant)                             # outputs > C_in
    first.W = keep
    assert not first._fused_spectral(model, rows, sparse.Adjacency(CpuGraph(), None, torch.ones(12)))
    first.activation = torch.tanh
    assert not first._fused_spectral(model, rows, constant)
    first.activation = gnntf.linear
    assert first._fused_spectral(model, rows, constant)
    first.transform_first = True
    assert not first._fused_spectral(model, rows, constant)
    first.transform_first = False
    first.dropout = 1.0
    assert not first._fused_spectral(model, rows, constant)                             # a rate of 1 stays with torch in training mode
    model.training_mode(False)
    assert first._fused_spectral(model, rows, constant)                                 # ... and is not looked at in eval mode
    first.dropout = 0.5
    with torch.no_grad():
        assert first._fused_spectral(model, rows, constant)
        model.inference_dtype = torch.bfloat16
        assert not first._fused_spectral(model, rows, constant)                         # a bf16 inference forward keeps its path
    assert first._fused_spectral(model, rows, constant)                                 # ... and only that forward
    model.inference_dtype = torch.float32
    plain = layer_of(gnntf.GCNLayer, gcn_spectral="fused")
    assert not any(hasattr(l, "_fused_spectral") or l._fused_gcn(plain[0], rows, constant) for l in plain[1])

    class Mine(gnntf.GCNSpectralPreservingLayer):
        pass
    first.__class__ = Mine
    assert not first._fused_spectral(model, rows, constant)


def test_host_function_keeps_the_composed_ops(monkeypatch):
    """sparse.gcn_step_spectral itself: CPU tensors equal the layer's current forward; a DroppedAdjacency without edge_dropout="fused",
    a diagonal and a rate outside [0, 1) are today's ops."""
    from gnntf import sparse
    dense_adj = cpu_world(monkeypatch)
    rng = np.random.default_rng(8)
    X = torch.from_numpy(rng.standard_normal((12, 16)).astype(np.float32))
    W = torch.from_numpy((rng.standard_normal((16, 7)) / 4).astype(np.float32))
    bias = torch.from_numpy(rng.uniform(-0.3, 0.3, size=(1, 7)).astype(np.float32))

    def layer_forward(b, relu):                          # GCNSpectralPreservingLayer.__forward__ in eval mode (blocks.affine on CPU tensors)
        activated = (dense_adj @ X) @ W + b
        activated = torch.relu(activated) if relu else activated
        return 2 * (activated - b)

    for relu in (True, False):
        assert torch.equal(sparse.gcn_step_spectral(sparse.Adjacency(CpuGraph()), X, W, bias, relu=relu), layer_forward(bias, relu))
    assert torch.equal(sparse.gcn_step_spectral(sparse.Adjacency(CpuGraph()), X, W, None, relu=True), layer_forward(0, True))
    rows = [torch.Tensor._make_subclass(OnDevice, t) for t in (X, W, bias)]
    monkeypatch.setattr(sparse, "dense", lambda T, M, b, relu: torch.relu(T @ M + b) if relu else T @ M + b)
    want = layer_forward(bias, True)
    dropped = sparse.DroppedAdjacency(CpuGraph(), 0.5, 1, 0, D=torch.ones(12))
    assert torch.equal(sparse.gcn_step_spectral(dropped, *rows), want)
    assert torch.equal(sparse.gcn_step_spectral(sparse.Adjacency(CpuGraph(), None, torch.ones(12)), *rows), want)
    torch.manual_seed(1)
    got = sparse.gcn_step_spectral(sparse.Adjacency(CpuGraph()), *rows, dropout=(1.0, 7, 3))      # torch's dropout at rate 1: zeros
    assert got.shape == want.shape and not bool(got.any())


# ---- the gate words ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 7, 32, 33, 40, 64])
def test_gate_words_pack_and_unpack(C):
    rng = np.random.default_rng(C)
    bits = rng.random((37, C)) < 0.5
    words = sref.pack_gate(bits)
    assert words.dtype == np.int32 and words.shape == (37, sref.gate_words(C)) == (37, (C + 31) // 32)
    back, clear = sref.unpack_gate(words, C)
    assert clear and np.array_equal(back, bits)
    for c in (0, C - 1):                                  # bit c & 31 of word c >> 5
        one = np.zeros((1, C), dtype=bool)
        one[0, c] = True
        w = sref.pack_gate(one).view(np.uint32)
        assert w[0, c >> 5] == np.uint32(1) << np.uint32(c & 31) and int(w.astype(np.uint64).sum()) == 1 << (c & 31)
    if C % 32:
        dirty = words.copy().view(np.uint32)
        dirty[0, -1] |= np.uint32(1) << np.uint32(C % 32)
        assert not sref.unpack_gate(dirty, C)[1]


# ---- the operands' condition and the bound -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(regime, C_in, C_out, relu, with_bias, p):
    c = structure(regime)
    op = sref.operands(c["n"], C_in, C_out)
    mask = sref.keep(7, 2, p, c["n"], C_out) if p else None
    return sref.spectral_ref(c["A"], op["X"], op["W"], op["bias"] if with_bias else None, relu, p, mask, L=c["L"])


@pytest.mark.parametrize("regime, C_in, C_out", sref.CASES)
def test_operands_leave_the_gate_decided(regime, C_in, C_out):
    """The condition of the gate tests, on the float64 reference alone: at most AMBIGUOUS_SHARE of the elements lie inside the band
    |P'| <= P_bound, and both signs occur among the decided elements of the hub rows, the rows without entries and the ragged tile."""
    c = structure(regime)
    info = c["info"]
    want = reference(regime, C_in, C_out, True, True, 0.0)
    decided = np.abs(want["P"]) > want["P_bound"]
    share = 1.0 - decided.mean()
    print(f"{regime} {C_in}->{C_out}: undecided share {share:.2e}")
    assert share <= sref.AMBIGUOUS_SHARE
    assert sref.gate_check(want["P"] > 0, want["P"], want["P_bound"]) == (0, share)
    if C_out >= 2:
        for rows in (info["hub"], info["empty"], info["ragged"]):
            sign = (want["P"] > 0)[rows][decided[rows]]
            assert sign.any() and not sign.all()
    assert decided[info["empty"]].all()                  # P' = b exactly there, and the bias is drawn away from 0


@pytest.mark.parametrize("regime, C_in, C_out", [("T", 64, 64), ("T", 64, 40), ("T", 64, 7), ("T", 32, 1), ("T", 24, 24), ("S", 64, 40)])
def test_bound_admits_the_float32_emulations(regime, C_in, C_out):
    c = structure(regime)
    info = c["info"]
    op = sref.operands(c["n"], C_in, C_out)
    for relu in (True, False):
        for with_bias in (True, False):
            for p in sref.RATES:
                bias = op["bias"] if with_bias else None
                mask = sref.keep(7, 2, p, c["n"], C_out) if p else None
                want = reference(regime, C_in, C_out, relu, with_bias, p)
                assert np.isfinite(want["out_bound"]).all()
                for order in ("library", "sequential", "chunked"):
                    agg, P, out = sref.spectral_f32(c["A32"], op["X"], op["W"], bias, relu, order, c["L"], p, mask)
                    assert out.dtype == np.float32
                    worst = sref.ratio(out, want["out"], want["out_bound"])
                    worst_P = sref.ratio(P, want["P"], want["P_bound"])
                    assert worst <= 1.0 and worst_P <= 1.0, (relu, with_bias, p, order, worst, worst_P)
                    assert sref.ratio(agg, want["agg"], want["agg_bound"]) <= 1.0
                    for rows in (info["hub"], info["empty"], info["ragged"]):
                        assert len(rows) and sref.ratio(out, want["out"], want["out_bound"], rows) <= 1.0
                    if p:
                        assert not out[~mask].any() and not np.signbit(out[~mask]).any()          # dropped values are +0
                    if with_bias and relu:
                        wrong, share = sref.gate_check(P > 0, want["P"], want["P_bound"])
                        assert wrong == 0 and share <= sref.AMBIGUOUS_SHARE
    # a lost "- bias" is far outside the bound
    want = reference(regime, C_in, C_out, False, True, 0.0)
    assert sref.ratio(want["out"] + 2 * op["bias"][None, :], want["out"], want["out_bound"]) > 1e3


def test_backward_bound_admits_the_float32_emulations():
    import gcn_fused_ref as gref
    c = structure("T")
    C_in, C_out, p = 64, 40, 0.5
    op = sref.operands(c["n"], C_in, C_out)
    mask = sref.keep(7, 2, p, c["n"], C_out)
    agg32, P, _ = sref.spectral_f32(c["A32"], op["X"], op["W"], op["bias"], True, "sequential", c["L"], p, mask)
    G32, terms = sref.gate_pass_f32(op["G"], P > 0, p, mask)
    want = sref.backward_ref(c["A"], agg32, G32, terms, op["W"], L=c["L"])
    for order in ("library", "sequential", "chunked"):
        dX, dW, _ = gref.backward_f32(c["A32"], agg32, G32, op["W"], order, c["L"])
        db = terms.sum(axis=0, dtype=np.float32) if order == "library" else gref.matmul_f32(np.ones((1, len(terms)), dtype=np.float32), terms, order)[0]
        for name, got in (("dX", dX), ("dW", dW), ("db", db.reshape(1, -1))):
            worst = sref.ratio(got, want[name].reshape(got.shape), want[name + "_bound"].reshape(got.shape))
            print(f"{order} {name}: error / bound = {worst:.3f}")
            assert worst <= 1.0 and np.abs(got).max() > 0
    assert sref.saved_bytes(c["n"], C_in, C_out) == c["n"] * (4 * C_in + 8) + 4 * C_in * C_out      # 4 C_in + C_out / 8 per row, in whole words
