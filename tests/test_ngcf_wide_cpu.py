"""The NGCF layer at width 128 (gnx_step_wide_ngcf, sparse.ngcf_step(wide=), GNN(ngcf_wide=)) as far as it goes without a GPU: the header
declares the entry and the binding carries its argument types, the entry answers a NULL handle, a width without the launch and misaligned
rows with the documented code and text before it looks at a device, the keywords refuse what they do not know, and -- over counting
fakes of the launches -- width 128 with both keywords takes the new entry once per layer while everything else makes exactly today's
calls.  Last, from the float64 reference alone: the operands of the GPU tests leave far less than 1 % of the gate bits undecided at
width 128, and the bounds admit a float32 evaluation there."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from abi_header import ctypes_of, prototype as header_prototype
import ngcf_fused_ref as nref
from test_gcn_fused_cpu import CpuGraph, OnDevice, tiny_graph
from test_ngcf_fused_cpu import PROTOTYPES, cpu_world, structure

NAME = "gnx_step_wide_ngcf"
UNSUPPORTED, INVALID = -4, -1


def test_header_library_and_binding_agree():
    """The parameter list is gnx_ngcf_step's, the symbol is exported and probed for, and the ABI number stays."""
    from gnntf import _native
    assert header_prototype(NAME) == PROTOTYPES["gnx_ngcf_step"]
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), NAME) and _native.has_symbol(NAME) and NAME in _native.PROBED
    want = ctypes_of(PROTOTYPES["gnx_ngcf_step"])
    assert _native.SIGNATURES[NAME] == (ctypes.c_int, want) == _native.SIGNATURES["gnx_ngcf_step"]
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION            # added within ABI 0.9: the number stays


def test_checks_that_need_no_device():
    """The NULL handle, a rate outside [0, 1), the widths without the launch and misaligned rows are answered before the handle (the one
    below is not one) or any buffer is looked at: nothing can have been launched.  Every message names the entry and the cause."""
    from gnntf import _native
    lib = _native.lib()
    handle = ctypes.c_void_p(16)
    buf = [ctypes.c_void_p(256 * k) for k in range(1, 12)]

    def step(h=handle, X=buf[0], ldx=128, C_in=128, C_out=128, rate=0.0, agg=buf[6], work=None, work_floats=0):
        return lib.gnx_step_wide_ngcf(h, None, X, ldx, C_in, buf[1], C_out, buf[2], C_out, C_out, buf[3], buf[4], 2, rate, 1, 2, 1, buf[5], C_out,
                                      agg, buf[7], buf[8], work, work_floats, None)

    for change, code, cause in ((dict(h=None), INVALID, "NULL handle"), (dict(rate=1.0), INVALID, "dropout rate 1 outside [0, 1)"),
                                (dict(C_out=0), INVALID, "not in [1, 2^20]"),
                                (dict(C_in=64, C_out=64, ldx=64), UNSUPPORTED, "widths 64 -> 64 are not supported"),
                                (dict(C_in=256, C_out=128, ldx=256), UNSUPPORTED, "widths 256 -> 128 are not supported"),
                                (dict(C_out=129), UNSUPPORTED, "widths 128 -> 129 are not supported"),
                                (dict(ldx=130), UNSUPPORTED, "misaligned rows (ldx 130"),
                                (dict(X=ctypes.c_void_p(260)), UNSUPPORTED, "misaligned rows"),
                                (dict(agg=ctypes.c_void_p(1028)), UNSUPPORTED, "misaligned rows"),
                                (dict(agg=None, work=ctypes.c_void_p(4104), work_floats=1 << 20), UNSUPPORTED, "misaligned rows")):
        rc = step(**change)
        message = lib.gnx_last_error().decode()
        assert rc == code and message.startswith(NAME + ": ") and cause in message, (cause, rc, message)
        assert code == INVALID or "keep gnx_ngcf_step elsewhere" in message


def test_keywords_are_validated():
    import gnntf
    from gnntf import sparse
    assert sparse.NGCF_WIDES == ("composed", "fused") and sparse.NGCF_WIDE_WIDTHS == (128,)
    X = np.zeros((3, 4), dtype=np.float32)
    for make in (lambda **k: gnntf.GNN(tiny_graph(), X, **k), lambda **k: gnntf.NGCF(tiny_graph(), X, 2, **k)):
        with pytest.raises(Exception, match="ngcf_wide must be one of"):
            make(ngcf_wide="bogus")
        with pytest.raises(Exception, match="ngcf_wide must be one of"):
            make(ngcf_wide=True)
    with pytest.raises(Exception, match="ngcf_step: wide must be one of"):
        sparse.ngcf_step(None, None, None, None, None, None, wide="bogus")


# ---- which entry a call takes ------------------------------------------------------------------------------------------------------------
class FakeLibrary:
    """Stands for the loaded library: both forward entries succeed without doing anything and are counted with their arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in ("gnx_ngcf_step", NAME):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class HubGraph(CpuGraph):
    handle = ctypes.c_void_p(16)
    n_hub_rows = 2


@pytest.fixture
def launches(monkeypatch):
    """sparse._ngcf_launch itself over a fake library, on CPU tensors that answer is_cuda."""
    from gnntf import _native, sparse
    fake = FakeLibrary()
    monkeypatch.setattr(_native, "lib", lambda: fake)
    monkeypatch.setattr(_native, "current_stream", lambda: None)
    monkeypatch.setattr(_native, "on_device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(sparse, "_same_device", lambda *a: None)
    return fake


def rows(n, C, ld=None):
    return torch.Tensor._make_subclass(OnDevice, torch.zeros(n, ld or C)[:, :C])


@pytest.mark.parametrize("C_in, C_out, ld, wide, keep, entry, floats", [
    (128, 128, None, "fused", True, NAME, 0), (128, 7, None, "fused", False, NAME, 12 * 128), (128, 128, 136, "fused", True, NAME, 0),
    (128, 128, None, "composed", True, "gnx_ngcf_step", 12 * 256), (64, 64, None, "fused", True, "gnx_ngcf_step", 2 * 128),
    (128, 128, 130, "fused", True, "gnx_ngcf_step", 12 * 256), (256, 128, None, "fused", False, "gnx_ngcf_step", 12 * 640)])
def test_which_entry_the_launch_takes(launches, C_in, C_out, ld, wide, keep, entry, floats):
    """wide="fused" at C_in = 128, C_out <= 128 over aligned rows is the new entry, with the scratch of the aggregated rows alone where
    they are not kept; the default, width 64, rows of stride 130 and width 256 are gnx_ngcf_step with today's arguments and scratch."""
    from gnntf import sparse
    X, W1, W2 = rows(12, C_in, ld), rows(C_in, C_out), rows(C_in, C_out)
    how = dict() if wide == "composed" else dict(wide=wide)
    out, agg, gate, rnorm = sparse._ngcf_launch(sparse.Adjacency(HubGraph()), X, W1, None, W2, None, "leaky", keep=keep, **how)
    (name, args), = launches.calls
    assert name == entry and len(args) == 25
    assert args[3:5] == (ld or C_in, C_in) and args[9] == C_out and args[12] == 2 and args[16] == 1 and args[23] == floats
    assert out.shape == (12, C_out) and (agg is not None) == keep and (gate is not None) == keep and (rnorm is not None) == keep


def test_a_library_without_the_symbol_is_an_error_not_a_fallback(launches, monkeypatch):
    from gnntf import _native, sparse
    monkeypatch.setattr(_native, "has_symbol", lambda name: False)
    with pytest.raises(Exception, match="needs gnx_step_wide_ngcf"):
        sparse._ngcf_launch(sparse.Adjacency(HubGraph()), rows(12, 128), rows(128, 128), None, rows(128, 128), None, "leaky", keep=False, wide="fused")
    assert launches.calls == []


def test_the_node_threads_the_keyword_and_keeps_its_backward(monkeypatch):
    """Under autograd wide="fused" reaches _ngcf_launch by name and the default names nothing (today's call, argument for argument);
    the backward at width 128 is the composed one whatever ``backward`` says."""
    from gnntf import sparse
    dense_adj = cpu_world(monkeypatch)
    seen, calls = [], []

    def fake_launch(adj, X, W1, b1, W2, b2, activation, keep, dropout=None, normalize=True, **more):
        seen.append(more)
        agg = dense_adj @ X
        P1, P2 = (X * agg) @ W1, agg @ W2
        x = sparse._ngcf_act(P1, activation) + sparse._ngcf_act(P2, activation)
        r = 1 / x.norm(dim=1).clamp_min(1e-6)
        return (x * r[:, None]).detach(), agg.detach(), torch.stack([P1 > 0, P2 > 0]), r.detach()

    def fake_gate(graph, g, y, rnorm, gate, activation, dropout=None):
        calls.append("_ngcf_back_gate")
        gs = rnorm[:, None] * (g - y * (y * g).sum(dim=1, keepdim=True))
        return gs * torch.where(gate[0], 1.0, 0.2), gs * torch.where(gate[1], 1.0, 0.2)

    monkeypatch.setattr(sparse, "_ngcf_launch", fake_launch)
    monkeypatch.setattr(sparse, "_ngcf_back_gate", fake_gate)
    monkeypatch.setattr(sparse, "_ngcf_back_launch", lambda *a, **k: pytest.fail("the fused backward has no launch at width 128"))
    monkeypatch.setattr(sparse, "_dense_wgrad", lambda T, G: T.t() @ G)
    monkeypatch.setattr(sparse, "_dense_launch", lambda G, Wt, b, relu: G @ Wt)
    monkeypatch.setattr(sparse, "_launch", lambda adj, T, H0, beta, alpha, act, transposed=False: dense_adj.t() @ T)
    rng = np.random.default_rng(8)
    X, W1, W2 = (torch.from_numpy((rng.standard_normal(s) / 4).astype(np.float32)) for s in ((12, 128), (128, 128), (128, 128)))
    on = lambda t: torch.Tensor._make_subclass(OnDevice, t.clone())
    for how, named in ((dict(wide="fused", backward="fused"), dict(wide="fused")), (dict(), dict()), (dict(wide="composed"), dict())):
        del seen[:], calls[:]
        leaves = [on(t).requires_grad_() for t in (X, W1, W2)]
        out = sparse.ngcf_step(sparse.Adjacency(CpuGraph()), leaves[0], leaves[1], None, leaves[2], None, **how)
        assert seen == [named]
        out.sum().backward()
        assert calls == ["_ngcf_back_gate"] and all(leaf.grad is not None for leaf in leaves)
    del seen[:]
    with torch.no_grad():
        sparse.ngcf_step(sparse.Adjacency(CpuGraph()), on(X), on(W1), None, on(W2), None, wide="fused")
    assert seen == [dict(wide="fused")]


def model_calls(monkeypatch, width, mutate=None, features=None, **option):
    """(the keyword arguments of every sparse.ngcf_step call, the width of every sparse.spmm call) of one eval-mode pass through the three
    layers of NGCF(num_classes=width) over device rows of that width; an spmm call is a layer on today's composed path."""
    import gnntf
    from gnntf import sparse
    cpu_world(monkeypatch)
    seen, composed = [], []
    spmm = sparse.spmm

    def fake(adj, X, W1, b1, W2, b2, **kwargs):
        seen.append(kwargs)
        return torch.ones(12, W1.shape[1])

    def counted(adj, X, storage=torch.float32):
        composed.append(X.shape[1])
        return spmm(adj, X)

    def dense(T, M, bias=None, relu=False):               # (the composed layer's transform of device rows, without a device)
        out = T.as_subclass(torch.Tensor) @ M + (bias if isinstance(bias, torch.Tensor) else 0)
        return torch.relu(out) if relu else out

    monkeypatch.setattr(sparse, "ngcf_step", fake)
    monkeypatch.setattr(sparse, "spmm", counted)
    monkeypatch.setattr(sparse, "dense", dense)
    model = gnntf.NGCF(CpuGraph(), np.zeros((12, width), dtype=np.float32), width, dropout=0.25, **option)
    layers = [l for l in model.layers() if isinstance(l, gnntf.NGCFLayer)]
    assert len(layers) == 3
    for layer in layers:
        if mutate is not None:
            mutate(layer)
    features = torch.Tensor._make_subclass(OnDevice, torch.zeros(12, width)) if features is None else features
    model.training_mode(False)
    with torch.no_grad():
        for layer in layers:                              # (layer by layer over the same rows: the fake's output is a plain CPU tensor)
            layer.__forward__(model, features)
    return seen, composed


def test_width_128_with_both_keywords_takes_the_new_entry_once_per_layer(monkeypatch):
    seen, composed = model_calls(monkeypatch, 128, ngcf_layer="fused", ngcf_wide="fused")
    assert seen == [dict(activation="leaky", wide="fused")] * 3 and composed == []


def test_the_three_call_shapes_carry_the_keyword(monkeypatch):
    """Eval mode, the mask in the launch, and torch's dropout behind normalize=False: wide="fused" stands in each at width 128 and in
    none at width 16, where the calls stay today's argument for argument."""
    import gnntf
    from gnntf import graph_model, sparse
    cpu_world(monkeypatch)
    seen = []

    def fake(adj, X, W1, b1, W2, b2, **kwargs):
        seen.append(kwargs)
        return torch.ones(12, W1.shape[1])

    monkeypatch.setattr(sparse, "ngcf_step", fake)
    monkeypatch.setattr(graph_model.NGCFLayer, "_fused_ngcf", lambda self, gcn, features: True)
    for width, named in ((128, dict(wide="fused")), (16, dict())):
        X = np.zeros((12, width), dtype=np.float32)
        del seen[:]
        masked = gnntf.NGCF(CpuGraph(), X, width, ngcf_layer="fused", ngcf_wide="fused", feature_dropout="fused", dropout=0.25)
        with masked:
            masked(masked.features)
        assert len(seen) == 3 and all(set(k) == {"activation", "dropout"} | set(named) and k.get("wide") == named.get("wide") for k in seen), seen
        del seen[:]
        masked.training_mode(False)
        masked(masked.features)
        assert seen == [dict(activation="leaky", **named)] * 3
        del seen[:]
        torch_drop = gnntf.NGCF(CpuGraph(), X, width, ngcf_layer="fused", ngcf_wide="fused", dropout=0.25)
        with torch_drop:
            torch_drop(torch_drop.features)
        assert seen == [dict(activation="leaky", normalize=False, **named)] * 3


def test_everything_else_makes_todays_calls(monkeypatch):
    """Width 128 with ngcf_layer="fused" alone, with ngcf_wide="fused" alone and with neither are the composed layer (no ngcf_step call,
    one spmm per layer); width 64 with both keywords is today's fused call without the keyword; a subclass, tanh, one bias without the
    other, an adjacency with a diagonal and CPU tensors at width 128 with both keywords are the composed layer."""
    import gnntf
    from gnntf import sparse
    both = dict(ngcf_layer="fused", ngcf_wide="fused")
    for option in (dict(ngcf_layer="fused"), dict(ngcf_wide="fused"), dict()):
        seen, composed = model_calls(monkeypatch, 128, **option)
        assert seen == [] and composed == [128] * 3, option
    seen, composed = model_calls(monkeypatch, 64, **both)
    assert seen == [dict(activation="leaky")] * 3 and composed == []

    class Mine(gnntf.NGCFLayer):
        pass

    def subclass(layer):
        layer.__class__ = Mine

    def tanh(layer):
        layer.activation = torch.tanh

    def one_bias(layer):
        layer.b1 = 0

    def diagonal(layer):
        layer.adjacency = sparse.Adjacency(CpuGraph(), None, torch.ones(12))

    for mutate in (subclass, tanh, one_bias, diagonal):
        seen, composed = model_calls(monkeypatch, 128, mutate=mutate, **both)
        assert seen == [] and composed == [128] * 3, mutate.__name__
    seen, composed = model_calls(monkeypatch, 128, features=torch.zeros(12, 128), **both)
    assert seen == [] and composed == [128] * 3


# ---- the reference at width 128: the gate bits it decides, and a float32 evaluation inside its bounds -------------------------------------
@pytest.mark.parametrize("C_out", [128, 100, 7])
def test_reference_decides_the_gate_bits_and_admits_float32(C_out):
    """Regime T with the operands of tests/test_gpu_ngcf_wide.py.  The derivation of tests/ngcf_fused_ref.py carries C_in as a number
    ((t + C_in + 8) u ..): nothing in it assumes C_in <= 64.  Measured: at most 0.020 % of the gate bits are undecided, against the cap of 1 % (asserted here: 0.1 %)."""
    c = structure("T")
    info = c["info"]
    op = nref.operands(c["n"], 128, C_out, 900 + 7 * 128 + C_out)
    for act in ("leaky", "relu"):
        full = nref.forward_ref(c["A"], op["X"], op["W1"], op["b1"], op["W2"], op["b2"], act, L=c["L"])
        d1, d2, share = nref.gate_share(full)
        print(f"T 128->{C_out} {act}: {share:.5%} of the gate bits are undecided by the float64 reference")
        assert share <= 1e-3 and d1[info["empty"]].all() and d2[info["empty"]].all()
    for normalize in (True, False):
        want = nref.forward_ref(c["A"], op["X"], op["W1"], op["b1"], op["W2"], op["b2"], "leaky", normalize, L=c["L"])
        got = nref.forward_f32(c["A32"], op["X"], op["W1"], op["b1"], op["W2"], op["b2"], "leaky", normalize, "library", c["L"])
        worst = nref.ratio(got["out"], want["out"], want["out_bound"])
        print(f"T 128->{C_out} normalize={normalize}: float32 error / bound = {worst:.3f}")
        assert worst <= 1.0
