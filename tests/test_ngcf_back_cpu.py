"""The fused NGCF backward (gnx_step_back_ngcf, sparse.ngcf_step(backward=), GNN(ngcf_backward=)) as far as it goes without a GPU: the
header declares the entry and the binding carries its argument types, the entry refuses bad arguments before it looks at a device, the
keywords refuse what they do not know, CPU tensors and width 128 keep today's calls whatever the keyword says while width 16 takes the
one launch, and the bounds of tests/ngcf_back_ref.py admit a float32 emulation of the entry's rounding points and reject two broken
backwards."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from abi_header import ctypes_of, prototype as header_prototype
import ngcf_back_ref as bref
import ngcf_fused_ref as nref
from test_gcn_fused_cpu import CpuGraph, OnDevice, tiny_graph
from test_ngcf_fused_cpu import cpu_world, one_step, structure

PROTOTYPE = ["gnx_graph_t g", "const float *d_vals_t", "const float *d_g", "int64_t ldg", "const float *d_y", "int64_t ldy", "const float *d_rnorm",
             "const uint32_t *d_gate", "int64_t C_out", "int act", "double dropout_p", "uint64_t seed", "uint64_t stream_id", "const float *d_X",
             "int64_t ldx", "const float *d_agg", "int64_t C_in", "const float *d_W1", "int64_t ldw1", "const float *d_W2", "int64_t ldw2",
             "float *d_G1", "float *d_G2", "int64_t ldG", "float *d_P", "float *d_db1", "float *d_db2", "float *d_dA", "float *d_R", "float *d_dX",
             "int64_t lddx", "float *d_work", "int64_t work_floats", "void *stream"]


def test_header_library_and_binding_agree():
    from gnntf import _native
    assert header_prototype("gnx_step_back_ngcf") == PROTOTYPE
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "gnx_step_back_ngcf")
    want = ctypes_of(PROTOTYPE)
    restype, argtypes = _native.SIGNATURES["gnx_step_back_ngcf"]
    assert restype is ctypes.c_int and argtypes == want
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION            # added within ABI 0.9: the number stays


def test_checks_that_need_no_device():
    """The NULL handle, a rate outside [0, 1), a width without the launch and C_out > C_in are refused before the handle (the one below
    is not one) or any buffer is looked at.  Every message names the entry and the cause."""
    from gnntf import _native
    lib = _native.lib()
    handle = ctypes.c_void_p(16)
    buf = [ctypes.c_void_p(256 * k) for k in range(1, 20)]

    def back(h=handle, C_out=16, C_in=16, act=2, rate=0.0):
        return lib.gnx_step_back_ngcf(h, buf[0], buf[1], 16, buf[2], 16, buf[3], buf[4], C_out, act, rate, 1, 2, buf[5], C_in, buf[6], C_in, buf[7],
                                      C_out, buf[8], C_out, buf[9], buf[10], 16, buf[11], buf[12], buf[13], buf[14], buf[15], buf[16], C_in, buf[17],
                                      1 << 20, None)

    for change, cause in ((dict(h=None), "NULL handle"), (dict(rate=1.0), "dropout rate 1 outside [0, 1)"),
                          (dict(rate=-0.1), "dropout rate -0.1 outside [0, 1)"), (dict(act=7), "invalid activation 7"),
                          (dict(C_in=48), "width 48 is not supported"), (dict(C_in=128, C_out=128), "width 128 is not supported"),
                          (dict(C_in=16, C_out=32), "C_out 32 > C_in 16"), (dict(C_out=0), "not in [1, 2^20]")):
        rc = back(**change)
        message = lib.gnx_last_error().decode()
        assert rc < 0 and message.startswith("gnx_step_back_ngcf: ") and cause in message, (cause, rc, message)


SHARED_FAULTS = (("d_g", None, "NULL g / G1 / G2 or a row stride below C_out"), ("ldg", 1, "NULL g / G1 / G2 or a row stride below C_out"),
                 ("d_y", None, "d_rnorm needs y"), ("d_gate", None, "relu / leaky_relu need d_gate"), ("d_X", None, "NULL X / agg, or ldx"),
                 ("ldx", 1, "NULL X / agg, or ldx 1 < C_in"), ("d_dA", None, "dX needs W1, W2, d_dA and d_R"), ("ldw1", 1, "ldw1 1 or ldw2"),
                 ("lddx", 1, "lddx 1 < C_in"), ("work_floats", -1, "work_floats -1 without d_work, or negative"),
                 ("d_work", None, "work_floats 5 without d_work, or negative"))


def test_both_backward_entries_answer_the_shared_argument_faults_alike():
    """One table of the argument faults that the two entries of this parameter list check with one piece of code, against
    gnx_step_back_ngcf at 16 -> 16 and gnx_step_back_wide_ngcf at 128 -> 128: each is refused, under the entry's own name and with the same
    cause, before the handle (the one below is not one) or any buffer is looked at."""
    from gnntf import _native
    lib = _native.lib()
    names = [arg.rsplit(" ", 1)[1].lstrip("*") for arg in PROTOTYPE]
    for entry, C in (("gnx_step_back_ngcf", 16), ("gnx_step_back_wide_ngcf", 128)):
        good = {name: ctypes.c_void_p(256 * (k + 1)) if "*" in arg else C for k, (name, arg) in enumerate(zip(names, PROTOTYPE))}
        good.update(g=ctypes.c_void_p(16), act=1, dropout_p=0.0, seed=1, stream_id=2, work_floats=5, stream=None)
        for name, value, cause in SHARED_FAULTS:
            assert name in good
            rc = getattr(lib, entry)(*[value if n == name else good[n] for n in names])
            message = lib.gnx_last_error().decode()
            assert rc < 0 and message.startswith(entry + ": ") and cause in message, (entry, name, rc, message)


def test_keywords_are_validated():
    import gnntf
    from gnntf import sparse
    assert sparse.NGCF_BACKWARDS == ("composed", "fused")
    assert callable(sparse._ngcf_back_launch)
    X = np.zeros((3, 4), dtype=np.float32)
    for make in (lambda **k: gnntf.GNN(tiny_graph(), X, **k), lambda **k: gnntf.NGCF(tiny_graph(), X, 2, **k)):
        with pytest.raises(Exception, match="ngcf_backward must be one of"):
            make(ngcf_backward="bogus")
        with pytest.raises(Exception, match="ngcf_backward must be one of"):
            make(ngcf_backward=True)
    with pytest.raises(Exception, match="ngcf_step: backward must be one of"):
        sparse.ngcf_step(None, None, None, None, None, None, backward="bogus")
    # the bias slabs: s = max(1, min(8192, ceil(ceil(n / 16) / 4))) and ceil(s / 64) group sums, 2 C_out floats each
    assert sparse._ngcf_back_work_floats(1547, 7) == (25 + 1) * 14 and sparse._ngcf_back_work_floats(1, 64) == 2 * 128
    assert sparse._ngcf_back_work_floats(5000, 16) == (79 + 2) * 32 and sparse._ngcf_back_work_floats(10_000_000, 64) == (8192 + 128) * 128


def test_cpu_tensors_keep_the_composed_ops(monkeypatch):
    from gnntf import sparse
    cpu_world(monkeypatch)
    monkeypatch.setattr(sparse, "_ngcf_back_launch", lambda *a, **k: pytest.fail("the fused backward ran"))
    fused = one_step(ngcf_layer="fused", ngcf_backward="fused", feature_dropout="fused")
    default = one_step()
    assert fused[0] == default[0] and np.isfinite(fused[0])
    assert all(torch.equal(a, b) for a, b in zip(fused[1], default[1]))
    assert len(fused[1]) == 12 and any(float(g.abs().max()) > 0 for g in fused[1])


TODAY = ["_ngcf_launch", "_ngcf_back_gate", "_dense_wgrad", "_dense_wgrad", "_dense_launch", "_dense_launch", "_launch"]


@pytest.mark.parametrize("C_in, C_out, how, want", [(128, 128, "fused", TODAY), (16, 7, "composed", TODAY), (24, 8, "fused", TODAY),
                                                    (16, 32, "fused", TODAY),
                                                    (16, 7, "fused", ["_ngcf_launch", "_ngcf_back_launch", "_dense_wgrad", "_dense_wgrad"])])
def test_what_the_node_calls(monkeypatch, C_in, C_out, how, want):
    """Over counting fakes of the launches: width 128, a width without the launch, a widening layer and backward="composed" make exactly
    today's calls in today's order; width 16 with backward="fused" is the one entry and the two weight gradients.  Either way the
    gradients are those of torch's autograd over the formula."""
    from gnntf import sparse
    dense_adj = cpu_world(monkeypatch)
    rng = np.random.default_rng(8)
    n = 12
    X, W1, W2 = (torch.from_numpy((rng.standard_normal(s) / 2).astype(np.float32)) for s in ((n, C_in), (C_in, C_out), (C_in, C_out)))
    b1, b2 = (torch.from_numpy(rng.uniform(-0.3, 0.3, size=(1, C_out)).astype(np.float32)) for _ in range(2))

    def formula(X, W1, b1, W2, b2):
        agg = dense_adj @ X
        u = sparse._ngcf_act((X * agg) @ W1 + b1, "leaky") + sparse._ngcf_act(agg @ W2 + b2, "leaky")
        return torch.nn.functional.normalize(u, dim=1, eps=1e-12)

    calls = []

    def recorded(name, fn):
        def wrapped(*args, **kwargs):
            calls.append(name)
            return fn(*args, **kwargs)
        monkeypatch.setattr(sparse, name, wrapped)

    def fake_launch(adj, X, W1, b1, W2, b2, activation, keep, dropout=None, normalize=True):
        agg = dense_adj @ X
        P1, P2 = (X * agg) @ W1 + b1, agg @ W2 + b2
        x = sparse._ngcf_act(P1, activation) + sparse._ngcf_act(P2, activation)
        r = 1 / x.norm(dim=1).clamp_min(1e-6)
        return (x * r[:, None]).detach(), agg.detach(), torch.stack([P1 > 0, P2 > 0]), r.detach()

    def fake_gate(graph, g, y, rnorm, gate, activation, dropout=None):
        gs = rnorm[:, None] * (g - y * (y * g).sum(dim=1, keepdim=True))
        slope = sparse.NGCF_SLOPES[activation]
        return gs * torch.where(gate[0], 1.0, slope), gs * torch.where(gate[1], 1.0, slope)

    def fake_back(adj, g, y, rnorm, gate, activation, dropout, X, A, W1, W2, want_P=True, want_db=(True, True), want_dX=True):
        assert want_P and want_db == (True, True) and want_dX
        G1, G2 = fake_gate(adj.graph, g, y, rnorm, gate, activation, dropout)
        Q1, Q2 = G1 @ W1.t(), G2 @ W2.t()
        dA, R = Q1 * X + Q2, Q1 * A
        return dict(G1=G1, G2=G2, P=X * A, db1=G1.sum(dim=0), db2=G2.sum(dim=0), dA=dA, R=R, dX=dense_adj.t() @ dA + R)

    recorded("_ngcf_launch", fake_launch)
    recorded("_ngcf_back_gate", fake_gate)
    recorded("_ngcf_back_launch", fake_back)
    recorded("_dense_wgrad", lambda T, G: T.t() @ G)
    recorded("_dense_launch", lambda G, Wt, b, relu: G @ Wt)
    recorded("_launch", lambda adj, T, H0, beta, alpha, act, transposed=False: dense_adj.t() @ T)
    upstream = torch.from_numpy(rng.standard_normal((n, C_out)).astype(np.float32))
    leaves = [torch.Tensor._make_subclass(OnDevice, t.clone()).requires_grad_() for t in (X, W1, b1, W2, b2)]
    out = sparse.ngcf_step(sparse.Adjacency(CpuGraph()), *leaves, activation="leaky", backward=how)
    assert calls == ["_ngcf_launch"]
    out.backward(upstream, retain_graph=True)
    assert calls == want, calls
    plain = [t.clone().requires_grad_() for t in (X, W1, b1, W2, b2)]
    formula(*plain).backward(upstream)
    for name, got, ref in zip(("X", "W1", "b1", "W2", "b2"), leaves, plain):
        assert got.grad.shape == ref.grad.shape and torch.allclose(got.grad, ref.grad, rtol=1e-4, atol=1e-5), name
    # the saved tensors stay: a second backward over the retained graph makes the same calls again
    first = [leaf.grad.clone() for leaf in leaves]
    for leaf in leaves:
        leaf.grad = None
    out.backward(upstream)
    assert calls == want + want[1:] and all(torch.equal(leaf.grad, g) for leaf, g in zip(leaves, first))


def test_the_model_passes_the_keyword_to_every_call(monkeypatch):
    """GNN(ngcf_backward="fused") reaches all three ngcf_step calls of a layer -- eval / no dropout, the mask in the launch, torch's dropout
    -- and the default names no ``backward`` at all: today's calls, argument for argument."""
    import gnntf
    from gnntf import graph_model, sparse
    cpu_world(monkeypatch)
    X = np.zeros((12, 16), dtype=np.float32)
    seen = []

    def fake(adj, X, W1, b1, W2, b2, **kwargs):
        seen.append(kwargs)
        return torch.ones(12, W1.shape[1])

    monkeypatch.setattr(sparse, "ngcf_step", fake)
    monkeypatch.setattr(graph_model.NGCFLayer, "_fused_ngcf", lambda self, gcn, features: True)
    for how in ("fused", None):
        option = dict() if how is None else dict(ngcf_backward=how)
        named = dict() if how is None else dict(backward=how)
        del seen[:]
        masked = gnntf.NGCF(CpuGraph(), X, 16, ngcf_layer="fused", feature_dropout="fused", dropout=0.25, **option)
        assert masked.ngcf_backward == (how or "composed")
        with masked:
            masked(masked.features)
        assert len(seen) == 3 and all(set(k) == {"activation", "dropout"} | set(named) and k.get("backward") == how for k in seen), seen
        del seen[:]
        masked.training_mode(False)
        masked(masked.features)
        assert seen == [dict(activation="leaky", **named)] * 3
        del seen[:]
        torch_drop = gnntf.NGCF(CpuGraph(), X, 16, ngcf_layer="fused", dropout=0.25, **option)
        with torch_drop:
            torch_drop(torch_drop.features)
        assert seen == [dict(activation="leaky", normalize=False, **named)] * 3


# ---- the bounds admit the entry's rounding points and reject two broken backwards ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def emulated(C_in, C_out, p):
    """Regime T: the float64 references with their bounds, and the float32 forward (numpy, library order) whose y, r and A . X a float32
    backward reads, with the gated gradients in float32 (every operation rounded once)."""
    c = structure("T")
    n = c["n"]
    f32 = np.float32
    op = nref.operands(n, C_in, C_out, 77 + C_in)
    mask = None if p == 0 else np.random.default_rng(78).random((n, C_out)) >= p
    keep = np.ones((n, C_out), dtype=bool) if mask is None else mask
    f = nref.forward_ref(c["A"], op["X"], op["W1"], op["b1"], op["W2"], op["b2"], "leaky", True, p, mask, L=c["L"])
    bit1, bit2 = f["P1"] > 0, f["P2"] > 0
    gated = nref.back_gate_ref(f, op["g"], bit1, bit2, "leaky", True, p, mask)
    want = nref.backward_ref(c["A"], f, op["X"], op["W1"], op["W2"], *gated, L=c["L"])
    agg = nref.spmm_f32(c["A32"], op["X"], "library", c["L"])
    want.update(bref.products_ref(op["X"], agg, op["W1"], op["W2"], *gated))
    M = (op["X"] * agg).astype(f32)
    act = lambda P: np.where(P > 0, P, (f32(0.2) * P).astype(f32)).astype(f32)
    x = ((act((M @ op["W1"] + op["b1"]).astype(f32)) + act((agg @ op["W2"] + op["b2"]).astype(f32))) * nref.scale(p) * keep).astype(f32)
    r = (f32(1) / np.sqrt(np.maximum((x * x).sum(axis=1, dtype=f32), f32(1e-12)), dtype=f32)).astype(f32)[:, None]
    y = (x * r).astype(f32)
    d = (y * op["g"]).sum(axis=1, dtype=f32)[:, None]
    gu = np.where(keep, (r * (op["g"] - y * d)).astype(f32) * nref.scale(p), f32(0)).astype(f32)
    G1 = np.where(bit1, gu, (gu * f32(0.2)).astype(f32)).astype(f32)
    G2 = np.where(bit2, gu, (gu * f32(0.2)).astype(f32)).astype(f32)
    return dict(c=c, op=op, want=want, agg=agg, G1=G1, G2=G2, At32=bref.transposed32(c["A32"]))


def judged(got, want, keys):
    out = dict()
    for key in keys:
        value = np.asarray(got[key])
        shape = (-1, value.shape[-1])
        bound = want["e_" + key] if "e_" + key in want else want[key + "_bound"]
        out[key] = nref.ratio(value.reshape(shape), want[key].reshape(shape), bound.reshape(shape))
    return out


@pytest.mark.parametrize("C_in, C_out, p", [(64, 7, 0.25), (16, 16, 0.0)])
def test_bounds_admit_the_float32_emulation(C_in, C_out, p):
    e = emulated(C_in, C_out, p)
    c, op, want = e["c"], e["op"], e["want"]
    got = bref.backward_f32(e["At32"], op["X"], e["agg"], op["W1"], op["W2"], e["G1"], e["G2"], c["L"])
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["P"], op["X"] * e["agg"])
    worst = judged(got, want, ("dA", "R", "db1", "db2", "dX"))
    for key, value in worst.items():
        print(f"T {C_in}->{C_out} p={p} {key}: float32 error / bound = {value:.3f}")
        assert value <= 1.0, key
    for rows in (c["info"]["hub"], c["info"]["empty"], c["info"]["ragged"]):
        for key in ("dA", "R", "dX"):
            bound = want["e_" + key] if key != "dX" else want["dX_bound"]
            assert nref.ratio(got[key], want[key], bound, rows) <= 1.0, key
    assert float(np.abs(got["dX"]).max()) > 0 and float(np.abs(got["R"]).max()) > 0


@pytest.mark.parametrize("C_in, C_out, p", [(64, 7, 0.25), (16, 16, 0.0)])
def test_bounds_reject_two_broken_backwards(C_in, C_out, p):
    """dX without R = Q1 * A, and dA without the product with X: both terms are of the gradient's own size, and the bound -- which carries
    the forward's error through the hub rows' weights -- is under a hundredth of it.  Measured on the CPU: the lost R is 271 (64 -> 7)
    and 144 (16 -> 16) times the bound, the lost product 246 and 144 times; the test asks for 10."""
    e = emulated(C_in, C_out, p)
    c, op, want = e["c"], e["op"], e["want"]
    for broken in (dict(with_R=False), dict(with_X=False)):
        got = bref.backward_f32(e["At32"], op["X"], e["agg"], op["W1"], op["W2"], e["G1"], e["G2"], c["L"], **broken)
        factor = nref.ratio(got["dX"], want["dX"], want["dX_bound"])
        print(f"T {C_in}->{C_out} {broken}: dX error / bound = {factor:.3g}")
        assert factor > 10, broken
