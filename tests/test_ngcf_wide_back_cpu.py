"""The NGCF backward at width 128 (gnx_step_back_wide_ngcf, sparse.ngcf_step(wide_backward=), GNN(ngcf_wide_backward=)) as far as it goes
without a GPU: the header declares the entry with gnx_step_back_ngcf's parameter list and the binding carries its argument types and
probes for it, the entry refuses a NULL handle, the widths without the launch and misaligned rows before it looks at a device, the
keywords refuse what they do not know, a model built without the keyword makes today's calls, the node takes the new route -- one launch
helper and the two weight gradients -- only where the keyword, the width and the alignment allow it, and the bounds of
tests/ngcf_back_ref.py at C_in = 128 admit a float32 emulation of the entry's rounding points and reject two broken backwards."""
import ctypes

import numpy as np
import pytest
import torch

from abi_header import ctypes_of, prototype as header_prototype
import ngcf_back_ref as bref
import ngcf_fused_ref as nref
from test_gcn_fused_cpu import CpuGraph, OnDevice, tiny_graph
from test_ngcf_back_cpu import PROTOTYPE, TODAY, emulated, judged
from test_ngcf_fused_cpu import cpu_world
from test_ngcf_wide_cpu import model_calls

NAME = "gnx_step_back_wide_ngcf"
UNSUPPORTED, INVALID = -4, -1


def test_header_library_and_binding_agree():
    """The parameter list is gnx_step_back_ngcf's, the symbol is exported and probed for, and the ABI number stays."""
    from gnntf import _native
    assert header_prototype(NAME) == PROTOTYPE == header_prototype("gnx_step_back_ngcf")
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), NAME) and _native.has_symbol(NAME)
    assert NAME in _native.SIGNATURES and NAME in _native.PROBED
    want = ctypes_of(PROTOTYPE)
    assert _native.SIGNATURES[NAME] == (ctypes.c_int, want) == _native.SIGNATURES["gnx_step_back_ngcf"]
    assert _native.lib().gnx_version() == 900 == _native.ABI_VERSION            # added within ABI 0.9: the number stays
    # (tests/test_layer_entries_cpu.py pins the names that begin with the layers' prefixes: the layer's name stands behind the verb)
    assert not NAME.startswith(("gnx_ngcf_", "gnx_gcn_", "gnx_gcnii_", "gnx_feature_dropout"))


def test_checks_that_need_no_device():
    """The NULL handle -- under the entry's own name --, a rate outside [0, 1), an unknown activation, the widths without the launch and
    NULL operands are answered before the handle (the one below is not one) or any buffer is looked at: nothing can have been launched."""
    from gnntf import _native
    lib = _native.lib()
    handle = ctypes.c_void_p(16)
    buf = [ctypes.c_void_p(256 * k) for k in range(1, 20)]

    def back(h=handle, C_out=128, C_in=128, act=2, rate=0.0, g=buf[1], ldg=128):
        return lib.gnx_step_back_wide_ngcf(h, buf[0], g, ldg, buf[2], 128, buf[3], buf[4], C_out, act, rate, 1, 2, buf[5], C_in, buf[6], C_in,
                                           buf[7], C_out, buf[8], C_out, buf[9], buf[10], 128, buf[11], buf[12], buf[13], buf[14], buf[15],
                                           buf[16], C_in, buf[17], 1 << 20, None)

    assert back(h=None) == INVALID and lib.gnx_last_error() == b"gnx_step_back_wide_ngcf: NULL handle"
    for change, code, cause in ((dict(rate=1.0), INVALID, "dropout rate 1 outside [0, 1)"), (dict(act=7), INVALID, "invalid activation 7"),
                                (dict(C_out=0), INVALID, "not in [1, 2^20]"),
                                (dict(C_in=64, C_out=64), UNSUPPORTED, "widths 64 -> 64 are not supported"),
                                (dict(C_in=256), UNSUPPORTED, "widths 256 -> 128 are not supported"),
                                (dict(C_out=129), UNSUPPORTED, "widths 128 -> 129 are not supported"),
                                (dict(g=None), INVALID, "NULL g / G1 / G2"), (dict(ldg=127), INVALID, "a row stride below C_out")):
        rc = back(**change)
        message = lib.gnx_last_error().decode()
        assert rc == code and message.startswith(NAME + ": ") and cause in message, (cause, rc, message)
        assert code == INVALID or "keep the composed backward elsewhere" in message


def test_keywords_are_validated():
    import gnntf
    from gnntf import sparse
    assert sparse.NGCF_WIDE_BACKWARDS == ("composed", "fused")
    assert callable(sparse._ngcf_wide_back_launch)
    X = np.zeros((3, 4), dtype=np.float32)
    for make in (lambda **k: gnntf.GNN(tiny_graph(), X, **k), lambda **k: gnntf.NGCF(tiny_graph(), X, 2, **k)):
        with pytest.raises(Exception, match="ngcf_wide_backward must be one of"):
            make(ngcf_wide_backward="bogus")
        with pytest.raises(Exception, match="ngcf_wide_backward must be one of"):
            make(ngcf_wide_backward=True)
    with pytest.raises(Exception, match="ngcf_step: wide_backward must be one of"):
        sparse.ngcf_step(None, None, None, None, None, None, wide_backward="bogus")
    # the bias slabs: s = max(1, min(1024, ceil(n / 512))) of 2 C_out floats each
    assert sparse._ngcf_wide_back_work_floats(1547, 7) == 4 * 14 and sparse._ngcf_wide_back_work_floats(1, 128) == 256
    assert sparse._ngcf_wide_back_work_floats(2 ** 15 + 11, 40) == 65 * 80 and sparse._ngcf_wide_back_work_floats(10_000_000, 128) == 1024 * 256


def test_the_model_names_the_keyword_only_where_it_acts(monkeypatch):
    """Without the keyword the calls are today's, argument for argument; with it, width 128 under both other keywords names it in every
    call and width 64 does not; without ngcf_layer="fused" or ngcf_wide="fused" a width-128 layer never reaches ngcf_step at all."""
    both = dict(ngcf_layer="fused", ngcf_wide="fused")
    seen, composed = model_calls(monkeypatch, 128, **both)
    assert seen == [dict(activation="leaky", wide="fused")] * 3 and composed == []
    seen, composed = model_calls(monkeypatch, 128, ngcf_wide_backward="composed", **both)
    assert seen == [dict(activation="leaky", wide="fused")] * 3 and composed == []
    seen, composed = model_calls(monkeypatch, 128, ngcf_wide_backward="fused", **both)
    assert seen == [dict(activation="leaky", wide="fused", wide_backward="fused")] * 3 and composed == []
    seen, composed = model_calls(monkeypatch, 64, ngcf_wide_backward="fused", **both)
    assert seen == [dict(activation="leaky")] * 3 and composed == []
    for option in (dict(ngcf_layer="fused"), dict(ngcf_wide="fused"), dict()):
        seen, composed = model_calls(monkeypatch, 128, ngcf_wide_backward="fused", **option)
        assert seen == [] and composed == [128] * 3, option


WIDE = ["_ngcf_launch", "_ngcf_wide_back_launch", "_dense_wgrad", "_dense_wgrad"]


@pytest.mark.parametrize("C_in, C_out, ld, how, want", [
    (128, 128, None, dict(wide_backward="fused"), WIDE), (128, 7, None, dict(wide="fused", wide_backward="fused"), WIDE),
    (128, 40, 136, dict(wide_backward="fused", backward="fused"), WIDE), (128, 128, None, dict(wide="fused", backward="fused"), TODAY),
    (128, 128, None, dict(), TODAY), (128, 128, 130, dict(wide_backward="fused"), TODAY), (64, 64, None, dict(wide_backward="fused"), TODAY),
    (256, 128, None, dict(wide_backward="fused"), TODAY)])
def test_what_the_node_calls(monkeypatch, C_in, C_out, ld, how, want):
    """Over counting fakes of the launches: wide_backward="fused" at C_in = 128, C_out <= 128 over aligned rows -- whichever call made the
    forward -- is the one entry and the two weight gradients; the default, backward="fused" alone, rows of stride 130 and the widths 64
    and 256 make exactly today's calls in today's order.  Either way the gradients are those of torch's autograd over the formula, and
    a second backward over the retained graph makes the same calls again."""
    from gnntf import sparse
    dense_adj = cpu_world(monkeypatch)
    rng = np.random.default_rng(8)
    n = 12
    X, W1, W2 = (torch.from_numpy((rng.standard_normal(s) / 4).astype(np.float32)) for s in ((n, C_in), (C_in, C_out), (C_in, C_out)))
    b1, b2 = (torch.from_numpy(rng.uniform(-0.3, 0.3, size=(1, C_out)).astype(np.float32)) for _ in range(2))
    if ld is not None:
        wider = torch.zeros(n, ld)
        wider[:, :C_in] = X
        X = wider[:, :C_in]

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

    def fake_launch(adj, X, W1, b1, W2, b2, activation, keep, dropout=None, normalize=True, **more):
        agg = dense_adj @ X
        P1, P2 = (X * agg) @ W1 + b1, agg @ W2 + b2
        x = sparse._ngcf_act(P1, activation) + sparse._ngcf_act(P2, activation)
        r = 1 / x.norm(dim=1).clamp_min(1e-6)
        return (x * r[:, None]).detach(), agg.detach().contiguous(), torch.stack([P1 > 0, P2 > 0]), r.detach()

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
    recorded("_ngcf_wide_back_launch", fake_back)
    monkeypatch.setattr(sparse, "_ngcf_back_launch", lambda *a, **k: pytest.fail("the narrow backward has no launch at these widths"))
    recorded("_dense_wgrad", lambda T, G: T.t() @ G)
    recorded("_dense_launch", lambda G, Wt, b, relu: G @ Wt)
    recorded("_launch", lambda adj, T, H0, beta, alpha, act, transposed=False: dense_adj.t() @ T)
    upstream = torch.from_numpy(rng.standard_normal((n, C_out)).astype(np.float32))
    on = lambda t: torch.Tensor._make_subclass(OnDevice, t)
    leaves = [on(X).requires_grad_()] + [on(t.clone()).requires_grad_() for t in (W1, b1, W2, b2)]
    out = sparse.ngcf_step(sparse.Adjacency(CpuGraph()), *leaves, activation="leaky", **how)
    assert calls == ["_ngcf_launch"]
    out.backward(upstream, retain_graph=True)
    assert calls == want, calls
    plain = [t.clone().requires_grad_() for t in (X, W1, b1, W2, b2)]
    formula(*plain).backward(upstream)
    for name, got, ref in zip(("X", "W1", "b1", "W2", "b2"), leaves, plain):
        assert got.grad.shape == ref.grad.shape and torch.allclose(got.grad, ref.grad, rtol=1e-4, atol=1e-5), name
    first = [leaf.grad.clone() for leaf in leaves]
    for leaf in leaves:
        leaf.grad = None
    out.backward(upstream)
    assert calls == want + want[1:] and all(torch.equal(leaf.grad, g) for leaf, g in zip(leaves, first))


def test_a_library_without_the_symbol_is_an_error_not_a_fallback(monkeypatch):
    from gnntf import _native, sparse
    monkeypatch.setattr(_native, "has_symbol", lambda name: False)
    monkeypatch.setattr(sparse, "_ngcf_back_launch", lambda *a, **k: pytest.fail("launched without the symbol"))
    with pytest.raises(Exception, match="needs gnx_step_back_wide_ngcf"):
        sparse._ngcf_wide_back_launch(None, None, None, None, None, "leaky", None, None, None, None, None)


# ---- the bounds at C_in = 128 admit the entry's rounding points and reject two broken backwards ---------------------------------------------
BOUND_CASES = [(128, 128, 0.0), (128, 40, 0.25), (128, 7, 0.25)]


@pytest.mark.parametrize("C_in, C_out, p", BOUND_CASES)
def test_bounds_admit_the_float32_emulation_at_128(C_in, C_out, p):
    """Regime T: ngcf_back_ref.backward_f32 -- every Q one fmaf chain over the output columns ascending, dA one fused multiply-add, R and P
    one multiply -- against products_ref and backward_ref, over all rows and over the hub rows, the rows without entries and the ragged
    tile.  The bounds carry C_out and C_in as numbers: nothing in them assumes C_in <= 64."""
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


@pytest.mark.parametrize("C_in, C_out, p", BOUND_CASES)
def test_bounds_reject_two_broken_backwards_at_128(C_in, C_out, p):
    """dX without R = Q1 * A, and dA without the product with X: each lost term is of the gradient's own size, so a bound that passed
    either would be slack.  The test asks for ten times the bound, as tests/test_ngcf_back_cpu.py does at the narrow widths; the
    figures are printed."""
    e = emulated(C_in, C_out, p)
    c, op, want = e["c"], e["op"], e["want"]
    for broken in (dict(with_R=False), dict(with_X=False)):
        got = bref.backward_f32(e["At32"], op["X"], e["agg"], op["W1"], op["W2"], e["G1"], e["G2"], c["L"], **broken)
        factor = nref.ratio(got["dX"], want["dX"], want["dX_bound"])
        print(f"T {C_in}->{C_out} {broken}: dX error / bound = {factor:.3g}")
        assert factor > 10, broken
