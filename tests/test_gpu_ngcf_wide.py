"""The NGCF layer at width 128 on the MI355X (gnx_step_wide_ngcf, sparse.ngcf_step(wide="fused"), GNN(ngcf_wide="fused")): gnx_spmm, then
one row-local launch (k_ngcf_rows).

Judged as tests/test_gpu_ngcf_fused.py judges the one-launch layer: against the float64 reference of tests/ngcf_fused_ref.py over the very
float32 weights the kernels read, max |got - want| / bound <= 1 (its derivation carries C_in as a number and holds at 128 as it stands;
tests/test_ngcf_wide_cpu.py checks that a float32 evaluation stays inside and that the gate bits are decided), at regime T (n = 1547: a
ragged last tile, hub rows, a whole tile of rows without entries), regime S (n = 2^15 + 11: 2049 tiles, one more than 256 CUs x 8 waves,
so a persistent wave takes a second tile), a graph of 5 rows (one partial tile) and X as a view of a wider buffer.  Where existing code is
the reference the comparison is bit for bit: the aggregated rows against sparse.spmm, the mask against the unmasked result times the scale."""
import functools

import numpy as np
import pytest
import torch

import ngcf_fused_ref as nref
from test_gpu_gcnii_drop import keep_mask
from test_gpu_ngcf_fused import ACTS, SEED, SENTINEL, STREAM, CountingLibrary, act32, bits, dev, host, reference, row_sets, weights_csr

pytestmark = pytest.mark.gpu

NAME = "gnx_step_wide_ngcf"


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


@pytest.fixture(scope="module")
def world(gnntf):
    """Regimes T and S and a graph of 5 rows, bipartite-normalised: the handle, its adjacency and the weights read back, made once."""
    out = dict()
    for name in ("T", "S", "tiny"):
        if name == "tiny":                                   # five rows, one of them (row 3) without entries
            coo = np.array([[0, 1], [1, 0], [0, 2], [2, 0], [1, 4], [4, 1], [2, 4], [4, 2]], dtype=np.int64)
            vals, shape = np.ones(len(coo), dtype=np.float32), (5, 5)
            info = dict(hub=np.array([], dtype=np.int64), empty=np.array([3]), ragged=np.arange(5))
        else:
            coo, vals, shape, info = nref.regime_graph(name)
        g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
        adj = gnntf.normalize(g, "bipartite")
        out[name] = dict(g=g, adj=adj, A=weights_csr(g, adj.vals), info=info, n=shape[0], L=g.long_row_threshold)
    assert out["T"]["g"].n_hub_rows > 0 and out["S"]["n"] == 2 ** 15 + 11
    return out


@functools.lru_cache(maxsize=None)
def operands(n, C_out):
    return nref.operands(n, 128, C_out, 900 + 7 * 128 + C_out)


def wide_name(drop=False, norm=True):
    return "spmm+k_ngcf_rows<128>" + ("_drop" if drop else "") + ("_norm" if norm else "")


def sets_of(info):
    return [(name, rows) for name, rows in row_sets(info) if rows is None or len(rows) > 0]


def launch(sparse, w, op, act, bias=True, normalize=True, keep=False, dropout=None, X=None):
    b1, b2 = (dev(op["b1"]), dev(op["b2"])) if bias else (None, None)
    return sparse._ngcf_launch(w["adj"], dev(op["X"]) if X is None else X, dev(op["W1"]), b1, dev(op["W2"]), b2, act, keep=keep, dropout=dropout,
                               normalize=normalize, wide="fused")


# ---- the forward against float64, the aggregated rows against sparse.spmm, the rows without entries, the name ------------------------------
FORWARD_CASES = [("T", 128, False), ("T", 100, False), ("T", 7, False), ("S", 128, False), ("tiny", 128, False), ("T", 100, True)]


@pytest.mark.parametrize("regime, C_out, view", FORWARD_CASES)
def test_forward_against_float64(gnntf, world, regime, C_out, view):
    sparse = gnntf.sparse
    w = world[regime]
    g, info, n = w["g"], w["info"], w["n"]
    op = operands(n, C_out)
    X = None
    if view:                                                 # ldx = 136 != C_in: X as the first 128 columns of a wider buffer
        buffer = torch.full((n, 136), SENTINEL, device="cuda")
        buffer[:, :128] = dev(op["X"])
        X = buffer[:, :128]
        assert X.stride(0) == 136
    spmm = sparse.spmm(w["adj"], dev(op["X"]))
    worst = 0.0
    for act in ACTS:
        for bias in (True, False):
            for normalize in (True, False):
                where = f"{regime} 128->{C_out} view={view} {act} bias={bias} normalize={normalize}"
                want = reference(w, op, act, bias, normalize)
                out, agg, gate, rnorm = launch(sparse, w, op, act, bias, normalize, keep=True, X=X)
                assert g.last_kernel() == wide_name(norm=normalize), (where, g.last_kernel())
                assert out.shape == (n, C_out) and out.stride(0) == C_out
                assert np.array_equal(bits(agg), bits(spmm)), where                      # d_agg is gnx_spmm's result, hub rows included
                assert (gate is None) == (act == "none") and (rnorm is None) == (not normalize)
                for name, rows in sets_of(info):
                    r_out = nref.ratio(host(out), want["out"], want["out_bound"], rows)
                    worst = max(worst, r_out)
                    print(f"{where} {name} rows: out error / bound = {r_out:.3f}")
                    assert r_out <= 1, (where, name)
                # without keep (the aggregated rows in d_work, no gate, no rnorm): the same bits
                assert np.array_equal(bits(out), bits(launch(sparse, w, op, act, bias, normalize, X=X)[0])), where
                empty = host(out)[info["empty"]]
                if not bias:                                 # a row without entries and without bias: exact zeros, the clamp's 0 * 1e6
                    assert not empty.any(), where
                    if normalize:
                        assert np.array_equal(host(rnorm)[info["empty"]], np.full(len(info["empty"]), -1e6, dtype=np.float32)), where
                elif not normalize:                          # ... with biases: P = b exactly, so act(b1) + act(b2) bit for bit
                    x = (act32(op["b1"], act) + act32(op["b2"], act)).astype(np.float32)
                    assert np.array_equal(empty, np.broadcast_to(x, empty.shape)), where
                if normalize:
                    norms = np.linalg.norm(host(out).astype(np.float64), axis=1)
                    assert np.abs(norms[norms > 0] - 1).max() < 1e-5, where
    print(f"{regime} 128->{C_out} view={view}: the largest error / bound = {worst:.3f}")


SENTINEL_CASES = [("T", 100, 104, 0, False), ("T", 100, 101, 0, False), ("T", 7, 7, 0, False), ("T", 7, 8, 0, False), ("T", 7, 8, 1, False),
                  ("T", 128, 132, 0, False), ("S", 128, 132, 0, False), ("S", 128, 129, 0, False), ("tiny", 128, 132, 0, False),
                  ("tiny", 128, 129, 0, False), ("tiny", 100, 104, 0, False), ("tiny", 7, 7, 0, False), ("T", 100, 104, 0, True),
                  ("T", 100, 101, 0, True)]


@pytest.mark.parametrize("regime, C_out, ldo, shift, view", SENTINEL_CASES)
def test_nothing_is_written_past_the_last_column(gnntf, world, regime, C_out, ldo, shift, view):
    """out as [n, C_out] inside a sentinel-filled wider buffer, with d_agg, d_gate and d_rnorm sentinel-filled behind their last row: whole
    16-byte stores (ldo % 4 == 0, aligned base; C_out = 100 ends on a piece, C_out = 7 inside one), single values (ldo = 101, 129, 7, a
    base that is not 16-byte aligned), on regime T, on regime S (a wave's second tile), on the graph of 5 rows (11 dead rows in the only
    tile, both store paths) and with X as a view of an [n, 136] buffer: the same block each time, every other element untouched."""
    nat = gnntf.sparse.nat
    w = world[regime]
    n, g, pad = w["n"], w["g"], 64
    op = operands(n, C_out)
    Xd, W1d, W2d, b1d, b2d = (dev(op[k]) for k in ("X", "W1", "W2", "b1", "b2"))
    ldx = 128
    if view:
        buffer = torch.full((n, 136), SENTINEL, device="cuda")
        buffer[:, :128] = Xd
        Xd, ldx = buffer[:, :128], 136
    words = 2 * ((C_out + 31) // 32)
    whole = torch.full((pad + shift + n * ldo + pad,), SENTINEL, device="cuda")
    out = whole[pad + shift:pad + shift + n * ldo]
    agg, rnorm = torch.full((n + 16, 128), SENTINEL, device="cuda"), torch.full((n + 64,), SENTINEL, device="cuda")
    gate = torch.full((n + 16, words), 77, dtype=torch.int32, device="cuda")
    rc = nat.lib().gnx_step_wide_ngcf(g.handle, nat.ptr(w["adj"].vals), nat.ptr(Xd), ldx, 128, nat.ptr(W1d), C_out, nat.ptr(W2d), C_out, C_out,
                                      nat.ptr(b1d), nat.ptr(b2d), nat.ACT_LEAKY, 0.0, 0, 0, 1, nat.ptr(out), ldo, nat.ptr(agg), nat.ptr(gate),
                                      nat.ptr(rnorm), None, 0, nat.current_stream())
    assert rc == 0, nat.lib().gnx_last_error()
    assert g.last_kernel() == wide_name()
    torch.cuda.synchronize()
    block = out.view(n, ldo)
    assert bool((whole[:pad + shift] == SENTINEL).all()) and bool((whole[pad + shift + n * ldo:] == SENTINEL).all())
    assert bool((block[:, C_out:] == SENTINEL).all()) and not bool((block[:, :C_out] == SENTINEL).any())
    assert bool((agg[n:] == SENTINEL).all()) and bool((rnorm[n:] == SENTINEL).all()) and bool((gate[n:] == 77).all())
    assert not bool((rnorm[:n] == SENTINEL).any())
    if view:
        assert bool((buffer[:, 128:] == SENTINEL).all())
    want = launch(gnntf.sparse, w, op, "leaky", keep=True)                                   # whichever stores made it
    assert torch.equal(block[:, :C_out], want[0]) and torch.equal(agg[:n], want[1]) and torch.equal(gate[:n], want[2])
    assert torch.equal(rnorm[:n], want[3])


def test_refusals_write_nothing(gnntf, world):
    nat = gnntf.sparse.nat
    lib = nat.lib()
    w = world["T"]
    n, g = w["n"], w["g"]
    op = operands(n, 100)
    Xd, W1d, W2d = (dev(op[k]) for k in ("X", "W1", "W2"))
    out, work = torch.full((n, 100), SENTINEL, device="cuda"), torch.full((n * 128,), SENTINEL, device="cuda")

    def step(X=Xd, ldx=128, C_in=128, C_out=100, out_=out, work_=work, work_floats=n * 128, agg=None):
        return lib.gnx_step_wide_ngcf(g.handle, nat.ptr(w["adj"].vals), nat.ptr(X), ldx, C_in, nat.ptr(W1d), 100, nat.ptr(W2d), 100, C_out, None, None,
                                      nat.ACT_LEAKY, 0.0, 0, 0, 1, nat.ptr(out_), 100, nat.ptr(agg), None, None, nat.ptr(work_), work_floats,
                                      nat.current_stream())

    for call, code, causes in ((lambda: step(work_floats=n * 128 - 4), -1, (b"needs d_work of %d floats" % (n * 128), b"without d_agg")),
                               (lambda: step(C_in=64, ldx=64, C_out=64), -4, (b"widths 64 -> 64 are not supported",)),
                               (lambda: step(X=work[1:], ldx=128), -4, (b"misaligned rows",)),
                               (lambda: step(out_=Xd), -1, (b"out must not alias an input",)),
                               (lambda: step(agg=W2d), -1, (b"d_agg must be a buffer of its own",))):
        rc = call()
        message = lib.gnx_last_error()
        assert rc == code and message.startswith(NAME.encode()) and all(c in message for c in causes), message
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((work == SENTINEL).all())
    assert step() == 0, lib.gnx_last_error()
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


# ---- the gate words -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime, C_out", [("T", 128), ("T", 100), ("T", 7), ("S", 128)])
def test_gate_bits_are_the_float64_signs(gnntf, world, regime, C_out):
    """Bit (P > 0) of P1 and P2 against the float64 sign wherever |P| exceeds its forward bound; the undecided share of the reference
    alone is at most 1 % (tests/test_ngcf_wide_cpu.py measures it on regime T: 0.020 % at most).  Bits beyond C_out are zero."""
    sparse = gnntf.sparse
    w = world[regime]
    op = operands(w["n"], C_out)
    W = (C_out + 31) // 32
    for act in ("leaky", "relu"):
        want = reference(w, op, act)
        d1, d2, share = nref.gate_share(want)
        assert share <= 1e-2
        _, _, gate, rnorm = launch(sparse, w, op, act, keep=True)
        assert gate.dtype == torch.int32 and tuple(gate.shape) == (w["n"], 2 * W) and rnorm.shape == (w["n"],)
        b1, b2 = nref.unpack_gate(host(gate), C_out)
        assert np.array_equal(b1[d1], (want["P1"] > 0)[d1]) and np.array_equal(b2[d2], (want["P2"] > 0)[d2]), (regime, C_out, act)
        assert d1[w["info"]["empty"]].all() and d2[w["info"]["empty"]].all()
        if C_out % 32:
            assert not (host(gate).view(np.uint32)[:, [W - 1, 2 * W - 1]] >> np.uint32(C_out % 32)).any()
        r = host(rnorm).astype(np.float64)
        size = np.sqrt((want["x"] ** 2).sum(axis=1))
        sound = size > 1e-3
        assert sound.mean() > 0.5 and (r[sound] > 0).all() and np.abs(r[sound] * size[sound] - 1).max() < 1e-4
    assert launch(sparse, w, op, "none", keep=True)[2] is None


# ---- the mask; two calls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_out", [128, 100, 7])
def test_feature_mask_and_determinism(gnntf, world, C_out):
    sparse = gnntf.sparse
    w = world["T"]
    g, n = w["g"], w["n"]
    op = operands(n, C_out)
    for p in (0.5, 0.25):
        plain = launch(sparse, w, op, "leaky", normalize=False)[0]
        masked, agg, _, _ = launch(sparse, w, op, "leaky", normalize=False, keep=True, dropout=(p, SEED, STREAM))
        assert g.last_kernel() == wide_name(True, False)
        keep = keep_mask(SEED, STREAM, p, n, C_out)
        want = np.where(keep, host(plain) * nref.scale(p), np.float32(0)).astype(np.float32)
        np.testing.assert_array_equal(bits(masked), want.view(np.int32))         # kept: unmasked x scale; dropped: +0
        assert np.array_equal(bits(agg), bits(sparse.spmm(w["adj"], dev(op["X"]))))             # d_agg stays undropped
        ref = reference(w, op, "leaky", True, True, p, keep)
        first = launch(sparse, w, op, "leaky", keep=True, dropout=(p, SEED, STREAM))
        assert g.last_kernel() == wide_name(True, True)
        for name, rows in sets_of(w["info"]):
            assert nref.ratio(host(first[0]), ref["out"], ref["out_bound"], rows) <= 1, (C_out, p, name)
        second = launch(sparse, w, op, "leaky", keep=True, dropout=(p, SEED, STREAM))
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, second))             # out, agg, gate, rnorm: the same bits


# ---- gradients ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_out", [128, 7])
def test_autograd_against_float64(gnntf, world, C_out):
    sparse = gnntf.sparse
    w = world["T"]
    g, n = w["g"], w["n"]
    op = operands(n, C_out)
    names = ("X", "W1", "b1", "W2", "b2")
    for mask in (None, (0.5, SEED, STREAM)):
        for normalize in (True, False):
            where = f"T 128->{C_out} mask={mask is not None} normalize={normalize}"
            grads = dict()
            for how in ("composed", "fused"):
                leaves = [dev(op[k]).requires_grad_() for k in names]
                out = gnntf.ngcf_step(w["adj"], *leaves, activation="leaky", dropout=mask, normalize=normalize, backward=how, wide="fused")
                assert g.last_kernel() == wide_name(mask is not None, normalize), where
                out.backward(dev(op["g"]))
                grads[how] = [leaf.grad for leaf in leaves]
            assert all(torch.equal(a, b) for a, b in zip(grads["composed"], grads["fused"])), where      # backward="fused" is inert at 128
            p = 0.0 if mask is None else mask[0]
            keep = None if mask is None else keep_mask(SEED, STREAM, p, n, C_out)
            f = reference(w, op, "leaky", True, normalize, p, keep)
            assert nref.ratio(host(out), f["out"], f["out_bound"]) <= 1, where
            gate = launch(sparse, w, op, "leaky", True, normalize, keep=True, dropout=mask)[2]
            bit1, bit2 = nref.unpack_gate(host(gate), C_out)       # the bits the kernel reported (judged on their own above)
            gated = nref.back_gate_ref(f, op["g"], bit1, bit2, "leaky", normalize, p, keep)
            want = nref.backward_ref(w["A"], f, op["X"], op["W1"], op["W2"], *gated, L=w["L"])
            for key, grad in zip(("dX", "dW1", "db1", "dW2", "db2"), grads["composed"]):
                got = host(grad)
                worst = nref.ratio(got.reshape(1, -1) if got.ndim == 1 else got, want[key].reshape(-1, got.shape[-1]),
                                   want[key + "_bound"].reshape(-1, got.shape[-1]))
                print(f"{where} {key}: error / bound = {worst:.3g}")
                assert worst <= 1 and float(np.abs(got).max()) > 0, (where, key)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_sided():
    """300 users and 200 items, about 2 400 user-item pairs without duplicates, stored in both directions; features without columns."""
    rng = np.random.default_rng(31)
    n_u, n_i = 300, 200
    pairs = np.unique(np.stack([rng.integers(0, n_u, size=2400), n_u + rng.integers(0, n_i, size=2400)], axis=1), axis=0)
    coo = np.concatenate([pairs, pairs[:, ::-1]]).astype(np.int64)
    return dict(coo=coo, vals=np.ones(len(coo), dtype=np.float32), shape=(n_u + n_i, n_u + n_i), pairs=pairs, n_u=n_u)


def make_model(gnntf, data, **option):
    """The shape of the reference's library_recommendation demo: Structural(dims=128) over empty features, NGCF(num_classes=128)."""
    gnntf.set_seed(11)
    torch.manual_seed(3)
    n = data["shape"][0]
    model = gnntf.NGCF(gnntf.SparseCOO(data["coo"], data["vals"], data["shape"]), np.zeros((n, 0), dtype=np.float32), num_classes=128,
                       preprocessor=gnntf.Structural(dims=128, regularize=0, bipartite=data["n_u"]), ngcf_layer="fused", ngcf_wide="fused", **option)
    model.reset()
    return model


def recorded_steps(gnntf, monkeypatch):
    """Every sparse.ngcf_step call from here on: (adjacency, X, W1, b1, W2, b2, keywords, out, the kernel the handle reported)."""
    sparse = gnntf.sparse
    real, steps = sparse.ngcf_step, []

    def recording(adj, X, W1, b1, W2, b2, **kwargs):
        out = real(adj, X, W1, b1, W2, b2, **kwargs)
        steps.append((adj, X, W1, b1, W2, b2, kwargs, out, adj.graph.last_kernel()))
        return out

    monkeypatch.setattr(sparse, "ngcf_step", recording)
    return real, steps


def test_model_eval_is_the_layers_pushed_through_the_entry(gnntf, two_sided, monkeypatch):
    nat = gnntf.sparse.nat
    counting = CountingLibrary(nat.lib())
    monkeypatch.setattr(nat, "lib", lambda: counting)
    real, steps = recorded_steps(gnntf, monkeypatch)
    model = make_model(gnntf, two_sided)
    n = two_sided["shape"][0]
    model.training_mode(False)
    counting.calls.clear()
    with torch.no_grad():
        out = model(model.features)
    layers = [l for l in model.layers() if isinstance(l, gnntf.NGCFLayer)]
    assert len(layers) == 3 and all(tuple(l.W1.shape) == (128, 128) for l in layers) and out.shape == (3 * n, 128)
    assert len(steps) == 3 and all(s[6] == dict(activation="leaky", wide="fused") and s[8] == wide_name() for s in steps)
    assert "gnx_ngcf_step" not in counting.calls and counting.calls.count(NAME) >= 3         # every layer took the new entry
    with torch.no_grad():
        H, rows = steps[0][1], []
        assert tuple(H.shape) == (n, 128)
        for l in layers:                                     # the same weights, layer by layer through the entry
            H = real(l.adjacency, H, l.W1, l.b1, l.W2, l.b2, wide="fused")
            rows.append(H)
    assert torch.equal(out, torch.cat(rows, dim=0))
    # ... and against float64 over each layer's own float32 input
    A32 = weights_csr(model.graph, layers[0].adjacency.vals)
    for k, (l, s) in enumerate(zip(layers, steps)):
        W1, b1, W2, b2 = (host(t) for t in (l.W1, l.b1, l.W2, l.b2))
        want = nref.forward_ref(A32, host(s[1]), W1, b1, W2, b2, "leaky", L=model.graph.long_row_threshold)
        worst = nref.ratio(host(s[7]), want["out"], want["out_bound"])
        print(f"layer {k}: error / bound = {worst:.3f}")
        assert worst <= 1


def test_what_a_training_forward_saves(gnntf, two_sided, monkeypatch):
    """Per layer the node saves its input, A . X and its output as [n, 128] matrices -- the input is the previous layer's output -- so
    the three layers hold 1 + 2 * 3 distinct ones (the composed layer saves the product, both pre-activations, both activations, their
    sum and the dropped rows besides)."""
    _, steps = recorded_steps(gnntf, monkeypatch)
    model = make_model(gnntf, two_sided, feature_dropout="fused", dropout=0.25)
    n = two_sided["shape"][0]
    saved = []
    with model:
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
            out = model(model.features)
    assert out.requires_grad and len(steps) == 3 and all(s[8] == wide_name(True, True) and s[6]["wide"] == "fused" for s in steps)
    wide = {t.data_ptr() for t in saved if tuple(t.shape) == (n, 128) and t.dtype == torch.float32}
    assert len(wide) == 1 + 2 * 3, len(wide)
    assert {s[1].data_ptr() for s in steps} | {s[7].data_ptr() for s in steps} <= wide


def run_training(gnntf, data, capture, epochs=3):
    import random
    random.seed(0)
    np.random.seed(0)
    model = make_model(gnntf, data, feature_dropout="fused", dropout=0.25)
    positives = data["pairs"][::25]
    sampler = gnntf.device_negative_sampling(positives, model, negative_nodes=np.arange(300, 500))
    task = gnntf.LinkPrediction(sampler)
    torch.manual_seed(5)
    model.train(train=task, epochs=epochs, patience=50, capture=capture, verbose=False,
                optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
    assert sampler.fallbacks() == 0
    return [v.var.detach().clone() for v in model.vars()], model._mask_calls, model.graph.last_kernel()


def test_captured_training_equals_eager(gnntf, two_sided):
    """Three epochs of the demo-shaped model with the mask in the launch and negatives drawn on the device: the replayed graphs give the
    eager run's parameters bit for bit."""
    eager, eager_masks, _ = run_training(gnntf, two_sided, False)
    captured, captured_masks, _ = run_training(gnntf, two_sided, True)
    assert eager_masks == captured_masks and len(eager) == len(captured) >= 14          # two embeddings, four variables per layer
    assert all(torch.equal(e, c) for e, c in zip(eager, captured))
    start = [v.var.detach().clone() for v in make_model(gnntf, two_sided, feature_dropout="fused", dropout=0.25).vars()]
    assert any(not torch.equal(s, e) for s, e in zip(start, eager))                     # ... and it trained
