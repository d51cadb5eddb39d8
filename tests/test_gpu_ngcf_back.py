"""The fused NGCF backward on the MI355X (gnx_step_back_ngcf, sparse.ngcf_step(backward="fused"), GNN(ngcf_backward="fused")).

Where existing code is the reference the comparison is bit for bit: G1 / G2 against gnx_ngcf_back_gate, P against X * A, the weight
gradients against the composed backward's, dX against gnx_spmm_tv over the entry's own dA and R.  dA, R, the bias sums and dX are judged
against the float64 references of tests/ngcf_fused_ref.py / tests/ngcf_back_ref.py with max |got - want| / bound <= 1, at regime T
(n = 1547: a ragged last tile, hub rows at the threshold of 512, a whole tile of rows without entries) and regime S (n = 2^15 + 11,
threshold 128) of tests/gcnii_shapes_ref.py, bipartite-normalised.  The regime graphs' transposes are hub-free, so "Tt" and "St" are the
same graphs with every entry reversed: there the transposed structure, which the backward's SpMM walks, has the hub rows, the tile of
rows without entries and the ragged tile."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ngcf_back_ref as bref
import ngcf_fused_ref as nref
from test_gpu_gcnii_drop import keep_mask

pytestmark = pytest.mark.gpu

SEED, STREAM = 7, 2                                      # the feature mask's
MASK = (0.5, SEED, STREAM)
SENTINEL = 1234.5
ACTS = ("leaky", "relu", "none")


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()           # (a copy: the shared operands are read-only)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def weights_csr(g, vals):
    rowptr, colidx, _ = g.csr_arrays()
    return sp.csr_matrix((host(vals).astype(np.float64), host(colidx), host(rowptr)), shape=(g.n_rows, g.n_cols))


@pytest.fixture(scope="module")
def world(gnntf):
    """Regimes T and S and their reversals Tt and St, bipartite-normalised: the handle, its adjacency and the weights read back, made
    once and never changed; ``sets``: the rows the float64 comparisons are judged over, besides all of them."""
    out = dict()
    for name in ("T", "S", "Tt", "St"):
        coo, vals, shape, info = nref.regime_graph(name[0])
        if name.endswith("t"):
            coo = coo[:, ::-1].copy()
        g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
        adj = gnntf.normalize(g, "bipartite")
        A = weights_csr(g, adj.vals)
        deg, in_deg = np.diff(A.indptr), np.bincount(A.indices, minlength=shape[0])
        sets = dict(hub_t=np.flatnonzero(in_deg > info["L"]), empty=np.flatnonzero(deg == 0), empty_t=np.flatnonzero(in_deg == 0),
                    ragged=info["ragged"])
        assert g.long_row_threshold == info["L"] and g.n_hub_rows_t == len(sets["hub_t"])
        if name.endswith("t"):
            assert g.n_hub_rows == 0 and len(sets["hub_t"]) == len(info["hub"]) > 0 and len(sets["empty_t"]) >= 16
        else:
            assert g.n_hub_rows == len(info["hub"]) > 0 and len(sets["empty"]) >= 16
        assert len(sets["ragged"]) == shape[0] % 16 > 0
        out[name] = dict(g=g, adj=adj, A=A, info=info, n=shape[0], L=info["L"], sets=sets)
    return out


@functools.lru_cache(maxsize=None)
def operands(n, C_in, C_out):
    return nref.operands(n, C_in, C_out, 900 + 7 * C_in + C_out)


def back_name(C_in, drop=False, dX=True):
    return f"k_ngcf_back<{C_in}>" + ("_drop" if drop else "") + ("+spmm_tv" if dX else "")


def forward(sparse, w, op, act, normalize=True, dropout=None):
    """(out, agg, gate, rnorm) of gnx_ngcf_step as the training forward keeps them"""
    return sparse._ngcf_launch(w["adj"], dev(op["X"]), dev(op["W1"]), dev(op["b1"]), dev(op["W2"]), dev(op["b2"]), act, keep=True, dropout=dropout,
                               normalize=normalize)


def entry(sparse, w, op, act, kept, normalize=True, dropout=None, **want):
    out, agg, gate, rnorm = kept
    return sparse._ngcf_back_launch(w["adj"], dev(op["g"]), out if normalize else None, rnorm, gate, act, dropout, dev(op["X"]), agg, dev(op["W1"]),
                                    dev(op["W2"]), **want)


def storage(G):
    """the padded rows behind a [n, C] view of row stride roundup4(C)"""
    return torch.as_strided(G, (G.shape[0], G.stride(0)), (G.stride(0), 1))


CASES = [("T", 64, 64), ("T", 64, 7), ("T", 32, 32), ("T", 16, 16), ("S", 64, 40)]
FORMS = [(act, normalize, dropout) for act in ACTS for normalize in (True, False) for dropout in (None, MASK)]


# ---- 1. existing code as the reference, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime, C_in, C_out", CASES + [("Tt", 64, 64), ("St", 64, 40)])
def test_bit_for_bit_against_existing_code(gnntf, world, regime, C_in, C_out):
    sparse, nat = gnntf.sparse, gnntf.sparse.nat
    w = world[regime]
    g, n = w["g"], w["n"]
    op = operands(n, C_in, C_out)
    X = dev(op["X"])
    for act, normalize, dropout in FORMS:
        where = f"{regime} {C_in}->{C_out} {act} normalize={normalize} mask={dropout is not None}"
        kept = forward(sparse, w, op, act, normalize, dropout)
        out, agg, gate, rnorm = kept
        made = entry(sparse, w, op, act, kept, normalize, dropout)
        assert g.last_kernel() == back_name(C_in, dropout is not None), (where, g.last_kernel())
        G1, G2 = sparse._ngcf_back_gate(g, dev(op["g"]), out if normalize else None, rnorm, gate, act, dropout)
        assert same_bits(storage(made["G1"]), storage(G1)) and same_bits(storage(made["G2"]), storage(G2)), where
        assert float(made["G1"].abs().max()) > 0 and float(made["G2"].abs().max()) > 0
        assert same_bits(made["P"], X * agg), where
        assert same_bits(sparse._dense_wgrad(made["P"], made["G1"]), sparse._dense_wgrad(X * agg, G1)), where
        assert same_bits(sparse._dense_wgrad(agg, made["G2"]), sparse._dense_wgrad(agg, G2)), where
        dX = sparse._launch(w["adj"], made["dA"], made["R"], 1.0, 1.0, nat.ACT_NONE, transposed=True)
        assert same_bits(made["dX"], dX) and float(dX.abs().max()) > 0, where


# ---- 2. against float64 ---------------------------------------------------------------------------------------------------------------------
def references(w, op, act, normalize, dropout, gate, agg):
    """backward_ref's gradients and products_ref's intermediates with their bounds, from the float64 forward and the gate bits the kernel
    reported (judged on their own in tests/test_gpu_ngcf_fused.py)"""
    n, C_out = op["g"].shape
    p = 0.0 if dropout is None else dropout[0]
    keep = None if dropout is None else keep_mask(SEED, STREAM, p, n, C_out)
    f = nref.forward_ref(w["A"], op["X"], op["W1"], op["b1"], op["W2"], op["b2"], act, normalize, p, keep, L=w["L"])
    ones = np.ones((n, C_out), dtype=bool)
    bit1, bit2 = (ones, ones) if gate is None else nref.unpack_gate(host(gate), C_out)
    gated = nref.back_gate_ref(f, op["g"], bit1, bit2, act, normalize, p, keep)
    want = nref.backward_ref(w["A"], f, op["X"], op["W1"], op["W2"], *gated, L=w["L"])
    want.update(bref.products_ref(op["X"], host(agg), op["W1"], op["W2"], *gated))
    return f, want


def bound_of(want, key):
    return want["e_" + key] if "e_" + key in want else want[key + "_bound"]


@pytest.mark.parametrize("regime, C_in, C_out", CASES + [("Tt", 64, 7), ("St", 32, 32)])
def test_against_float64(gnntf, world, regime, C_in, C_out):
    sparse = gnntf.sparse
    w = world[regime]
    op = operands(w["n"], C_in, C_out)
    worst = 0.0
    for act, normalize, dropout in [("leaky", True, None), ("leaky", True, MASK), ("leaky", False, MASK), ("relu", True, MASK), ("none", False, None)]:
        where = f"{regime} {C_in}->{C_out} {act} normalize={normalize} mask={dropout is not None}"
        kept = forward(sparse, w, op, act, normalize, dropout)
        made = entry(sparse, w, op, act, kept, normalize, dropout)
        _, want = references(w, op, act, normalize, dropout, kept[2], kept[1])
        for key in ("db1", "db2"):
            r = nref.ratio(host(made[key]).reshape(1, -1), want[key].reshape(1, -1), want[key + "_bound"].reshape(1, -1))
            worst = max(worst, r)
            print(f"{where} {key}: error / bound = {r:.3g}")
            assert r <= 1 and float(made[key].abs().max()) > 0, (where, key)
        for key in ("dA", "R", "dX"):
            for name, rows in [("all", None)] + list(w["sets"].items()):
                if rows is not None and len(rows) == 0:
                    continue
                r = nref.ratio(host(made[key]), want[key], bound_of(want, key), rows)
                worst = max(worst, r)
                print(f"{where} {key} {name} rows: error / bound = {r:.3g}")
                assert r <= 1, (where, key, name)
        # a row the transposed structure gives nothing: dX is +0 + R, R itself up to the sign of a zero
        lonely = w["sets"]["empty_t"]
        assert torch.equal(made["dX"][lonely], made["R"][lonely])
    print(f"{regime} {C_in}->{C_out}: the largest error / bound = {worst:.3g}")


# ---- 3. under autograd ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime, C_in, C_out", [("T", 64, 64), ("T", 64, 7), ("T", 16, 16), ("S", 32, 32)])
def test_autograd_against_float64(gnntf, world, regime, C_in, C_out):
    sparse = gnntf.sparse
    w = world[regime]
    g, n = w["g"], w["n"]
    op = operands(n, C_in, C_out)
    names = ("X", "W1", "b1", "W2", "b2")
    up = dev(op["g"])
    for dropout in (None, MASK):
        for normalize in (True, False):
            where = f"{regime} {C_in}->{C_out} mask={dropout is not None} normalize={normalize}"
            leaves = [dev(op[k]).requires_grad_() for k in names]
            out = gnntf.ngcf_step(w["adj"], *leaves, activation="leaky", dropout=dropout, normalize=normalize, backward="fused")
            plain = [dev(op[k]).requires_grad_() for k in names]
            composed = gnntf.ngcf_step(w["adj"], *plain, activation="leaky", dropout=dropout, normalize=normalize)
            assert same_bits(out, composed), where                 # the forward does not know the keyword
            out.backward(up, retain_graph=True)
            first = [leaf.grad.clone() for leaf in leaves]
            kept = forward(sparse, w, op, "leaky", normalize, dropout)
            _, want = references(w, op, "leaky", normalize, dropout, kept[2], kept[1])
            for key, got in zip(("dX", "dW1", "db1", "dW2", "db2"), first):
                got = host(got)
                r = nref.ratio(got.reshape(1, -1) if got.ndim == 1 else got, want[key].reshape(-1, got.shape[-1]),
                               want[key + "_bound"].reshape(-1, got.shape[-1]))
                print(f"{where} {key}: error / bound = {r:.3g}")
                assert r <= 1 and float(np.abs(got).max()) > 0, (where, key)
            # dW1 / dW2 are the composed backward's bits: the same G1 / G2, the same X * A, the same kernel
            composed.backward(up)
            assert same_bits(first[1], plain[1].grad) and same_bits(first[3], plain[3].grad), where
            # a second backward over the retained graph: the saved tensors are still there, the bits are the same
            for leaf in leaves:
                leaf.grad = None
            out.backward(up)
            assert all(same_bits(leaf.grad, was) for leaf, was in zip(leaves, first)), where


def test_autograd_launches_what_is_needed(gnntf, world, monkeypatch):
    """X.requires_grad = False: no products, no transposed SpMM -- the entry reports no "+spmm_tv"; W1 without a gradient: no P."""
    sparse = gnntf.sparse
    w = world["T"]
    op = operands(w["n"], 64, 7)
    seen = []
    real = sparse._ngcf_back_launch

    def spy(*args, **kwargs):
        made = real(*args, **kwargs)
        seen.append((w["g"].last_kernel(), kwargs, {k: v is not None for k, v in made.items()}))
        return made

    monkeypatch.setattr(sparse, "_ngcf_back_launch", spy)
    for frozen, name in ((("X",), back_name(64, True, dX=False)), (("W1", "b2"), back_name(64, True)), ((), back_name(64, True))):
        leaves = [dev(op[k]).requires_grad_(k not in frozen) for k in ("X", "W1", "b1", "W2", "b2")]
        out = gnntf.ngcf_step(w["adj"], *leaves, activation="leaky", dropout=MASK, backward="fused")
        del seen[:]
        out.backward(dev(op["g"]))
        (kernel, kwargs, made), = seen
        assert kernel == name, (frozen, kernel)
        assert kwargs["want_dX"] == ("X" not in frozen) and kwargs["want_P"] == ("W1" not in frozen)
        assert kwargs["want_db"] == ("b1" not in frozen, "b2" not in frozen)
        assert made["dX"] == made["dA"] == made["R"] == ("X" not in frozen) and made["P"] == ("W1" not in frozen)
        assert made["db1"] == ("b1" not in frozen) and made["db2"] == ("b2" not in frozen)
        for k, leaf in zip(("X", "W1", "b1", "W2", "b2"), leaves):
            assert (leaf.grad is None) == (k in frozen), (frozen, k)


# ---- 4. determinism, padding, sentinels, refusals ---------------------------------------------------------------------------------------------
class Raw:
    """One direct call of gnx_step_back_ngcf at regime T, C_in -> 7 into rows of stride 8, every output inside sentinels."""
    PAD = 64

    def __init__(self, gnntf, w, C_in=64, C_out=7):
        self.sparse, self.nat, self.w, self.C_in, self.C_out = gnntf.sparse, gnntf.sparse.nat, w, C_in, C_out
        n = self.n = w["n"]
        self.op = op = operands(n, C_in, C_out)
        self.out, self.agg, self.gate, self.rnorm = forward(self.sparse, w, op, "leaky", True, MASK)
        up = torch.full((n, 8), float("nan"), device="cuda")          # the padding column of g holds NaN: nothing may read it
        up[:, :C_out] = dev(op["g"])
        self.up = up
        self.X, self.W1, self.W2 = dev(op["X"]), dev(op["W1"]), dev(op["W2"])
        self.floats = self.sparse._ngcf_back_work_floats(n, C_out)
        self.sizes = dict(G1=n * 8, G2=n * 8, P=n * C_in, db1=C_out, db2=C_out, dA=n * C_in, R=n * C_in, dX=n * C_in, work=self.floats)
        self.fresh()

    def fresh(self):
        self.whole = {k: torch.full((2 * self.PAD + size,), SENTINEL, device="cuda") for k, size in self.sizes.items()}
        self.buf = {k: t[self.PAD:self.PAD + self.sizes[k]] for k, t in self.whole.items()}

    def call(self, **change):
        nat, b = self.nat, self.buf
        a = dict(X=self.X, ldx=self.C_in, C_in=self.C_in, C_out=self.C_out, ldG=8, work_floats=self.floats, dX=b["dX"], G2=b["G2"], P=b["P"], rate=MASK[0])
        a.update(change)
        ldw = a["C_out"]
        return nat.lib().gnx_step_back_ngcf(
            self.w["g"].handle, nat.ptr(self.w["adj"].transposed_values()), nat.ptr(self.up), 8, nat.ptr(self.out), self.out.stride(0), nat.ptr(self.rnorm),
            nat.ptr(self.gate), a["C_out"], nat.ACT_LEAKY, a["rate"], SEED, STREAM, nat.ptr(a["X"]), a["ldx"], nat.ptr(self.agg), a["C_in"], nat.ptr(self.W1),
            ldw, nat.ptr(self.W2), ldw, nat.ptr(b["G1"]), nat.ptr(a["G2"]), a["ldG"], nat.ptr(a["P"]), nat.ptr(b["db1"]), nat.ptr(b["db2"]), nat.ptr(b["dA"]),
            nat.ptr(b["R"]), nat.ptr(a["dX"]), a["C_in"], nat.ptr(b["work"]), a["work_floats"], nat.current_stream())

    def untouched(self, keys=None):
        torch.cuda.synchronize()
        return all(bool((self.whole[k] == SENTINEL).all()) for k in (keys or self.whole))

    def margins_intact(self):
        torch.cuda.synchronize()
        P = self.PAD
        return all(bool((t[:P] == SENTINEL).all()) and bool((t[P + self.sizes[k]:] == SENTINEL).all()) for k, t in self.whole.items())


@pytest.mark.parametrize("C_in", [64, 16])
def test_two_calls_same_bits_padding_and_sentinels(gnntf, world, C_in):
    raw = Raw(gnntf, world["T"], C_in)
    lib = raw.nat.lib()
    assert raw.call() == 0, lib.gnx_last_error()
    assert world["T"]["g"].last_kernel() == back_name(C_in, True)
    assert raw.margins_intact()
    first = {k: v.clone() for k, v in raw.buf.items()}
    for k in ("G1", "G2", "P", "db1", "db2", "dA", "R", "dX"):
        assert not bool((first[k] == SENTINEL).any()), k           # every element of every output was written
    G1, G2 = first["G1"].view(raw.n, 8), first["G2"].view(raw.n, 8)
    assert not bool(G1[:, 7].any()) and not bool(G2[:, 7].any()) and bool(G1[:, :7].any())      # the padding column: zeros
    for k in ("G1", "G2", "P", "db1", "db2", "dA", "R", "dX"):
        assert bool(torch.isfinite(first[k]).all()), k             # the NaN in the padding of g reached nothing
    # ... and the results are those of the helper's call over the same operands (whose g has no padding at all)
    made = entry(raw.sparse, raw.w, raw.op, "leaky", (raw.out, raw.agg, raw.gate, raw.rnorm), True, MASK)
    assert same_bits(first["dA"].view(raw.n, C_in), made["dA"]) and same_bits(first["dX"].view(raw.n, C_in), made["dX"])
    assert same_bits(first["db1"], made["db1"]) and same_bits(first["db2"], made["db2"])
    raw.fresh()
    assert raw.call() == 0, lib.gnx_last_error()
    assert raw.margins_intact()
    for k in ("G1", "G2", "P", "db1", "db2", "dA", "R", "dX"):
        assert same_bits(raw.buf[k], first[k]), k
    # the bias sums are the column sums of G1 / G2 to rounding, in float64
    for k, G in (("db1", G1), ("db2", G2)):
        want = host(G[:, :7]).astype(np.float64).sum(axis=0)
        assert np.allclose(host(first[k]), want, rtol=1e-4, atol=1e-5), k


def test_refusals_name_their_cause_and_write_nothing(gnntf, world):
    raw = Raw(gnntf, world["T"])
    lib = raw.nat.lib()
    n = raw.n

    def refused(rc, code, *causes):
        message = lib.gnx_last_error()
        assert rc == code and message.startswith(b"gnx_step_back_ngcf: ") and all(c in message for c in causes), (rc, message)
        assert raw.untouched()

    refused(raw.call(C_in=48, ldx=48), -4, b"width 48 is not supported")
    shifted = torch.zeros(n * 64 + 4, device="cuda")[1:1 + n * 64]
    refused(raw.call(X=shifted), -4, b"misaligned buffer")
    refused(raw.call(ldx=66), -4, b"misaligned buffer")                      # rows that are no whole 16-byte pieces
    refused(raw.call(ldG=7), -4, b"misaligned buffer")
    refused(raw.call(C_out=65), -4, b"C_out 65 > C_in 64")
    refused(raw.call(work_floats=raw.floats - 1), -1, b"needs d_work of %d floats" % raw.floats, b"group sums of 2 * C_out floats")
    refused(raw.call(dX=raw.buf["R"]), -1, b"d_dX must be a buffer of its own")
    refused(raw.call(G2=raw.buf["G1"]), -1, b"d_G2 must be a buffer of its own")
    refused(raw.call(P=raw.X), -1, b"d_P must be a buffer of its own")
    refused(raw.call(ldx=63), -1, b"ldx 63 < C_in 64")
    refused(raw.call(rate=1.0), -1, b"dropout rate 1 outside [0, 1)")
    assert raw.call() == 0, lib.gnx_last_error()                             # the call itself is well formed
    assert not raw.untouched(("dX",)) and raw.margins_intact()


# ---- 5. the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_sided():
    """300 users and 200 items, about 2 400 user-item pairs without duplicates, stored in both directions; 16-wide features (the graph of
    tests/test_gpu_ngcf_fused.py, built again)."""
    import networkx as nx
    rng = np.random.default_rng(31)
    n_u, n_i = 300, 200
    pairs = np.unique(np.stack([rng.integers(0, n_u, size=2400), n_u + rng.integers(0, n_i, size=2400)], axis=1), axis=0)
    coo = np.concatenate([pairs, pairs[:, ::-1]]).astype(np.int64)
    G = nx.Graph(); G.add_nodes_from(range(n_u + n_i)); G.add_edges_from((int(u), int(v)) for u, v in pairs)
    X = rng.standard_normal((n_u + n_i, 16)).astype(np.float32)
    return dict(coo=coo, vals=np.ones(len(coo), dtype=np.float32), shape=(n_u + n_i, n_u + n_i), X=X, G=G, pairs=pairs)


def make_model(gnntf, data, **option):
    gnntf.set_seed(11)
    torch.manual_seed(3)
    model = gnntf.NGCF(gnntf.SparseCOO(data["coo"], data["vals"], data["shape"]), data["X"], num_classes=16, **option)
    model.reset()
    return model


class CountingLibrary:
    """The loaded library with every access to one of the NGCF entries counted."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if "ngcf" in name:
            self.calls.append(name)
        return getattr(self.real, name)


def matched_edges(data, count=90):
    """(edges, labels): a positive pair, then one negative pair of the same user, every user in one positive pair and every item in one
    pair at all -- a row of the edge scores' backward then receives at most two addends and has the same bits in whatever order they
    arrive (tests/test_gpu_ngcf_fused.py explains)."""
    users, items, positives = set(), set(), []
    for u, v in data["pairs"]:
        if u not in users and v not in items and len(positives) < count:
            users.add(int(u)), items.add(int(v)), positives.append((int(u), int(v)))
    free = [w for w in range(300, 500) if w not in items]
    edges = []
    for u, v in positives:
        w = next(w for w in free if not data["G"].has_edge(u, w))
        free.remove(w)
        edges += [(u, v), (u, w)]
    assert len(positives) == count
    return np.array(edges, dtype=np.int64), np.tile([1, 0], count)


def trained(gnntf, data, counting, capture, **option):
    import random
    sparse = gnntf.sparse

    class DeviceEdges(sparse.DeviceIndex):
        def __len__(self):
            return self.tensor.shape[0]

    random.seed(0)
    np.random.seed(0)
    model = make_model(gnntf, data, ngcf_layer="fused", feature_dropout="fused", dropout=0.25, **option)
    edges, labels = matched_edges(data)
    task = gnntf.LinkPrediction(edges, labels)
    task.edges = DeviceEdges(edges, torch.device("cuda:0"), None)
    gnntf.set_seed(11)
    torch.manual_seed(5)
    counting.calls.clear()
    model.train(train=task, epochs=2, patience=50, capture=capture,
                optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
    return [v.var.detach().clone() for v in model.vars()], list(counting.calls), model


def test_captured_training_equals_eager_and_the_default_is_untouched(gnntf, two_sided, monkeypatch):
    nat = gnntf.sparse.nat
    counting = CountingLibrary(nat.lib())
    monkeypatch.setattr(nat, "lib", lambda: counting)
    eager, eager_calls, model = trained(gnntf, two_sided, counting, False, ngcf_backward="fused")
    assert model.ngcf_backward == "fused"
    assert "gnx_step_back_ngcf" in eager_calls and "gnx_ngcf_back_gate" not in eager_calls and eager_calls.count("gnx_ngcf_step") >= 6
    captured, captured_calls, _ = trained(gnntf, two_sided, counting, True, ngcf_backward="fused")
    assert "gnx_step_back_ngcf" in captured_calls and "gnx_ngcf_back_gate" not in captured_calls
    assert len(eager) == len(captured) == 12 and all(torch.equal(e, c) for e, c in zip(eager, captured))
    # without the keyword: the entry is never looked up, and the parameters are those of ngcf_backward="composed", bit for bit
    default, default_calls, plain = trained(gnntf, two_sided, counting, False)
    named, named_calls, _ = trained(gnntf, two_sided, counting, False, ngcf_backward="composed")
    assert plain.ngcf_backward == "composed" and "gnx_step_back_ngcf" not in default_calls + named_calls
    assert "gnx_ngcf_back_gate" in default_calls and default_calls == named_calls
    assert all(torch.equal(d, m) for d, m in zip(default, named))
