"""The NGCF backward at width 128 on the MI355X (gnx_step_back_wide_ngcf, sparse.ngcf_step(wide_backward="fused"),
GNN(ngcf_wide_backward="fused")): the gate pass, one row-local launch (k_ngcf_rows_back), the transposed SpMM.

Judged as tests/test_gpu_ngcf_back.py judges the narrow backward.  Where existing code is the reference the comparison is bit for bit:
G1 / G2 against gnx_ngcf_back_gate, P against X * A, dX against gnx_spmm_tv over the entry's own dA and R.  dA, R, the bias sums and dX
are judged against the float64 references of tests/ngcf_fused_ref.py / tests/ngcf_back_ref.py with max |got - want| / bound <= 1
(tests/test_ngcf_wide_back_cpu.py checks that the bounds at C_in = 128 admit the stated rounding points and reject two broken backwards).
The shapes are those of tests/test_gpu_ngcf_wide.py -- regime T (n = 1547: a ragged last tile, hub rows, a whole tile of rows without
entries), regime S (n = 2^15 + 11: 2049 tiles, one more than 256 CUs x 8 waves, so a persistent wave takes a second tile), a graph of 5
rows, X as a view of a wider buffer (ldx = 136) -- and the reversals Tt and St of tests/test_gpu_ngcf_back.py, where the transposed
structure, which the backward's SpMM walks, has the hub rows.  C_out = 128 (a full weight image), 64 (half), 40 (a partial last block of
16), 7 (ldG = 8: a zero column inside the only step of four)."""
import functools

import numpy as np
import pytest
import torch

import ngcf_fused_ref as nref
from test_gpu_ngcf_back import FORMS, MASK, SEED, SENTINEL, STREAM, bound_of, dev, host, references, same_bits, storage, weights_csr

pytestmark = pytest.mark.gpu

NAME = "gnx_step_back_wide_ngcf"
C = 128


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


@pytest.fixture(scope="module")
def world(gnntf):
    """Regimes T and S, their reversals Tt and St and a graph of 5 rows, bipartite-normalised: the handle, its adjacency and the weights
    read back, made once and never changed; ``sets``: the rows the float64 comparisons are judged over, besides all of them."""
    out = dict()
    for name in ("T", "S", "Tt", "St", "tiny"):
        if name == "tiny":                                   # five rows, one of them (row 3) without entries
            coo = np.array([[0, 1], [1, 0], [0, 2], [2, 0], [1, 4], [4, 1], [2, 4], [4, 2]], dtype=np.int64)
            vals, shape, ragged = np.ones(len(coo), dtype=np.float32), (5, 5), np.arange(5)
        else:
            coo, vals, shape, info = nref.regime_graph(name[0])
            ragged = info["ragged"]
            if name.endswith("t"):
                coo = coo[:, ::-1].copy()
        g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
        adj = gnntf.normalize(g, "bipartite")
        A = weights_csr(g, adj.vals)
        deg, in_deg = np.diff(A.indptr), np.bincount(A.indices, minlength=shape[0])
        L = g.long_row_threshold
        sets = dict(hub_t=np.flatnonzero(in_deg > L), empty=np.flatnonzero(deg == 0), empty_t=np.flatnonzero(in_deg == 0), ragged=ragged)
        assert g.n_hub_rows_t == len(sets["hub_t"]) and len(ragged) == shape[0] % 16 > 0
        if name in ("Tt", "St"):
            assert g.n_hub_rows == 0 and len(sets["hub_t"]) == len(info["hub"]) > 0 and len(sets["empty_t"]) >= 16
        elif name in ("T", "S"):
            assert L == info["L"] and g.n_hub_rows == len(info["hub"]) > 0 and len(sets["empty"]) >= 16
        out[name] = dict(g=g, adj=adj, A=A, n=shape[0], L=L, sets=sets)
    assert out["S"]["n"] == 2 ** 15 + 11 and out["T"]["L"] != out["S"]["L"]      # both long-row regimes
    return out


@functools.lru_cache(maxsize=None)
def operands(n, C_out):
    return nref.operands(n, C, C_out, 900 + 7 * C + C_out)


def back_name(drop=False, dX=True):
    return "k_ngcf_rows_back<128>" + ("_drop" if drop else "") + ("+spmm_tv" if dX else "")


def rows_of(op, view):
    """X on the device: as it is, or as the first 128 columns of an [n, 136] buffer whose other columns hold the sentinel"""
    if not view:
        return dev(op["X"]), None
    buffer = torch.full((op["X"].shape[0], 136), SENTINEL, device="cuda")
    buffer[:, :C] = dev(op["X"])
    return buffer[:, :C], buffer


def forward(sparse, w, op, act, normalize=True, dropout=None, X=None):
    """(out, agg, gate, rnorm) of gnx_step_wide_ngcf as the training forward keeps them"""
    return sparse._ngcf_launch(w["adj"], dev(op["X"]) if X is None else X, dev(op["W1"]), dev(op["b1"]), dev(op["W2"]), dev(op["b2"]), act, keep=True,
                               dropout=dropout, normalize=normalize, wide="fused")


def entry(sparse, w, op, act, kept, normalize=True, dropout=None, X=None, **want):
    out, agg, gate, rnorm = kept
    return sparse._ngcf_wide_back_launch(w["adj"], dev(op["g"]), out if normalize else None, rnorm, gate, act, dropout,
                                         dev(op["X"]) if X is None else X, agg, dev(op["W1"]), dev(op["W2"]), **want)


# ---- 1. existing code as the reference, bit for bit -----------------------------------------------------------------------------------------
BIT_CASES = [("T", 128, False), ("T", 64, False), ("T", 40, False), ("T", 7, False), ("S", 128, False), ("S", 40, False), ("tiny", 128, False),
             ("tiny", 7, False), ("T", 40, True), ("Tt", 64, False), ("St", 7, False)]


@pytest.mark.parametrize("regime, C_out, view", BIT_CASES)
def test_bit_for_bit_against_existing_code(gnntf, world, regime, C_out, view):
    sparse, nat = gnntf.sparse, gnntf.sparse.nat
    w = world[regime]
    g, n = w["g"], w["n"]
    op = operands(n, C_out)
    X, buffer = rows_of(op, view)
    pad = (C_out + 3) // 4 * 4
    for act, normalize, dropout in FORMS:
        where = f"{regime} 128->{C_out} view={view} {act} normalize={normalize} mask={dropout is not None}"
        kept = forward(sparse, w, op, act, normalize, dropout, X)
        out, agg, gate, rnorm = kept
        made = entry(sparse, w, op, act, kept, normalize, dropout, X)
        assert g.last_kernel() == back_name(dropout is not None), (where, g.last_kernel())
        G1, G2 = sparse._ngcf_back_gate(g, dev(op["g"]), out if normalize else None, rnorm, gate, act, dropout)
        assert made["G1"].stride(0) == pad and same_bits(storage(made["G1"]), storage(G1)) and same_bits(storage(made["G2"]), storage(G2)), where
        assert not bool(storage(made["G1"])[:, C_out:].any()) and not bool(storage(made["G2"])[:, C_out:].any()), where      # zero padding
        assert float(made["G1"].abs().max()) > 0 and float(made["G2"].abs().max()) > 0
        assert same_bits(made["P"], X * agg), where
        dX = sparse._launch(w["adj"], made["dA"], made["R"], 1.0, 1.0, nat.ACT_NONE, transposed=True)
        assert same_bits(made["dX"], dX) and float(dX.abs().max()) > 0, where
        # two calls: the same bits in every output
        again = entry(sparse, w, op, act, kept, normalize, dropout, X)
        for key in ("G1", "G2", "P", "db1", "db2", "dA", "R", "dX"):
            assert same_bits(made[key], again[key]), (where, key)
    if view:
        assert bool((buffer[:, C:] == SENTINEL).all())


# ---- 2. against float64 ---------------------------------------------------------------------------------------------------------------------
F64_FORMS = [("leaky", True, None), ("leaky", True, MASK), ("leaky", False, MASK), ("relu", True, MASK), ("none", False, None)]
F64_CASES = [("T", 128, F64_FORMS), ("T", 64, F64_FORMS[:2]), ("T", 40, F64_FORMS), ("T", 7, F64_FORMS), ("S", 128, F64_FORMS[1:2]),
             ("S", 40, F64_FORMS[3:]), ("Tt", 128, F64_FORMS[:2]), ("Tt", 7, F64_FORMS[2:]), ("St", 64, F64_FORMS[1:2]), ("tiny", 128, F64_FORMS)]


@pytest.mark.parametrize("regime, C_out, forms", F64_CASES)
def test_against_float64(gnntf, world, regime, C_out, forms):
    sparse = gnntf.sparse
    w = world[regime]
    op = operands(w["n"], C_out)
    worst = 0.0
    for act, normalize, dropout in forms:
        where = f"{regime} 128->{C_out} {act} normalize={normalize} mask={dropout is not None}"
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
    print(f"{regime} 128->{C_out}: the largest error / bound = {worst:.3g}")


# ---- 3. / 4. determinism, padding, sentinels, refusals ----------------------------------------------------------------------------------------
class Raw:
    """One direct call of gnx_step_back_wide_ngcf, 128 -> C_out into rows of stride roundup4(C_out) + ``extra``, every output inside
    sentinels; the upstream gradient has four columns of NaN behind its last: nothing may read them."""
    PAD = 64

    def __init__(self, gnntf, w, C_out=7, view=False, extra=0):
        self.sparse, self.nat, self.w, self.C_out = gnntf.sparse, gnntf.sparse.nat, w, C_out
        n = self.n = w["n"]
        self.op = op = operands(n, C_out)
        self.X, self.buffer = rows_of(op, view)
        self.ldx = self.X.stride(0)
        self.out, self.agg, self.gate, self.rnorm = forward(self.sparse, w, op, "leaky", True, MASK, self.X)
        self.pad = (C_out + 3) // 4 * 4
        self.ldG = ldG = self.pad + extra
        up = torch.full((n, ldG + 4), float("nan"), device="cuda")
        up[:, :C_out] = dev(op["g"])
        self.up = up
        self.W1, self.W2 = dev(op["W1"]), dev(op["W2"])
        self.floats = self.sparse._ngcf_wide_back_work_floats(n, C_out)
        self.sizes = dict(G1=n * ldG, G2=n * ldG, P=n * C, db1=C_out, db2=C_out, dA=n * C, R=n * C, dX=n * C, work=self.floats)
        self.fresh()

    def fresh(self):
        self.whole = {k: torch.full((2 * self.PAD + size,), SENTINEL, device="cuda") for k, size in self.sizes.items()}
        self.buf = {k: t[self.PAD:self.PAD + self.sizes[k]] for k, t in self.whole.items()}

    def call(self, **change):
        nat, b = self.nat, self.buf
        a = dict(X=self.X, ldx=self.ldx, C_in=C, C_out=self.C_out, ldG=self.ldG, work_floats=self.floats, dX=b["dX"], G2=b["G2"], P=b["P"], rate=MASK[0])
        a.update(change)
        ldw = self.C_out
        return nat.lib().gnx_step_back_wide_ngcf(
            self.w["g"].handle, nat.ptr(self.w["adj"].transposed_values()), nat.ptr(self.up), self.up.stride(0), nat.ptr(self.out), self.out.stride(0),
            nat.ptr(self.rnorm), nat.ptr(self.gate), a["C_out"], nat.ACT_LEAKY, a["rate"], SEED, STREAM, nat.ptr(a["X"]), a["ldx"], nat.ptr(self.agg),
            a["C_in"], nat.ptr(self.W1), ldw, nat.ptr(self.W2), ldw, nat.ptr(b["G1"]), nat.ptr(a["G2"]), a["ldG"], nat.ptr(a["P"]), nat.ptr(b["db1"]),
            nat.ptr(b["db2"]), nat.ptr(b["dA"]), nat.ptr(b["R"]), nat.ptr(a["dX"]), C, nat.ptr(b["work"]), a["work_floats"], nat.current_stream())

    def untouched(self, keys=None):
        torch.cuda.synchronize()
        return all(bool((self.whole[k] == SENTINEL).all()) for k in (keys or self.whole))

    def margins_intact(self):
        torch.cuda.synchronize()
        P = self.PAD
        return all(bool((t[:P] == SENTINEL).all()) and bool((t[P + self.sizes[k]:] == SENTINEL).all()) for k, t in self.whole.items())


OUTPUTS = ("G1", "G2", "P", "db1", "db2", "dA", "R", "dX")


@pytest.mark.parametrize("regime, C_out, view, extra", [("T", 7, False, 0), ("T", 7, False, 4), ("T", 40, False, 0), ("T", 128, False, 0),
                                                        ("T", 64, True, 8), ("S", 128, False, 0), ("tiny", 7, False, 0), ("tiny", 128, False, 4)])
def test_two_calls_same_bits_padding_and_sentinels(gnntf, world, regime, C_out, view, extra):
    """Nothing is written past the last column or the last row of any output -- on regime T (a ragged tile), on regime S (a wave's second
    tile), on the graph of 5 rows (11 dead rows in the only tile) and with X as a view --, every element inside is written, the padding
    of G1 / G2 is zero up to roundup4(C_out) and untouched behind it where ldG is wider, the NaN behind g's last column reaches nothing,
    and a second call gives the same bits."""
    raw = Raw(gnntf, world[regime], C_out, view, extra)
    lib, n, ldG, pad = raw.nat.lib(), raw.n, raw.ldG, raw.pad
    assert raw.call() == 0, lib.gnx_last_error()
    assert world[regime]["g"].last_kernel() == back_name(True)
    assert raw.margins_intact()
    first = {k: v.clone() for k, v in raw.buf.items()}
    G1, G2 = first["G1"].view(n, ldG), first["G2"].view(n, ldG)
    for k in OUTPUTS:
        inside = first[k].view(n, ldG)[:, :pad] if k in ("G1", "G2") else first[k]
        assert not bool((inside == SENTINEL).any()), k             # every element of every output was written
        assert bool(torch.isfinite(first[k]).all()), k             # the NaN in the padding of g reached nothing
    assert not bool(G1[:, C_out:pad].any()) and not bool(G2[:, C_out:pad].any()) and bool(G1[:, :C_out].any())      # the padding columns: zeros
    assert bool((G1[:, pad:] == SENTINEL).all()) and bool((G2[:, pad:] == SENTINEL).all())                          # ... and nothing behind them
    if view:
        assert bool((raw.buffer[:, C:] == SENTINEL).all())
    # ... and the results are those of the helper's call over the same operands (whose g has no padding at all)
    made = entry(raw.sparse, raw.w, raw.op, "leaky", (raw.out, raw.agg, raw.gate, raw.rnorm), True, MASK, raw.X)
    assert same_bits(first["dA"].view(n, C), made["dA"]) and same_bits(first["dX"].view(n, C), made["dX"])
    assert same_bits(first["db1"], made["db1"]) and same_bits(first["db2"], made["db2"])
    raw.fresh()
    assert raw.call() == 0, lib.gnx_last_error()
    assert raw.margins_intact()
    for k in OUTPUTS:
        assert same_bits(raw.buf[k], first[k]), k
    # the bias sums are the column sums of G1 / G2 to rounding, in float64
    for k, G in (("db1", G1), ("db2", G2)):
        want = host(G[:, :C_out]).astype(np.float64)
        assert np.allclose(host(first[k]), want.sum(axis=0), rtol=0, atol=(n + 8) * 2.0 ** -24 * np.abs(want).sum(axis=0).max()), k


@pytest.mark.parametrize("C_out", [7, 128])
def test_without_dX_nothing_but_P_and_the_sums(gnntf, world, C_out):
    """d_dX == NULL: no products and no SpMM -- dA and R keep their sentinels, the name carries no "+spmm_tv" -- while G1, G2, P and the
    bias sums are the full call's; with d_P NULL too, P stays untouched as well."""
    raw = Raw(gnntf, world["T"], C_out)
    lib = raw.nat.lib()
    assert raw.call() == 0, lib.gnx_last_error()
    full = {k: v.clone() for k, v in raw.buf.items()}
    raw.fresh()
    assert raw.call(dX=None) == 0, lib.gnx_last_error()
    assert world["T"]["g"].last_kernel() == back_name(True, dX=False)
    assert raw.untouched(("dA", "R", "dX")) and raw.margins_intact()
    for k in ("G1", "G2", "P", "db1", "db2"):
        assert same_bits(raw.buf[k], full[k]), k
    raw.fresh()
    assert raw.call(dX=None, P=None) == 0, lib.gnx_last_error()
    assert world["T"]["g"].last_kernel() == back_name(True, dX=False)
    assert raw.untouched(("dA", "R", "dX", "P")) and raw.margins_intact()
    for k in ("G1", "G2", "db1", "db2"):
        assert same_bits(raw.buf[k], full[k]), k


def test_refusals_name_their_cause_and_write_nothing(gnntf, world):
    raw = Raw(gnntf, world["T"])
    lib = raw.nat.lib()
    n = raw.n

    def refused(rc, code, *causes):
        message = lib.gnx_last_error()
        assert rc == code and message.startswith(NAME.encode() + b": ") and all(c in message for c in causes), (rc, message)
        assert raw.untouched()

    refused(raw.call(work_floats=raw.floats - 1), -1, b"needs d_work of %d floats" % raw.floats, b"slabs of 2 * C_out floats")
    refused(raw.call(dX=raw.buf["R"]), -1, b"d_dX must be a buffer of its own")
    refused(raw.call(C_in=64, ldx=64), -4, b"widths 64 -> 7 are not supported", b"keep the composed backward elsewhere")
    shifted = torch.zeros(n * C + 4, device="cuda")[1:1 + n * C]
    refused(raw.call(X=shifted), -4, b"misaligned rows", b"keep the composed backward elsewhere")
    refused(raw.call(ldx=130), -4, b"misaligned rows (ldx 130")              # rows that are no whole 16-byte pieces
    refused(raw.call(ldG=7), -4, b"misaligned rows")
    refused(raw.call(C_out=129), -4, b"widths 128 -> 129 are not supported")
    refused(raw.call(G2=raw.buf["G1"]), -1, b"d_G2 must be a buffer of its own")
    refused(raw.call(P=raw.X), -1, b"d_P must be a buffer of its own")
    refused(raw.call(ldx=127), -1, b"ldx 127 < C_in 128")
    refused(raw.call(rate=1.0), -1, b"dropout rate 1 outside [0, 1)")
    assert raw.call() == 0, lib.gnx_last_error()                             # the call itself is well formed
    assert not raw.untouched(("dX",)) and raw.margins_intact()


# ---- 5. under autograd ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime, C_out", [("T", 128), ("T", 7), ("S", 40)])
def test_autograd_against_float64(gnntf, world, regime, C_out):
    sparse = gnntf.sparse
    w = world[regime]
    g, n = w["g"], w["n"]
    op = operands(n, C_out)
    names = ("X", "W1", "b1", "W2", "b2")
    up = dev(op["g"])
    for dropout, normalize in ((None, True), (MASK, True), (MASK, False)) if regime == "T" else ((MASK, True),):
        where = f"{regime} 128->{C_out} mask={dropout is not None} normalize={normalize}"
        leaves = [dev(op[k]).requires_grad_() for k in names]
        out = gnntf.ngcf_step(w["adj"], *leaves, activation="leaky", dropout=dropout, normalize=normalize, wide="fused", wide_backward="fused")
        plain = [dev(op[k]).requires_grad_() for k in names]
        composed = gnntf.ngcf_step(w["adj"], *plain, activation="leaky", dropout=dropout, normalize=normalize, wide="fused")
        assert same_bits(out, composed), where                     # the forward does not know the keyword
        out.backward(up, retain_graph=True)
        assert g.last_kernel() == back_name(dropout is not None), where
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
        # ... and after the composed forward (gnx_ngcf_step) the route is the same: what is saved has one format
        mixed = [dev(op[k]).requires_grad_() for k in names]
        gnntf.ngcf_step(w["adj"], *mixed, activation="leaky", dropout=dropout, normalize=normalize, wide_backward="fused").backward(up)
        assert g.last_kernel() == back_name(dropout is not None), where


def test_backward_fused_alone_stays_inert_at_128(gnntf, world):
    w = world["T"]
    op = operands(w["n"], 40)
    names = ("X", "W1", "b1", "W2", "b2")
    grads = dict()
    for how in ("composed", "fused"):
        leaves = [dev(op[k]).requires_grad_() for k in names]
        out = gnntf.ngcf_step(w["adj"], *leaves, activation="leaky", dropout=MASK, backward=how, wide="fused")
        out.backward(dev(op["g"]))
        assert "k_ngcf_rows_back" not in w["g"].last_kernel()
        grads[how] = [leaf.grad for leaf in leaves]
    assert all(torch.equal(a, b) for a, b in zip(grads["composed"], grads["fused"]))


def test_autograd_launches_what_is_needed(gnntf, world, monkeypatch):
    """X.requires_grad = False: no products, no transposed SpMM -- the entry reports no "+spmm_tv"; W1 without a gradient: no P."""
    sparse = gnntf.sparse
    w = world["T"]
    op = operands(w["n"], 7)
    seen = []
    real = sparse._ngcf_wide_back_launch

    def spy(*args, **kwargs):
        made = real(*args, **kwargs)
        seen.append((w["g"].last_kernel(), kwargs, {k: v is not None for k, v in made.items()}))
        return made

    monkeypatch.setattr(sparse, "_ngcf_wide_back_launch", spy)
    for frozen, name in ((("X",), back_name(True, dX=False)), (("W1", "b2"), back_name(True)), ((), back_name(True))):
        leaves = [dev(op[k]).requires_grad_(k not in frozen) for k in ("X", "W1", "b1", "W2", "b2")]
        out = gnntf.ngcf_step(w["adj"], *leaves, activation="leaky", dropout=MASK, wide="fused", wide_backward="fused")
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


# ---- 6. the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_sided():
    """300 users and 200 items, about 2 400 user-item pairs without duplicates, stored in both directions; features without columns (the
    graph of tests/test_gpu_ngcf_wide.py, built again)."""
    rng = np.random.default_rng(31)
    n_u, n_i = 300, 200
    pairs = np.unique(np.stack([rng.integers(0, n_u, size=2400), n_u + rng.integers(0, n_i, size=2400)], axis=1), axis=0)
    coo = np.concatenate([pairs, pairs[:, ::-1]]).astype(np.int64)
    return dict(coo=coo, vals=np.ones(len(coo), dtype=np.float32), shape=(n_u + n_i, n_u + n_i), pairs=pairs, n_u=n_u)


def run_training(gnntf, data, capture, kernels, epochs=3, **option):
    """The shape of the reference's library_recommendation demo -- Structural(dims=128) over empty features, the 3-layer
    NGCF(num_classes=128) -- with the mask in the launch and negatives drawn on the device."""
    import random
    random.seed(0)
    np.random.seed(0)
    gnntf.set_seed(11)
    torch.manual_seed(3)
    n = data["shape"][0]
    model = gnntf.NGCF(gnntf.SparseCOO(data["coo"], data["vals"], data["shape"]), np.zeros((n, 0), dtype=np.float32), num_classes=128,
                       preprocessor=gnntf.Structural(dims=128, regularize=0, bipartite=data["n_u"]), ngcf_layer="fused", ngcf_wide="fused",
                       feature_dropout="fused", dropout=0.25, **option)
    model.reset()
    start = [v.var.detach().clone() for v in model.vars()]
    positives = data["pairs"][::25]
    sampler = gnntf.device_negative_sampling(positives, model, negative_nodes=np.arange(300, 500))
    task = gnntf.LinkPrediction(sampler)
    torch.manual_seed(5)
    del kernels[:]
    model.train(train=task, epochs=epochs, patience=50, capture=capture, verbose=False,
                optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
    assert sampler.fallbacks() == 0
    return [v.var.detach().clone() for v in model.vars()], start, model


def test_captured_training_equals_eager_and_every_layer_takes_the_entry(gnntf, two_sided, monkeypatch):
    sparse = gnntf.sparse
    kernels = []
    real = sparse._ngcf_wide_back_launch

    def spy(adj, *args, **kwargs):
        made = real(adj, *args, **kwargs)
        kernels.append(adj.graph.last_kernel())
        return made

    monkeypatch.setattr(sparse, "_ngcf_wide_back_launch", spy)
    eager, start, model = run_training(gnntf, two_sided, False, kernels, ngcf_wide_backward="fused")
    assert model.ngcf_wide_backward == "fused"
    # three layers a step, each layer's backward the new launch with the mask and -- its input needs a gradient -- the transposed SpMM
    assert len(kernels) >= 3 * 3 and len(kernels) % 3 == 0 and set(kernels) == {back_name(True)}, kernels
    captured, _, _ = run_training(gnntf, two_sided, True, kernels, ngcf_wide_backward="fused")
    assert len(kernels) >= 3 and set(kernels) == {back_name(True)}, kernels
    assert len(eager) == len(captured) >= 14 and all(torch.equal(e, c) for e, c in zip(eager, captured))
    assert any(not torch.equal(s, e) for s, e in zip(start, eager))                     # ... and it trained
    # without the keyword the entry is never reached
    _, _, plain = run_training(gnntf, two_sided, False, kernels)
    assert plain.ngcf_wide_backward == "composed" and kernels == []
