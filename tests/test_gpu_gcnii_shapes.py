"""The GCNII layer family on the MI355X against float64 at every long-row regime of build_long_plan (tests/gcnii_shapes_ref.py: the
structures, the references, the derived bound; tests/test_gcnii_shapes_cpu.py shows that the bound discriminates).
Regime T (n = 1547: threshold 512, 23 hub rows = two MFMA tiles of the row list, the second ragged) and regime S (n = 2^15 + 11:
threshold and chunk 128, 154 hub rows = two blocks of the dense kernel over the row list), each as handle ``a`` (hub rows in the forward
structure) and ``t`` (its transpose: hub rows only in the transposed structure, which the backward walks); rows of exactly L - 1, L,
L + 1, 2 L, 2 L + 1 entries; the regime boundary itself; the drop and bf16 entries at these structures; a row window; a pitched M;
raw values; a seeded sweep.  The criterion against float64 is max |got - want| / bound <= 1 everywhere; the relations between
entries are bitwise.  Measured ratios: profiles/NOTES.md, "GCNII at every long-row regime"."""
import functools

import numpy as np
import pytest
import torch

import gcnii_shapes_ref as ref
from oracle import gnntf_oracle as orc

pytestmark = pytest.mark.gpu

A_MIX = 0.1
FUSED, COMPOSED = (16, 32, 64), 40
WIDTHS = FUSED + (COMPOSED,)
RATES = (0.6, 0.25)
SEED, STREAM = 7, 2
KEYS = [("T", "a"), ("T", "t"), ("S", "a"), ("S", "t")]
RATIOS = {}                                            # (entry, regime) -> the worst error / bound seen (printed by the last test)


def forward_name(C, suffix=""):
    return ("spmm_gcnii_mfma" if C in FUSED else "spmm+dense_mfma") + suffix


def backward_name(C):
    return "spmm_gcnii_back_mfma" if C in FUSED else "dense+spmm_back"


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()            # (a copy: the shared operands are read-only)


def poisoned(n, C, dtype=torch.float32):
    """A result buffer full of NaN: a row that no path writes stays visible (torch.empty may hand back an earlier result)."""
    return torch.full((n, C), float("nan"), dtype=dtype, device="cuda")


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


class Handle:
    """A graph on the device, its symmetric normalisation, the un-normalised adjacency, and the float32 weights the kernels read as
    float64 CSR matrices (tests/test_gpu_gcnii_bf16.py's Case: the normalisation's own rounding stays out of the comparison)."""

    made = 0

    def __init__(self, gnntf, coo, vals, shape, window=0, adj_vals=None):
        import scipy.sparse as sp
        Handle.made += 1
        self.uid = Handle.made                                     # what the cached references are keyed by
        self.g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
        if window:
            self.g.set_row_window(window)
        self.adj = gnntf.normalize(self.g, "symmetric") if adj_vals is None else gnntf.Adjacency(self.g, adj_vals, None)
        self.raw = gnntf.Adjacency(self.g)
        rowptr, colidx, raw = (x.cpu().numpy() for x in self.g.csr_arrays())
        self.n = shape[0]
        self.A = sp.csr_matrix((self.adj.vals.cpu().numpy().astype(np.float64), colidx, rowptr), shape=shape)
        self.A_raw = sp.csr_matrix((raw.astype(np.float64), colidx, rowptr), shape=shape)
        self.L = ref.plan_threshold(self.n)
        self.deg, self.in_deg = np.diff(rowptr), np.bincount(colidx, minlength=self.n)
        self.hub, self.hub_t = np.flatnonzero(self.deg > self.L), np.flatnonzero(self.in_deg > self.L)
        self.empty, self.no_in = np.flatnonzero(self.deg == 0), np.flatnonzero(self.in_deg == 0)
        self.ragged = np.arange(self.n - self.n % 16, self.n)


def make_handle(gnntf, regime, kind, seed=0, window=0, adj_vals=None):
    coo, vals, shape, info = ref.regime_graph(regime, seed)
    h = Handle(gnntf, coo if kind == "a" else coo[:, ::-1].copy(), vals, shape, window, adj_vals)
    h.info, h.regime, h.kind = info, regime, kind
    mine, other = (h.hub, h.hub_t) if kind == "a" else (h.hub_t, h.hub)
    assert np.array_equal(mine, info["hub"]) and len(other) == 0                     # hub rows in ONE of the two structures
    assert len(mine) > (16 if regime == "T" else 128)
    return h


@pytest.fixture(scope="module")
def handles(gnntf):
    """Made once, never re-planned or changed.  When the module is done, everything it cached on the device and the host goes."""
    yield {key: make_handle(gnntf, *key) for key in KEYS}
    for cache in (_device_operands, _references, _sweep_handles):
        cache.clear()
    for cached in (operands, keep_mask):
        cached.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def operands(n, C):
    return ref.operands(n, C, seed=1000 + C)


_device_operands = {}


def device_operands(n, C):
    if (n, C) not in _device_operands:
        _device_operands[n, C] = {k: dev(v) for k, v in operands(n, C).items()}
    return _device_operands[n, C]


_references = {}


def want_forward(h, C, relu, a=A_MIX, A=None, tag="adj"):
    """The float64 forward of handle ``h`` at width C: computed once per (handle, width, a, weights), relu applied on a copy."""
    key = ("f", h.uid, C, a, tag)
    if key not in _references:
        op = operands(h.n, C)
        _references[key] = ref.forward_ref(h.A if A is None else A, op["H"], op["H0"], op["M"], a, False)
    want = dict(_references[key])
    if relu:
        want["out"] = np.maximum(want["out"], 0.0)
    return want


def want_backward(h, C, s_alpha, a=A_MIX, A=None, tag="adj"):
    key = ("b", h.uid, C, a, tag, s_alpha)
    if key not in _references:
        op = operands(h.n, C)
        _references[key] = ref.backward_ref(h.A if A is None else A, op["G"], op["Mt"], a, op["S_in"], s_alpha)
    return _references[key]


def within(entry, h, got, want, bound, rows=None, what="all rows"):
    """The criterion, recorded per entry and regime."""
    r = ref.ratio(host(got) if torch.is_tensor(got) else got, want, bound, rows)
    RATIOS[entry, h.regime] = max(RATIOS.get((entry, h.regime), 0.0), r)
    assert r <= 1.0, f"{entry}, regime {h.regime}, handle {h.kind}, {what}: error / bound = {r:.3f}"
    return r


@functools.lru_cache(maxsize=None)
def keep_mask(p, n, C):
    """The mask in numpy, from the oracle's integers: kept iff hash_u24(seed, stream, row, col, 0) >= dropout_threshold(p)."""
    rows, cols = np.repeat(np.arange(n), C), np.tile(np.arange(C), n)
    keep = (orc.hash_u24(SEED, STREAM, rows, cols, np.zeros(n * C, dtype=np.int64)) >= orc.dropout_threshold(p)).reshape(n, C)
    keep.setflags(write=False)
    return keep


def dropped(x, keep, p):
    assert x.dtype == np.float32
    return np.where(keep, x * (np.float32(1.0) / (np.float32(1.0) - np.float32(p))), np.float32(0))


def raw_forward(gnntf, h, C, relu, adj=None, M=None, a=A_MIX, dropout=None, H=None):
    """gnx_gcnii_step / gnx_gcnii_step_drop themselves into poisoned buffers: (out, T), every element written."""
    nat = gnntf.sparse.nat
    d = device_operands(h.n, C)
    adj, M, H = h.adj if adj is None else adj, d["M"] if M is None else M, d["H"] if H is None else H
    out, mixed = poisoned(h.n, C), poisoned(h.n, C)
    layer = (h.g.handle, nat.ptr(adj.vals), nat.ptr(H), nat.ptr(d["H0"]), float(a), C, nat.ptr(M), M.stride(0), nat.ACT_RELU if relu else nat.ACT_NONE)
    if dropout is not None:
        nat.check(nat.lib().gnx_gcnii_step_drop(*layer, *dropout, nat.ptr(out), nat.ptr(mixed), nat.current_stream()))
    else:
        nat.check(nat.lib().gnx_gcnii_step(*layer, nat.ptr(out), nat.ptr(mixed), nat.current_stream()))
    assert h.g.last_kernel() == forward_name(C, "_drop" if dropout is not None else "")
    assert not torch.isnan(out).any() and not torch.isnan(mixed).any(), "a row was written by no path"
    return out, mixed


def run_forward(gnntf, h, C, relu, adj=None, M=None, a=A_MIX):
    """(out of the inference launch, out and T of the training launch) with the names checked; the training launch's results are
    the bits of the C entry's over poisoned buffers."""
    d = device_operands(h.n, C)
    adj, M = h.adj if adj is None else adj, d["M"] if M is None else M
    out = gnntf.gcnii_step(adj, d["H"], d["H0"], a, M, relu=relu)
    assert h.g.last_kernel() == forward_name(C)
    out_T, T = gnntf.sparse._gcnii_launch(adj, d["H"], d["H0"], a, M, relu, keep_mixed=True)
    assert h.g.last_kernel() == forward_name(C)
    raw_out, raw_T = raw_forward(gnntf, h, C, relu, adj, M, a)
    assert torch.equal(bits(raw_out), bits(out_T)) and torch.equal(bits(raw_T), bits(T))
    return out, out_T, T


def run_backward(gnntf, h, C, s_alpha, adj=None, Mt=None, a=A_MIX):
    d = device_operands(h.n, C)
    adj, Mt = h.adj if adj is None else adj, d["Mt"] if Mt is None else Mt
    dH, S = gnntf.gcnii_step_back(adj, d["G"], a, Mt, S_in=d["S_in"], s_alpha=s_alpha)
    assert h.g.last_kernel() == backward_name(C)
    return dH, S


# ---- 1. the forward against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("key", KEYS, ids="-".join)
def test_forward_against_float64(gnntf, handles, key, C, relu):
    h = handles[key]
    want = want_forward(h, C, relu)
    out, out_T, T = run_forward(gnntf, h, C, relu)
    assert torch.equal(bits(out_T), bits(out))                                       # the training launch: the inference launch's bits
    got, got_T = host(out), host(T)
    within("gnx_gcnii_step out", h, got, want["out"], want["out_bound"])
    within("gnx_gcnii_step T", h, got_T, want["T"], want["T_bound"])
    if h.kind == "a":
        L, rows_of = h.L, h.info["rows_of"]
        classes = [(f"the row of {d} entries (L = {L})", rows_of[d]) for d in (L - 1, L, L + 1, 2 * L, 2 * L + 1)]
        classes += [("the ragged last tile", h.ragged), ("row n - 1", [h.n - 1]), ("row 0", [0]), ("the hub rows", h.hub)]
        for what, rows in classes:
            within("gnx_gcnii_step out", h, got, want["out"], want["out_bound"], rows, what)
            within("gnx_gcnii_step T", h, got_T, want["T"], want["T_bound"], rows, what)
    # rows without entries: act((alpha H0) M)
    op = operands(h.n, C)
    assert len(h.empty) >= (17 if h.kind == "a" else 3)
    alpha = ref.mix_constants(A_MIX)[1]
    lone = (alpha * ref.f64(op["H0"][h.empty])) @ ref.f64(op["M"])
    lone_bound = (C + 6) * ref.U32 * ((alpha * np.abs(ref.f64(op["H0"][h.empty]))) @ np.abs(ref.f64(op["M"])))
    r = ref.ratio(got[h.empty], np.maximum(lone, 0.0) if relu else lone, lone_bound)
    assert r <= 1.0, f"rows without entries: error / bound = {r:.3f}"


# ---- 2. the backward against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s_alpha", [1.0, 0.5])
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("key", KEYS, ids="-".join)
def test_backward_against_float64(gnntf, handles, key, C, s_alpha):
    nat = gnntf.sparse.nat
    h = handles[key]
    want = want_backward(h, C, s_alpha)
    dH, S = run_backward(gnntf, h, C, s_alpha)
    got_dH, got_S = host(dH), host(S)
    within("gnx_gcnii_step_back dH", h, got_dH, want["dH"], want["dH_bound"])
    within("gnx_gcnii_step_back S", h, got_S, want["S"], want["S_bound"])
    assert len(h.no_in) >= 3 and (got_dH[h.no_in] == 0).all()                        # rows without in-entries: dH = 0 exactly, written
    if h.kind == "t":       # the hub rows of the transposed structure: more than one tile / block of the row list, transformed in place in dH
        assert len(h.hub_t) > (16 if h.regime == "T" else 128)
        within("gnx_gcnii_step_back dH", h, got_dH, want["dH"], want["dH_bound"], h.hub_t, "the hub rows of the transposed structure")
        L, rows_of = h.L, h.info["rows_of"]
        for d in (L - 1, L, L + 1, 2 * L, 2 * L + 1):
            within("gnx_gcnii_step_back dH", h, got_dH, want["dH"], want["dH_bound"], rows_of[d], f"the row of {d} entries (L = {L})")
        within("gnx_gcnii_step_back dH", h, got_dH, want["dH"], want["dH_bound"], h.ragged, "the ragged last tile")
    # A in place of A^T is far outside: the check is not vacuous
    op = operands(h.n, C)
    wrong = ref.backward_ref(h.A.T, op["G"], op["Mt"], A_MIX)
    assert ref.ratio(got_dH, wrong["dH"], wrong["dH_bound"]) > 100
    # in place: S_in is S_out (the raw entry)
    d = device_operands(h.n, C)
    running, dH2 = d["S_in"].clone(), torch.full_like(d["G"], float("nan"))
    work = torch.empty_like(d["G"]) if C not in FUSED else None
    nat.check(nat.lib().gnx_gcnii_step_back(h.g.handle, nat.ptr(h.adj.transposed_values()), nat.ptr(d["G"]), A_MIX, C, nat.ptr(d["Mt"]), C,
                                            nat.ptr(dH2), nat.ptr(running), s_alpha, nat.ptr(running), nat.ptr(work), nat.current_stream()))
    assert not torch.isnan(dH2).any(), "a row of dH was written by no path"
    assert torch.equal(bits(running), bits(S)) and torch.equal(bits(dH2), bits(dH))


# ---- 3. the regime boundary -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["a", "t"])
@pytest.mark.parametrize("n", ref.BOUNDARY_NS)
def test_regime_boundary(gnntf, n, kind):
    """The same 300-entry row at n = 2^15 - 1 (threshold 512: a short row) and n = 2^15 (threshold 128: a hub row of three chunks)."""
    coo, vals, shape = ref.boundary_graph(n)
    h = Handle(gnntf, coo if kind == "a" else coo[:, ::-1].copy(), vals, shape)
    h.regime, h.kind = f"boundary n={n}", kind
    small = n >= ref.TINY_ROWS
    assert h.L == (128 if small else 512)
    if kind == "a":
        assert h.deg[ref.BOUNDARY_ROW] == ref.BOUNDARY_LEN and np.array_equal(h.hub, [ref.BOUNDARY_ROW] if small else [])
        with torch.no_grad():                                       # the probe of test_the_shaped_graph_has_a_long_row
            gnntf.spmm(h.adj, dev(np.ones((n, 16), dtype=np.float32)), storage=torch.bfloat16)
        name = h.g.last_kernel()
        assert ("+chunks" in name or "+long" in name) == small, name
    else:
        assert h.in_deg[ref.BOUNDARY_ROW] == ref.BOUNDARY_LEN and np.array_equal(h.hub_t, [ref.BOUNDARY_ROW] if small else []) and len(h.hub) == 0
    for C in WIDTHS:
        want = want_forward(h, C, True)
        out, out_T, T = run_forward(gnntf, h, C, True)
        assert torch.equal(bits(out_T), bits(out))
        for rows, what in ((None, "all rows"), ([ref.BOUNDARY_ROW], "the 300-entry row")):
            within("gnx_gcnii_step out", h, out, want["out"], want["out_bound"], rows, what)
            within("gnx_gcnii_step T", h, T, want["T"], want["T_bound"], rows, what)
        back = want_backward(h, C, 0.5)
        dH, S = run_backward(gnntf, h, C, 0.5)
        for rows, what in ((None, "all rows"), ([ref.BOUNDARY_ROW], "the 300-entry row")):
            within("gnx_gcnii_step_back dH", h, dH, back["dH"], back["dH_bound"], rows, what)
        within("gnx_gcnii_step_back S", h, S, back["S"], back["S_bound"])
    for key in [k for k in _references if k[1] == h.uid]:           # the handle goes: so do its references
        del _references[key]


# ---- 4. drop at the new structures ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("key", KEYS, ids="-".join)
def test_drop_is_the_plain_entry_times_the_mask(gnntf, handles, key, C, p):
    sparse = gnntf.sparse
    h = handles[key]
    d = device_operands(h.n, C)
    keep = keep_mask(p, h.n, C)
    for relu in (True, False):
        plain, _, T_plain = run_forward(gnntf, h, C, relu)
        got = gnntf.gcnii_step(h.adj, d["H"], d["H0"], A_MIX, d["M"], relu=relu, dropout=(p, SEED, STREAM))
        assert h.g.last_kernel() == forward_name(C, "_drop")
        want = dropped(host(plain), keep, p)
        np.testing.assert_array_equal(host(got), want)
        assert not np.signbit(host(got)[~keep]).any()                                # dropped: +0
        out_T, T = sparse._gcnii_launch(h.adj, d["H"], d["H0"], A_MIX, d["M"], relu, keep_mixed=True, dropout=(p, SEED, STREAM))
        assert h.g.last_kernel() == forward_name(C, "_drop")
        assert torch.equal(bits(T), bits(T_plain)) and torch.equal(bits(out_T), bits(got))
        raw_out, raw_T = raw_forward(gnntf, h, C, relu, dropout=(p, SEED, STREAM))
        assert torch.equal(bits(raw_out), bits(got)) and torch.equal(bits(raw_T), bits(T_plain))
        if not relu and h.kind == "a":      # not vacuous where the mask is a pass over the row list, and in the partial tile
            for rows in (h.hub, h.ragged):
                assert 0 < keep[rows].mean() < 1
                np.testing.assert_array_equal(host(got)[rows] != 0, keep[rows] & (host(plain)[rows] != 0))
                assert (host(got)[rows] != 0).any() and (host(got)[rows] == 0).any()


# ---- 5. the bf16 forms at the new structures --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("key,C", [(key, C) for key in KEYS for C in FUSED] + [(key, 24) for key in KEYS if key[0] == "S"],
                         ids=lambda v: "-".join(v) if isinstance(v, tuple) else str(v))
def test_bf16_inference_entry_gives_the_bits_of_the_f32_entry(gnntf, handles, key, C, relu):
    sparse = gnntf.sparse
    h = handles[key]
    d = device_operands(h.n, C)
    Hb = sparse.to_bf16(d["H"])
    want, _ = raw_forward(gnntf, h, C, relu, H=Hb.float())
    assert torch.equal(bits(gnntf.gcnii_step(h.adj, Hb.float(), d["H0"], A_MIX, d["M"], relu=relu)), bits(want))
    got = sparse._gcnii_launch_bf16(h.adj, Hb, d["H0"], A_MIX, d["M"], relu, False, out=poisoned(h.n, C), work=poisoned(h.n, C))
    assert h.g.last_kernel() == forward_name(C, "_bf16") and got.dtype == torch.float32
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(gnntf.gcnii_step(h.adj, Hb, d["H0"], A_MIX, d["M"], relu=relu, storage=torch.bfloat16)), bits(want))
    rounded = sparse._gcnii_launch_bf16(h.adj, Hb, d["H0"], A_MIX, d["M"], relu, True, out=poisoned(h.n, C, torch.bfloat16), work=poisoned(h.n, C))
    assert h.g.last_kernel() == forward_name(C, "_bf16") and rounded.dtype == torch.bfloat16
    assert torch.equal(bits(rounded), bits(sparse.to_bf16(want)))
    via_option = gnntf.gcnii_step(h.adj, Hb, d["H0"], A_MIX, d["M"], relu=relu, storage=torch.bfloat16, out_storage=torch.bfloat16)
    assert torch.equal(bits(via_option), bits(rounded))


@pytest.mark.parametrize("p", [0.6, 0.0])
@pytest.mark.parametrize("C", FUSED)
@pytest.mark.parametrize("key", KEYS, ids="-".join)
def test_bf16_training_pair_gives_the_bits_of_the_f32_pair(gnntf, handles, key, C, p):
    sparse = gnntf.sparse
    h = handles[key]
    d = device_operands(h.n, C)
    nat = sparse.nat
    triple = (p, SEED, STREAM) if p > 0 else None
    Hb = sparse.to_bf16(d["H"])
    for relu in (True, False):
        want_out, want_T = raw_forward(gnntf, h, C, relu, dropout=triple, H=Hb.float())
        for out_bf16 in (0, 1):                                     # the C entry itself, every buffer poisoned
            out, T, work = poisoned(h.n, C, torch.bfloat16 if out_bf16 else torch.float32), poisoned(h.n, C), poisoned(h.n, C)
            nat.check(nat.lib().gnx_gcnii_step_train_bf16(h.g.handle, nat.ptr(h.adj.vals), nat.ptr(Hb), nat.ptr(d["H0"]), A_MIX, C, nat.ptr(d["M"]), C,
                                                          nat.ACT_RELU if relu else nat.ACT_NONE, p, SEED, STREAM, nat.ptr(out), out_bf16, nat.ptr(T),
                                                          nat.ptr(work), nat.current_stream()))
            assert h.g.last_kernel() == "spmm_gcnii_mfma_train_bf16"
            assert torch.equal(bits(out), bits(sparse.to_bf16(want_out) if out_bf16 else want_out)) and torch.equal(bits(T), bits(want_T))
            wrapped = sparse.gcnii_step_train_bf16(h.adj, Hb, d["H0"], A_MIX, d["M"], relu, triple, out_bf16=bool(out_bf16))
            assert torch.equal(bits(wrapped[0]), bits(out)) and torch.equal(bits(wrapped[1]), bits(T))
    # the backward over a bf16-representable gradient
    Gb = sparse.to_bf16(d["G"])
    G = Gb.float()
    want_dH, want_S = gnntf.gcnii_step_back(h.adj, G, A_MIX, d["Mt"], S_in=d["S_in"], s_alpha=0.5)
    assert h.g.last_kernel() == "spmm_gcnii_back_mfma"
    dH, S = poisoned(h.n, C), poisoned(h.n, C)
    nat.check(nat.lib().gnx_gcnii_step_back_bf16(h.g.handle, nat.ptr(h.adj.transposed_values()), nat.ptr(Gb), nat.ptr(G), A_MIX, C, nat.ptr(d["Mt"]), C,
                                                 nat.ptr(dH), nat.ptr(d["S_in"]), 0.5, nat.ptr(S), None, nat.current_stream()))
    assert h.g.last_kernel() == "spmm_gcnii_back_mfma_bf16"
    assert not torch.isnan(dH).any() and not torch.isnan(S).any(), "a row was written by no path"
    assert torch.equal(bits(dH), bits(want_dH)) and torch.equal(bits(S), bits(want_S))
    wrapped = sparse.gcnii_step_back_bf16(h.adj, Gb, G, A_MIX, d["Mt"], S_in=d["S_in"], s_alpha=0.5)
    assert torch.equal(bits(wrapped[0]), bits(dH)) and torch.equal(bits(wrapped[1]), bits(S))


# ---- 6. a row window --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids="-".join)
def test_row_window_keeps_the_bits(gnntf, handles, key):
    """Another row_order of the matrix and of the transposed structure: the same sums in the same per-row order (include/gnx.h)."""
    h = handles[key]
    default = {}
    for C in (16, 64, COMPOSED):
        d = device_operands(h.n, C)
        default[C] = (run_forward(gnntf, h, C, True), run_backward(gnntf, h, C, 0.5),
                      gnntf.gcnii_step(h.adj, d["H"], d["H0"], A_MIX, d["M"], relu=True, dropout=(0.6, SEED, STREAM)))
    fresh = make_handle(gnntf, *key, adj_vals=h.adj.vals)          # the shared handles are never re-planned
    for window in (64, 1000):
        fresh.g.set_row_window(window)
        fresh.adj = gnntf.Adjacency(fresh.g, h.adj.vals, None)      # (values in transposed order: permuted again under the new plan)
        for C in (16, 64, COMPOSED):
            d = device_operands(h.n, C)
            (out0, _, T0), (dH0, S0), drop0 = default[C]
            out, out_T, T = run_forward(gnntf, fresh, C, True, adj=fresh.adj)
            assert torch.equal(bits(out), bits(out0)) and torch.equal(bits(out_T), bits(out0)) and torch.equal(bits(T), bits(T0)), (window, C)
            dH, S = run_backward(gnntf, fresh, C, 0.5, adj=fresh.adj)
            assert torch.equal(bits(dH), bits(dH0)) and torch.equal(bits(S), bits(S0)), (window, C)
            drop = gnntf.gcnii_step(fresh.adj, d["H"], d["H0"], A_MIX, d["M"], relu=True, dropout=(0.6, SEED, STREAM))
            assert fresh.g.last_kernel() == forward_name(C, "_drop") and torch.equal(bits(drop), bits(drop0)), (window, C)
            want, back = want_forward(h, C, True), want_backward(h, C, 0.5)
            within("row window out", h, out, want["out"], want["out_bound"])
            within("row window dH", h, dH, back["dH"], back["dH_bound"])


# ---- 7. a pitched M / Mt, raw values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("regime", ["T", "S"])
def test_pitched_transform_keeps_the_bits(gnntf, handles, regime, C):
    """M as the first C columns of a [C, C + 4] buffer (rows 16-byte aligned) and of a [C, C + 1] buffer (rows unaligned: the dense
    kernel's other W loads), forward on ``a`` and backward on ``t``: the hub rows' dense_rows sees the pitch."""
    a, t = handles[regime, "a"], handles[regime, "t"]
    d = device_operands(a.n, C)
    out0, _, T0 = run_forward(gnntf, a, C, True)
    dH0, S0 = run_backward(gnntf, t, C, 0.5)
    for pad in (4, 1):
        M = torch.full((C, C + pad), 7.0, device="cuda")
        Mt = torch.full((C, C + pad), 7.0, device="cuda")
        M[:, :C], Mt[:, :C] = d["M"], d["Mt"]
        M, Mt = M[:, :C], Mt[:, :C]
        assert M.stride(0) == C + pad and gnntf.sparse._as_f32_rows(M).data_ptr() == M.data_ptr()       # passed on as it is
        out, out_T, T = run_forward(gnntf, a, C, True, M=M)
        assert torch.equal(bits(out), bits(out0)) and torch.equal(bits(out_T), bits(out0)) and torch.equal(bits(T), bits(T0)), pad
        dH, S = run_backward(gnntf, t, C, 0.5, Mt=Mt)
        assert torch.equal(bits(dH), bits(dH0)) and torch.equal(bits(S), bits(S0)), pad


@pytest.mark.parametrize("kind", ["a", "t"])
def test_raw_values(gnntf, handles, kind):
    """d_vals == NULL / d_vals_t == NULL: the handle's own values, un-normalised, in regime T at C = 32."""
    nat = gnntf.sparse.nat
    h, C = handles["T", kind], 32
    assert h.raw.vals is None and 0.5 <= h.A_raw.data.min() and h.A_raw.data.max() < 1.5
    want = want_forward(h, C, True, A=h.A_raw, tag="raw")
    out, out_T, T = run_forward(gnntf, h, C, True, adj=h.raw)
    assert torch.equal(bits(out_T), bits(out))
    within("raw values out", h, out, want["out"], want["out_bound"])
    within("raw values T", h, T, want["T"], want["T_bound"])
    back = want_backward(h, C, 0.5, A=h.A_raw, tag="raw")
    d = device_operands(h.n, C)
    dH, S = torch.full_like(d["G"], float("nan")), torch.full_like(d["G"], float("nan"))
    nat.check(nat.lib().gnx_gcnii_step_back(h.g.handle, None, nat.ptr(d["G"]), A_MIX, C, nat.ptr(d["Mt"]), C, nat.ptr(dH), nat.ptr(d["S_in"]), 0.5,
                                            nat.ptr(S), None, nat.current_stream()))
    assert h.g.last_kernel() == backward_name(C)
    within("raw values dH", h, dH, back["dH"], back["dH_bound"])
    within("raw values S", h, S, back["S"], back["S_bound"])
    # ... and they are not the normalised ones
    assert ref.ratio(host(out), want_forward(h, C, True)["out"], want_forward(h, C, True)["out_bound"]) > 100


# ---- 8. a seeded sweep ------------------------------------------------------------------------------------------------------------------
def sweep_draws(count=24, seed=20260101):
    rng = np.random.default_rng(seed)
    return [dict(regime=str(rng.choice(["T", "S"])), seed=int(rng.integers(0, 3)), kind=str(rng.choice(["a", "t"])),
                 C=int(rng.choice(WIDTHS)), relu=bool(rng.integers(0, 2)), a=float(rng.choice([0.05, 0.1, 0.5])),
                 window=int(rng.choice([0, 64]))) for _ in range(count)]


_sweep_handles = {}


@pytest.mark.parametrize("draw", sweep_draws(), ids=lambda d: "{regime}{seed}{kind}-C{C}-relu{relu:d}-a{a}-w{window}".format(**d))
def test_sweep(gnntf, draw):
    key = (draw["regime"], draw["kind"], draw["seed"], draw["window"])
    if key not in _sweep_handles:
        _sweep_handles.clear()                                      # one handle of the sweep alive at a time
        for ref_key in [k for k in _references if k[4] == "sweep"]:
            del _references[ref_key]
        _sweep_handles[key] = make_handle(gnntf, draw["regime"], draw["kind"], seed=draw["seed"], window=draw["window"])
    h, C, a = _sweep_handles[key], draw["C"], draw["a"]
    want = want_forward(h, C, draw["relu"], a=a, tag="sweep")
    out, out_T, T = run_forward(gnntf, h, C, draw["relu"], a=a)
    assert torch.equal(bits(out_T), bits(out)), draw
    back = want_backward(h, C, 0.5, a=a, tag="sweep")
    dH, S = run_backward(gnntf, h, C, 0.5, a=a)
    try:
        within("sweep out", h, out, want["out"], want["out_bound"])
        within("sweep T", h, T, want["T"], want["T_bound"])
        within("sweep dH", h, dH, back["dH"], back["dH_bound"])
        within("sweep S", h, S, back["S"], back["S_bound"])
    except AssertionError as e:
        raise AssertionError(f"{e} -- draw {draw}") from None


def test_sweep_draws_are_fixed_and_reach_both_regimes():
    draws = sweep_draws()
    assert draws == sweep_draws() and len(draws) == 24
    for field, values in (("regime", {"T", "S"}), ("kind", {"a", "t"}), ("C", set(WIDTHS)), ("relu", {True, False}), ("a", {0.05, 0.1, 0.5}),
                          ("window", {0, 64})):
        assert {d[field] for d in draws} == values, field


def test_report_the_worst_ratios(capsys):
    """Not a check of its own: prints what the tests above measured (profiles/NOTES.md records a run)."""
    with capsys.disabled():
        print("\n[gcnii shapes, MI355X] worst error / bound per entry and regime:")
        for (entry, regime), value in sorted(RATIOS.items()):
            print(f"    {entry:28s} {regime:20s} {value:.3f}")
    assert all(value <= 1.0 for value in RATIOS.values())
