"""The GCNII weight gradient without stored mixed rows on the MI355X (gnx_gcnii_wgrad, gnx_gcnii_wgrad_bf16) and the bf16 forward that
goes with it (gnx_gcnii_step_drop_bf16), at the long-row regimes of tests/gcnii_shapes_ref.py: regime T (n = 1547: a ragged last tile, a
whole tile without entries, hub rows at the threshold +- 1 and at chunk boundaries, lengths 3 / 4 / 5 round the U = 4 tail) and regime S
(n = 2^15 + 11: threshold 128, 154 hub rows), each at C = 16, 32, 64.

Against float64 the criterion is max |got - want| / bound <= 1 with want = f64(T)^T f64(G), T from forward_ref, and
    bound = gamma (|T|^T |G|) + T_bound^T |G|,   gamma = (n + 4) u / (1 - (n + 4) u):
the standard bound of a float32 sum of n + 4 terms in ANY order (n products, and at most four more additions for the waves, the slabs
and the pass over them -- far fewer than the sum's own slack), plus forward_ref's own bound on the rows of T.  Nothing in it is tuned to
a kernel, and gnx_dense_wgrad over the stored T has to pass it too.  The relations between entries are bitwise."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcnii_shapes_ref as ref

pytestmark = pytest.mark.gpu

A_MIX = 0.1
WIDTHS = (16, 32, 64)
REGIMES = ("T", "S")
SEED, STREAM = 7, 2
INVALID, UNSUPPORTED = -1, -4
SENTINEL = 9.0


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()            # (a copy: the shared operands are read-only)


def poisoned(*shape):
    """A result buffer full of NaN: an element that no path writes stays visible."""
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return (t + 0.0).view(torch.int32)                                 # (+ 0.0: the sign of a zero does not matter)


class Handle:
    """A regime's graph on the device, its symmetric normalisation, and the float32 weights the kernels read as a float64 CSR."""

    def __init__(self, gnntf, regime):
        coo, vals, shape, self.info = ref.regime_graph(regime, 0)
        self.regime, self.n = regime, shape[0]
        self.g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
        self.adj = gnntf.normalize(self.g, "symmetric")
        rowptr, colidx, _ = (x.cpu().numpy() for x in self.g.csr_arrays())
        self.A = sp.csr_matrix((self.adj.vals.cpu().numpy().astype(np.float64), colidx, rowptr), shape=shape)
        self.L = ref.plan_threshold(self.n)
        self.deg = np.diff(rowptr)


@pytest.fixture(scope="module")
def handles(gnntf):
    """Made once, never changed.  When the module is done, everything it cached goes."""
    yield {regime: Handle(gnntf, regime) for regime in REGIMES}
    _device_operands.clear()
    _references.clear()
    operands.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def operands(n, C):
    return ref.operands(n, C, seed=1000 + C)


_device_operands, _references = {}, {}


def device_operands(n, C):
    if (n, C) not in _device_operands:
        _device_operands[n, C] = {k: dev(v) for k, v in operands(n, C).items()}
    return _device_operands[n, C]


def want_wgrad(h, C):
    """(want, bound) of dM = T^T G at handle ``h`` and width C over the shared operands, computed once."""
    if (h.regime, C) not in _references:
        op = operands(h.n, C)
        fwd = ref.forward_ref(h.A, op["H"], op["H0"], op["M"], A_MIX, False)
        beta, alpha = ref.mix_constants(A_MIX)
        absT = beta * (abs(h.A) @ np.abs(ref.f64(op["H"]))) + alpha * np.abs(ref.f64(op["H0"]))
        absG = np.abs(ref.f64(op["G"]))
        terms = (h.n + 4) * ref.U32
        gamma = terms / (1.0 - terms)
        _references[h.regime, C] = (fwd["T"].T @ ref.f64(op["G"]), gamma * (absT.T @ absG) + fwd["T_bound"].T @ absG)
    return _references[h.regime, C]


def within(what, h, C, got):
    want, bound = want_wgrad(h, C)
    r = ref.ratio(host(got), want, bound)
    print(f"{what}, regime {h.regime}, C = {C}: error / bound = {r:.4f}")
    assert r <= 1.0, f"{what}, regime {h.regime}, C = {C}: error / bound = {r:.3f}"


def default_slabs(n, C):
    return max(1, min(2048, (n + 255) // 256, (1 << 28) // (C * C)))      # sparse._dense_wgrad's sizing


def raw_wgrad(gnntf, h, C, H=None, G=None, slabs=None):
    """gnx_gcnii_wgrad (f32 ``H``) or gnx_gcnii_wgrad_bf16 (bf16 ``H``) itself, into poisoned buffers: every element of dM written."""
    nat = gnntf.sparse.nat
    d = device_operands(h.n, C)
    H, G = d["H"] if H is None else H, d["G"] if G is None else G
    bf16 = H.dtype == torch.bfloat16
    slabs = default_slabs(h.n, C) if slabs is None else slabs
    dM, work, hub = poisoned(C, C), poisoned(slabs * C * C), poisoned(h.n, C)
    entry = nat.lib().gnx_gcnii_wgrad_bf16 if bf16 else nat.lib().gnx_gcnii_wgrad
    nat.check(entry(h.g.handle, nat.ptr(h.adj.vals), nat.ptr(H), nat.ptr(d["H0"]), A_MIX, C, nat.ptr(G), nat.ptr(dM), nat.ptr(hub), nat.ptr(work),
                    work.numel(), nat.current_stream()))
    assert h.g.last_kernel() == ("gcnii_wgrad_mfma_bf16" if bf16 else "gcnii_wgrad_mfma")
    assert not torch.isnan(dM).any(), "an element of dM was written by no path"
    written = ~torch.isnan(hub).all(dim=1)
    assert np.array_equal(np.flatnonzero(written.cpu().numpy()), h.info["hub"])      # the hub rows, and only they, go through memory
    return dM


def stored_rows(gnntf, h, C, H=None):
    """The d_mixed that gnx_gcnii_step writes over the same operands."""
    nat = gnntf.sparse.nat
    d = device_operands(h.n, C)
    H = d["H"] if H is None else H
    out, mixed = poisoned(h.n, C), poisoned(h.n, C)
    nat.check(nat.lib().gnx_gcnii_step(h.g.handle, nat.ptr(h.adj.vals), nat.ptr(H), nat.ptr(d["H0"]), A_MIX, C, nat.ptr(d["M"]), C, nat.ACT_RELU,
                                       nat.ptr(out), nat.ptr(mixed), nat.current_stream()))
    assert not torch.isnan(mixed).any()
    return mixed


def test_the_handle_tells_its_hub_rows(gnntf, handles):
    for h in handles.values():
        assert h.g.n_hub_rows == len(h.info["hub"]) > 0 and h.g.long_row_threshold == h.L


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("regime", REGIMES)
def test_against_float64(gnntf, handles, regime, C):
    h = handles[regime]
    d = device_operands(h.n, C)
    dM = raw_wgrad(gnntf, h, C)
    within("gnx_gcnii_wgrad", h, C, dM)
    # the functional form is that call (the same slabs, so the same bits), its scratch allocated here
    assert torch.equal(bits(gnntf.gcnii_wgrad(h.adj, d["H"], d["H0"], A_MIX, d["G"])), bits(dM))
    assert h.g.last_kernel() == "gcnii_wgrad_mfma"
    # the path it replaces passes the same criterion: the bound is not vacuous for it
    within("gnx_dense_wgrad over the stored T", h, C, gnntf.sparse._dense_wgrad(stored_rows(gnntf, h, C), d["G"]))


def chosen_rows(h, C):
    """For each column j a row r_j: one of every planted length (0, 1, 3, 4, 5, L - 1, L, L + 1, 2 L, 2 L + 1, 3 L + 7: an empty row, short
    rows, rows at the threshold, hub rows at the chunk boundaries), row 0 and row n - 1 (hub rows; n - 1 in the ragged tile), a short
    row of the ragged tile, a row of the tile without entries, a drawn hub row, then drawn rows."""
    info = h.info
    rows = [info["rows_of"][d][0] for d in ref.planted_lengths(h.L)] + [0, h.n - 1]
    rows.append(int(next(r for r in info["ragged"] if 0 < h.deg[r] <= h.L)))
    rows.append(ref.EMPTY_RUN[0] + 4)
    rng = np.random.default_rng(C)
    rows.append(int(rng.choice(info["hub"])))
    assert len(rows) == 16
    rows += [int(r) for r in rng.integers(0, h.n, size=C - len(rows))]
    return np.array(rows)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("regime", REGIMES)
def test_the_recomputed_row_is_the_stored_row(gnntf, handles, regime, C):
    """G[r_j, j] = 1 and 0 elsewhere: dM[:, j] = T[r_j, :] exactly (a product by one and sums of zeros are exact), so it must be, bit for
    bit, row r_j of the d_mixed gnx_gcnii_step writes."""
    h = handles[regime]
    rows = chosen_rows(h, C)
    G = np.zeros((h.n, C), dtype=np.float32)
    G[rows, np.arange(C)] = 1.0
    dM = raw_wgrad(gnntf, h, C, G=dev(G))
    T = stored_rows(gnntf, h, C)
    want = T[torch.from_numpy(rows).cuda()].t().contiguous()             # column j = row r_j of T
    differs = (bits(dM) != bits(want)).any(dim=0).cpu().numpy()
    assert not differs.any(), f"columns {np.flatnonzero(differs)}: rows {rows[differs]} of lengths {h.deg[rows[differs]]}"
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("regime", REGIMES)
def test_two_calls_give_the_same_bits(gnntf, handles, regime, C):
    h = handles[regime]
    one, two = raw_wgrad(gnntf, h, C), raw_wgrad(gnntf, h, C)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))
    # another work_floats is another summation order: one slab, three slabs, more slabs than blocks of tiles
    for slabs in (1, 3, 4096):
        other = raw_wgrad(gnntf, h, C, slabs=slabs)
        within(f"gnx_gcnii_wgrad with {slabs} slabs", h, C, other)
        assert torch.equal(other.view(torch.int32), raw_wgrad(gnntf, h, C, slabs=slabs).view(torch.int32))


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("regime", REGIMES)
def test_bf16_rows_give_the_bits_of_the_widened_rows(gnntf, handles, regime, C):
    h = handles[regime]
    Hb = device_operands(h.n, C)["H"].to(torch.bfloat16)
    got = raw_wgrad(gnntf, h, C, H=Hb)
    assert torch.equal(got.view(torch.int32), raw_wgrad(gnntf, h, C, H=Hb.float()).view(torch.int32))
    assert torch.equal(bits(gnntf.gcnii_wgrad(h.adj, Hb, device_operands(h.n, C)["H0"], A_MIX, device_operands(h.n, C)["G"])), bits(got))
    assert h.g.last_kernel() == "gcnii_wgrad_mfma_bf16"


@pytest.mark.parametrize("p", (0.0, 0.5))
@pytest.mark.parametrize("out_bf16", (0, 1))
@pytest.mark.parametrize("C", WIDTHS)
def test_the_forward_without_mixed_rows_gives_the_bits_of_the_training_forward(gnntf, handles, C, out_bf16, p):
    """gnx_gcnii_step_drop_bf16 against gnx_gcnii_step_train_bf16's out, on the graph with hub rows."""
    h = handles["T"]
    nat = gnntf.sparse.nat
    lib = nat.lib()
    d = device_operands(h.n, C)
    Hb = d["H"].to(torch.bfloat16)
    dtype = torch.bfloat16 if out_bf16 else torch.float32
    layer = (h.g.handle, nat.ptr(h.adj.vals), nat.ptr(Hb), nat.ptr(d["H0"]), A_MIX, C, nat.ptr(d["M"]), C, nat.ACT_RELU, p, SEED, STREAM)
    want, mixed, work = poisoned(h.n, C).to(dtype), poisoned(h.n, C), poisoned(h.n, C)
    nat.check(lib.gnx_gcnii_step_train_bf16(*layer, nat.ptr(want), out_bf16, nat.ptr(mixed), nat.ptr(work), nat.current_stream()))
    got, work = poisoned(h.n, C).to(dtype), poisoned(h.n, C)
    nat.check(lib.gnx_gcnii_step_drop_bf16(*layer, nat.ptr(got), out_bf16, nat.ptr(work), nat.current_stream()))
    assert h.g.last_kernel() == "spmm_gcnii_mfma_drop_bf16"
    assert not torch.isnan(got.float()).any() and float(got.float().abs().max()) > 0
    view = torch.int16 if out_bf16 else torch.int32
    assert torch.equal(got.view(view), want.view(view))
    # the functional form: the same out, no T
    out, T = gnntf.sparse.gcnii_step_train_bf16(h.adj, Hb, d["H0"], A_MIX, d["M"], True, (p, SEED, STREAM), out_bf16=bool(out_bf16), keep_mixed=False)
    assert T is None and torch.equal(out.view(view), want.view(view))
    # without hub-row scratch the graph with hub rows is refused, naming it
    rc = lib.gnx_gcnii_step_drop_bf16(*layer, nat.ptr(got), out_bf16, None, nat.current_stream())
    assert rc == INVALID and b"gnx_gcnii_step_drop_bf16:" in lib.gnx_last_error() and b"d_work" in lib.gnx_last_error()


# ---- refusals: one thing wrong each ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refusal_buffers(gnntf, handles):
    """Per width: operands (zeros), sentinel-filled results, all of n C + 4 floats so that a view can start 4 bytes in; a handle with
    hub rows (regime T), the same entries in an n x (n + 1) shape, and a graph without hub rows.  Every handle has run one launch."""
    h = handles["T"]
    n = h.n
    coo, vals, shape, _ = ref.regime_graph("T", 0)
    wide = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, (n, n + 1)), device="cuda:0")
    short = coo[h.deg[coo[:, 0]] <= 8]
    flat = gnntf.DeviceGraph(gnntf.SparseCOO(short, vals[:len(short)], shape), device="cuda:0")
    assert flat.n_hub_rows == 0 and wide.n_hub_rows == h.g.n_hub_rows
    graphs = dict(hub=h.g, wide=wide, flat=flat)
    for g, cols in ((h.g, n), (wide, n + 1), (flat, n)):
        gnntf.spmm(gnntf.Adjacency(g), torch.zeros(cols, 16, device="cuda"))
    out = dict(graphs=graphs)
    for C in (16, 40):
        zeros = lambda: torch.zeros(n * C + 4, device="cuda")
        full = lambda k: torch.full((k,), SENTINEL, device="cuda")
        out[C] = dict(H=zeros(), Hb=torch.zeros(n * C + 4, device="cuda", dtype=torch.bfloat16), H0=zeros(), G=zeros(), dM=full(C * C + 4),
                      hub=full(n * C + 4), work=full(4 * C * C + 4), work_floats=4 * C * C)
    torch.cuda.synchronize()
    return out


def refusal_rows():
    """(graph, C, the one thing wrong, code, words of the message); a str names a buffer, ("off", name) that buffer 4 bytes in (2 bytes for
    the bf16 rows)"""
    t = [
        ("hub", 40, dict(), UNSUPPORTED, ["width 40"]),
        ("hub", 16, dict(G=None), INVALID, ["NULL H / H0 / G / dM"]),
        ("hub", 16, dict(dM=None), INVALID, ["NULL H / H0 / G / dM"]),
        ("hub", 16, dict(H=None), INVALID, ["NULL H / H0 / G / dM"]),
        ("hub", 16, dict(H0=None), INVALID, ["NULL H / H0 / G / dM"]),
        ("wide", 16, dict(), INVALID, ["square graph"]),
        ("hub", 16, dict(work_floats=16 * 16 - 1), INVALID, ["work_floats 255", "C * C"]),
        ("hub", 16, dict(work=None), INVALID, ["d_work must be a buffer of its own"]),
        ("hub", 16, dict(hub=None), INVALID, ["d_hub_rows", "hub rows"]),
    ]
    t += [("hub", 16, dict(dM=other), INVALID, ["dM must not alias"]) for other in ("H", "H0", "G")]
    t += [("hub", 16, dict(work=other), INVALID, ["d_work must be a buffer of its own"]) for other in ("H", "H0", "G", "dM")]
    t += [("hub", 16, dict(hub=other), INVALID, ["d_hub_rows must be a buffer of its own"]) for other in ("H", "H0", "G", "dM", "work")]
    t += [("hub", 16, {name: ("off", name)}, UNSUPPORTED, ["misaligned buffer"]) for name in ("H", "H0", "G", "dM", "hub", "work")]
    return [(entry,) + row for row in t for entry in ("gnx_gcnii_wgrad", "gnx_gcnii_wgrad_bf16")]


def refusal_id(row):
    entry, graph, C, wrong = row[:4]
    return "-".join([entry[4:], graph, str(C)] + [f"{k}={v[1] + '+4' if isinstance(v, tuple) else v}" for k, v in wrong.items()])


@pytest.mark.parametrize("row", refusal_rows(), ids=refusal_id)
def test_refusal_names_the_cause_and_launches_nothing(gnntf, refusal_buffers, row):
    entry, graph, C, wrong, code, words = row
    nat = gnntf.sparse.nat
    lib = nat.lib()
    g = refusal_buffers["graphs"][graph]
    buf = dict(refusal_buffers[C])
    if entry.endswith("_bf16"):
        buf["H"] = buf["Hb"]
    args = dict(dict(H="H", H0="H0", G="G", dM="dM", hub="hub", work="work", work_floats=buf["work_floats"]), **wrong)

    def pointer(v):
        if v is None or isinstance(v, int):
            return v
        if isinstance(v, tuple):
            return nat.ptr(buf[v[1]][1:])                                    # one element in: 4 bytes (f32), 2 bytes (bf16)
        return nat.ptr(buf[v])

    before = g.last_kernel()
    assert before
    rc = getattr(lib, entry)(g.handle, None, pointer(args["H"]), pointer(args["H0"]), A_MIX, C, pointer(args["G"]), pointer(args["dM"]),
                             pointer(args["hub"]), pointer(args["work"]), args["work_floats"], nat.current_stream())
    message = lib.gnx_last_error()
    assert rc == code and all(word.encode() in message for word in [entry + ":"] + words), (rc, message)
    torch.cuda.synchronize()
    assert all(bool((refusal_buffers[C][k] == SENTINEL).all()) for k in ("dM", "hub", "work"))
    assert g.last_kernel() == before


def test_a_graph_without_hub_rows_needs_no_scratch(gnntf, refusal_buffers):
    """d_hub_rows may be NULL exactly when the handle has no hub rows; the call then reports its name."""
    nat = gnntf.sparse.nat
    g, C = refusal_buffers["graphs"]["flat"], 16
    n = g.n_rows
    H, H0, G = (torch.randn(n, C, device="cuda") for _ in range(3))
    dM, work = poisoned(C, C), poisoned(4 * C * C)
    nat.check(nat.lib().gnx_gcnii_wgrad(g.handle, None, nat.ptr(H), nat.ptr(H0), A_MIX, C, nat.ptr(G), nat.ptr(dM), None, nat.ptr(work), work.numel(),
                                        nat.current_stream()))
    assert g.last_kernel() == "gcnii_wgrad_mfma" and not torch.isnan(dM).any()
    adj = gnntf.Adjacency(g)
    assert torch.equal(bits(gnntf.gcnii_wgrad(adj, H, H0, A_MIX, G)), bits(gnntf.gcnii_wgrad(adj, H, H0, A_MIX, G, hub_rows=torch.empty_like(H))))
    with pytest.raises(Exception, match="constant adjacency"):
        gnntf.gcnii_wgrad(gnntf.sparse.DroppedAdjacency(g, 0.5, 1, 2, D=torch.ones(n, device="cuda")), H, H0, A_MIX, G)
    with pytest.raises(Exception, match="width 16, 32 or 64"):
        gnntf.gcnii_wgrad(adj, torch.randn(n, 40, device="cuda"), torch.randn(n, 40, device="cuda"), A_MIX, torch.randn(n, 40, device="cuda"))
