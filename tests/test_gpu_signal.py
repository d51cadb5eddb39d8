"""The node signals at width 1 on the MI355X (csrc/gnx_signal.hip; sparse.signal_project / signal_spmv / signal_ppr / sweep / smoothness;
PPRSweep, FastReg, GCNIIReg) against the float64 references and any-order bounds of tests/signal_ref.py.

Graphs: regimes T (n = 1547, long-row threshold 512) and S (n = 2^15 + 11, threshold 128) of gcnii_shapes_ref.regime_graph and their
reversals (rows and columns swapped: the planted graphs have a hub-free transpose, so only the reversals put hub rows into the
transposed walk).  Together: rows of 0, 1, 3, 4, 5, L - 1, L, L + 1, 2 L + 1 and 3 L + 7 entries, a run of 16 empty rows, columns nothing
points at (D_j = 0).  The criterion against float64 is max |got - want| / bound <= 1; relations between entries are bitwise.  The worst
ratios seen are printed by the last test."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcnii_shapes_ref as shapes
import signal_ref as ref

pytestmark = pytest.mark.gpu

KEYS = [("T", "a"), ("T", "t"), ("S", "a"), ("S", "t")]
GROUP = 8                                               # lanes per short row (csrc/gnx_signal.hip)
SEED, STREAM = 7, 2
RATIOS = {}


def note(name, value):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(value))
    return value


def kernel_name(what, hubs):
    return f"signal_{what}_group{GROUP}" + ("+long" if hubs else "")


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


class Handle:
    """A graph on the device, its symmetric normalisation and its un-normalised adjacency, and the float32 weights the kernels read as
    float64 CSR matrices."""

    def __init__(self, gnntf, coo, vals, shape):
        self.coo, self.vals, self.shape = coo, vals, shape
        self.g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
        self.adj = gnntf.normalize(self.g, "symmetric")
        self.raw = gnntf.Adjacency(self.g)
        rowptr, colidx, raw = (x.cpu().numpy() for x in self.g.csr_arrays())
        self.n = shape[0]
        self.A = sp.csr_matrix((self.adj.vals.cpu().numpy().astype(np.float64), colidx, rowptr), shape=shape)
        self.A_raw = sp.csr_matrix((raw.astype(np.float64), colidx, rowptr), shape=shape)
        self.L = shapes.plan_threshold(self.n)
        self.deg, self.in_deg = np.diff(rowptr), np.bincount(colidx, minlength=self.n)
        self.hub, self.hub_t = np.flatnonzero(self.deg > self.L), np.flatnonzero(self.in_deg > self.L)
        self.empty, self.no_in = np.flatnonzero(self.deg == 0), np.flatnonzero(self.in_deg == 0)


@pytest.fixture(scope="module")
def handles(gnntf):
    out = {}
    for regime, kind in KEYS:
        coo, vals, shape, info = shapes.regime_graph(regime)
        h = Handle(gnntf, coo if kind == "a" else coo[:, ::-1].copy(), vals, shape)
        h.planted = info["planted"]
        mine, other = (h.hub, h.hub_t) if kind == "a" else (h.hub_t, h.hub)
        assert np.array_equal(mine, info["hub"]) and len(other) == 0 and len(h.no_in if kind == "a" else h.empty) >= 3
        out[(regime, kind)] = h
    yield out
    operands.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def operands(n, C=64, seed=0):
    """x, h0 [n], X [n, C], w [C]: seeded, float32, read-only."""
    rng = np.random.default_rng(seed + n + C)
    out = dict(x=rng.standard_normal(n).astype(np.float32), h0=rng.standard_normal(n).astype(np.float32),
               X=rng.standard_normal((n, C)).astype(np.float32), w=rng.uniform(-1, 1, size=C).astype(np.float32) / np.float32(np.sqrt(C) / 2))
    for v in out.values():
        v.setflags(write=False)
    return out


def row_sets(h, transposed):
    hub, empty = (h.hub_t, h.no_in) if transposed else (h.hub, h.empty)
    return dict(all=None, hub=hub, empty=empty, planted=h.planted)


def raw_spmv(h, vals, transposed, x, h0, beta, alpha):
    """gnx_signal_spmv into a buffer with 64 sentinel values behind the last row, which must stay as they were."""
    from gnntf import _native as nat
    out = torch.full((h.n + 64,), float("nan"), dtype=torch.float32, device="cuda")
    nat.check(nat.lib().gnx_signal_spmv(h.g.handle, nat.ptr(vals), 1 if transposed else 0, nat.ptr(x), nat.ptr(h0), float(beta), float(alpha),
                                        nat.ptr(out), nat.current_stream()))
    assert bool(torch.isnan(out[h.n:]).all()) and not bool(torch.isnan(out[:h.n]).any())
    return out[:h.n].clone()


# ---- 1. the SpMV ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", (False, True))
@pytest.mark.parametrize("key", KEYS)
def test_spmv_against_float64(gnntf, handles, key, transposed):
    from gnntf import sparse
    h = handles[key]
    ops = operands(h.n)
    x, h0 = dev(ops["x"]), dev(ops["h0"])
    beta, alpha = 0.9, 0.1
    sets = row_sets(h, transposed)
    for name, adj, A in (("normalised", h.adj, h.A), ("raw", h.raw, h.A_raw)):
        vals = None if adj.vals is None else (adj.transposed_values() if transposed else adj.vals)
        walked = sp.csr_matrix(A.T) if transposed else A
        for with_h0 in (True, False):
            got = raw_spmv(h, vals, transposed, x, h0 if with_h0 else None, beta, alpha)
            assert h.g.last_kernel() == kernel_name("spmv", len(sets["hub"]) > 0)
            want, bound = ref.spmv_ref(walked, ops["x"], ops["h0"] if with_h0 else None, beta, alpha, h.L)
            for which, rows in sets.items():
                note(f"spmv {'t' if transposed else 'a'} {which}", ref.ratio1(host(got), want, bound, rows))
                assert ref.ratio1(host(got), want, bound, rows) <= 1, (name, with_h0, which)
            # a row without entries is exactly alpha * h0
            mix = np.float32(alpha) * (ops["h0"] if with_h0 else np.ones(h.n, dtype=np.float32))
            assert np.array_equal(host(got)[sets["empty"]], mix[sets["empty"]]) and len(sets["empty"]) >= 3
            assert torch.equal(bits(got), bits(sparse.signal_spmv(adj, x, h0 if with_h0 else None, beta, alpha, transposed=transposed)))
            if not with_h0:     # the constant 1 is bit for bit a vector of ones
                ones = torch.ones(h.n, dtype=torch.float32, device="cuda")
                assert torch.equal(bits(got), bits(raw_spmv(h, vals, transposed, x, ones, beta, alpha)))
        # beta = 1, alpha = 0: the plain product; empty rows give +0
        plain = raw_spmv(h, vals, transposed, x, None, 1.0, 0.0)
        assert bool((bits(plain)[dev(sets["empty"])] == 0).all())


# ---- 2. the PPR loop ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_ppr_is_ten_spmv_calls_and_within_its_bound(gnntf, handles, key):
    from gnntf import sparse
    h = handles[key]
    ops = operands(h.n)
    for h0_np in (ops["h0"], None):
        h0 = None if h0_np is None else dev(h0_np)
        got = sparse.signal_ppr(h.adj, h0, 0.1, 10)
        x = torch.ones(h.n, dtype=torch.float32, device="cuda") if h0 is None else h0
        beta, alpha = shapes.mix_constants(0.1)
        for _ in range(10):
            x = sparse.signal_spmv(h.adj, x, h0, beta, alpha)
        assert torch.equal(bits(got), bits(x))
        want, bound = ref.ppr_ref(h.A, h0_np, 0.1, 10, h.L)
        assert note("ppr K=10", ref.ratio1(host(got), want, bound)) <= 1
        for K in (1, 2, 3):                                # either parity of the ping-pong
            x = torch.ones(h.n, dtype=torch.float32, device="cuda") if h0 is None else h0
            for _ in range(K):
                x = sparse.signal_spmv(h.adj, x, h0, beta, alpha)
            assert torch.equal(bits(sparse.signal_ppr(h.adj, h0, 0.1, K)), bits(x))
        zero = sparse.signal_ppr(h.adj, h0, 0.1, 0)
        assert torch.equal(zero, torch.ones_like(zero) if h0 is None else h0)
    assert h.g.last_kernel() == kernel_name("spmv", len(h.hub) > 0)        # (the loop reports the SpMV's names)


# ---- 3. the projection -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", ("C", "C+3", "aligned+tail", "aligned pitch, base off by one"))
@pytest.mark.parametrize("C", (1, 3, 7, 40, 64, 100))
def test_project_against_float64(gnntf, C, pitch):
    """``aligned pitch, base off by one``: the slice X[:, 1:] of an aligned matrix whose pitch is a multiple of 4 -- every row start is 4
    bytes past a 16-byte boundary, so the 16-byte loads must not be taken although the pitch would allow them."""
    from gnntf import sparse
    n = 1000 + 7
    col0 = 1 if pitch.endswith("off by one") else 0
    ld = {"C": C, "C+3": C + 3, "aligned+tail": (C + 3) // 4 * 4 + 4, "aligned pitch, base off by one": (C + 4) // 4 * 4 + 4}[pitch]
    rng = np.random.default_rng(100 * C + ld + col0)
    rows = rng.standard_normal((n, ld)).astype(np.float32)
    w = rng.uniform(-1, 1, size=C).astype(np.float32)
    w[0] = np.float32(0.75)
    data = rows[:, col0:col0 + C]                       # a view: the planted rows below land in ``rows``
    data[5, :], data[6, :] = 0, 0
    data[5, 0], data[6, 0] = np.float32(100 / 0.75), np.float32(-100 / 0.75)     # dot products of +-100
    X = dev(rows)[:, col0:col0 + C]
    assert X.stride(0) == ld and X.data_ptr() % 16 == 4 * col0 and (col0 == 0 or ld % 4 == 0)
    for act in (1, 0):
        got = host(sparse.signal_project(X, dev(w), sigmoid=bool(act)))
        want, bound = ref.project_ref(data, w, act)
        assert np.isfinite(got).all()
        assert note(f"project act={act}", ref.ratio1(got, want, bound)) <= 1
    f = host(sparse.signal_project(X, dev(w)))
    assert f[5] == 1.0 and f[6] == 0.0 and ((f >= 0) & (f <= 1)).all()


# ---- 4. the smoothness forward -------------------------------------------------------------------------------------------------------------
def smooth_forward(h, adj, X, w, D):
    """(f, d, sums) of gnx_signal_smoothness over the projection, as sparse._Smoothness calls it."""
    from gnntf import _native as nat, sparse
    f = sparse.signal_project(X, w)
    d = torch.full((h.n,), float("nan"), dtype=torch.float32, device="cuda")
    sums = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    work = torch.empty(sparse.smoothness_work_floats(h.n), dtype=torch.float32, device="cuda")
    nat.check(nat.lib().gnx_signal_smoothness(h.g.handle, nat.ptr(adj.vals), nat.ptr(f), nat.ptr(D), nat.ptr(d), nat.ptr(sums), nat.ptr(work),
                                              nat.current_stream()))
    return f, d, sums


def colsum32(h):
    return np.asarray(h.A_raw.sum(axis=0)).reshape(-1).astype(np.float32)


_REFS = {}                                              # (regime key, C, upstream) -> signal_ref.smoothness_ref, computed once


def smooth_reference(h, key, C, upstream=1.0):
    if (key, C, upstream) not in _REFS:
        ops = operands(h.n, C)
        _REFS[(key, C, upstream)] = ref.smoothness_ref(h.A_raw, ops["X"], ops["w"], colsum32(h), h.L, h.L, upstream)
    return _REFS[(key, C, upstream)]


@pytest.mark.parametrize("key", KEYS)
def test_smoothness_forward(gnntf, handles, key):
    from gnntf import sparse
    h = handles[key]
    ops = operands(h.n, 64)
    X, w, D = dev(ops["X"]), dev(ops["w"]), dev(colsum32(h))
    want = smooth_reference(h, key, 64)
    f, d, sums = smooth_forward(h, h.raw, X, w, D)
    assert h.g.last_kernel() == kernel_name("smooth", len(h.hub) > 0)
    s = host(sums)
    assert note("smoothness f", ref.ratio1(host(f), want["f"], want["f_bound"])) <= 1
    assert note("smoothness d", ref.ratio1(host(d), want["d"], want["d_bound"])) <= 1
    assert note("smoothness num", ref.ratio1(s[0], want["num"], want["num_bound"])) <= 1
    assert note("smoothness den", ref.ratio1(s[1], want["den"], want["den_bound"])) <= 1
    assert note("smoothness lambda", ref.ratio1(s[2], want["lam"], want["lam_bound"])) <= 1
    assert s[2] == np.float32(s[0]) / np.float32(s[1]) and (colsum32(h)[h.no_in] == 0).all()
    # two calls, and the functional form, give the same bits
    again = smooth_forward(h, h.raw, X, w, D)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((f, d, sums), again))
    lam = sparse.smoothness(h.raw, X, dev(ops["w"]).reshape(-1, 1), colsum=D)
    assert lam.dim() == 0 and torch.equal(bits(lam.reshape(1)), bits(sums[2:3]))
    # the default column sums: gnx_graph_colsum over the raw values, within the colsum bound, and A^T . 1 for values of its own
    D_want, D_bound = ref.colsum_ref(h.A_raw)
    assert note("colsum", ref.ratio1(host(sparse.signal_colsum(h.raw)), D_want, D_bound)) <= 1
    Dn_want, Dn_bound = ref.spmv_ref(sp.csr_matrix(h.A.T), np.ones(h.n, dtype=np.float32), None, 1.0, 0.0, h.L)
    assert ref.ratio1(host(sparse.signal_colsum(h.adj)), Dn_want, Dn_bound) <= 1
    # the same graph with its COO shuffled differently: the handle coalesces and sorts
    perm = np.random.default_rng(99).permutation(len(h.coo))
    other = Handle(gnntf, h.coo[perm], h.vals[perm], h.shape)
    shuffled = smooth_forward(other, other.raw, X, w, D)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((f, d, sums), shuffled))


def test_smoothness_of_a_graph_without_entries(gnntf):
    from gnntf import sparse
    n = 300
    g = gnntf.DeviceGraph(gnntf.SparseCOO(np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.float32), (n, n)), device="cuda:0")
    ops = operands(n, 7)
    X, w = dev(ops["X"]), dev(ops["w"])
    f = host(sparse.signal_project(X, w)).astype(np.float64)
    with np.errstate(divide="ignore"):
        lam = sparse.smoothness(gnntf.Adjacency(g), X, w)
    holder = Handle.__new__(Handle)
    holder.g, holder.n = g, n
    _, d, sums = smooth_forward(holder, gnntf.Adjacency(g), X, w, torch.zeros(n, device="cuda"))
    s = host(sums)
    assert np.array_equal(host(d).astype(np.float64), f)
    assert abs(s[0] - (f * f).sum()) <= (n + 2) * ref.U32 * (f * f).sum() and s[1] == 0.0
    assert np.isinf(s[2]) and s[2] > 0 and bool(torch.isinf(lam))            # num / 0 as IEEE gives it


# ---- 5. the smoothness backward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upstream", (-1.0, 0.37))
@pytest.mark.parametrize("key", KEYS)
def test_smoothness_backward(gnntf, handles, key, upstream):
    from gnntf import _native as nat, sparse
    h = handles[key]
    ops = operands(h.n, 64)
    D = dev(colsum32(h))
    want = smooth_reference(h, key, 64, upstream)
    for fused in (True, False):
        X, w = dev(ops["X"]).requires_grad_(), dev(ops["w"]).reshape(-1, 1).requires_grad_()
        # (an adjacency of its own for the composition: spmm's backward leaves its transposed values on the object it was given)
        lam = sparse.smoothness(h.raw if fused else gnntf.Adjacency(h.g), X, w, colsum=D, fused=fused)
        (lam * upstream).backward()
        if fused:
            assert h.g.last_kernel() == kernel_name("back", len(h.hub_t) > 0)
        tag = "fused" if fused else "composed"
        assert note(f"dX {tag}", ref.ratio(host(X.grad), want["dX"], want["dX_bound"])) <= 1
        assert note(f"dw {tag}", ref.ratio1(host(w.grad), want["dw"], want["dw_bound"])) <= 1
        assert tuple(w.grad.shape) == (64, 1) and float(X.grad.abs().max()) > 0
        assert note(f"lambda {tag}", ref.ratio1(float(lam.detach()), want["lam"], want["lam_bound"])) <= 1
    # gz itself, from the entry
    X, w = dev(ops["X"]), dev(ops["w"])
    f, d, sums = smooth_forward(h, h.raw, X, w, D)
    gz = torch.full((h.n,), float("nan"), dtype=torch.float32, device="cuda")
    u = torch.tensor([upstream], dtype=torch.float32, device="cuda")
    nat.check(nat.lib().gnx_signal_smoothness_back(h.g.handle, None, nat.ptr(f), nat.ptr(d), nat.ptr(D), nat.ptr(sums), nat.ptr(u), nat.ptr(gz),
                                                   nat.current_stream()))
    assert note("gz", ref.ratio1(host(gz), want["gz"], want["gz_bound"])) <= 1
    # a frozen w gets no gradient
    X, w = dev(ops["X"]).requires_grad_(), dev(ops["w"]).reshape(-1, 1)
    sparse.smoothness(h.raw, X, w, colsum=D).backward()
    assert w.grad is None and X.grad is not None


# ---- 6. a dropped adjacency ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("T", "a"), ("S", "t")])
def test_dropped_adjacency(gnntf, handles, key):
    from gnntf import sparse
    h = handles[key]
    ops = operands(h.n, 64)
    X, w = dev(ops["X"]), dev(ops["w"])
    dropped = gnntf.normalize(h.g, "none", "none", 0.5, SEED, STREAM)
    assert dropped.raw_dropout == (0.5, SEED, STREAM)
    D = sparse.signal_colsum(dropped)
    lam = sparse.smoothness(dropped, X, w)
    vals = dropped.vals.cpu()
    share = float((vals == 0).float().mean())
    assert 0.4 < share < 0.6 and bool(((vals == 0) | (vals >= 1.0)).all())           # kept values doubled
    constant = gnntf.Adjacency(h.g, vals.cuda())
    assert torch.equal(bits(lam.reshape(1)), bits(sparse.smoothness(constant, X, w, colsum=D).reshape(1)))
    rowptr, colidx, _ = (x.cpu().numpy() for x in h.g.csr_arrays())
    A = sp.csr_matrix((vals.numpy().astype(np.float64), colidx, rowptr), shape=h.shape)
    D_want, D_bound = ref.colsum_ref(A)
    assert note("colsum dropped", ref.ratio1(host(D), D_want, D_bound)) <= 1
    # the column sums of a constant adjacency's own values are A^T . 1 at width 1
    own_want, own_bound = ref.spmv_ref(sp.csr_matrix(A.T), np.ones(h.n, dtype=np.float32), None, 1.0, 0.0, h.L)
    assert ref.ratio1(host(sparse.signal_colsum(constant)), own_want, own_bound) <= 1


# ---- the refusals that need a handle ---------------------------------------------------------------------------------------------------
def test_entries_refuse_null_buffers_and_aliases(gnntf, handles):
    """Behind a real handle: every NULL buffer, every output that aliases an operand and a non-square graph are refused with -1 and the
    entry's own prefix, and no output buffer is written (NaN sentinels stay).  tests/test_signal_cpu.py holds the refusals that need no
    handle."""
    from gnntf import _native as nat
    lib = nat.lib()
    h = handles[("T", "a")]
    n, g, s = h.n, h.g.handle, nat.current_stream()
    ops = operands(n)
    x, f, D = dev(ops["x"]), dev(ops["h0"]), dev(colsum32(h))
    out, out2, d, gz = (torch.full((n,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(4))
    sums = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    work = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    u = torch.ones(1, dtype=torch.float32, device="cuda")
    P = nat.ptr

    def refused(rc, prefix):
        message = lib.gnx_last_error()
        assert rc == -1 and message.startswith(prefix), (rc, message, prefix)

    # gnx_signal_spmv
    refused(lib.gnx_signal_spmv(g, None, 0, None, None, 0.9, 0.1, P(out), s), b"gnx_signal_spmv: NULL signal")
    refused(lib.gnx_signal_spmv(g, None, 1, P(x), None, 0.9, 0.1, None, s), b"gnx_signal_spmv: NULL output")
    refused(lib.gnx_signal_spmv(g, None, 0, P(out), None, 0.9, 0.1, P(out), s), b"gnx_signal_spmv: the output must not be")
    # gnx_signal_ppr
    refused(lib.gnx_signal_ppr(g, None, P(x), 0.1, 10, None, P(work), s), b"gnx_signal_ppr: NULL buffer")
    refused(lib.gnx_signal_ppr(g, None, P(x), 0.1, 2, P(out), None, s), b"gnx_signal_ppr: NULL buffer")
    refused(lib.gnx_signal_ppr(g, None, None, 0.1, 1, P(out), None, s), b"gnx_signal_ppr: NULL buffer")
    refused(lib.gnx_signal_ppr(g, None, P(x), 0.1, 10, P(out), P(out), s), b"gnx_signal_ppr: h0, out and work must be distinct")
    refused(lib.gnx_signal_ppr(g, None, P(out), 0.1, 10, P(out), P(work), s), b"gnx_signal_ppr: h0, out and work must be distinct")
    refused(lib.gnx_signal_ppr(g, None, P(x), 0.1, -1, P(out), P(work), s), b"gnx_signal_ppr: negative iteration count")
    # gnx_signal_smoothness: (f, colsum, diff, sums, work)
    full = [P(f), P(D), P(d), P(sums), P(work)]
    for missing in range(5):
        args = list(full)
        args[missing] = None
        refused(lib.gnx_signal_smoothness(g, None, *args, s), b"gnx_signal_smoothness: NULL buffer")
    refused(lib.gnx_signal_smoothness(g, None, P(d), P(D), P(d), P(sums), P(work), s), b"gnx_signal_smoothness: the differences must not")
    # gnx_signal_smoothness_back: (f, diff, colsum, sums, upstream, gz)
    ok_sums = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float32, device="cuda")
    full = [P(f), P(x), P(D), P(ok_sums), P(u), P(gz)]
    for missing in range(6):
        args = list(full)
        args[missing] = None
        refused(lib.gnx_signal_smoothness_back(g, None, *args, s), b"gnx_signal_smoothness_back: NULL buffer")
    refused(lib.gnx_signal_smoothness_back(g, None, P(f), P(gz), P(D), P(ok_sums), P(u), P(gz), s), b"gnx_signal_smoothness_back: the gradient must not")
    refused(lib.gnx_signal_smoothness_back(g, None, P(gz), P(x), P(D), P(ok_sums), P(u), P(gz), s), b"gnx_signal_smoothness_back: the gradient must not")
    # gnx_signal_uniform
    refused(lib.gnx_signal_uniform(g, 8, 1.0, 1, 2, None, s), b"gnx_signal_uniform: NULL output")
    refused(lib.gnx_signal_uniform(g, -1, 1.0, 1, 2, P(out), s), b"gnx_signal_uniform: count")
    # a graph that is not square
    wide = gnntf.DeviceGraph(gnntf.SparseCOO(np.array([[0, 1], [2, 3]], dtype=np.int64), np.ones(2, dtype=np.float32), (3, 4)), device="cuda:0")
    refused(lib.gnx_signal_ppr(wide.handle, None, P(x), 0.1, 2, P(out), P(work), s), b"gnx_signal_ppr: needs a square graph")
    refused(lib.gnx_signal_smoothness(wide.handle, None, P(f), P(D), P(d), P(sums), P(work), s), b"gnx_signal_smoothness: needs a square graph")
    refused(lib.gnx_signal_smoothness_back(wide.handle, None, *full, s), b"gnx_signal_smoothness_back: needs a square graph")
    torch.cuda.synchronize()
    for name, buffer in dict(out=out, out2=out2, d=d, gz=gz, sums=sums, work=work).items():
        assert bool(torch.isnan(buffer).all()), name
    # ... and the rectangular graph is served where squareness is not needed: 3 result rows forward, 4 transposed
    small = torch.full((8,), float("nan"), dtype=torch.float32, device="cuda")
    assert lib.gnx_signal_spmv(wide.handle, None, 0, P(x), None, 1.0, 0.0, P(small), s) == 0
    assert np.array_equal(host(small)[:3], np.array([ops["x"][1], 0.0, ops["x"][3]], dtype=np.float32)) and bool(torch.isnan(small[3:]).all())
    small.fill_(float("nan"))
    assert lib.gnx_signal_spmv(wide.handle, None, 1, P(x), None, 1.0, 0.0, P(small), s) == 0
    assert np.array_equal(host(small)[:4], np.array([0.0, ops["x"][0], 0.0, ops["x"][2]], dtype=np.float32)) and bool(torch.isnan(small[4:]).all())


# ---- 7. layers and models ------------------------------------------------------------------------------------------------------------------
def regime_inputs(width=40, classes=5):
    coo, vals, shape, _ = shapes.regime_graph("T")
    rng = np.random.default_rng(21)
    X = rng.standard_normal((shape[0], width)).astype(np.float32)
    nodes = rng.permutation(shape[0])[:400]
    return coo, vals, shape, X, nodes, rng.integers(0, classes, size=400)


def test_pprsweep_layer(gnntf):
    from gnntf import sparse
    coo, vals, shape, X, _, _ = regime_inputs(7)

    def model_with_sweep():
        gnntf.set_seed(SEED)
        model = gnntf.GNN(gnntf.SparseCOO(coo, vals, shape), X)
        model.add(gnntf.PPRSweep())
        return model

    model = model_with_sweep()
    model.training_mode(False)
    with torch.no_grad():
        out = model(model.features)
        adj = model.get_adjacency()
        signal = sparse.signal_ppr(adj, None, 0.1, 10)
        assert torch.equal(out, model.features / signal[:, None]) and torch.equal(out, sparse.sweep(adj, model.features))
        assert model.graph.last_kernel().startswith("signal_spmv_group")
        sparse.spmm(adj, model.features)
        other = model.graph.last_kernel()
        assert not other.startswith("signal_")
        again = model(model.features)
        assert model.graph.last_kernel() == other and torch.equal(again, out)       # the cached signal: no width-1 launch
    # the composition the layer replaces: ten PPR steps over a matrix of ones
    rowptr, colidx, _ = (x.cpu().numpy() for x in model.graph.csr_arrays())
    want, bound = ref.ppr_ref(sp.csr_matrix((host(adj.vals).astype(np.float64), colidx, rowptr), shape=shape), None, 0.1, 10, 512)
    assert ref.ratio1(host(signal), want, bound) <= 1
    ones = sparse.appnp_propagate(adj, torch.ones_like(model.features), 0.1, 10)
    assert float((ones - signal[:, None]).abs().max()) <= 1e-5 * float(signal.abs().max())
    # training mode: a dropped adjacency per forward; reproducible from the seed; differentiable w.r.t. the features alone
    train = model_with_sweep()
    with torch.no_grad():
        one, two = train(train.features), train(train.features)
    assert train.is_training() and train._mask_calls == 2 and not torch.equal(one, two)
    redo = model_with_sweep()
    with torch.no_grad():
        assert torch.equal(redo(redo.features), one) and torch.equal(redo(redo.features), two)
    feats = train.features.clone().requires_grad_()
    first = train._mask_calls
    train(feats).sum().backward()
    dropped = sparse.dropped_adjacency(train.graph, 0.5, SEED, first)
    assert torch.equal(feats.grad, (1.0 / sparse.signal_ppr(dropped, None, 0.1, 10))[:, None].expand_as(feats))


def build_reg_model(gnntf, inputs, **options):
    import model_step_ref as step
    coo, vals, shape, X, _, _ = inputs
    gnntf.set_seed(step.SEED)
    model = gnntf.GCNIIReg(gnntf.SparseCOO(coo, vals, shape), X, 5, latent_dims=[64], iterations=2, **options)
    layers = ref.gcniireg_layers(5, (64,), 2)
    start = step.initial_parameters(layers, X.shape[1], seed=31)
    assert [tuple(v.var.shape) for v in model.vars()] == [p.shape for p in start]
    for v, p in zip(model.vars(), start):
        v.assign(torch.from_numpy(p))
    return model, layers, start


class CountingLibrary:
    """The loaded library with every entry that is asked for recorded by name (tests/test_gpu_model_steps.py)."""

    def __init__(self, real):
        self.real, self.calls = real, set()

    def __getattr__(self, name):
        if name.startswith("gnx_"):
            self.calls.add(name)
        return getattr(self.real, name)


def test_gcniireg_training_step_against_float64(gnntf, monkeypatch):
    """One training step of GCNIIReg(iterations=2, latent_dims=[64]) on regime T: the loss and every parameter gradient against the dense
    float64 autograd restatement (signal_ref.gcniireg_reference over tests/model_step_ref.py), at that file's bar -- loss 1e-5 relative,
    gradients rtol 1e-3 and atol 2e-5 max|want| --; torch's feature masks are the same host-drawn ones on both sides, W and the stream
    numbering are read back from the model and compared with the restatement's own.
    No any-order bound of the WHOLE step is derived here (it would have to carry the bounds of two Dense layers, two GCNII layers, the
    head and their backwards through one another).  What FastReg adds to the step is held to its derived bound inside the step instead:
    the gradient the smoothness node hands to H0 in this very backward (tapped on a clone of its input) and the lambda it returned,
    against signal_ref.smoothness_ref over the operands the step used -- the model's float32 H0, the W it drew, the values of the
    adjacency it dropped and their column sums, upstream -1 -- with max |got - want| / bound <= 1."""
    import model_step_ref as step
    from gnntf import sparse
    from gnntf.training import _Objective
    tapped, real_smoothness = {}, sparse.smoothness

    def tapping_smoothness(adj, feats, w, **kwargs):
        tap = feats.clone()                             # the same values; its gradient is the node's dX alone
        tap.register_hook(lambda g: tapped.__setitem__("dX", g.detach().clone()))
        out = real_smoothness(adj, tap, w, **kwargs)
        tapped.update(adj=adj, X=feats.detach().clone(), w=w.detach().clone(), lam=out.detach().clone(), calls=tapped.get("calls", 0) + 1)
        return out

    monkeypatch.setattr(sparse, "smoothness", tapping_smoothness)
    inputs = regime_inputs()
    coo, vals, shape, X, nodes, labels = inputs
    nat = gnntf.sparse.nat
    counting = CountingLibrary(nat.lib())
    monkeypatch.setattr(nat, "lib", lambda: counting)
    model, layers, start = build_reg_model(gnntf, inputs)
    fixed = step.FixedMasks(23)
    model.dropout = lambda feats, p=0.5: feats if (not model.is_training() or p == 0) else \
        feats * torch.from_numpy(fixed.mask(tuple(feats.shape), p)).to(feats.device, feats.dtype)
    objective = _Objective(model, gnntf.NodeClassification(nodes, labels), step.WEIGHT_DECAY)
    before = len(model.vars())
    with model:
        loss = objective()
        loss.backward()
    fast = next(layer for layer in model.layers() if isinstance(layer, gnntf.FastReg))
    assert len(model.vars()) == before
    assert {"gnx_signal_uniform", "gnx_signal_project", "gnx_signal_smoothness", "gnx_signal_smoothness_back", "gnx_graph_colsum",
            "gnx_gcnii_step"} <= counting.calls
    assert model._mask_calls == 2                       # W's stream, then the dropped adjacency's
    reference = ref.gcniireg_reference(layers, coo, vals, shape, X, start, ("node", nodes, labels), step.WEIGHT_DECAY, step.SEED,
                                       step.FixedMasks(23))
    want_loss, want_grads = reference.step()
    assert reference.streams == model._mask_calls and reference.fastreg["w_stream"] == 0 and reference.fastreg["g_stream"] == 1
    assert np.array_equal(host(fast.W).reshape(-1), reference.fastreg["W"])             # the draw, read back from the model
    got_loss = float(loss.detach())
    got_grads = [host(v.var.grad).astype(np.float64) for v in model.vars()]
    ratios = [step.ratio_to_bar(g, w) for g, w in zip(got_grads, want_grads)]
    print(f"GCNIIReg step: loss {got_loss:.9g} against {want_loss:.9g} ({step.loss_ratio_to_bar(got_loss, want_loss):.3g} x the bar), "
          f"lambda {reference.fastreg['lam']:.6g}; worst gradient {max(ratios):.3g} x the bar")
    note("GCNIIReg gradient / bar", max(ratios))
    assert abs(reference.fastreg["lam"]) > 1e-3 * abs(want_loss)                        # the penalty is part of what is compared
    assert abs(got_loss - want_loss) <= step.LOSS_RTOL * abs(want_loss)
    for i, (g, w) in enumerate(zip(got_grads, want_grads)):
        scale = np.abs(w).max()
        assert scale > step.NON_TRIVIAL, i
        np.testing.assert_allclose(g, w, rtol=step.GRAD_RTOL, atol=step.GRAD_ATOL * scale, err_msg=f"variable {i}")
    # FastReg's part of the step at its derived bound
    assert tapped["calls"] == 1 and tuple(tapped["dX"].shape) == (shape[0], 64) and torch.equal(tapped["w"], fast.W)
    adj = tapped["adj"]
    assert adj.raw_dropout == (0.5, step.SEED, 1)
    rowptr, colidx, _ = (x.cpu().numpy() for x in model.graph.csr_arrays())
    kept = host(adj.vals)
    assert 0.4 < (kept == 0).mean() < 0.6
    A = sp.csr_matrix((kept.astype(np.float64), colidx, rowptr), shape=shape)
    D = host(sparse.signal_colsum(adj))                 # the bits the step's node read: the same call over the same values
    D_want, D_bound = ref.colsum_ref(A)
    assert ref.ratio1(D, D_want, D_bound) <= 1
    part = ref.smoothness_ref(A, host(tapped["X"]), host(tapped["w"]), D, 512, 512, upstream=-1.0)
    print(f"FastReg inside the step: lambda {float(tapped['lam']):.9g} against {part['lam']:.9g}, "
          f"{ref.ratio1(float(tapped['lam']), part['lam'], part['lam_bound']):.3g} of its bound; dH0 "
          f"{ref.ratio(host(tapped['dX']), part['dX'], part['dX_bound']):.3g} of its bound, largest |dH0| {np.abs(part['dX']).max():.3g}")
    assert note("FastReg in the step: lambda", ref.ratio1(float(tapped["lam"]), part["lam"], part["lam_bound"])) <= 1
    assert note("FastReg in the step: dH0", ref.ratio(host(tapped["dX"]), part["dX"], part["dX_bound"])) <= 1
    assert np.abs(part["dX"]).max() > 1e-4
    # without the penalty the first Dense's gradient is another one: the step above saw FastReg
    bare = ref.gcniireg_reference([layer for layer in layers if layer["kind"] != "fastreg"], coo, vals, shape, X, start,
                                  ("node", nodes, labels), step.WEIGHT_DECAY, step.SEED, step.FixedMasks(23)).step()[1]
    assert step.ratio_to_bar(got_grads[0], bare[0]) > 10


def test_gcniireg_captured_training_equals_eager(gnntf):
    """train(capture=True, epochs=3) against the eager run, torch.equal on every parameter: with the counter RNG's feature masks
    (feature_dropout / dense_dropout "fused") every draw of a step -- FastReg's W among them -- follows from (seed, stream + counter)."""
    inputs = regime_inputs()
    _, _, _, _, nodes, labels = inputs
    results = []
    for capture in (False, True):
        model, _, _ = build_reg_model(gnntf, inputs, feature_dropout="fused", dense_dropout="fused")
        gnntf.set_seed(11)
        torch.manual_seed(5)
        train, valid = gnntf.NodeClassification(nodes[:300], labels[:300]), gnntf.NodeClassification(nodes[300:], labels[300:])
        start = [v.var.detach().clone() for v in model.vars()]
        model.train(train=train, valid=valid, epochs=3, patience=50, capture=capture,
                    optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
        results.append(([v.var.detach().clone() for v in model.vars()], model._mask_calls, start))
    (eager, eager_masks, start), (captured, captured_masks, _) = results
    print("captured vs eager, max |difference| per variable:", [float((e - c).abs().max()) for e, c in zip(eager, captured)])
    assert eager_masks == captured_masks and eager_masks % 3 == 0
    assert all(torch.equal(e, c) for e, c in zip(eager, captured))
    assert any(not torch.equal(e, s) for e, s in zip(eager, start))


def test_appnpreg_runs_its_iterations_as_one_fused_run(gnntf):
    """APPNPReg is APPNP without the leading Dropout: its PPRIteration layers execute as the fused run APPNP's do (same bits)."""
    coo, vals, shape, X, _, _ = regime_inputs()
    outs = []
    for cls in (gnntf.APPNPReg, gnntf.APPNP):
        gnntf.set_seed(3)
        torch.manual_seed(3)
        model = cls(gnntf.SparseCOO(coo, vals, shape), X, 5, latent_dims=[16])
        model.reset()
        for i, v in enumerate(model.vars()):                # the same parameters in both
            v.assign(torch.from_numpy(np.random.default_rng(i).uniform(-0.3, 0.3, size=tuple(v.var.shape)).astype(np.float32)))
        model.training_mode(False)
        with torch.no_grad():
            outs.append(model(model.features))
        iterations = [layer for layer in model.layers() if isinstance(layer, gnntf.PPRIteration)]
        assert len(iterations) == 10 and iterations[0].__dict__.get("_pending_value") is not None      # a run: inner values are pending
    assert torch.equal(outs[0], outs[1])


def test_ratios_seen():
    """The worst error / bound per quantity over this module's tests (printed; each was asserted where it was measured)."""
    for name in sorted(RATIOS):
        print(f"{name}: {RATIOS[name]:.3g}")
    assert all(v <= 1 for k, v in RATIOS.items() if "bar" not in k)
