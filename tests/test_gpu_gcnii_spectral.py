"""The fused GCNIISpectralPreservingLayer on the MI355X (gnx_gcnii_step_spectral, gnx_gcnii_spectral_back, sparse.gcnii_step_spectral,
GCNII(gcnii_spectral="fused")) against float64 with the derived bound of tests/gcnii_spectral_ref.py (criterion: max |got - want| /
bound <= 1; tests/test_gcnii_spectral_cpu.py holds the float32 emulations against the same bound), the gate bits against the float64
sign, and bitwise relations: a row's bits under a permutation of the row ids, p = 0 against p = 0.5 (s = 2: the kept values are exact
doubles), reproducibility, the dropout counter, the gate pass on constructed bits, autograd with the saved bytes counted, the model.
Shapes: regime T (n = 1547, 23 hub rows, a tile without entries, a ragged last tile) at C = 16, 32, 64, regime S (n = 2^15 + 11, 154 hub
rows: more than one block of the row-list pass) at C = 64, and C = 24 on regime T (two launches and the pass over all rows)."""
import functools

import numpy as np
import pytest
import torch

import gcnii_shapes_ref as ref
import gcnii_spectral_ref as sref
import graphs
from oracle import gnntf_oracle as orc

pytestmark = pytest.mark.gpu

A_MIX = 0.1
SEED, STREAM = 7, 2
CASES = [("T", 16), ("T", 32), ("T", 64), ("S", 64), ("T", 24)]
RATES = (0.0, 0.5)
FUSED = (16, 32, 64)
INVALID = -1
SENTINEL = 9.0


def kernel_name(C, p):
    return ("spmm_gcnii_spectral_mfma" if C in FUSED else "spmm+dense_mfma_spectral") + ("_drop" if p != 0 else "")


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()            # (a copy: the shared operands are read-only)


def host(t):
    return t.detach().cpu().numpy()


class Handle:
    """A graph on the device, its symmetric normalisation, and the float32 weights the kernels read as a float64 CSR matrix."""

    def __init__(self, gnntf, coo, vals, shape, normalised=True):
        import scipy.sparse as sp
        self.g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
        self.adj = gnntf.normalize(self.g, "symmetric") if normalised else gnntf.Adjacency(self.g, self.g.csr_arrays()[2])
        rowptr, colidx, _ = (x.cpu().numpy() for x in self.g.csr_arrays())
        self.n = shape[0]
        self.A = sp.csr_matrix((self.adj.vals.cpu().numpy().astype(np.float64), colidx, rowptr), shape=shape)
        self.L = ref.plan_threshold(self.n)
        self.deg = np.diff(rowptr)
        self.hub, self.empty = np.flatnonzero(self.deg > self.L), np.flatnonzero(self.deg == 0)
        self.ragged = np.arange(self.n - self.n % 16, self.n)


_runs = {}


@pytest.fixture(scope="module")
def handles(gnntf):
    out = {}
    for regime in ("T", "S"):
        coo, vals, shape, info = ref.regime_graph(regime)
        h = Handle(gnntf, coo, vals, shape)
        assert np.array_equal(h.hub, info["hub"]) and len(h.hub) == (23 if regime == "T" else 154) and h.g.n_hub_rows == len(h.hub)
        assert len(h.empty) > 16 and h.n % 16 == 11 and (h.deg[h.ragged] > h.L).any() and h.deg[0] > h.L
        out[regime] = h
    yield out
    _runs.clear()
    _wants.clear()
    operands.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def operands(n, C):
    return sref.operands(n, C, 1000 + C)


def entry(gnntf, h, C, relu, p, stream=STREAM, train=True, adj=None, ops=None, seed=SEED):
    """gnx_gcnii_step_spectral itself into poisoned buffers: (out, T, gate words) as device tensors (T, gate None without ``train``)."""
    nat = gnntf.sparse.nat
    op = operands(h.n, C) if ops is None else ops
    d = {k: dev(op[k]) for k in ("H", "H0", "M", "bias")}
    out = torch.full((h.n, C), float("nan"), device="cuda")
    mixed = torch.full((h.n, C), float("nan"), device="cuda") if train or C not in FUSED else None
    gate = torch.full((h.n, sref.gate_words(C)), 0x55555555, dtype=torch.int32, device="cuda") if train and relu else None
    adj = h.adj if adj is None else adj
    nat.check(nat.lib().gnx_gcnii_step_spectral(h.g.handle, nat.ptr(adj.vals), nat.ptr(d["H"]), nat.ptr(d["H0"]), A_MIX, C, nat.ptr(d["M"]), C,
                                                nat.ptr(d["bias"]), nat.ACT_RELU if relu else nat.ACT_NONE, float(p), seed, stream,
                                                nat.ptr(out), nat.ptr(mixed), nat.ptr(gate), nat.current_stream()))
    assert h.g.last_kernel() == kernel_name(C, p)
    assert not torch.isnan(out).any(), "a row was written by no path"
    assert mixed is None or not torch.isnan(mixed).any()
    return out, mixed if train else None, gate


def run(gnntf, handles, regime, C, p, relu):
    """The training form of one case, once: host arrays out, T, gate words."""
    key = (regime, C, p, relu)
    if key not in _runs:
        out, T, gate = entry(gnntf, handles[regime], C, relu, p)
        _runs[key] = (host(out), host(T), None if gate is None else host(gate))
    return _runs[key]


_wants = {}


def reference(h, regime, C, p, relu):
    key = (regime, C, p, relu)
    if key not in _wants:
        op = operands(h.n, C)
        _wants[key] = sref.spectral_ref(h.A, op["H"], op["H0"], op["M"], op["bias"], A_MIX, relu, p, sref.keep(SEED, STREAM, p, h.n, C), h.L)
    return _wants[key]


# ---- 1. the forward against float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("regime, C", CASES)
def test_forward_against_float64(gnntf, handles, regime, C, p, relu):
    h = handles[regime]
    out, T, _ = run(gnntf, handles, regime, C, p, relu)
    want = reference(h, regime, C, p, relu)
    worst = ref.ratio(out, want["out"], want["out_bound"])
    parts = {name: ref.ratio(out, want["out"], want["out_bound"], rows) for name, rows in (("hub", h.hub), ("empty", h.empty), ("ragged", h.ragged))}
    print(f"forward {regime} C={C} p={p} relu={relu}: error / bound = {worst:.3f}, {parts}")
    assert worst <= 1.0 and all(r <= 1.0 for r in parts.values())
    mask = sref.keep(SEED, STREAM, p, h.n, C)
    assert not out[~mask].any() and not np.signbit(out[~mask]).any()               # a dropped value is +0
    assert p == 0 or relu or 0.4 < (out == 0).mean() < 0.6
    # the mixed rows: the bits of gnx_gcnii_step's
    op = operands(h.n, C)
    _, T_plain = gnntf.sparse._gcnii_launch(h.adj, dev(op["H"]), dev(op["H0"]), A_MIX, dev(op["M"]), relu, keep_mixed=True)
    assert np.array_equal(T.view(np.int32), host(T_plain).view(np.int32))
    # the inference form (the host function without autograd: no T, no gate) has the bits of the training form
    with torch.no_grad():
        got = gnntf.gcnii_step_spectral(h.adj, dev(op["H"]), dev(op["H0"]), A_MIX, dev(op["M"]), dev(op["bias"]), relu=relu,
                                        dropout=(p, SEED, STREAM))
    assert h.g.last_kernel() == kernel_name(C, p)
    assert np.array_equal(host(got).view(np.int32), out.view(np.int32))


# ---- 2. the gate bits against the float64 sign ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("regime, C", CASES)
def test_gate_bits_against_the_float64_sign(gnntf, handles, regime, C, p):
    h = handles[regime]
    _, _, words = run(gnntf, handles, regime, C, p, True)
    want = reference(h, regime, C, p, True)
    bits, pad_clear = sref.unpack_gate(words, C)
    assert pad_clear, "a pad bit is set (or a row's word was not written)"
    wrong, share = sref.gate_check(bits, want["P"], want["P_bound"])
    print(f"gate {regime} C={C} p={p}: {wrong} wrong, {share * bits.size:.0f} of {bits.size} undecided")
    assert share <= sref.AMBIGUOUS_SHARE
    assert wrong == 0
    decided = np.abs(want["P"]) > want["P_bound"]
    for rows in (h.hub, h.empty, h.ragged):                                         # both signs occur in every class of rows
        assert decided[rows].mean() > 0.99 and 0 < bits[rows].mean() < 1
    assert np.array_equal(words, run(gnntf, handles, regime, C, 0.0, True)[2])     # the gate does not depend on the mask


# ---- 3. a row's bits under a permutation of the row ids; rates, streams, the counter ------------------------------------------------------
N_SHORT = 1547


@pytest.fixture(scope="module")
def short(gnntf):
    """A short-rowed graph (no row above 40 entries, ids 32 .. 47 and the last 5 rows without entries) as it is and with its ROW ids
    permuted (column ids stay): row pi(i) of the second holds the entries of row i of the first, in the same order, so a row's sums are
    the same sums -- while its tile, its place in the tile and its neighbours there are others.  Raw values: no normalisation between."""
    rng = np.random.default_rng(21)
    n = N_SHORT
    deg = rng.integers(0, 41, size=n)
    deg[32:48] = 0
    deg[-5:] = 0
    rows = np.repeat(np.arange(n), deg)
    cols = np.concatenate([rng.choice(n, size=d, replace=False) for d in deg])
    vals = rng.uniform(0.5, 1.5, size=len(rows)).astype(np.float32)
    pi = rng.permutation(n)
    plain = Handle(gnntf, np.stack([rows, cols], axis=1).astype(np.int64), vals, (n, n), normalised=False)
    moved = Handle(gnntf, np.stack([pi[rows], cols], axis=1).astype(np.int64), vals, (n, n), normalised=False)
    assert plain.g.n_hub_rows == 0 and moved.g.n_hub_rows == 0 and len(plain.hub) == 0
    assert np.array_equal(moved.deg[pi], plain.deg) and (pi // 16 != np.arange(n) // 16).mean() > 0.9
    return plain, moved, pi


@pytest.mark.parametrize("C", [16, 32, 64, 24])
def test_rows_keep_their_bits_under_a_row_permutation(gnntf, short, C):
    plain, moved, pi = short
    op = dict(operands(N_SHORT, C))
    moved_op = dict(op)
    H0_moved = np.empty_like(op["H0"])
    H0_moved[pi] = op["H0"]
    moved_op["H0"] = H0_moved
    out, T, gate = (host(x) for x in entry(gnntf, plain, C, True, 0.0, ops=op))
    out_m, T_m, gate_m = (host(x) for x in entry(gnntf, moved, C, True, 0.0, ops=moved_op))
    assert np.array_equal(T_m[pi].view(np.int32), T.view(np.int32))
    assert np.array_equal(out_m[pi].view(np.int32), out.view(np.int32)) and np.array_equal(gate_m[pi], gate)
    assert 0.2 < sref.unpack_gate(gate, C)[0].mean() < 0.8
    # p = 0.5: s = 2 exactly, so a kept value is the exact double of the p = 0 value and the gate is the same, on either handle
    for h, ops, out0, gate0 in ((plain, op, out, gate), (moved, moved_op, out_m, gate_m)):
        out_p, _, gate_p = (host(x) if x is not None else None for x in entry(gnntf, h, C, True, 0.5, ops=ops))
        mask = sref.keep(SEED, STREAM, 0.5, N_SHORT, C)
        assert np.array_equal(out_p.view(np.int32), np.where(mask, np.float32(2) * out0, np.float32(0)).view(np.int32))
        assert np.array_equal(gate_p, gate0)
    # the inference form of the same call: the same out, nothing else written
    out_i, T_i, gate_i = entry(gnntf, plain, C, True, 0.0, train=False, ops=op)
    assert T_i is None and gate_i is None and np.array_equal(host(out_i).view(np.int32), out.view(np.int32))


@pytest.mark.parametrize("C", [64, 24])
def test_two_calls_agree_streams_differ_and_the_counter_shifts(gnntf, handles, C):
    h = handles["T"]
    first = entry(gnntf, h, C, True, 0.5, stream=8)
    second = entry(gnntf, h, C, True, 0.5, stream=8)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    other = entry(gnntf, h, C, False, 0.5, stream=9)[0]
    reseeded = entry(gnntf, h, C, False, 0.5, stream=8, seed=SEED + 1)[0]
    same = entry(gnntf, h, C, False, 0.5, stream=8)[0]
    for different in (other, reseeded):
        assert 0.3 < float(((same != 0) != (different != 0)).float().mean()) < 0.7
    up = dev(operands(h.n, C)["G"])
    back = gnntf.sparse._gcnii_spectral_gate(h.g, up, first[2], True, (0.5, SEED, 8))
    counter = torch.tensor([3], dtype=torch.int64, device="cuda")
    h.g.set_dropout_counter(counter)
    try:
        shifted = entry(gnntf, h, C, True, 0.5, stream=5)
        shifted_back = gnntf.sparse._gcnii_spectral_gate(h.g, up, shifted[2], True, (0.5, SEED, 5))
        torch.cuda.synchronize()
    finally:
        h.g.set_dropout_counter(None)
    assert all(torch.equal(a, b) for a, b in zip(shifted, first))
    assert all(torch.equal(a, b) for a, b in zip(shifted_back, back))
    assert all(torch.equal(a, b) for a, b in zip(entry(gnntf, h, C, True, 0.5, stream=8), first))      # the counter is gone again


# ---- 4. the gate pass on constructed gate bits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("n, C", [(1547, 16), (1547, 24), (1547, 32), (1547, 64), (1547, 7), ((1 << 15) + 11, 64)])
def test_gate_pass_on_constructed_bits(gnntf, handles, n, C, p):
    sparse = gnntf.sparse
    nat = sparse.nat
    g = handles["T"].g                                                 # (lends its dropout counter; any handle will do)
    rng = np.random.default_rng(n + C)
    bits = rng.random((n, C)) < 0.6
    up = rng.standard_normal((n, C)).astype(np.float32)
    words = sref.pack_gate(bits)
    mask = sref.keep(SEED, STREAM, p, n, C)
    triple = (p, SEED, STREAM)
    want_G, terms = sref.gate_pass_f32(up, bits, p, mask)
    G, dbias = sparse._gcnii_spectral_gate(g, dev(up), dev(words), True, triple)
    assert np.array_equal(host(G).view(np.int32), want_G.view(np.int32))
    want_db, bound = sref.column_sum_ref(terms)
    assert (bound > 0).all()
    worst = float((np.abs(host(dbias).astype(np.float64) - want_db) / bound).max())
    print(f"gate pass n={n} C={C} p={p}: dbias error / bound = {worst:.4f}")
    assert worst <= 1.0
    G2, dbias2 = sparse._gcnii_spectral_gate(g, dev(up), dev(words), True, triple)
    assert torch.equal(G, G2) and torch.equal(dbias.view(torch.int32), dbias2.view(torch.int32))
    # the identity: no gate, G' = u, dbias exact zeros (over a poisoned buffer: written)
    want_u, _ = sref.gate_pass_f32(up, None, p, mask)
    upd, Gi, dbi = dev(up), torch.full((n, C), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
    nat.check(nat.lib().gnx_gcnii_spectral_back(g.handle, nat.ptr(upd), C, None, n, C, nat.ACT_NONE, float(p), SEED, STREAM, nat.ptr(Gi), C,
                                                nat.ptr(dbi), None, 0, nat.current_stream()))
    assert np.array_equal(host(Gi).view(np.int32), want_u.view(np.int32))
    assert np.array_equal(host(dbi).view(np.int32), np.zeros(C, dtype=np.int32))
    # in place: G is g
    work = torch.empty(max(1, min(2048, (n + 255) // 256)) * C, device="cuda")
    wd, db = dev(words), torch.empty(C, device="cuda")
    nat.check(nat.lib().gnx_gcnii_spectral_back(g.handle, nat.ptr(upd), C, nat.ptr(wd), n, C, nat.ACT_RELU, float(p), SEED, STREAM, nat.ptr(upd), C,
                                                nat.ptr(db), nat.ptr(work), work.numel(), nat.current_stream()))
    assert torch.equal(upd, G) and torch.equal(db.view(torch.int32), dbias.view(torch.int32))


# ---- 5. autograd ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backward", ["composed", "fused"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C", [64, 24])
def test_autograd_against_float64(gnntf, handles, C, relu, backward):
    h = handles["T"]
    n, p = h.n, 0.5
    op = operands(n, C)
    mask = sref.keep(SEED, STREAM, p, n, C)
    leaves = [dev(op[k]).requires_grad_() for k in ("H", "H0", "M")] + [dev(op["bias"]).reshape(1, C).requires_grad_()]
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        out = gnntf.gcnii_step_spectral(h.adj, leaves[0], leaves[1], A_MIX, leaves[2], leaves[3], relu=relu, dropout=(p, SEED, STREAM),
                                        backward=backward)
    assert h.g.last_kernel() == kernel_name(C, p)
    assert out.grad_fn is not None and type(out.grad_fn).__name__ == "_GCNIISpectralStepBackward"
    # what the node keeps: T, M and (relu) the gate words -- neither act(P') nor out nor a byte mask
    words_per_row = sref.gate_words(C)
    want_bytes = 4 * n * C + 4 * C * C + (4 * n * words_per_row if relu else 0)
    assert sum(t.numel() * t.element_size() for t in saved) == want_bytes and len(saved) == (3 if relu else 2)
    T = host([t for t in saved if tuple(t.shape) == (n, C)][0])
    fwd_out, fwd_T, fwd_gate = run(gnntf, handles, "T", C, p, relu)
    assert np.array_equal(host(out).view(np.int32), fwd_out.view(np.int32)) and np.array_equal(T.view(np.int32), fwd_T.view(np.int32))
    bits = None
    if relu:
        words = host([t for t in saved if t.dtype == torch.int32][0])
        assert np.array_equal(words, fwd_gate)
        bits = sref.unpack_gate(words, C)[0]
    out.backward(dev(op["G"]))
    dH, dH0, dM, dbias = (host(leaf.grad) for leaf in leaves)
    assert dbias.shape == (1, C)
    # the float64 backward from the launch's own gate bits and the explicit mask
    G32, terms = sref.gate_pass_f32(op["G"], bits, p, mask)
    want = ref.backward_ref(h.A, G32, op["Mt"], A_MIX, L=h.L)
    want_dM, dM_bound = sref.wgrad_ref(T, G32)
    want_db, db_bound = sref.column_sum_ref(terms)
    ratios = dict(dH=ref.ratio(dH, want["dH"], want["dH_bound"]), dH0=ref.ratio(dH0, want["S"], want["S_bound"]),
                  dM=ref.ratio(dM, want_dM, dM_bound))
    if relu:
        ratios["dbias"] = ref.ratio(dbias, want_db[None, :], db_bound[None, :])    # (a column whose relu is open in every row: 0 within 0)
    else:
        assert not dbias.any()
    print(f"autograd C={C} relu={relu} {backward}: error / bound = {ratios}")
    assert all(r <= 1.0 for r in ratios.values()), ratios
    assert np.abs(dH).max() > 0 and np.abs(dM).max() > 0 and (not relu or np.abs(dbias).max() > 0)


# ---- 6. the model -------------------------------------------------------------------------------------------------------------------------
def spectral_model(gnntf, **option):
    """The three-layer spectral GCNII of tests/test_gpu_dense.py::test_spectral_preserving_layer_variants: its graph, seeds and weights."""
    coo, vals, shape = graphs.rmat_symmetric_coo(900, 7000, seed=6)
    rng = np.random.default_rng(6)
    X = rng.standard_normal((900, 24)).astype(np.float32)
    rng.uniform(-0.3, 0.3, size=(1, 16)), rng.uniform(-0.3, 0.3, size=(1, 5))      # (the draws that test's GCN half takes first)
    gnntf.set_seed(0)
    torch.manual_seed(0)
    model = gnntf.GCNII(gnntf.SparseCOO(coo, vals, shape), X, num_classes=5, latent_dims=[32], iterations=3,
                        layer_type=gnntf.GCNIISpectralPreservingLayer, **option)
    model.reset()
    convs = [l for l in model.layers() if isinstance(l, gnntf.GCNIISpectralPreservingLayer)]
    for l in convs:
        with torch.no_grad():
            l.W.copy_(dev((rng.standard_normal((32, 32)) * 0.2).astype(np.float32)))
            l.bias.copy_(dev(rng.uniform(-0.2, 0.2, size=(1, 32)).astype(np.float32)))
    return model, convs, (coo, vals, shape, X)


def test_model_eval_against_float64_and_the_default_is_untouched(gnntf):
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    fused, convs, (coo, vals, shape, X) = spectral_model(gnntf, gcnii_spectral="fused")
    default, _, _ = spectral_model(gnntf)
    again, _, _ = spectral_model(gnntf, gcnii_spectral="composed")
    assert default.gcnii_spectral == "composed" and fused.gcnii_spectral == "fused"
    for a_, b_ in zip(default.vars(), fused.vars()):                 # the same parameters in the three models
        assert torch.equal(a_.var, b_.var)
    ai, av = orc.get_adjacency(coo, vals, shape, dtype=np.float64)
    dense = [l for l in fused.layers() if isinstance(l, gnntf.Dense)]
    H0 = np.maximum(X.astype(np.float64) @ f64(dense[0].W) + f64(dense[0].b), 0)
    H = H0
    for k, l in enumerate(convs):
        beta = np.log1p(0.5 / (k + 1))
        T = orc.ppr_iteration(ai, av, shape, H, H0, 0.1)
        H = 2 * (np.maximum(T @ ((1 - beta) * np.eye(32) + beta * f64(l.W)) + f64(l.bias), 0) - f64(l.bias))
    want = H @ f64(dense[1].W) + f64(dense[1].b)
    outs, names = [], []
    for model in (fused, default, again):
        model.training_mode(False)
        with torch.no_grad():
            outs.append(model(model.features))
        names.append(model.graph.last_kernel())
    np.testing.assert_allclose(host(outs[0]), want, rtol=1e-4, atol=1e-4)          # that test's tolerances
    np.testing.assert_allclose(host(outs[1]), want, rtol=1e-4, atol=1e-4)
    assert names[0] == "spmm_gcnii_spectral_mfma"
    assert names[1] == names[2] and names[1] and "spectral" not in names[1]        # today's SpMM + mix, then the dense kernel
    assert torch.equal(outs[1], outs[2])
    # feature_dropout="fused" on a spectral stack keeps today's path; a plain stack does not notice gcnii_spectral
    other, _, _ = spectral_model(gnntf, feature_dropout="fused")
    other.training_mode(False)
    with torch.no_grad():
        assert torch.equal(other(other.features), outs[1]) and other.graph.last_kernel() == names[1]


@pytest.fixture(scope="module")
def cora():
    coo, vals, shape, X = graphs.cora_shaped(seed=4)
    labels = np.random.default_rng(4).integers(0, 7, size=shape[0])
    weights = [(np.random.default_rng(40 + k).standard_normal((32, 32)) / 6).astype(np.float32) for k in range(4)]
    biases = [np.random.default_rng(60 + k).uniform(-0.2, 0.2, size=(1, 32)).astype(np.float32) for k in range(4)]
    return dict(coo=coo, vals=vals, shape=shape, X=X, labels=labels, weights=weights, biases=biases, train=np.arange(0, 300),
                valid=np.arange(300, 600))


def make_model(gnntf, cora, seeded_weights=True, layer_type=None, **option):
    gnntf.set_seed(11)
    torch.manual_seed(3)
    layer_type = gnntf.GCNIISpectralPreservingLayer if layer_type is None else layer_type
    model = gnntf.GCNII(gnntf.SparseCOO(cora["coo"], cora["vals"], cora["shape"]), cora["X"], 7, latent_dims=[32], iterations=4,
                        layer_type=layer_type, **option)
    model.reset()
    convs = [layer for layer in model.layers() if isinstance(layer, gnntf.GCNIILayer)]
    assert len(convs) == 4
    if seeded_weights:                                  # the reference initialises W and the bias to zero
        for layer, W, b in zip(convs, cora["weights"], cora["biases"]):
            layer.W.data.copy_(dev(W))
            if hasattr(layer, "bias"):
                layer.bias.data.copy_(dev(b))
    return model


def three_steps(gnntf, cora, model):
    """Three plain gradient steps in training mode (tests/test_gpu_gcnii_drop.py): (losses, gradients of every step, mask streams taken)."""
    task = gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]])
    losses, grads = [], []
    first = model._mask_calls
    for _ in range(3):
        with model:
            for v in model.vars():
                v.var.grad = None
            loss = task.loss(model(model.features))
            loss.backward()
        losses.append(float(loss.detach()))
        grads.append([v.var.grad.clone() for v in model.vars()])
        with torch.no_grad():
            for v in model.vars():
                v.var -= 0.05 * v.var.grad
    return losses, grads, model._mask_calls - first


@pytest.mark.parametrize("backward", ["composed", "fused"])
def test_training_step_is_reproducible_from_the_seed(gnntf, cora, backward):
    option = dict(gcnii_spectral="fused", gcnii_backward=backward)
    model = make_model(gnntf, cora, **option)
    one = three_steps(gnntf, cora, model)
    assert model.graph.last_kernel() != "" and one[2] == 3 * 5          # per step: the input features' mask and one per spectral layer
    two = three_steps(gnntf, cora, make_model(gnntf, cora, **option))
    assert one[0] == two[0] and len(set(one[0])) == 3 and all(np.isfinite(one[0]))
    for step_one, step_two in zip(one[1], two[1]):
        assert len(step_one) > 8 and all(torch.equal(a_, b_) for a_, b_ in zip(step_one, step_two))
    spectral = [l for l in model.layers() if isinstance(l, gnntf.GCNIISpectralPreservingLayer)]
    assert len(spectral) == 4 and all(float(l.bias.grad.abs().max()) > 0 and float(l.W.grad.abs().max()) > 0 for l in spectral)
    with model, torch.no_grad():                                         # a training-mode forward: the fused launch with its mask
        model(model.features)
    assert model.graph.last_kernel() == "spmm_gcnii_spectral_mfma_drop"
    model = make_model(gnntf, cora, **option)
    gnntf.set_seed(12)                                                   # the same parameters, other masks
    other = three_steps(gnntf, cora, model)
    assert other[0] != one[0]
    # a plain GCNIILayer stack does not notice the switch
    plain = three_steps(gnntf, cora, make_model(gnntf, cora, layer_type=gnntf.GCNIILayer, gcnii_spectral="fused"))
    plain_default = three_steps(gnntf, cora, make_model(gnntf, cora, layer_type=gnntf.GCNIILayer))
    assert plain[0] == plain_default[0] and all(torch.equal(a_, b_) for a_, b_ in zip(plain[1][2], plain_default[1][2]))


def test_captured_training_equals_eager(gnntf, cora, monkeypatch):
    """train(capture=True, epochs=2), bit for bit the eager run (the pattern of tests/test_gpu_gcnii_drop.py)."""
    from gnntf import training
    observed, observe = [], training._BestSoFar.observe
    monkeypatch.setattr(training._BestSoFar, "observe", lambda self, loss: (observed[-1].append(loss), observe(self, loss))[1])
    results = []
    for capture in (False, True):
        observed.append([])
        model = make_model(gnntf, cora, seeded_weights=False, gcnii_spectral="fused")
        gnntf.set_seed(11)
        torch.manual_seed(5)
        valid = gnntf.NodeClassification(cora["valid"], cora["labels"][cora["valid"]])
        model.train(train=gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]]), valid=valid, epochs=2, patience=50,
                    capture=capture, optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
        results.append(([v.var.detach().clone() for v in model.vars()], float(model.loss(valid)), model._mask_calls))
    (eager, eager_loss, eager_masks), (captured, captured_loss, captured_masks) = results
    assert eager_masks == captured_masks == 2 * 5
    print("captured vs eager, max |difference| per variable:", [float((e - c).abs().max()) for e, c in zip(eager, captured)])
    assert all(torch.equal(e, c) for e, c in zip(eager, captured))
    assert eager_loss == captured_loss
    assert len(observed[0]) == len(observed[1]) == 2 and observed[0] == observed[1] and len(set(observed[0])) == 2


# ---- 7. what the entries refuse -------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_write_nothing(gnntf, handles):
    nat = gnntf.sparse.nat
    lib = nat.lib()
    h = handles["T"]
    n, C = h.n, 16
    zeros = lambda *shape: torch.zeros(*shape, device="cuda")
    b = dict(H=zeros(n, C), H0=zeros(n, C), M=torch.eye(C, device="cuda"), bias=zeros(C), g=zeros(n, C),
             out=torch.full((n, C), SENTINEL, device="cuda"), mixed=torch.full((n, C), SENTINEL, device="cuda"),
             gate=torch.full((n, 1), 7, dtype=torch.int32, device="cuda"), G=torch.full((n, C), SENTINEL, device="cuda"),
             dbias=torch.full((C,), SENTINEL, device="cuda"), work=torch.full((2048 * C,), SENTINEL, device="cuda"))
    coo, vals, shape, _ = ref.regime_graph("T")
    wide = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, (shape[0], shape[1] + 1)), device="cuda:0")
    gnntf.spmm(gnntf.Adjacency(h.g), zeros(n, 16))
    before = h.g.last_kernel()

    def step(handle=h.g, **wrong):
        a = dict(H="H", H0="H0", a=A_MIX, C=C, M="M", ldm=C, bias="bias", act=1, p=0.5, seed=SEED, stream_id=STREAM, out="out", mixed="mixed",
                 gate="gate")
        a.update(wrong)
        values = [nat.ptr(b[v]) if isinstance(v, str) else v for v in a.values()]
        return lib.gnx_gcnii_step_spectral(handle.handle, None, *values, nat.current_stream())

    def back(**wrong):
        a = dict(g="g", ldg=C, gate="gate", n=n, C=C, act=1, p=0.5, seed=SEED, stream_id=STREAM, G="G", ldG=C, dbias="dbias", work="work",
                 work_floats=2048 * C)
        a.update(wrong)
        values = [nat.ptr(b[v]) if isinstance(v, str) else v for v in a.values()]
        return lib.gnx_gcnii_spectral_back(h.g.handle, *values, nat.current_stream())

    table = [
        (step, dict(p=1.0), ["gnx_gcnii_step_spectral:", "outside [0, 1)"]),
        (step, dict(p=-0.1), ["gnx_gcnii_step_spectral:", "outside [0, 1)"]),
        (step, dict(bias=None), ["gnx_gcnii_step_spectral:", "NULL bias"]),
        (step, dict(gate=None), ["gnx_gcnii_step_spectral:", "needs d_gate"]),
        (step, dict(gate="out"), ["gnx_gcnii_step_spectral:", "d_gate must be a buffer of its own"]),
        (step, dict(gate="mixed"), ["gnx_gcnii_step_spectral:", "d_gate must be a buffer of its own"]),
        (step, dict(bias="H0"), ["gnx_gcnii_step_spectral:", "d_bias must be a buffer of its own"]),
        (step, dict(mixed="out"), ["gnx_gcnii_step_spectral:", "d_mixed must be a buffer of its own"]),
        (step, dict(out="H"), ["gnx_gcnii_step_spectral:", "out must not alias X"]),
        (step, dict(act=7), ["gnx_gcnii_step_spectral:", "invalid activation"]),
        (step, dict(handle=wide), ["gnx_gcnii_step_spectral:", "square graph"]),
        (back, dict(p=1.0), ["gnx_gcnii_spectral_back:", "outside [0, 1)"]),
        (back, dict(gate=None), ["gnx_gcnii_spectral_back:", "relu needs d_gate"]),
        (back, dict(gate="G"), ["gnx_gcnii_spectral_back:", "relu needs d_gate"]),
        (back, dict(dbias="G"), ["gnx_gcnii_spectral_back:", "dbias must be a buffer of its own"]),
        (back, dict(work="G"), ["gnx_gcnii_spectral_back:", "d_work must be a buffer of its own"]),
        (back, dict(work_floats=C), ["gnx_gcnii_spectral_back:", "work_floats"]),
        (back, dict(ldg=C - 1), ["gnx_gcnii_spectral_back:", "row stride below C"]),
    ]
    for call, wrong, words in table:
        rc = call(**wrong)
        message = lib.gnx_last_error()
        assert rc == INVALID and all(w.encode() in message for w in words), (wrong, rc, message)
    torch.cuda.synchronize()
    for k in ("out", "mixed", "G", "dbias", "work"):
        assert bool((b[k] == SENTINEL).all()), k
    assert bool((b["gate"] == 7).all()) and h.g.last_kernel() == before
    # a missing gate is fine where nothing needs it: inference (no d_mixed), and the identity
    assert step(gate=None, mixed=None) == 0 and step(gate=None, act=0) == 0
    torch.cuda.synchronize()
    assert not bool((b["out"] == SENTINEL).any())
