"""Opt-in bf16 feature storage of the fused GCNII layer (gnx_gcnii_step_bf16, sparse.gcnii_step(storage=), GCNII(inference_dtype=)):
bit-exactness against the f32 entry over bf16-representable rows, the one rounding store, the argument rules, a stack of layers against
a float64 emulation of the rounding points in include/gnx.h with a first-order bound computed here, and the model-level chain."""
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import graphs
from bf16_ref import U, bf16_round

pytestmark = pytest.mark.gpu

A_MIX = 0.1
N = 3003                 # 3000 R-MAT vertices + 3 isolated ones; 3003 = 16 * 187 + 11: the last tile of the fused kernel is ragged
FUSED = (16, 32, 64)


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def shaped_coo(hub):
    """A symmetric R-MAT of 3000 vertices / 20000 entries, with ``hub`` one row / column of 900 entries more (tests/test_gpu_dense.py's
    hub_graph recipe: longer than the handle's long-row threshold), and vertices 3000 .. 3002 without any entry.  Without ``hub`` the
    graph is hub-FREE: an R-MAT grows heavy rows of its own, so every entry of a vertex with more than 300 entries is dropped (both
    directions: the pattern stays symmetric, no row can grow)."""
    coo, _, _ = graphs.rmat_symmetric_coo(3000, 20000, seed=11)
    if not hub:
        heavy = np.bincount(coo[:, 0], minlength=3000) > 300
        coo = coo[~(heavy[coo[:, 0]] | heavy[coo[:, 1]])]
    if hub:
        others = np.random.default_rng(11).choice(np.arange(1, 3000), size=900, replace=False)
        extra = np.concatenate([np.stack([np.zeros_like(others), others], 1), np.stack([others, np.zeros_like(others)], 1)])
        coo = np.unique(np.concatenate([coo, extra]), axis=0)
    return coo, np.ones(len(coo), dtype=np.float32), (N, N)


def tiny_coo():
    """11 vertices: fewer rows than one 16-row tile; vertex 10 isolated."""
    pairs = np.array([(0, 1), (0, 2), (0, 3), (1, 2), (2, 5), (3, 4), (4, 6), (5, 6), (6, 7), (7, 8), (8, 9), (1, 9), (0, 9)])
    coo = np.concatenate([pairs, pairs[:, ::-1]])
    return coo, np.ones(len(coo), dtype=np.float32), (11, 11)


class Case:
    def __init__(self, gnntf, coo, vals, shape):
        self.g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
        self.adj = gnntf.normalize(self.g, "symmetric")
        rowptr, colidx, _ = self.g.csr_arrays()
        # the very weights the kernels read, as float64
        self.A = sp.csr_matrix((self.adj.vals.cpu().numpy().astype(np.float64), colidx.cpu().numpy(), rowptr.cpu().numpy()), shape=shape)
        self.n = shape[0]


@pytest.fixture(scope="module")
def cases(gnntf):
    return {"hub": Case(gnntf, *shaped_coo(True)), "flat": Case(gnntf, *shaped_coo(False)), "tiny": Case(gnntf, *tiny_coo())}


def operands(n, C, seed, layers=1):
    """H, H0 seeded normal; M_l = (1-b) I + b W_l with seeded W_l, b = log1p(0.5 / (l + 1)) as the model makes it."""
    rng = np.random.default_rng(seed)
    H, H0 = rng.standard_normal((n, C)).astype(np.float32), rng.standard_normal((n, C)).astype(np.float32)
    Ms = []
    for l in range(layers):
        b = np.log1p(0.5 / (l + 1))
        Ms.append(((1 - b) * np.eye(C) + b * rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32))
    return H, H0, Ms


def cast_bf16(gnntf, X):
    return gnntf.sparse.to_bf16(X)


def call_bf16(gnntf, case, Hb, H0, M, act, out_bf16, work="own", out=None):
    """The raw entry; returns (rc, out)."""
    nat = gnntf.sparse.nat
    n, C = H0.shape
    if out is None:
        out = torch.full((n, C), float("nan"), dtype=torch.bfloat16 if out_bf16 else torch.float32, device="cuda")
    if isinstance(work, str):
        work = torch.full((n, C), float("nan"), dtype=torch.float32, device="cuda")
    rc = nat.lib().gnx_gcnii_step_bf16(case.g.handle, nat.ptr(case.adj.vals), nat.ptr(Hb), nat.ptr(H0), A_MIX, C, nat.ptr(M), M.stride(0),
                                       int(act), nat.ptr(out), 1 if out_bf16 else 0, nat.ptr(work), nat.current_stream())
    torch.cuda.synchronize()
    return rc, out


def call_f32(gnntf, case, H, H0, M, act, mixed=None):
    nat = gnntf.sparse.nat
    n, C = H0.shape
    out = torch.full((n, C), float("nan"), dtype=torch.float32, device="cuda")
    if mixed is None and C not in FUSED:
        mixed = torch.empty((n, C), dtype=torch.float32, device="cuda")
    nat.check(nat.lib().gnx_gcnii_step(case.g.handle, nat.ptr(case.adj.vals), nat.ptr(H), nat.ptr(H0), A_MIX, C, nat.ptr(M), M.stride(0),
                                       int(act), nat.ptr(out), nat.ptr(mixed), nat.current_stream()))
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def test_the_shaped_graph_has_a_long_row(gnntf, cases):
    """The hub row really exceeds the handle's long-row threshold at this size, and the hub-free graph has no such row: the bf16 SpMM
    names the chunk kernels on the one and not on the other."""
    X = dev(np.ones((N, 16), dtype=np.float32))
    with torch.no_grad():
        gnntf.spmm(cases["hub"].adj, X, storage=torch.bfloat16)
        assert "+chunks" in cases["hub"].g.last_kernel() or "+long" in cases["hub"].g.last_kernel()
        gnntf.spmm(cases["flat"].adj, X, storage=torch.bfloat16)
        assert "+chunks" not in cases["flat"].g.last_kernel() and "+long" not in cases["flat"].g.last_kernel()
    assert N % 16 != 0
    degree = np.diff(cases["hub"].A.indptr)
    assert degree.max() > 512 and (degree[3000:] == 0).all()
    flat = np.diff(cases["flat"].A.indptr)
    assert 0 < flat.max() <= 300 and (flat[3000:] == 0).all() and cases["flat"].A.nnz > 10000


GRID = [(name, C) for C in FUSED for name in ("hub", "flat", "tiny")] + [(name, C) for C in (24, 128) for name in ("hub", "tiny")]
_results = {}


def results(gnntf, cases, name, C, relu):
    """Every case once: the f32 entry over the widened rows, the bf16 entry with an f32 and with a bf16 result (twice), the names."""
    key = (name, C, relu)
    if key not in _results:
        case = cases[name]
        H, H0, (M,) = operands(case.n, C, seed=100 * C + len(name))
        act = gnntf.sparse.nat.ACT_RELU if relu else gnntf.sparse.nat.ACT_NONE
        Hb = cast_bf16(gnntf, dev(H))
        wide = Hb.float()                                   # bf16-representable f32 rows: the exact widening
        H0d, Md = dev(H0), dev(M)
        want = call_f32(gnntf, case, wide, H0d, Md, act)
        name_f32 = case.g.last_kernel()
        rc0, got0 = call_bf16(gnntf, case, Hb, H0d, Md, act, 0)
        name_bf16 = case.g.last_kernel()
        rc1, got1 = call_bf16(gnntf, case, Hb, H0d, Md, act, 1)
        name_bf16_out = case.g.last_kernel()
        rc2, got2 = call_bf16(gnntf, case, Hb, H0d, Md, act, 1)
        _results[key] = dict(rc=(rc0, rc1, rc2), want=want, got0=got0, got1=got1, got2=got2, names=(name_f32, name_bf16, name_bf16_out))
    return _results[key]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name,C", GRID)
def test_exact_against_the_f32_entry(gnntf, cases, name, C, relu):
    """Over bf16-representable H the bf16 entry with an f32 result IS the f32 entry: same gather order, same sums, the same hub path,
    the same MFMA transform -- no tolerance."""
    r = results(gnntf, cases, name, C, relu)
    assert r["rc"][0] == 0
    assert not torch.isnan(r["want"]).any() and not torch.isnan(r["got0"]).any()            # every row was written
    assert torch.equal(bits(r["got0"]), bits(r["want"]))
    assert r["names"][0] == ("spmm_gcnii_mfma" if C in FUSED else "spmm+dense_mfma")
    assert r["names"][1] == r["names"][2] == ("spmm_gcnii_mfma_bf16" if C in FUSED else "spmm+dense_mfma_bf16")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name,C", GRID)
def test_the_one_rounding_store(gnntf, cases, name, C, relu):
    """out_bf16 = 1 is gnx_cast_bf16 of the out_bf16 = 0 result, bit for bit; two calls give the same bits."""
    r = results(gnntf, cases, name, C, relu)
    assert r["rc"] == (0, 0, 0)
    assert r["got1"].dtype == torch.bfloat16 and not torch.isnan(r["got1"].float()).any()
    assert torch.equal(bits(r["got1"]), bits(cast_bf16(gnntf, r["got0"])))
    assert torch.equal(bits(r["got1"]), bits(r["got2"]))


def test_argument_rules(gnntf, cases):
    nat = gnntf.sparse.nat
    lib = nat.lib()
    H, H0, (M,) = operands(N, 64, seed=7)
    Hb, H0d, Md = cast_bf16(gnntf, dev(H)), dev(H0), dev(M)
    # NULL d_work: fine on a hub-free graph at a fused width, and the same bits as with one
    rc, without = call_bf16(gnntf, cases["flat"], Hb, H0d, Md, nat.ACT_RELU, 0, work=None)
    assert rc == 0 and cases["flat"].g.last_kernel() == "spmm_gcnii_mfma_bf16"
    assert torch.equal(bits(without), bits(call_bf16(gnntf, cases["flat"], Hb, H0d, Md, nat.ACT_RELU, 0)[1]))
    rc, _ = call_bf16(gnntf, cases["flat"], Hb, H0d, Md, nat.ACT_RELU, 1, work=None)
    assert rc == 0
    # ... refused with the hub, and at an unfused width
    rc, _ = call_bf16(gnntf, cases["hub"], Hb, H0d, Md, nat.ACT_RELU, 0, work=None)
    assert rc == -1 and b"d_work" in lib.gnx_last_error()
    H24, H024, (M24,) = operands(N, 24, seed=8)
    rc, _ = call_bf16(gnntf, cases["flat"], cast_bf16(gnntf, dev(H24)), dev(H024), dev(M24), nat.ACT_NONE, 0, work=None)
    assert rc == -1 and b"d_work" in lib.gnx_last_error()
    # d_work must be a buffer of its own
    out = torch.empty((N, 64), dtype=torch.float32, device="cuda")
    rc, _ = call_bf16(gnntf, cases["hub"], Hb, H0d, Md, nat.ACT_RELU, 0, work=out, out=out)
    assert rc == -1 and b"d_work" in lib.gnx_last_error()
    rc, _ = call_bf16(gnntf, cases["hub"], Hb, H0d, Md, nat.ACT_RELU, 0, work=H0d)
    assert rc == -1 and b"d_work" in lib.gnx_last_error()
    # a rectangular graph
    coo, vals, _ = shaped_coo(False)
    wide = types.SimpleNamespace(g=gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, (N, N + 5)), device="cuda:0"),
                                 adj=types.SimpleNamespace(vals=None))           # (raw values: d_vals = NULL)
    rc, _ = call_bf16(gnntf, wide, Hb, H0d, Md, nat.ACT_RELU, 0)
    assert rc == -1 and b"square" in lib.gnx_last_error()
    rc, _ = call_bf16(gnntf, cases["hub"], Hb, H0d, Md, 7, 0)
    assert rc == -1 and b"activation" in lib.gnx_last_error()


@pytest.mark.parametrize("out_bf16", [0, 1])
def test_rows_off_the_8_byte_rule_take_the_unfused_path(gnntf, cases, out_bf16):
    """A bf16 H whose rows start 2 bytes off: the fused launch does not apply, the SpMM + dense form does and gives the bits of the f32
    entry over the widened rows.  The f32 reference is put on ITS two-launch form the same way (rows 4 bytes off, d_mixed given): the
    fused kernel and the dense kernel feed the 16x16x4 MFMA different groups of four k, so the two forms of either entry agree to f32
    rounding only -- checked as well, against the aligned result."""
    nat = gnntf.sparse.nat
    case = cases["hub"]
    H, H0, (M,) = operands(N, 64, seed=9)
    Hb, H0d, Md = cast_bf16(gnntf, dev(H)), dev(H0), dev(M)
    off_b = torch.empty(N * 64 + 1, dtype=torch.bfloat16, device="cuda")[1:].view(N, 64)
    off_b.copy_(Hb)
    off_f = torch.empty(N * 64 + 1, dtype=torch.float32, device="cuda")[1:].view(N, 64)
    off_f.copy_(Hb.float())
    assert off_b.data_ptr() % 8 == 2 and off_f.data_ptr() % 16 == 4
    want = call_f32(gnntf, case, off_f, H0d, Md, nat.ACT_RELU, mixed=torch.empty((N, 64), dtype=torch.float32, device="cuda"))
    assert case.g.last_kernel() == "spmm+dense_mfma"
    rc, got = call_bf16(gnntf, case, off_b, H0d, Md, nat.ACT_RELU, out_bf16)
    assert rc == 0 and case.g.last_kernel() == "spmm+dense_mfma_bf16"
    assert torch.equal(bits(got), bits(cast_bf16(gnntf, want) if out_bf16 else want))
    aligned = call_f32(gnntf, case, Hb.float(), H0d, Md, nat.ACT_RELU)
    assert case.g.last_kernel() == "spmm_gcnii_mfma"
    np.testing.assert_allclose(want.cpu().numpy(), aligned.cpu().numpy(), rtol=1e-5, atol=1e-5)


# ---- a stack of layers -------------------------------------------------------------------------------------------------------------
LAYERS = 8


def stack_f64(A, H, H0, Ms, rounded):
    """The stack in float64: out_l = relu(((1-a) A X_l + a H0) M_l).  ``rounded``: the rounding points of gnx_gcnii_step_bf16
    (include/gnx.h) -- X_0 = bf(H), X_{l+1} = bf(out_l) for every layer but the last; the constants are the f32 ones the kernels use.
    Returns (result, [|out_l| of every layer])."""
    beta, alpha = float(np.float32(1.0 - A_MIX)), float(np.float32(A_MIX))
    X = bf16_round(H).astype(np.float64) if rounded else H.astype(np.float64)
    sizes = []
    for l, M in enumerate(Ms):
        out = np.maximum((beta * (A @ X) + alpha * H0.astype(np.float64)) @ M.astype(np.float64), 0.0)
        sizes.append(np.abs(out))
        X = bf16_round(out).astype(np.float64) if rounded and l < len(Ms) - 1 else out
    return X, sizes


def first_order_bound(A, H, Ms, sizes):
    """E_0 = u |H|; E_{l+1} = ((1-a) |A| E_l) |M_l| + u |out_l| for every layer that stores bf16 (all but the last); relu is 1-Lipschitz."""
    absA = abs(A)
    E = U * np.abs(H.astype(np.float64))
    for l, M in enumerate(Ms):
        E = ((1.0 - A_MIX) * (absA @ E)) @ np.abs(M.astype(np.float64))
        if l < len(Ms) - 1:
            E = E + U * sizes[l]
    return E


@pytest.mark.parametrize("C", [64, 16])
def test_stack_of_layers_within_its_bound(gnntf, cases, C, capsys):
    """8 relu layers handing bf16 rows to each other against the float64 emulation of the rounding points, and against plain float64:
    no element beyond the first-order bound + 4 x the elementwise deviation of the f32 gnx_gcnii_step stack from plain float64 (the
    parent's path; the factor covers a rounding that falls on the other side of a tie after an f32-level difference).
    Measured (MI355X): see profiles/NOTES.md, "bf16 storage in the GCNII layer"."""
    case = cases["hub"]
    H, H0, Ms = operands(N, C, seed=40 + C, layers=LAYERS)
    Hd, H0d, Md = dev(H), dev(H0), [dev(M) for M in Ms]
    with torch.no_grad():
        X = Hd
        for l in range(LAYERS):
            X = gnntf.gcnii_step(case.adj, X, H0d, A_MIX, Md[l], relu=True)
        f32_stack = X.cpu().numpy().astype(np.float64)
        X = Hd
        for l in range(LAYERS):
            X = gnntf.gcnii_step(case.adj, X, H0d, A_MIX, Md[l], relu=True, storage=torch.bfloat16,
                                 out_storage=torch.float32 if l == LAYERS - 1 else torch.bfloat16)
            assert X.dtype == (torch.float32 if l == LAYERS - 1 else torch.bfloat16)
            assert case.g.last_kernel() == "spmm_gcnii_mfma_bf16"
        got = X.cpu().numpy().astype(np.float64)
        chained = gnntf.sparse.gcnii_chain_bf16(case.adj, Hd, [(H0d, A_MIX, Md[l], True) for l in range(LAYERS)])
    assert np.array_equal(chained.cpu().numpy(), X.cpu().numpy())
    plain, sizes = stack_f64(case.A, H, H0, Ms, rounded=False)
    emulated, _ = stack_f64(case.A, H, H0, Ms, rounded=True)
    bound = first_order_bound(case.A, H, Ms, sizes) + 4.0 * np.abs(f32_stack - plain)
    rel = lambda x, y: float(np.linalg.norm(x - y) / np.linalg.norm(y))
    with capsys.disabled():
        print(f"\n[gcnii bf16 stack C={C}] rel. Frobenius: bf16 vs emulation {rel(got, emulated):.3e}, bf16 vs float64 {rel(got, plain):.3e}, "
              f"f32 vs float64 {rel(f32_stack, plain):.3e}, bound {float(np.linalg.norm(bound) / np.linalg.norm(plain)):.3e}; "
              f"max |got - emulation| / bound {float((np.abs(got - emulated) / np.maximum(bound, 1e-300)).max()):.3f}, "
              f"max |got - float64| / bound {float((np.abs(got - plain) / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (np.abs(got - emulated) <= bound).all()
    assert (np.abs(got - plain) <= bound).all()


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def build_model(gnntf, dtype):
    coo, vals, shape = shaped_coo(True)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N, 20)).astype(np.float32)
    gnntf.set_seed(3)
    torch.manual_seed(3)
    model = gnntf.GCNII(gnntf.SparseCOO(coo, vals, shape), X, 7, iterations=LAYERS, inference_dtype=dtype)
    model.reset()
    convs = [l for l in model.layers() if isinstance(l, gnntf.GCNIILayer)]
    for l in convs:                       # the reference initialises W to zero: use seeded weights
        l.W.data.copy_(dev((rng.standard_normal((64, 64)) / 8).astype(np.float32)))
    model.training_mode(False)
    return model, convs


def test_model_runs_the_bf16_chain(gnntf, capsys):
    model, convs = build_model(gnntf, torch.bfloat16)
    plain_model, plain_convs = build_model(gnntf, torch.float32)
    for a_, b_ in zip(model.vars(), plain_model.vars()):
        assert torch.equal(a_.var, b_.var)
    assert len(convs) == LAYERS
    sparse = gnntf.sparse
    with torch.no_grad():
        out = model(model.features)
        assert model.graph.last_kernel() == "spmm_gcnii_mfma_bf16"
        H0 = convs[0].H0.value
        adj = model.get_adjacency(0)
        # the hand-chained calls: input cast once, bf16 between the layers, f32 out of the last
        X = sparse.to_bf16(H0)
        inner = []
        for k, layer in enumerate(convs):
            last = k == LAYERS - 1
            X = sparse.gcnii_step(adj, X, H0, layer.a, layer._transform(), relu=True, storage=torch.bfloat16,
                                  out_storage=torch.float32 if last else torch.bfloat16)
            inner.append(X)
        assert torch.equal(convs[-1].value, inner[-1]) and convs[-1].value.dtype == torch.float32
        tail = model.layers()[-1]
        assert torch.equal(out, tail(model, inner[-1]))
        # an inner layer's value: f32, the exact widening of its bf16 rows, made when somebody reads it
        assert convs[3].__dict__.get("_pending_value") is not None
        v = convs[3].value
        assert v.dtype == torch.float32 and torch.equal(v, inner[3].float()) and convs[3].__dict__.get("_pending_value") is None
        assert torch.equal(convs[0].value, inner[0].float())
        # the default inference_dtype: the f32 chain, the parent's bits
        plain_out = plain_model(plain_model.features)
        assert plain_model.graph.last_kernel() == "spmm_gcnii_mfma"
        X = plain_convs[0].H0.value
        assert torch.equal(X, H0)
        for layer in plain_convs:
            X = sparse.gcnii_step(adj, X, H0, layer.a, layer._transform(), relu=True)
            assert torch.equal(layer.value, X)
        assert torch.equal(plain_out, plain_model.layers()[-1](plain_model, X))
        changed = int((out.argmax(1) != plain_out.argmax(1)).sum())
    with capsys.disabled():
        print(f"\n[gcnii bf16 model] predictions that change with inference_dtype=bfloat16: {changed} of {N}; "
              f"rel. Frobenius of the logits {float(torch.linalg.norm(out - plain_out) / torch.linalg.norm(plain_out)):.3e}")
    # with grad enabled (eval mode) the bf16 model runs the f32 path: the default model's bits
    graded = model(model.features)
    assert model.graph.last_kernel() == "spmm_gcnii_mfma" and graded.requires_grad
    assert torch.equal(graded.detach(), plain_out)
    # ... and in training mode, with or without grad
    with model:
        with torch.no_grad():
            model(model.features)
        assert model.graph.last_kernel() == "spmm_gcnii_mfma"
        model(model.features)
        assert model.graph.last_kernel() == "spmm_gcnii_mfma"
    # a layer the chain does not take keeps f32: the spectral-preserving variant
    coo, vals, shape = shaped_coo(True)
    other = gnntf.GCNII(gnntf.SparseCOO(coo, vals, shape), np.zeros((N, 20), dtype=np.float32), 7, iterations=2,
                        layer_type=gnntf.GCNIISpectralPreservingLayer, inference_dtype=torch.bfloat16)
    other.reset()
    other.training_mode(False)
    with torch.no_grad():
        other(other.features)
    assert "bf16" not in other.graph.last_kernel()
