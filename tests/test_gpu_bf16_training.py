"""Opt-in bf16 feature storage of the fused TRAINING propagation on the MI355X (gnx_spmm_dropped_chained_bf16,
gnx_spmm_dropped_back_bf16, sparse.ppr_loop(storage=bf16), GNN(training_dtype=bf16)) against the float64 emulation of
tests/bf16_train_ref.py -- the oracle's masks, kept sums and degree scales plus bf() at the library's rounding points."""
import numpy as np
import pytest
import torch

import bf16_train_ref as ref
import graphs
from oracle import gnntf_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-3           # relative Frobenius error against the emulation: f32-vs-f64 summation and the rare bf16 rounding flip
                     # (the figure of test_gpu_bf16.py::test_k_loop_against_emulation_and_f32 for the same kind of comparison)
A = 0.1
SEED, FIRST = 0x5EED1234, 11


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def make_graph(gnntf, coo, vals, shape):
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    if g.nnz_entries != g.nnz:
        g.enable_entry_dropout()
    return g


def _plain():
    return graphs.rmat_symmetric_coo(1500, 12000, seed=3)


def _doubled():
    coo, _, _ = _plain()
    return orc.graph2adj(range(1500), [tuple(e) for e in coo])            # the reference's own input: every entry twice


def _unequal():
    return graphs.random_coo(1200, 1200, 16000, seed=5, weighted=True, dup_frac=0.3)   # duplicates with unequal (positive) values


GRAPHS = {"plain": _plain, "doubled": _doubled, "unequal": _unequal}


@pytest.fixture(scope="module")
def prepared(gnntf):
    out = {}
    for name, build in GRAPHS.items():
        coo, vals, shape = build()
        out[name] = (np.asarray(coo), np.asarray(vals, dtype=np.float32), shape, make_graph(gnntf, coo, vals, shape))
    assert out["plain"][3].nnz_entries == out["plain"][3].nnz and out["doubled"][3].nnz_entries == 2 * out["doubled"][3].nnz
    return out


_mats = {}


def mats_of(name, coo, vals, shape, p, K):
    key = (name, p, K)
    if key not in _mats:
        _mats[key] = ref.dropped_matrices(coo, vals, shape, p, SEED, FIRST, K)
    return _mats[key]


def adjacencies(sparse, g, p, K):
    D = sparse.dropped_degree_scales(g, p, SEED, FIRST, K)
    return [sparse.DroppedAdjacency(g, p, SEED, FIRST + k, D=D[k]) for k in range(K)]


def expected_class(C):
    """The dispatch class of contiguous [n, C] buffers: up to 8 bf16 per lane, one wave per row above 32 lanes."""
    vec = next(v for v in (8, 4, 2, 1) if C % v == 0)
    lanes = (C + vec - 1) // vec
    return "wave" if lanes > 32 else "group32" if lanes > 16 else "group16" if lanes > 8 else "group8"


def bf16_step(sparse, adjs, H0, G):
    """Forward and backward through the private loops (whatever BF16_TRAIN_MIN_WIDTH says), and the kernel names they report."""
    g = adjs[0].graph
    H = sparse._forward_chained_bf16(adjs, H0, A)
    fwd_name = g.last_kernel()
    dH0 = sparse._backward_chained_bf16(adjs, G, A)
    return H, dH0, fwd_name, g.last_kernel()


def f32_step(sparse, adjs, H0, G):
    """The f32 training step through the public loop (the default path)."""
    H0 = H0.clone().requires_grad_(True)
    H = sparse.ppr_loop(lambda k, bwd=False: adjs[k], H0, A, len(adjs))
    H.backward(G)
    return H.detach(), H0.grad


def check_case(sparse, name, coo, vals, shape, g, C, K, p, capsys=None):
    rng = np.random.default_rng(1000 * C + K)
    H0 = rng.standard_normal((shape[0], C)).astype(np.float32)
    G = rng.standard_normal((shape[0], C)).astype(np.float32)
    adjs = adjacencies(sparse, g, p, K)
    H, dH0, fwd_name, bwd_name = bf16_step(sparse, adjs, dev(H0), dev(G))
    H2, dH02, _, _ = bf16_step(sparse, adjs, dev(H0), dev(G))
    assert torch.equal(H, H2) and torch.equal(dH0, dH02)                       # two runs give equal bits
    tail = "_entries_bf16" if g.nnz_entries != g.nnz else "_drop_bf16"
    for kernel in (fwd_name, bwd_name):
        assert kernel.endswith(tail) and expected_class(C) in kernel, (kernel, C)
    mats = mats_of(name, coo, vals, shape, p, K)
    emu_f, emu_b = ref.forward(mats, H0, A), ref.backward(mats, G, A)
    err_f, err_b = ref.rel_fro(H.cpu().numpy(), emu_f), ref.rel_fro(dH0.cpu().numpy(), emu_b)
    # distance from the f32 step, the yardstick made from the emulation on the CPU
    H32, dH032 = f32_step(sparse, adjs, dev(H0), dev(G))
    orc_f = ref.oracle_forward(coo, vals, shape, H0, A, K, p, SEED, FIRST)
    orc_b = ref.oracle_backward(coo, vals, shape, G, A, K, p, SEED, FIRST)
    dist_f = float(np.linalg.norm(H.cpu().numpy().astype(np.float64) - H32.cpu().numpy()))
    dist_b = float(np.linalg.norm(dH0.cpu().numpy().astype(np.float64) - dH032.cpu().numpy()))
    yard_f, yard_b = float(np.linalg.norm(emu_f - orc_f)), float(np.linalg.norm(emu_b - orc_b))
    print(f"{name} C={C} K={K} p={p}: err fwd {err_f:.2e} bwd {err_b:.2e}; |bf16-f32| fwd {dist_f:.3e} (emulation {yard_f:.3e}) "
          f"bwd {dist_b:.3e} (emulation {yard_b:.3e}); {fwd_name}")
    assert err_f <= TOL and err_b <= TOL
    assert dist_f <= 2.0 * yard_f and dist_b <= 2.0 * yard_b
    assert dist_f > 0 and dist_b > 0                                             # bf16 did run


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("C", [7, 8, 40, 64, 128, 256])
def test_loops_against_emulation_and_f32(gnntf, prepared, name, C):
    """Forward and backward loops against the emulation (relative Frobenius error <= 1e-3), equal bits on a second run, the kernel
    names, and the distance from the f32 step: ||bf16 - f32||_F of H_K and of dH0 at most 2 x the distance between the emulation
    and the f32 oracle (float64, no rounding), both computed here on the CPU -- the factor 2 covers the f32 roundings on both
    sides.  No closed-form bound is asserted: the dropped A_k are not symmetric (the two directions of an edge draw separate
    masks), so the u / a bound of the eval-mode loop does not carry over."""
    from gnntf import sparse
    coo, vals, shape, g = prepared[name]
    for K in (1, 2, 10):
        for p in (0.5, 0.1):
            check_case(sparse, name, coo, vals, shape, g, C, K, p)


@pytest.mark.parametrize("C", [100, 260, 520])
def test_wave_and_unaligned_widths(gnntf, prepared, C):
    """Widths beyond the issue's list that reach the remaining dispatch classes: 4 values per lane (100), one wave per row (260),
    and rows of more than one tile (520)."""
    from gnntf import sparse
    for name in ("plain", "unequal"):
        coo, vals, shape, g = prepared[name]
        check_case(sparse, name, coo, vals, shape, g, C, 2, 0.5)


def test_no_dropout_through_the_private_helpers(gnntf, prepared):
    """p = 0 (can_fuse_dropout refuses it, so the public loop never gets here): every entry is kept."""
    from gnntf import sparse
    for name in ("plain", "doubled"):
        coo, vals, shape, g = prepared[name]
        check_case(sparse, name, coo, vals, shape, g, 64, 2, 0.0)


def hub_coo(n, m, seed, hubs):
    coo, _, shape = graphs.rmat_symmetric_coo(n, m, seed=seed)
    rng = np.random.default_rng(seed + 1)
    extra = []
    for i, h in enumerate(hubs):
        nb = rng.choice(np.arange(len(hubs), n), size=h, replace=False)
        extra += [np.stack([np.full(h, i), nb], 1), np.stack([nb, np.full(h, i)], 1)]
    coo = np.unique(np.concatenate([coo] + extra), axis=0).astype(np.int64)
    return coo, np.ones(len(coo), dtype=np.float32), shape


@pytest.mark.parametrize("regime", ["40k", "40k_doubled", "1M"])
def test_size_regimes(gnntf, regime):
    """40 000 vertices with hub rows above 128 and above 512 entries -- also with every entry stored twice and a share a third time
    with another value (the _entries instantiations over long rows) -- and 2^20 vertices / 4M entries (rows padded to the bf16
    line-friendly width there): the long rows run through the chunk kernels (the name contains "+long"); K = 2 against the
    emulation.  Widths: 8-, 16- and 32-lane groups (8 / 64, 128, 256) and one wave per chunk (520) on the 40k graphs.  At 2^20
    vertices -- inside the allowance -- the public loop runs the same bits without being forced."""
    from gnntf import sparse
    if regime.startswith("40k"):
        coo, vals, shape = hub_coo(40000, 150000, 21, hubs=(200, 400, 700, 1500))
        widths = (8, 64, 128, 256, 520)
        if regime == "40k_doubled":
            third = np.arange(0, len(coo), 5)
            coo, vals = np.concatenate([coo, coo, coo[third]]), np.concatenate([vals, vals, vals[third] * np.float32(0.5)])
            widths = (8, 128, 256, 520)
    else:
        coo, vals, shape = graphs.rmat_symmetric_coo(1 << 20, 2_000_000, seed=22)
        widths = (8, 128)
    g = make_graph(gnntf, coo, vals, shape)
    tail = "_drop_entries_bf16" if regime == "40k_doubled" else "_drop_bf16"
    assert (g.nnz_entries != g.nnz) == (regime == "40k_doubled")
    deg = np.bincount(np.unique(coo, axis=0)[:, 0], minlength=shape[0])
    assert deg.max() > 512 and ((deg > 128) & (deg <= 512)).any()
    K, p = 2, 0.5
    mats = ref.dropped_matrices(coo, vals, shape, p, SEED, FIRST, K)
    adjs = adjacencies(sparse, g, p, K)
    for C in widths:
        assert sparse.friendly_width_bf16(C, shape[0]) == C
        rng = np.random.default_rng(C)
        H0 = rng.standard_normal((shape[0], C)).astype(np.float32)
        G = rng.standard_normal((shape[0], C)).astype(np.float32)
        H, dH0, fwd_name, bwd_name = bf16_step(sparse, adjs, dev(H0), dev(G))
        H2, dH02, _, _ = bf16_step(sparse, adjs, dev(H0), dev(G))
        assert torch.equal(H, H2) and torch.equal(dH0, dH02)
        for kernel in (fwd_name, bwd_name):
            assert "+long" in kernel and kernel.endswith(tail) and expected_class(C) in kernel, (fwd_name, bwd_name)
        err_f = ref.rel_fro(H.cpu().numpy(), ref.forward(mats, H0, A))
        err_b = ref.rel_fro(dH0.cpu().numpy(), ref.backward(mats, G, A))
        print(f"{regime} C={C}: err fwd {err_f:.2e} bwd {err_b:.2e}; {fwd_name} / {bwd_name}")
        assert err_f <= TOL and err_b <= TOL
        if C >= sparse.BF16_TRAIN_MIN_WIDTH and shape[0] >= sparse.BF16_TRAIN_MIN_ROWS:
            Hr = dev(H0).requires_grad_(True)
            out = sparse.ppr_loop(lambda k, bwd=False: adjs[k], Hr, A, K, storage=torch.bfloat16)
            out.backward(dev(G))
            assert torch.equal(out.detach(), H) and torch.equal(Hr.grad, dH0) and g.last_kernel().endswith(tail)


def test_public_loop_allowance_and_fallbacks(gnntf, prepared, monkeypatch):
    """ppr_loop(storage=bf16): f32 bits -- the default's -- on a graph below BF16_TRAIN_MIN_ROWS; with that row threshold lifted
    (the test graphs are small) the bits of the private loops from BF16_TRAIN_MIN_WIDTH on, and f32 bits below it, with relu, and
    on an adjacency that is no DroppedAdjacency."""
    from gnntf import sparse
    coo, vals, shape, g = prepared["doubled"]
    K, p = 3, 0.5
    adjs = adjacencies(sparse, g, p, K)
    make = lambda k, bwd=False: adjs[k]

    def run(C, **kw):
        rng = np.random.default_rng(C)
        H0 = dev(rng.standard_normal((shape[0], C)).astype(np.float32)).requires_grad_(True)
        G = dev(rng.standard_normal((shape[0], C)).astype(np.float32))
        H = sparse.ppr_loop(kw.pop("make", make), H0, A, K, **kw)
        name = g.last_kernel()
        H.backward(G)
        return H.detach(), H0.grad, name, g.last_kernel(), H0.detach(), G

    wide = max(40, sparse.BF16_TRAIN_MIN_WIDTH)
    if shape[0] < sparse.BF16_TRAIN_MIN_ROWS:
        got, ref32 = run(wide, storage=torch.bfloat16), run(wide)
        assert torch.equal(got[0], ref32[0]) and torch.equal(got[1], ref32[1]) and "bf16" not in got[2] + got[3]
    monkeypatch.setattr(sparse, "BF16_TRAIN_MIN_ROWS", 0)
    H, dH0, n1, n2, H0, G = run(wide, storage=torch.bfloat16)
    assert n1.endswith("_entries_bf16") and n2.endswith("_entries_bf16")
    Hp, dH0p, _, _ = bf16_step(sparse, adjs, H0, G)
    assert torch.equal(H, Hp) and torch.equal(dH0, dH0p)
    if sparse.BF16_TRAIN_MIN_WIDTH > 1:
        narrow = sparse.BF16_TRAIN_MIN_WIDTH - 1
        got, ref32 = run(narrow, storage=torch.bfloat16), run(narrow)
        assert torch.equal(got[0], ref32[0]) and torch.equal(got[1], ref32[1]) and "bf16" not in got[2] + got[3]
    got, ref32 = run(wide, storage=torch.bfloat16, relu=True), run(wide, relu=True)
    assert torch.equal(got[0], ref32[0]) and torch.equal(got[1], ref32[1]) and "bf16" not in got[2] + got[3]
    mat = [sparse.normalize(g, "symmetric", "none", p, SEED, FIRST + k) for k in range(K)]
    mk = lambda k, bwd=False: mat[k]
    got, ref32 = run(wide, storage=torch.bfloat16, make=mk), run(wide, make=mk)
    assert torch.equal(got[0], ref32[0]) and torch.equal(got[1], ref32[1]) and "bf16" not in got[2] + got[3]


def test_refused_handles(gnntf):
    """A vertex block and a duplicate handle without its entry tables: GNX_ERR_UNSUPPORTED (-4) from both entries, with a message."""
    from gnntf import _native as nat
    lib, s = nat.lib(), nat.current_stream()
    D = torch.ones(64, device="cuda")
    Xb = torch.zeros((64, 16), dtype=torch.bfloat16, device="cuda")
    Yb = torch.zeros((64, 16), dtype=torch.bfloat16, device="cuda")
    S = torch.zeros((64, 16), device="cuda")
    out = torch.zeros((64, 16), device="cuda")

    def both(handle):
        rc1 = lib.gnx_spmm_dropped_chained_bf16(handle, nat.ptr(D), 0.5, 1, 1, 0, None, nat.ptr(Xb), 16, 16, nat.ptr(S), 16, 0.9, 0.1, 0,
                                                nat.ptr(out), 0, 16, s)
        m1 = lib.gnx_last_error()
        rc2 = lib.gnx_spmm_dropped_back_bf16(handle, nat.ptr(D), 0.5, 1, 1, 0, nat.ptr(D), nat.ptr(Xb), 16, 16, nat.ptr(S), 16, 1.0, 0.09,
                                             nat.ptr(S), 16, 0.9, nat.ptr(Yb), 16, 0, s)
        return rc1, m1, rc2, lib.gnx_last_error()

    coo, vals, shape = graphs.random_coo(20, 30, 80, seed=1, dup_frac=0.0)
    coo = np.unique(coo, axis=0)
    rect = gnntf.DeviceGraph(gnntf.SparseCOO(coo, np.ones(len(coo), dtype=np.float32), shape), device="cuda:0")
    gid = torch.arange(30, dtype=torch.int32, device="cuda")
    assert lib.gnx_graph_set_block(rect.handle, 100, 5, nat.ptr(gid), s) == 0
    rc1, m1, rc2, m2 = both(rect.handle)
    assert rc1 == rc2 == -4 and b"vertex block" in m1 and b"vertex block" in m2
    coo, vals, shape = graphs.random_coo(64, 64, 400, seed=2, dup_frac=0.3)
    dup = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    assert dup.nnz_entries > dup.nnz and not dup.entry_dropout
    rc1, m1, rc2, m2 = both(dup.handle)
    assert rc1 == rc2 == -4 and b"gnx_graph_enable_entry_dropout" in m1 and b"gnx_graph_enable_entry_dropout" in m2
    square = gnntf.DeviceGraph(gnntf.SparseCOO(np.unique(coo, axis=0), np.ones(len(np.unique(coo, axis=0)), dtype=np.float32), shape),
                               device="cuda:0")
    rc1, _, rc2, _ = both(square.handle)
    assert rc1 == rc2 == 0                                                       # the same calls on a plain square handle run
    torch.cuda.synchronize()


# ---- the model level --------------------------------------------------------------------------------------------------------
def _model_step(gnntf, fused, classes, record=None, **kw):
    from gnntf import sparse
    from gnntf.training import _Objective
    n, F = 600, 40
    coo, vals, shape = graphs.rmat_symmetric_coo(n, 4000, seed=3)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, F)).astype(np.float32)
    labels = rng.integers(0, classes, size=n)
    task = gnntf.NodeClassification(np.arange(200), labels[:200])
    gnntf.set_seed(17)
    model = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=classes, latent_dims=[16], fused=fused, **kw)
    model.reset()
    params = [v.var for v in model.vars() if v.trainable]
    names = []
    orig = sparse.ppr_loop

    def spy(make_adj, H0, a, iterations, relu=False, storage=torch.float32):
        out = orig(make_adj, H0, a, iterations, relu=relu, storage=storage)
        names.append(model.graph.last_kernel())
        if record is not None:
            record.update(H0_live=H0, H0=H0.detach().clone(), out=out.detach().clone(), adjs=[make_adj(k, False) for k in range(iterations)], a=a)
            if H0.requires_grad:
                H0.register_hook(lambda gr: record.__setitem__("dH0", gr.detach().clone()))
                out.register_hook(lambda gr: record.__setitem__("g", gr.detach().clone()))
        return out

    sparse.ppr_loop = spy
    try:
        with model:
            loss = _Objective(model, task, 5e-4)()
            loss.backward(retain_graph=record is not None)
    finally:
        sparse.ppr_loop = orig
    names.append(model.graph.last_kernel())
    if record is not None:
        # v -> (d H0 / d theta)^T v for every parameter: the head and the MLP in front of the propagation (no bf16 in them)
        live = record.pop("H0_live")
        record["push"] = lambda v: [torch.zeros_like(p) if gr is None else gr for p, gr in
                                    zip(params, torch.autograd.grad(live, params, grad_outputs=v, retain_graph=True, allow_unused=True))]
        record["train_rows"], record["labels"] = np.arange(200), labels[:200]
    return [loss.detach().clone()] + [p.grad.clone() for p in params], names, (coo, vals, shape)


def _cross_entropy64(logits, rows, labels):
    z = np.asarray(logits, dtype=np.float64)[rows]
    z = z - z.max(axis=1, keepdims=True)
    return float(np.mean(np.log(np.exp(z).sum(axis=1)) - z[np.arange(len(rows)), labels]))


@pytest.mark.parametrize("fused", [False, True])
def test_model_training_step(gnntf, fused, monkeypatch):
    """APPNP(training_dtype=bf16) on the 600-vertex model of test_gpu_bf16.py::test_training_step_is_untouched, with as many classes
    as the width allowance needs and the row threshold lifted (the model is far below it; with the threshold in place the step is
    bitwise the f32 one, checked first): one _Objective step runs, the bf16 kernels ran, loss and every gradient are finite.
    Compared at the boundary of the propagation (hooks on ppr_loop's H0 and result; H0 is bitwise the same in both steps: same
    seeds, same weights):
      - H_K and dH0 are the emulation's for the recorded H0 and the recorded upstream gradient (<= 1e-3);
      - ||H_K bf16 - H_K f32||_F <= 2 ||emulation(H0) - oracle(H0)||_F, and ||dH0 bf16 - dH0 f32||_F <= 2 ||emulation backward of
        the bf16 step's upstream gradient - oracle backward of the f32 step's||_F (the two upstream gradients differ because the
        two H_K do);
      - every parameter gradient: the parameters reach the loss through H0 alone (plus a regulariser that is the same in both
        steps), so their gradients differ by J^T (dH0 bf16 - dH0 f32) with J = d H0 / d theta, the Jacobian of the MLP and the head.
        The yardstick is J^T applied to the emulation-derived dH0 difference above (float64 on the CPU); J^T itself is applied by
        autograd through the step's own MLP graph -- a linear map both steps share, with no bf16 in it, whose f32 rounding (1e-6)
        is far inside the factor 2;
      - the loss: |loss bf16 - loss f32| <= 2 x |float64 cross entropy of the emulation's H_K - that of the oracle's H_K| over the
        training rows (the regulariser is the same in both steps), plus the f32 rounding of a loss of that size (2^-20 relative).
    With the default training_dtype the step is bitwise the torch.float32 one and no _bf16 kernel runs."""
    from gnntf import sparse
    classes = max(5, sparse.BF16_TRAIN_MIN_WIDTH)
    if sparse.BF16_TRAIN_MIN_ROWS > 600:
        kept16, names, _ = _model_step(gnntf, fused, classes, training_dtype=torch.bfloat16)
        kept32, _, _ = _model_step(gnntf, fused, classes)
        assert not any("bf16" in n for n in names) and all(torch.equal(x, y) for x, y in zip(kept16, kept32))
    monkeypatch.setattr(sparse, "BF16_TRAIN_MIN_ROWS", 0)
    rec16, rec32 = {}, {}
    res16, names16, (coo, vals, shape) = _model_step(gnntf, fused, classes, rec16, training_dtype=torch.bfloat16)
    res32, names32, _ = _model_step(gnntf, fused, classes, rec32, training_dtype=torch.float32)
    res_default, names_default, _ = _model_step(gnntf, fused, classes)
    assert all(n.endswith("_drop_bf16") for n in names16), names16
    assert not any("bf16" in n for n in names32 + names_default)
    assert len(res16) == len(res32) == len(res_default) > 1
    for x, y in zip(res32, res_default):
        assert torch.equal(x, y)
    assert all(torch.isfinite(t).all() for t in res16)
    assert torch.equal(rec16["H0"], rec32["H0"])
    adjs = rec16["adjs"]
    K, p, seed, first, a = len(adjs), adjs[0].p, adjs[0].seed, adjs[0].stream_id, rec16["a"]
    mats = ref.dropped_matrices(coo, vals, shape, p, seed, first, K)
    H0 = rec16["H0"].cpu().numpy()
    g16, g32 = rec16["g"].cpu().numpy(), rec32["g"].cpu().numpy()
    emu_f, emu_b = ref.forward(mats, H0, a), ref.backward(mats, g16, a)
    orc_f = ref.oracle_forward(coo, vals, shape, H0, a, K, p, seed, first)
    orc_b = ref.oracle_backward(coo, vals, shape, g32, a, K, p, seed, first)
    err_f, err_b = ref.rel_fro(rec16["out"].cpu().numpy(), emu_f), ref.rel_fro(rec16["dH0"].cpu().numpy(), emu_b)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    dist_f, yard_f = float(np.linalg.norm(f64(rec16["out"]) - f64(rec32["out"]))), float(np.linalg.norm(emu_f - orc_f))
    dist_b, yard_b = float(np.linalg.norm(f64(rec16["dH0"]) - f64(rec32["dH0"]))), float(np.linalg.norm(emu_b - orc_b))
    print(f"fused={fused}: boundary err fwd {err_f:.2e} bwd {err_b:.2e}; |H_K bf16 - f32| {dist_f:.3e} (emulation {yard_f:.3e}); "
          f"|dH0 bf16 - f32| {dist_b:.3e} (emulation {yard_b:.3e})")
    assert err_f <= TOL and err_b <= TOL
    assert 0 < dist_f <= 2.0 * yard_f and 0 < dist_b <= 2.0 * yard_b
    # every parameter gradient against J^T of the emulation-derived dH0 difference
    pushed = rec16["push"](dev((emu_b - orc_b).astype(np.float32)))
    for i, (g_bf, g_f32, yard) in enumerate(zip(res16[1:], res32[1:], pushed)):
        dist, bound = float(np.linalg.norm(f64(g_bf) - f64(g_f32))), float(np.linalg.norm(f64(yard)))
        print(f"  parameter {i} {tuple(g_bf.shape)}: |grad bf16 - f32| {dist:.3e} (emulation-derived {bound:.3e})")
        assert dist <= 2.0 * bound
    # the loss
    rows, labels = rec16["train_rows"], rec16["labels"]
    d_loss = abs(_cross_entropy64(emu_f, rows, labels) - _cross_entropy64(orc_f, rows, labels))
    got = abs(float(res16[0]) - float(res32[0]))
    print(f"  loss {float(res16[0]):.7f} vs {float(res32[0]):.7f}: |difference| {got:.3e} (emulation-derived {d_loss:.3e})")
    assert got <= 2.0 * d_loss + 2.0 ** -20 * abs(float(res32[0]))
    # a narrow head stays f32 when the allowance says so
    if sparse.BF16_TRAIN_MIN_WIDTH > 5:
        narrow16, names, _ = _model_step(gnntf, fused, 5, training_dtype=torch.bfloat16)
        narrow32, _, _ = _model_step(gnntf, fused, 5)
        assert not any("bf16" in n for n in names) and all(torch.equal(x, y) for x, y in zip(narrow16, narrow32))


def test_captured_training_replays(gnntf, monkeypatch):
    """train(capture=True) with training_dtype=bf16 on the Cora-shaped model: 3 epochs, bit for bit the eager run (same seeds, the
    dropout counter advancing the streams per replay).  Both runs are given the optimizer the captured run builds for itself
    (Adam, capturable=True): the default eager Adam keeps its step count on the host and rounds the bias correction differently
    (7e-8 after 3 epochs, measured here; test_gpu_training.py compares the two at rtol 2e-3 for that reason), which is the
    optimizer's doing and says nothing about the propagation."""
    from gnntf import sparse
    monkeypatch.setattr(sparse, "BF16_TRAIN_MIN_ROWS", 0)       # the Cora-shaped graph is below the row threshold: lifted here
    coo, vals, shape, X = graphs.cora_shaped(seed=4)
    classes = max(7, sparse.BF16_TRAIN_MIN_WIDTH)
    labels = np.random.default_rng(4).integers(0, classes, size=shape[0])
    train, valid = np.arange(0, 300), np.arange(300, 600)
    results = []
    for capture in (False, True):
        gnntf.set_seed(11)
        torch.manual_seed(3)
        model = gnntf.GNN(gnntf.SparseCOO(coo, vals, shape), X, training_dtype=torch.bfloat16)
        model.add(gnntf.Dense(16, activation=gnntf.relu))                       # no feature dropout: torch's generator stays out of it
        H0 = model.add(gnntf.Dense(classes, regularize=False))
        for _ in range(4):
            model.add(gnntf.PPRIteration(H0, 0.1, graph_dropout=0.5))
        torch.manual_seed(5)
        calls, orig = [], sparse._forward_chained_bf16

        def spy(adjs, H0_, a_):
            out = orig(adjs, H0_, a_)
            calls.append(adjs[0].graph.last_kernel())
            return out

        sparse._forward_chained_bf16 = spy
        try:
            model.train(train=gnntf.NodeClassification(train, labels[train]), valid=gnntf.NodeClassification(valid, labels[valid]),
                        epochs=3, patience=50, capture=capture,
                        optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
        finally:
            sparse._forward_chained_bf16 = orig
        assert calls and all(name.endswith("_bf16") for name in calls), calls      # the bf16 training kernels ran
        results.append([v.var.detach().clone() for v in model.vars()] + [model._mask_calls])
    assert results[0][-1] == results[1][-1] == 3 * 4
    diffs = [float((e - c).abs().max()) for e, c in zip(results[0][:-1], results[1][:-1])]
    print("captured vs eager, max |difference| per variable:", diffs)
    for eager, captured in zip(results[0][:-1], results[1][:-1]):
        assert torch.equal(eager, captured)
