"""bf16 row storage for GCNII training on the MI355X (gnx_gcnii_step_train_bf16, gnx_feature_dropout_back_bf16,
gnx_gcnii_step_back_bf16, sparse.gcnii_train_run_bf16, GCNII(gcnii_training_dtype=torch.bfloat16)).  Over bf16-representable operands
the three entries give the bits of their f32 namesakes, so those comparisons are exact; the run is the composition of its pieces bit
for bit; against the float64 emulation of tests/gcnii_bf16_train_ref.py it stays within the tolerance and the yardstick rule of
tests/test_gpu_bf16_training.py; the model takes the path only where GNN.__init__ says so."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcnii_bf16_train_ref as ref
import graphs
from bf16_ref import bf16_round
from oracle import gnntf_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-3           # relative Frobenius error against the emulation (tests/test_gpu_bf16_training.py: f32 against f64 sums and the rare
                     # bf16 rounding flip)
A_MIX = 0.1
N, HUB, N_HUB = 3000, 1500, 900
WIDTHS = (16, 32, 64)
RATES = (0.0, 0.25, 0.6)
SEED, STREAM = 7, 2
FWD, BACK = "spmm_gcnii_mfma_train_bf16", "spmm_gcnii_back_mfma_bf16"
INVALID, UNSUPPORTED = -1, -4


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


def directed_coo():
    """The graph of tests/test_gpu_gcnii_back.py: DIRECTED, 3 000 vertices, about 20 000 entries, no duplicates; sources below 2 900
    and targets from 100 up; column 1 500 holds 900 entries."""
    rng = np.random.default_rng(11)
    src, dst = rng.integers(0, N - 100, size=19100), rng.integers(100, N, size=19100)
    hub_src = rng.permutation(N - 100)[:N_HUB]
    key = np.unique(np.concatenate([src * N + dst, hub_src * N + HUB]))
    coo = np.stack([key // N, key % N], axis=1).astype(np.int64)
    coo = coo[rng.permutation(len(coo))]
    vals = rng.uniform(0.5, 1.5, size=len(coo)).astype(np.float32)
    return coo, vals, (N, N)


@pytest.fixture(scope="module")
def shared(gnntf):
    """Both orientations, made once and never changed: ``a`` = the graph itself (no hub row in its forward structure, 100 rows without
    entries at the end; its TRANSPOSED structure -- what the backward walks -- has the hub row and 100 empty rows at the start) and
    ``t`` = its transpose (the reverse).  Per orientation the handle, the normalised adjacency, the same adjacency in float64, and the
    hub / empty rows of the forward (``hub``, ``empty``) and of the transposed structure (``hub_t``, ``empty_t``)."""
    coo, vals, shape = directed_coo()
    out = dict()
    for name, idx in (("a", coo), ("t", coo[:, ::-1].copy())):
        g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, vals, shape), device="cuda:0")
        deg = np.diff(host(g.csr_arrays()[0]))
        ai, av = orc.get_adjacency(idx, vals, shape, dtype=np.float64)
        A = sp.csr_matrix((av, (ai[:, 0], ai[:, 1])), shape=shape)
        out[name] = dict(g=g, adj=gnntf.normalize(g, "symmetric"), A=A, hub=np.flatnonzero(deg > 512), empty=np.flatnonzero(deg == 0))
    for name, other in (("a", "t"), ("t", "a")):
        out[name]["hub_t"], out[name]["empty_t"] = out[other]["hub"], out[other]["empty"]
    assert 19000 < len(coo) < 21000 and N % 16 != 0
    assert HUB in out["t"]["hub"] and len(out["a"]["hub"]) == 0 and len(out["t"]["empty"]) >= 100 and len(out["a"]["empty"]) >= 100
    return out


@functools.lru_cache(maxsize=None)
def keep_mask(seed, stream, p, n, C):
    """The mask in numpy, from the oracle's integers: kept iff hash_u24(seed, stream, row, col, 0) >= dropout_threshold(p)."""
    rows, cols = np.repeat(np.arange(n), C), np.tile(np.arange(C), n)
    keep = (orc.hash_u24(seed, stream, rows, cols, np.zeros(n * C, dtype=np.int64)) >= orc.dropout_threshold(p)).reshape(n, C)
    keep.setflags(write=False)
    return keep


def scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


@functools.lru_cache(maxsize=None)
def operands(C):
    """H and an upstream gradient, both bf16-representable; two H0, a running sum and four transforms."""
    rng = np.random.default_rng(C)
    H, up = (bf16_round(rng.standard_normal((N, C)).astype(np.float32)) for _ in range(2))
    H0, H0b = (rng.standard_normal((N, C)).astype(np.float32) for _ in range(2))
    Ms = tuple((0.6 * np.eye(C) + 0.4 * rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32) for _ in range(4))
    S_in = rng.standard_normal((N, C)).astype(np.float32)
    for x in (H, up, S_in, H0, H0b) + Ms:
        x.setflags(write=False)
    return dict(H=H, up=up, S_in=S_in, H0=H0, H0b=H0b, Ms=Ms)


def triple(p, stream=STREAM):
    return (p, SEED, stream) if p > 0 else None


# ---- 1. the forward over bf16-representable H -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("C", WIDTHS)
def test_forward_gives_the_bits_of_the_f32_entry(gnntf, shared, C, p, relu):
    sparse = gnntf.sparse
    ops = operands(C)
    Hd, H0d, Md = dev(ops["H"]), dev(ops["H0"]), dev(ops["Ms"][0])
    Hb = Hd.to(torch.bfloat16)
    assert torch.equal(Hb.float(), Hd) and torch.equal(bits_of(sparse.to_bf16(Hd)), bits_of(Hb))        # representable: the cast is exact
    for name in ("t", "a"):
        g, adj, hub, empty = (shared[name][k] for k in ("g", "adj", "hub", "empty"))
        want_out, want_T = sparse._gcnii_launch(adj, Hd, H0d, A_MIX, Md, relu, keep_mixed=True, dropout=triple(p))
        assert g.last_kernel() == "spmm_gcnii_mfma" + ("_drop" if p > 0 else "")
        out, T = sparse.gcnii_step_train_bf16(adj, Hb, H0d, A_MIX, Md, relu, triple(p), out_bf16=False)
        assert g.last_kernel() == FWD
        assert out.dtype == torch.float32 and torch.equal(out, want_out) and torch.equal(T, want_T)
        outb, Tb = sparse.gcnii_step_train_bf16(adj, Hb, H0d, A_MIX, Md, relu, triple(p), out_bf16=True)
        assert outb.dtype == torch.bfloat16 and torch.equal(Tb, want_T)
        assert torch.equal(bits_of(outb), bits_of(sparse.to_bf16(want_out)))
        if p > 0 and not relu:                        # not vacuous on hub rows, rows without entries and the last partial tile: both kept
            plain = host(sparse._gcnii_launch(adj, Hd, H0d, A_MIX, Md, relu, keep_mixed=False)[0])      # and dropped values, the mask's
            keep = keep_mask(SEED, STREAM, p, N, C)
            for rows in (hub, empty, np.arange(N - N % 16, N)):
                if len(rows):                         # (the graph itself has no hub row)
                    assert 0 < keep[rows].mean() < 1
                    for got in (host(out), host(outb.float())):
                        np.testing.assert_array_equal(got[rows] != 0, keep[rows] & (plain[rows] != 0))
                        assert (got[rows] != 0).any() and (got[rows] == 0).any()
        assert float(T[dev(hub)].abs().max()) > 0 if len(hub) else True


def bits_of(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


# ---- 2. the gate -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("C", WIDTHS + (40, 7))
def test_gate_is_the_f32_gate_over_the_stored_rows(gnntf, shared, C, p):
    sparse = gnntf.sparse
    g = shared["t"]["g"]
    rng = np.random.default_rng(100 + C)
    X, up = rng.standard_normal((N, C)).astype(np.float32), rng.standard_normal((N, C)).astype(np.float32)
    keep = keep_mask(SEED, STREAM, p, N, C)
    y = np.where(keep, np.maximum(X, np.float32(0)) * scale(p), np.float32(0))         # the DROPPED forward output of a relu layer
    yb = sparse.to_bf16(dev(y))                                                        # ... as it was stored
    upd = dev(up)
    for relu in (True, False):
        G, Gb = sparse.feature_dropout_back_bf16(g, upd, yb if relu else None, triple(p), relu)
        want = sparse._feature_dropout_back(g, upd, yb.float(), p, SEED, STREAM, relu=relu)
        assert torch.equal(G, want) and Gb.dtype == torch.bfloat16
        assert torch.equal(bits_of(Gb), bits_of(sparse.to_bf16(G)))
        assert 0 < float((G != 0).float().mean()) < (1 if relu or p > 0 else 2)
        if p == 0:
            assert torch.equal(G, torch.ops.aten.threshold_backward(upd, yb.float(), 0.0) if relu else upd)
        else:
            np.testing.assert_array_equal(host(G) != 0, keep & (y > 0) if relu else keep)
    # in place (G is g), inside wider buffers
    wide_g, wide_G, wide_b = (torch.full((N, C + 8), 9.0, device="cuda", dtype=dt) for dt in (torch.float32, torch.float32, torch.bfloat16))
    wide_g[:, :C] = upd
    nat = sparse.nat
    nat.check(nat.lib().gnx_feature_dropout_back_bf16(g.handle, nat.ptr(wide_g), C + 8, nat.ptr(yb), C, N, C, p, SEED, STREAM, nat.ACT_RELU,
                                                      nat.ptr(wide_G), C + 8, nat.ptr(wide_b), C + 8, nat.current_stream()))
    want = sparse._feature_dropout_back(g, upd, yb.float(), p, SEED, STREAM, relu=True)
    assert torch.equal(wide_G[:, :C], want) and torch.equal(bits_of(wide_b[:, :C].contiguous()), bits_of(sparse.to_bf16(want)))
    assert bool((wide_G[:, C:] == 9.0).all()) and bool((wide_b[:, C:] == 9.0).all())
    nat.check(nat.lib().gnx_feature_dropout_back_bf16(g.handle, nat.ptr(wide_g), C + 8, nat.ptr(yb), C, N, C, p, SEED, STREAM, nat.ACT_RELU,
                                                      nat.ptr(wide_g), C + 8, nat.ptr(wide_b), C + 8, nat.current_stream()))
    assert torch.equal(wide_g[:, :C], want)


def test_gate_is_on_the_stored_value(gnntf, shared):
    """A positive f32 output that rounds to bf16 zero was stored as zero: no gradient passes."""
    sparse = gnntf.sparse
    y = np.full((4, 16), 1e-41, dtype=np.float32)                   # a denormal below half the smallest bf16: positive in f32, +0 as bf16
    y[:, 8:] = 1.0
    yb = sparse.to_bf16(dev(y))
    assert bool((yb.float()[:, :8] == 0).all()) and float(y.min()) > 0 and bool((bf16_round(y)[:, :8] == 0).all())
    G, Gb = sparse.feature_dropout_back_bf16(shared["t"]["g"], torch.ones(4, 16, device="cuda"), yb, None, True)
    assert bool((G[:, :8] == 0).all()) and bool((G[:, 8:] == 1).all()) and torch.equal(Gb.float(), G)


# ---- 3. the backward over bf16-representable G ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "t"])
@pytest.mark.parametrize("C", WIDTHS)
def test_backward_gives_the_bits_of_the_f32_entry(gnntf, shared, C, name):
    sparse = gnntf.sparse
    g, adj, hub_t, empty_t = (shared[name][k] for k in ("g", "adj", "hub_t", "empty_t"))
    ops = operands(C)
    Gd, Sd, Mtd = dev(ops["up"]), dev(ops["S_in"]), dev(np.ascontiguousarray(ops["Ms"][0].T))
    Gb = Gd.to(torch.bfloat16)
    assert torch.equal(Gb.float(), Gd)
    want_dH, want_S = gnntf.gcnii_step_back(adj, Gd, A_MIX, Mtd)                                    # without S_in
    assert g.last_kernel() == "spmm_gcnii_back_mfma"
    dH, S = sparse.gcnii_step_back_bf16(adj, Gb, Gd, A_MIX, Mtd)
    assert g.last_kernel() == BACK
    assert torch.equal(dH, want_dH) and torch.equal(S, want_S)
    want_dH2, want_S2 = gnntf.gcnii_step_back(adj, Gd, A_MIX, Mtd, S_in=Sd, s_alpha=0.5)             # with S_in
    dH2, S2 = sparse.gcnii_step_back_bf16(adj, Gb, Gd, A_MIX, Mtd, S_in=Sd, s_alpha=0.5)
    assert torch.equal(dH2, want_dH) and torch.equal(dH2, want_dH2) and torch.equal(S2, want_S2) and not torch.equal(S2, S)
    running = dev(ops["S_in"])                                                                      # in place: S_in == S_out
    dH3, S3 = sparse.gcnii_step_back_bf16(adj, Gb, Gd, A_MIX, Mtd, S_in=running, s_alpha=0.5, in_place=True)
    assert S3 is running and torch.equal(running, want_S2) and torch.equal(dH3, want_dH)
    dH4, none = sparse.gcnii_step_back_bf16(adj, Gb, None, A_MIX, Mtd, want_S=False)                 # d_S_out = NULL with d_G = NULL
    assert none is None and torch.equal(dH4, want_dH)
    # the hub row of the transposed structure went through the chunk kernels; rows without entries there get dH = 0, written
    assert len(empty_t) >= 100 and bool((dH[dev(empty_t)] == 0).all()) and float(S[dev(empty_t)].abs().max()) > 0
    if name == "a":
        assert HUB in hub_t and float(dH[HUB].abs().max()) > 0
    else:
        assert len(hub_t) == 0
    # the own-row product reads the f32 G: with a G that is NOT representable, S is the f32 entry's over G, dH the one over bf(G)
    rough = dev(np.random.default_rng(C).standard_normal((N, C)).astype(np.float32))
    rough_b = sparse.to_bf16(rough)
    dH5, S5 = sparse.gcnii_step_back_bf16(adj, rough_b, rough, A_MIX, Mtd)
    assert torch.equal(S5, gnntf.gcnii_step_back(adj, rough, A_MIX, Mtd)[1])
    assert torch.equal(dH5, gnntf.gcnii_step_back(adj, rough_b.float(), A_MIX, Mtd)[0])


# ---- 4. error paths -------------------------------------------------------------------------------------------------------------------
def test_error_paths_name_the_cause_and_launch_nothing(gnntf, shared):
    sparse = gnntf.sparse
    nat = sparse.nat
    lib = nat.lib()
    g, adj = shared["t"]["g"], shared["t"]["adj"]
    gnntf.gcnii_step(adj, dev(operands(16)["H"]), dev(operands(16)["H0"]), A_MIX, dev(operands(16)["Ms"][0]))
    before = g.last_kernel()
    assert before == "spmm_gcnii_mfma"
    s = nat.current_stream()

    def buffers(C):
        f32 = lambda: torch.full((N * C + 4,), 9.0, device="cuda")
        return dict(Hb=torch.zeros(N * C + 4, device="cuda", dtype=torch.bfloat16), H0=torch.zeros(N, C, device="cuda"),
                    M=torch.eye(C, device="cuda"), out=f32(), mixed=f32(), work=f32(), G=torch.zeros(N * C + 4, device="cuda"),
                    dH=f32(), S=f32())

    def forward(b, C, p=0.5, Hb=None, out=None, mixed="given", out_bf16=0):
        return lib.gnx_gcnii_step_train_bf16(g.handle, nat.ptr(adj.vals), nat.ptr(b["Hb"] if Hb is None else Hb), nat.ptr(b["H0"]), A_MIX, C,
                                             nat.ptr(b["M"]), C, 1, p, SEED, STREAM, nat.ptr(b["out"] if out is None else out), out_bf16,
                                             nat.ptr(b["mixed"]) if mixed == "given" else None, nat.ptr(b["work"]), s)

    def backward(b, C, Gb=None, G="given", S="given", dH=None):
        return lib.gnx_gcnii_step_back_bf16(g.handle, nat.ptr(adj.transposed_values()), nat.ptr(b["Hb"] if Gb is None else Gb),
                                            nat.ptr(b["G"]) if G == "given" else None, A_MIX, C, nat.ptr(b["M"]), C,
                                            nat.ptr(b["dH"] if dH is None else dH), None, 1.0, nat.ptr(b["S"]) if S == "given" else None, None, s)

    def refused(rc, code, *words):
        message = lib.gnx_last_error()
        assert rc == code and all(word in message for word in words), (rc, message)

    for C in (40, 7):                                               # other widths: unsupported, naming the width
        b = buffers(C)
        refused(forward(b, C), UNSUPPORTED, b"gnx_gcnii_step_train_bf16", b"width %d" % C)
        refused(backward(b, C), UNSUPPORTED, b"gnx_gcnii_step_back_bf16", b"width %d" % C)
        torch.cuda.synchronize()
        assert all(bool((b[k] == 9.0).all()) for k in ("out", "mixed", "work", "dH", "S"))
    b = buffers(16)
    refused(forward(b, 16, Hb=b["Hb"][1:]), UNSUPPORTED, b"gnx_gcnii_step_train_bf16", b"misaligned")          # a bf16 base at 2 mod 8
    refused(forward(b, 16, out=b["out"][1:]), UNSUPPORTED, b"misaligned")                                      # an f32 base at 4 mod 16
    refused(forward(b, 16, out=b["out"].view(torch.bfloat16)[1:], out_bf16=1), UNSUPPORTED, b"misaligned")
    refused(backward(b, 16, Gb=b["Hb"][1:]), UNSUPPORTED, b"gnx_gcnii_step_back_bf16", b"misaligned")
    refused(backward(b, 16, dH=b["dH"][1:]), UNSUPPORTED, b"misaligned")
    refused(forward(b, 16, mixed=None), INVALID, b"d_mixed")
    refused(forward(b, 16, p=1.0), INVALID, b"outside [0, 1)")
    refused(backward(b, 16, G=None), INVALID, b"d_G")
    refused(backward(b, 16, S=None), INVALID, b"d_G")                # ... and d_G without d_S_out
    refused(lib.gnx_feature_dropout_back_bf16(g.handle, nat.ptr(b["G"]), 16, nat.ptr(b["Hb"]), 16, N, 16, 1.0, SEED, STREAM, 1, nat.ptr(b["dH"]),
                                              16, nat.ptr(b["out"]), 16, s), INVALID, b"gnx_feature_dropout_back_bf16", b"outside [0, 1)")
    refused(lib.gnx_feature_dropout_back_bf16(g.handle, nat.ptr(b["G"]), 16, None, 0, N, 16, 0.5, SEED, STREAM, 1, nat.ptr(b["dH"]), 16,
                                              nat.ptr(b["out"]), 16, s), INVALID, b"relu needs y")
    torch.cuda.synchronize()
    assert all(bool((b[k] == 9.0).all()) for k in ("out", "mixed", "work", "dH", "S"))
    assert g.last_kernel() == before                                # nothing was launched
    # a graph with hub rows needs d_work, and says so
    rc = lib.gnx_gcnii_step_train_bf16(g.handle, nat.ptr(adj.vals), nat.ptr(b["Hb"]), nat.ptr(b["H0"]), A_MIX, 16, nat.ptr(b["M"]), 16, 1, 0.5,
                                       SEED, STREAM, nat.ptr(b["out"]), 0, nat.ptr(b["mixed"]), None, s)
    refused(rc, INVALID, b"d_work")
    # the functional layer refuses what the entries cannot take
    with pytest.raises(Exception, match="DroppedAdjacency"):
        sparse.gcnii_train_run_bf16(sparse.DroppedAdjacency(g, 0.5, 1, 0, D=torch.ones(N, device="cuda")), b["H0"], [(b["H0"], 0.1, b["M"], True, None)])
    with pytest.raises(Exception, match="add_eye"):
        sparse.gcnii_train_run_bf16(gnntf.normalize(g, "symmetric", "after"), b["H0"], [(b["H0"], 0.1, b["M"], True, None)])
    with pytest.raises(Exception, match="width 16, 32 or 64"):
        sparse.gcnii_train_run_bf16(adj, torch.zeros(N, 40, device="cuda"), [(torch.zeros(N, 40, device="cuda"), 0.1, torch.eye(40, device="cuda"), True, None)])


# ---- 5. determinism and the reported names ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
def test_two_calls_give_the_same_bits(gnntf, shared, C):
    sparse = gnntf.sparse
    ops = operands(C)
    rng = np.random.default_rng(5 * C)
    H, up = (dev(rng.standard_normal((N, C)).astype(np.float32)) for _ in range(2))      # not representable: the general case
    H0d, Md, Mtd = dev(ops["H0"]), dev(ops["Ms"][0]), dev(np.ascontiguousarray(ops["Ms"][0].T))
    for name in ("t", "a"):
        g, adj = shared[name]["g"], shared[name]["adj"]
        Hb = sparse.to_bf16(H)
        first = sparse.gcnii_step_train_bf16(adj, Hb, H0d, A_MIX, Md, True, triple(0.6))
        assert g.last_kernel() == FWD
        second = sparse.gcnii_step_train_bf16(adj, Hb, H0d, A_MIX, Md, True, triple(0.6))
        assert torch.equal(bits_of(first[0]), bits_of(second[0])) and torch.equal(first[1], second[1])
        gate = [sparse.feature_dropout_back_bf16(g, up, first[0], triple(0.6), True) for _ in range(2)]
        assert torch.equal(gate[0][0], gate[1][0]) and torch.equal(bits_of(gate[0][1]), bits_of(gate[1][1]))
        assert g.last_kernel() == FWD                               # the pass reports nothing
        back = [sparse.gcnii_step_back_bf16(adj, gate[0][1], gate[0][0], A_MIX, Mtd, S_in=H0d, s_alpha=1.0) for _ in range(2)]
        assert g.last_kernel() == BACK
        assert torch.equal(back[0][0], back[1][0]) and torch.equal(back[0][1], back[1][1])
        assert float(back[0][0].abs().max()) > 0


# ---- 6. the run is the composition of its pieces ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["aaa", "aab", "aba"])
@pytest.mark.parametrize("C", [16, 64])
def test_run_is_the_layer_by_layer_composition(gnntf, shared, C, pattern):
    sparse = gnntf.sparse
    ops = operands(C)
    g, adj = shared["t"]["g"], shared["t"]["adj"]
    rng = np.random.default_rng(C + len(pattern))
    Hd, upd = dev(rng.standard_normal((N, C)).astype(np.float32)), dev(rng.standard_normal((N, C)).astype(np.float32))
    relus, rates, a = (True, False, True), (0.6, 0.25, 0.0), A_MIX
    drops = [triple(p, STREAM + k) for k, p in enumerate(rates)]

    leaves = dict(H=Hd.clone().requires_grad_(), a=dev(ops["H0"]).requires_grad_(), b=dev(ops["H0b"]).requires_grad_())
    Ms = [dev(M).requires_grad_() for M in ops["Ms"][:3]]
    out = sparse.gcnii_train_run_bf16(adj, leaves["H"], [(leaves[key], a, M, relu, drop) for key, M, relu, drop in zip(pattern, Ms, relus, drops)])
    assert g.last_kernel() == FWD and out.dtype == torch.float32 and out.requires_grad
    out.backward(upd)
    assert g.last_kernel() == BACK

    with torch.no_grad():                                           # the explicit composition
        H0 = dict(a=dev(ops["H0"]), b=dev(ops["H0b"]))
        M = [dev(m) for m in ops["Ms"][:3]]
        X, stored, Ts = sparse.to_bf16(Hd), [], []
        for k in range(3):
            X, T = sparse.gcnii_step_train_bf16(adj, X, H0[pattern[k]], a, M[k], relus[k], drops[k], out_bf16=k < 2)
            stored.append(X)
            Ts.append(T)
        want_out = stored[-1]
        grad, dM, dH0 = upd, [None] * 3, dict()
        for k in (2, 1, 0):
            if k == 2:                                              # the f32 output: the existing gate, then the cast
                G = sparse._feature_dropout_back(g, grad, stored[k], *(drops[k] or (0.0, 0, 0)), relu=relus[k])
                Gb = sparse.to_bf16(G)
            else:
                G, Gb = sparse.feature_dropout_back_bf16(g, grad, stored[k], drops[k], relus[k])
            dM[k] = sparse._dense_wgrad(Ts[k], G)
            shares = k < 2 and pattern[k + 1] == pattern[k]         # consecutive layers with one H0: one running sum
            grad, S = sparse.gcnii_step_back_bf16(adj, Gb, G, a, M[k].t().contiguous(), S_in=dH0["running"] if shares else None, s_alpha=1.0)
            if not shares and "running" in dH0:                     # the sum of the layers after this one is complete
                key = pattern[k + 1]
                dH0[key] = dH0[key] + dH0.pop("running") if key in dH0 else dH0.pop("running")
            dH0["running"] = S
        key = pattern[0]
        dH0[key] = dH0[key] + dH0.pop("running") if key in dH0 else dH0.pop("running")
    assert torch.equal(out.detach(), want_out)
    assert torch.equal(leaves["H"].grad, grad)
    for key in set(pattern):
        assert torch.equal(leaves[key].grad, dH0[key]), key
    if "b" not in pattern:
        assert leaves["b"].grad is None
    else:
        assert not torch.equal(leaves["a"].grad, leaves["b"].grad)  # each H0 has its own sum
    for k in range(3):
        assert torch.equal(Ms[k].grad, dM[k]) and float(dM[k].abs().max()) > 0


def test_run_asks_only_for_the_gradients_autograd_wants(gnntf, shared):
    sparse = gnntf.sparse
    ops = operands(32)
    adj = shared["a"]["adj"]
    Hd, upd = dev(ops["H"]), dev(ops["up"])
    steps = lambda H0, Ms: [(H0, A_MIX, M, True, triple(0.25, STREAM + k)) for k, M in enumerate(Ms)]
    full = [Hd.clone().requires_grad_(), dev(ops["H0"]).requires_grad_()] + [dev(M).requires_grad_() for M in ops["Ms"][:2]]
    sparse.gcnii_train_run_bf16(adj, full[0], steps(full[1], full[2:])).backward(upd)
    only_M = [dev(M).requires_grad_() for M in ops["Ms"][:2]]
    sparse.gcnii_train_run_bf16(adj, Hd, steps(dev(ops["H0"]), only_M)).backward(upd)
    assert all(torch.equal(m.grad, f.grad) for m, f in zip(only_M, full[2:]))
    only_H = Hd.clone().requires_grad_()
    sparse.gcnii_train_run_bf16(adj, only_H, steps(dev(ops["H0"]), [dev(M) for M in ops["Ms"][:2]])).backward(upd)
    assert torch.equal(only_H.grad, full[0].grad)
    same = dev(ops["H0"]).requires_grad_()                          # the run's input IS its H0 (the first layer of a GCNII stack)
    sparse.gcnii_train_run_bf16(adj, same, steps(same, [dev(M) for M in ops["Ms"][:2]])).backward(upd)
    assert same.grad is not None and float(same.grad.abs().max()) > 0


# ---- 7. against the float64 emulation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t", "a"])
@pytest.mark.parametrize("C", [16, 64])
def test_four_layer_run_against_the_emulation(gnntf, shared, C, name):
    """Output and every gradient of a 4-layer run within TOL (relative Frobenius) of the emulation; the distance from the f32 "fused" run
    within 2 x the distance between the emulation with and without its roundings (each printed before it is asserted)."""
    sparse = gnntf.sparse
    ops = operands(C)
    g, adj, A = (shared[name][k] for k in ("g", "adj", "A"))
    rng = np.random.default_rng(7 * C)
    H, up = rng.standard_normal((N, C)).astype(np.float32), rng.standard_normal((N, C)).astype(np.float32)
    pattern, relus, rates = "aabb", (True, True, False, True), (0.6, 0.0, 0.25, 0.6)
    H0 = dict(a=ops["H0"], b=ops["H0b"])
    drops = [triple(p, STREAM + k) for k, p in enumerate(rates)]
    masks = [ref.mask_scale(SEED, STREAM + k, p, N, C) if p > 0 else None for k, p in enumerate(rates)]
    emu_steps = [(key, H0[key], A_MIX, M, relu, mask) for key, M, relu, mask in zip(pattern, ops["Ms"], relus, masks)]
    emu = ref.run(A, H, emu_steps, up)
    plain = ref.run(A, H, emu_steps, up, rnd=ref.identity)

    def device_run(bf16):
        leaves = dict(H=dev(H).requires_grad_(), a=dev(H0["a"]).requires_grad_(), b=dev(H0["b"]).requires_grad_())
        Ms = [dev(M).requires_grad_() for M in ops["Ms"]]
        if bf16:
            out = sparse.gcnii_train_run_bf16(adj, leaves["H"], [(leaves[key], A_MIX, M, relu, drop)
                                                                 for key, M, relu, drop in zip(pattern, Ms, relus, drops)])
        else:
            out = leaves["H"]
            for key, M, relu, drop in zip(pattern, Ms, relus, drops):
                out = gnntf.gcnii_step(adj, out, leaves[key], A_MIX, M, relu=relu, backward="fused", dropout=drop)
        out.backward(dev(up))
        return dict(out=host(out), dH=host(leaves["H"].grad), dH0a=host(leaves["a"].grad), dH0b=host(leaves["b"].grad),
                    **{f"dM{k}": host(M.grad) for k, M in enumerate(Ms)})

    got, f32 = device_run(True), device_run(False)
    assert g.last_kernel() == "spmm_gcnii_back_mfma"
    flat = lambda r: dict(out=r["out"], dH=r["dH"], dH0a=r["dH0"]["a"], dH0b=r["dH0"]["b"], **{f"dM{k}": m for k, m in enumerate(r["dM"])})
    emu, plain = flat(emu), flat(plain)
    failures = []
    for key in got:
        err = ref.rel_fro(got[key], emu[key])
        dist = float(np.linalg.norm(got[key].astype(np.float64) - f32[key]))
        yard = float(np.linalg.norm(emu[key] - plain[key]))
        print(f"{name} C={C} {key}: err {err:.2e}; |bf16 - f32| {dist:.3e} (emulation {yard:.3e}); f32 err {ref.rel_fro(f32[key], plain[key]):.2e}")
        if not (err <= TOL and 0 < dist <= 2.0 * yard):
            failures.append(key)
    assert not failures


# ---- 8. the model --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cora():
    coo, vals, shape, X = graphs.cora_shaped(seed=4)
    labels = np.random.default_rng(4).integers(0, 7, size=shape[0])
    weights = [(np.random.default_rng(40 + k).standard_normal((64, 64)) / 8).astype(np.float32) for k in range(4)]
    return dict(coo=coo, vals=vals, shape=shape, X=X, labels=labels, weights=weights, train=np.arange(0, 300), valid=np.arange(300, 600))


BF16 = dict(feature_dropout="fused", gcnii_backward="fused", gcnii_training_dtype=torch.bfloat16)
F32 = dict(feature_dropout="fused", gcnii_backward="fused")


def make_model(gnntf, cora, seeded_weights=True, **option):
    gnntf.set_seed(11)
    torch.manual_seed(3)
    model = gnntf.GCNII(gnntf.SparseCOO(cora["coo"], cora["vals"], cora["shape"]), cora["X"], 7, latent_dims=[64], iterations=4, **option)
    model.reset()
    convs = [layer for layer in model.layers() if isinstance(layer, gnntf.GCNIILayer)]
    assert len(convs) == 4
    if seeded_weights:                                  # the reference initialises W to zero: M would be a multiple of the identity
        for layer, W in zip(convs, cora["weights"]):
            layer.W.data.copy_(dev(W))
    return model


def three_steps(gnntf, cora, model):
    """Three plain gradient steps in training mode; (losses, gradients of every step, mask streams taken, kernels after forward / backward)."""
    task = gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]])
    losses, grads, kernels = [], [], []
    first = model._mask_calls
    for _ in range(3):
        with model:
            for v in model.vars():
                v.var.grad = None
            loss = task.loss(model(model.features))
            kernels.append(model.graph.last_kernel())
            loss.backward()
            kernels.append(model.graph.last_kernel())
        losses.append(float(loss.detach()))
        grads.append([v.var.grad.clone() for v in model.vars()])
        with torch.no_grad():
            for v in model.vars():
                v.var -= 0.05 * v.var.grad
    return losses, grads, model._mask_calls - first, kernels


@pytest.fixture
def no_row_gate(gnntf, monkeypatch):
    monkeypatch.setattr(gnntf.sparse, "GCNII_BF16_TRAIN_MIN_ROWS", 0)


def test_model_step_runs_the_bf16_kernels_and_is_reproducible(gnntf, cora, no_row_gate):
    one = three_steps(gnntf, cora, make_model(gnntf, cora, **BF16))
    two = three_steps(gnntf, cora, make_model(gnntf, cora, **BF16))
    assert one[3] == [FWD, BACK] * 3
    assert one[2] == two[2] == 3 * 5                    # per step: the input features' mask and one per GCNII layer, as the f32 "fused" path
    assert one[0] == two[0] and len(set(one[0])) == 3
    for step_one, step_two in zip(one[1], two[1]):
        assert len(step_one) > 4 and all(torch.equal(a_, b_) for a_, b_ in zip(step_one, step_two))
    # the masks are those of the f32 "fused" path under the same seed: the two first steps are close, not equal
    f32 = three_steps(gnntf, cora, make_model(gnntf, cora, **F32))
    assert f32[3] == ["spmm_gcnii_mfma_drop", "spmm_gcnii_back_mfma"] * 3 and f32[2] == 3 * 5
    # (first order: at most 8 roundings of relative size 2^-8 lie on the way to the loss -- the run's input and three stored outputs,
    # and nothing of the backward -- so 4 x 2^-8 bounds it; another mask would move the loss by far more)
    print("first loss, bf16 / f32:", one[0][0], f32[0][0])
    assert f32[0][0] != one[0][0] and abs(f32[0][0] - one[0][0]) <= 4 * 2.0 ** -8 * abs(f32[0][0])
    # an inner layer's value: the detached exact widening of its stored rows, made on first read
    model = make_model(gnntf, cora, **BF16)
    with model:
        out = model(model.features)
    convs = [layer for layer in model.layers() if isinstance(layer, gnntf.GCNIILayer)]
    assert convs[1].__dict__["_pending_value"] is not None
    inner = convs[1].value
    assert inner.dtype == torch.float32 and not inner.requires_grad and tuple(inner.shape) == (cora["shape"][0], 64)
    assert torch.equal(inner.to(torch.bfloat16).float(), inner) and float(inner.abs().max()) > 0 and convs[1].value is inner
    assert convs[3].value is not None and convs[3].value.requires_grad and out.requires_grad


def test_captured_training_equals_eager(gnntf, cora, no_row_gate, monkeypatch):
    """train(capture=True) for 3 epochs, bit for bit the eager run (the pattern of tests/test_gpu_gcnii_drop.py)."""
    from gnntf import training
    observed, observe = [], training._BestSoFar.observe
    monkeypatch.setattr(training._BestSoFar, "observe", lambda self, loss: (observed[-1].append(loss), observe(self, loss))[1])
    results = []
    for capture in (False, True):
        observed.append([])
        model = make_model(gnntf, cora, seeded_weights=False, **BF16)
        gnntf.set_seed(11)
        torch.manual_seed(5)
        valid = gnntf.NodeClassification(cora["valid"], cora["labels"][cora["valid"]])
        model.train(train=gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]]), valid=valid, epochs=3, patience=50,
                    capture=capture, optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
        results.append(([v.var.detach().clone() for v in model.vars()], float(model.loss(valid)), model._mask_calls, model.graph.last_kernel()))
    (eager, eager_loss, eager_masks, _), (captured, captured_loss, captured_masks, _) = results
    print("captured vs eager, max |difference| per variable:", [float((e - c).abs().max()) for e, c in zip(eager, captured)])
    assert all(torch.equal(e, c) for e, c in zip(eager, captured))
    assert eager_loss == captured_loss
    print("held-out losses per epoch, eager / captured:", observed)
    assert len(observed[0]) == len(observed[1]) == 3 and observed[0] == observed[1] and len(set(observed[0])) == 3


def test_everything_else_keeps_its_path(gnntf, cora, monkeypatch):
    """The default dtype, the shipped row gate, torch dropout and eval mode: the f32 kernels and the f32 bits."""
    f32 = three_steps(gnntf, cora, make_model(gnntf, cora, **F32))
    explicit = three_steps(gnntf, cora, make_model(gnntf, cora, gcnii_training_dtype=torch.float32, **F32))
    gated = three_steps(gnntf, cora, make_model(gnntf, cora, **BF16))             # 2 708 rows: below sparse.GCNII_BF16_TRAIN_MIN_ROWS
    assert gnntf.sparse.GCNII_BF16_TRAIN_MIN_ROWS > cora["shape"][0]
    for other in (explicit, gated):
        assert other[3] == f32[3] and not any("_bf16" in kernel for kernel in other[3])
        assert other[0] == f32[0] and all(torch.equal(a_, b_) for s1, s2 in zip(other[1], f32[1]) for a_, b_ in zip(s1, s2))
    monkeypatch.setattr(gnntf.sparse, "GCNII_BF16_TRAIN_MIN_ROWS", 0)
    # torch dropout with a rate: nothing fused sits between the layers, the run keeps f32
    torch_drop = make_model(gnntf, cora, gcnii_backward="fused", gcnii_training_dtype=torch.bfloat16)
    reference = make_model(gnntf, cora, gcnii_backward="fused")
    a_, b_ = three_steps(gnntf, cora, torch_drop), three_steps(gnntf, cora, reference)
    assert a_[3] == b_[3] == ["spmm_gcnii_mfma", "spmm_gcnii_back_mfma"] * 3
    # ... and with dropout = 0 it needs none
    no_drop = make_model(gnntf, cora, dropout=0, gcnii_training_dtype=torch.bfloat16)
    assert three_steps(gnntf, cora, no_drop)[3] == [FWD, BACK] * 3
    # fuse_runs = False
    off = make_model(gnntf, cora, **BF16)
    off.fuse_runs = False
    assert three_steps(gnntf, cora, off)[3] == f32[3]
    # eval mode is untouched: the same weights give the same bits, through the f32 inference kernel
    outs = []
    for option in (BF16, F32, dict()):
        model = make_model(gnntf, cora, **option)
        model.training_mode(False)
        with torch.no_grad():
            outs.append(model(model.features))
        assert model.graph.last_kernel() == "spmm_gcnii_mfma"
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and float(outs[0].abs().max()) > 0
