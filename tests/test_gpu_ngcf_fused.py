"""The fused NGCFLayer on the MI355X (gnx_ngcf_step, gnx_ngcf_back_gate, sparse.ngcf_step, GNN(ngcf_layer="fused")).

Forward and gradients are judged against the float64 references of tests/ngcf_fused_ref.py over the very float32 weights the kernels read,
with max |got - want| / bound <= 1 -- the first-order bound of a float32 evaluation in any order, derived there -- at regime T (n = 1547: a
ragged last tile, hub rows at the threshold of 512, a whole tile of rows without entries) and regime S (n = 2^15 + 11, threshold 128) of
tests/gcnii_shapes_ref.py, bipartite-normalised.  Where existing code is the reference the comparison is bit for bit: the aggregated
rows and (with W1 = 0) the whole layer against gnx_gcn_step, the mask against the unmasked result times the scale."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ngcf_fused_ref as nref
from test_gpu_gcnii_drop import keep_mask

pytestmark = pytest.mark.gpu

SEED, STREAM = 7, 2                                      # the feature mask's
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


def bits(t):
    return host(t).view(np.int32)


def weights_csr(g, vals):
    rowptr, colidx, _ = g.csr_arrays()
    return sp.csr_matrix((host(vals).astype(np.float64), host(colidx), host(rowptr)), shape=(g.n_rows, g.n_cols))


@pytest.fixture(scope="module")
def world(gnntf):
    """Regimes T and S, bipartite-normalised: the handle, its adjacency and the weights read back, made once and never changed."""
    out = dict()
    for name in ("T", "S"):
        coo, vals, shape, info = nref.regime_graph(name)
        g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
        adj = gnntf.normalize(g, "bipartite")
        assert g.long_row_threshold == info["L"] and g.n_hub_rows == len(info["hub"]) > 0
        out[name] = dict(g=g, adj=adj, A=weights_csr(g, adj.vals), info=info, n=shape[0], L=info["L"])
    return out


@functools.lru_cache(maxsize=None)
def operands(n, C_in, C_out):
    return nref.operands(n, C_in, C_out, 900 + 7 * C_in + C_out)


def row_sets(info):
    return (("all", None), ("hub", info["hub"]), ("empty", info["empty"]), ("ragged", info["ragged"]))


def fused_name(C_in, drop=False, norm=True, hubs=True):
    return f"k_spmm_ngcf<{C_in}>" + ("_drop" if drop else "") + ("_norm" if norm else "") + ("+long" if hubs else "")


def composed_name(drop=False, norm=True):
    return "spmm+dense_mfma_ngcf" + ("_drop" if drop else "") + ("_norm" if norm else "")


def launch(sparse, w, op, act, bias=True, normalize=True, keep=False, dropout=None):
    b1, b2 = (dev(op["b1"]), dev(op["b2"])) if bias else (None, None)
    return sparse._ngcf_launch(w["adj"], dev(op["X"]), dev(op["W1"]), b1, dev(op["W2"]), b2, act, keep=keep, dropout=dropout, normalize=normalize)


def reference(w, op, act, bias=True, normalize=True, p=0.0, mask=None):
    b1, b2 = (op["b1"], op["b2"]) if bias else (None, None)
    return nref.forward_ref(w["A"], op["X"], op["W1"], b1, op["W2"], b2, act, normalize, p, mask, L=w["L"])


def act32(P, act):
    return np.where(P > 0, P, (nref.SLOPE32[act] * P).astype(np.float32)).astype(np.float32)


# ---- 1. the forward against float64; 3. the gate bits ------------------------------------------------------------------------------------
FORWARD_CASES = [("T",) + s for s in nref.SHAPES] + [("S", 64, 40)]


@pytest.mark.parametrize("regime, C_in, C_out", FORWARD_CASES)
def test_forward_against_float64(gnntf, world, regime, C_in, C_out):
    sparse = gnntf.sparse
    w = world[regime]
    g, info = w["g"], w["info"]
    op = operands(w["n"], C_in, C_out)
    worst = 0.0
    for act in ACTS:
        for bias in (True, False):
            for normalize in (True, False):
                where = f"{regime} {C_in}->{C_out} {act} bias={bias} normalize={normalize}"
                want = reference(w, op, act, bias, normalize)
                out = launch(sparse, w, op, act, bias, normalize)[0]
                assert g.last_kernel() == fused_name(C_in, norm=normalize), (where, g.last_kernel())
                assert out.shape == (w["n"], C_out)
                for name, rows in row_sets(info):
                    assert rows is None or len(rows) > 0
                    r_out = nref.ratio(host(out), want["out"], want["out_bound"], rows)
                    worst = max(worst, r_out)
                    print(f"{where} {name} rows: out error / bound = {r_out:.3f}")
                    assert r_out <= 1, (where, name)
                empty = host(out)[info["empty"]]
                if not bias:                                 # a row without entries and without bias: exact zeros, the clamp's 0 * 1e6
                    assert not empty.any(), where
                else:                                        # ... with biases: P = b exactly, so act(b1) + act(b2) bit for bit, then the norm
                    x = (act32(op["b1"], act) + act32(op["b2"], act)).astype(np.float32)
                    if not normalize:
                        assert np.array_equal(empty, np.broadcast_to(x, empty.shape)), where
                if normalize:
                    norms = np.linalg.norm(host(out).astype(np.float64), axis=1)
                    assert np.abs(norms[norms > 0] - 1).max() < 1e-5, where
    print(f"{regime} {C_in}->{C_out}: the largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("regime, C_in, C_out", FORWARD_CASES)
def test_gate_bits_are_the_float64_signs(gnntf, world, regime, C_in, C_out):
    """Bit (P > 0) of P1 and P2 against the float64 sign wherever |P| exceeds its forward bound; with the biases of
    ngcf_fused_ref.operands the undecided share of the reference alone is far below 0.1 % (tests/test_ngcf_fused_cpu.py measures it:
    at most 0.033 % over these cases).  The fused rows, the hub rows (the row pass) and the rows without entries alike."""
    sparse = gnntf.sparse
    w = world[regime]
    op = operands(w["n"], C_in, C_out)
    for act in ("leaky", "relu"):
        want = reference(w, op, act)
        d1, d2, share = nref.gate_share(want)
        assert share <= 1e-3
        _, agg, gate, rnorm = launch(sparse, w, op, act, keep=True)
        assert gate.dtype == torch.int32 and tuple(gate.shape) == (w["n"], 2 * ((C_out + 31) // 32)) and rnorm.shape == (w["n"],)
        b1, b2 = nref.unpack_gate(host(gate), C_out)
        assert np.array_equal(b1[d1], (want["P1"] > 0)[d1]) and np.array_equal(b2[d2], (want["P2"] > 0)[d2]), (regime, C_in, C_out, act)
        assert d1[w["info"]["empty"]].all() and d2[w["info"]["empty"]].all()        # P = b there, far above its bound
        # nothing beyond C_out in the last word
        words = host(gate).view(np.uint32)
        if C_out % 32:
            W = (C_out + 31) // 32
            assert not (words[:, [W - 1, 2 * W - 1]] >> np.uint32(C_out % 32)).any()
        # the reciprocal norms: 1 / |x| of the float64 reference, positive; a row of exact zeros (the relu shut every column: decided
        # bits, all clear) was clamped, which the sign records
        r = host(rnorm).astype(np.float64)
        size = np.sqrt((want["x"] ** 2).sum(axis=1))
        sound = size > 1e-3
        assert sound.mean() > 0.5 and (r[sound] > 0).all() and np.abs(r[sound] * size[sound] - 1).max() < 1e-4
        zero = (size == 0) & d1.all(axis=1) & d2.all(axis=1)
        assert np.allclose(r[zero], -1e6, rtol=1e-6, atol=0)
    assert launch(sparse, w, op, "none", keep=True)[2] is None


# ---- 2. bit-for-bit anchors on existing code ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime, C_in, C_out", FORWARD_CASES)
def test_anchors_on_the_gcn_launch(gnntf, world, regime, C_in, C_out):
    sparse = gnntf.sparse
    w = world[regime]
    op = operands(w["n"], C_in, C_out)
    Xd, W2d = dev(op["X"]), dev(op["W2"])
    # d_agg is gnx_gcn_step's d_agg, hub rows included
    gcn_out, gcn_agg = sparse._gcn_launch(w["adj"], Xd, W2d, None, True, keep_agg=True)
    out, agg, gate, rnorm = launch(sparse, w, op, "leaky", keep=True)
    assert np.array_equal(bits(agg), bits(gcn_agg))
    # d_agg, d_gate and d_rnorm do not move a bit of out
    assert np.array_equal(bits(out), bits(launch(sparse, w, op, "leaky")[0]))
    # W1 = 0, no biases, relu, no norm: the GCN layer over W2
    zero = sparse._ngcf_launch(w["adj"], Xd, torch.zeros_like(W2d), None, W2d, None, "relu", keep=False, normalize=False)[0]
    assert w["g"].last_kernel() == fused_name(C_in, norm=False)
    assert torch.equal(zero, gcn_out), (regime, C_in, C_out)


@pytest.mark.parametrize("C_in, C_out", [(64, 40), (64, 7), (16, 16), (24, 8)])
def test_feature_mask(gnntf, world, C_in, C_out):
    sparse = gnntf.sparse
    w = world["T"]
    g, n = w["g"], w["n"]
    op = operands(n, C_in, C_out)
    fused = C_in in (16, 32, 64)
    for p in (0.5, 0.25):
        plain = launch(sparse, w, op, "leaky", normalize=False)[0]
        masked, agg, _, _ = launch(sparse, w, op, "leaky", normalize=False, keep=True, dropout=(p, SEED, STREAM))
        assert g.last_kernel() == (fused_name(C_in, True, False) if fused else composed_name(True, False))
        keep = keep_mask(SEED, STREAM, p, n, C_out)
        want = np.where(keep, host(plain) * nref.scale(p), np.float32(0)).astype(np.float32)
        np.testing.assert_array_equal(bits(masked), want.view(np.int32))         # kept: unmasked x scale; dropped: +0
        assert np.array_equal(bits(agg), bits(launch(sparse, w, op, "leaky", normalize=False, keep=True)[1]))     # d_agg stays undropped
        # ... and the norm over the masked rows, against float64
        ref = reference(w, op, "leaky", True, True, p, keep)
        normed = launch(sparse, w, op, "leaky", dropout=(p, SEED, STREAM))[0]
        assert g.last_kernel() == (fused_name(C_in, True, True) if fused else composed_name(True, True))
        for name, rows in row_sets(w["info"]):
            assert nref.ratio(host(normed), ref["out"], ref["out_bound"], rows) <= 1, (C_in, C_out, p, name)


@pytest.mark.parametrize("C_in", [64, 16])
def test_seven_columns_write_nothing_else(gnntf, world, C_in):
    """C_out = 7 into rows of stride 7 (single values), of stride 8 (a float4 and three single values per row) and of stride 8 from a
    base that is not 16-byte aligned: the same [n, 7] block each time, every other element of the buffers untouched."""
    nat = gnntf.sparse.nat
    w = world["T"]
    n, g, pad = w["n"], w["g"], 64
    op = operands(n, C_in, 7)
    Xd, W1d, W2d, b1d, b2d = (dev(op[k]) for k in ("X", "W1", "W2", "b1", "b2"))
    floats = gnntf.sparse._ngcf_work_floats(n, C_in, 7, g.n_hub_rows, False)
    work = torch.empty(floats, device="cuda")
    results = []
    for ldo, shift in ((7, 0), (8, 0), (8, 1)):
        whole = torch.full((pad + shift + n * ldo + pad,), SENTINEL, device="cuda")
        out = whole[pad + shift:pad + shift + n * ldo]
        rc = nat.lib().gnx_ngcf_step(g.handle, nat.ptr(w["adj"].vals), nat.ptr(Xd), C_in, C_in, nat.ptr(W1d), 7, nat.ptr(W2d), 7, 7, nat.ptr(b1d),
                                     nat.ptr(b2d), nat.ACT_LEAKY, 0.0, 0, 0, 1, nat.ptr(out), ldo, None, None, None, nat.ptr(work), floats,
                                     nat.current_stream())
        assert rc == 0, nat.lib().gnx_last_error()
        assert g.last_kernel() == fused_name(C_in)
        torch.cuda.synchronize()
        block = out.view(n, ldo)
        assert bool((whole[:pad + shift] == SENTINEL).all()) and bool((whole[pad + shift + n * ldo:] == SENTINEL).all()), (ldo, shift)
        assert bool((block[:, 7:] == SENTINEL).all()), (ldo, shift)
        assert not bool((block[:, :7] == SENTINEL).any())
        results.append(block[:, :7].clone())
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])
    want = reference(w, op, "leaky")
    assert nref.ratio(host(results[0]), want["out"], want["out_bound"]) <= 1


# ---- 4. the composed forms inside the entry; refusals ------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_in, C_out", [(24, 8), (16, 64)])
def test_composed_forms_inside_the_entry(gnntf, world, C_in, C_out):
    sparse = gnntf.sparse
    w = world["T"]
    g, info = w["g"], w["info"]
    op = operands(w["n"], C_in, C_out)
    for act in ACTS:
        for normalize in (True, False):
            want = reference(w, op, act, True, normalize)
            for keep in (False, True):
                out, agg, gate, rnorm = launch(sparse, w, op, act, True, normalize, keep=keep)
                assert g.last_kernel() == composed_name(norm=normalize), g.last_kernel()
                for name, rows in row_sets(info):
                    assert nref.ratio(host(out), want["out"], want["out_bound"], rows) <= 1, (C_in, C_out, act, normalize, name)
                    assert agg is None or nref.ratio(host(agg), want["agg"], want["e_agg"], rows) <= 1
            if act != "none":
                d1, d2, _ = nref.gate_share(want)
                b1, b2 = nref.unpack_gate(host(gate), C_out)
                assert np.array_equal(b1[d1], (want["P1"] > 0)[d1]) and np.array_equal(b2[d2], (want["P2"] > 0)[d2])


def test_refusals_name_their_cause_and_write_nothing(gnntf, world):
    sparse, nat = gnntf.sparse, gnntf.sparse.nat
    lib = nat.lib()
    w = world["T"]
    g, n = w["g"], w["n"]
    op = operands(n, 64, 40)
    Xd, W1d, W2d, b1d, b2d = (dev(op[k]) for k in ("X", "W1", "W2", "b1", "b2"))
    floats = sparse._ngcf_work_floats(n, 64, 40, g.n_hub_rows, True)
    assert floats == g.n_hub_rows * (64 + 40)              # beyond d_agg the scratch grows with the hub rows, not with n
    out, agg, work = (torch.full(shape, SENTINEL, device="cuda") for shape in ((n, 40), (n, 64), (floats,)))
    gate = torch.full((n, 4), 77, dtype=torch.int32, device="cuda")
    rnorm = torch.full((n,), SENTINEL, device="cuda")

    def step(X=Xd, ldx=64, C_in=64, W1=W1d, ldw1=40, W2=W2d, ldw2=40, C_out=40, b1=b1d, b2=b2d, act=nat.ACT_LEAKY, rate=0.0, normalize=1, out_=out,
             ldo=40, agg_=agg, gate_=gate, rnorm_=rnorm, work_=work, work_floats=floats):
        return lib.gnx_ngcf_step(g.handle, nat.ptr(w["adj"].vals), nat.ptr(X), ldx, C_in, nat.ptr(W1), ldw1, nat.ptr(W2), ldw2, C_out, nat.ptr(b1),
                                 nat.ptr(b2), act, rate, SEED, STREAM, normalize, nat.ptr(out_), ldo, nat.ptr(agg_), nat.ptr(gate_), nat.ptr(rnorm_),
                                 nat.ptr(work_), work_floats, nat.current_stream())

    def refused(rc, *causes):
        message = lib.gnx_last_error()
        assert rc == -1 and b"gnx_ngcf_step" in message and all(c in message for c in causes), message
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in (out, agg, work, rnorm)) and bool((gate == 77).all())

    refused(step(work_floats=floats - 1), b"needs d_work of", b"hub rows")
    refused(step(agg_=None), b"needs d_work of", b"without d_agg")          # the [n, C_in] share is missing now
    refused(step(out_=Xd, ldo=64), b"out must not alias an input")
    refused(step(out_=b2d), b"out must not alias an input")
    refused(step(agg_=W2d), b"d_agg must be a buffer of its own")
    refused(step(gate_=out), b"d_gate must be a buffer of its own")
    refused(step(rnorm_=agg), b"d_rnorm must be a buffer of its own")
    refused(step(work_=W1d), b"d_work must be a buffer of its own")
    refused(step(normalize=0), b"d_rnorm without normalize")
    refused(step(normalize=2), b"normalize must be 0 or 1")
    refused(step(W2=None), b"NULL X / W1 / W2 / out")
    refused(step(ldw2=39), b"ldw2 39 < C_out 40")
    refused(step(ldw1=39), b"ldw1 39")
    refused(step(ldo=39), b"ldo 39 < C_out 40")
    refused(step(ldx=63), b"ldx 63 < C_in 64")
    refused(step(rate=1.0), b"dropout rate 1 outside [0, 1)")
    refused(step(act=7), b"invalid activation 7")
    refused(step(work_=None), b"work_floats")
    # the composed forms need their rows too
    for C_in, C_out, why in ((24, 8, b"C_in is not 16, 32 or 64"), (16, 64, b"C_out > C_in")):
        o2 = operands(n, C_in, C_out)
        small = torch.full((n, C_out), SENTINEL, device="cuda")
        rc = step(X=dev(o2["X"]), ldx=C_in, C_in=C_in, W1=dev(o2["W1"]), ldw1=C_out, W2=dev(o2["W2"]), ldw2=C_out, C_out=C_out, b1=None, b2=None,
                  out_=small, ldo=C_out, agg_=None, gate_=None, rnorm_=None, work_floats=floats)
        message = lib.gnx_last_error()
        assert rc == -1 and b"needs d_work of" in message and why in message, message
        torch.cuda.synchronize()
        assert bool((small == SENTINEL).all()) and bool((work == SENTINEL).all())
    # an existing entry still refuses the new activation
    rc = lib.gnx_gcn_step(g.handle, None, nat.ptr(Xd), 64, 64, nat.ptr(W1d), 40, 40, None, nat.ACT_LEAKY, 0.0, 0, 0, nat.ptr(out), 40, nat.ptr(agg),
                          None, nat.current_stream())
    assert rc == -1 and b"gnx_gcn_step: invalid activation 2" in lib.gnx_last_error()
    assert lib.gnx_dense(nat.ptr(Xd), 64, n, 64, nat.ptr(W1d), 40, 40, None, nat.ACT_LEAKY, nat.ptr(out), 40, nat.current_stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((agg == SENTINEL).all())
    assert step() == 0, lib.gnx_last_error()                # the call itself is well formed
    torch.cuda.synchronize()
    assert not any(bool((t == SENTINEL).any()) for t in (out, agg, rnorm)) and not bool((gate == 77).all())
    assert g.last_kernel() == fused_name(64)


# ---- 5. gradients ------------------------------------------------------------------------------------------------------------------------
def test_back_gate_alone_against_float64(gnntf, world):
    """gnx_ngcf_back_gate over data of its own: unit rows y, their factors r (one row marked as clamped by a negative r, one whole row
    dropped by the mask), random gate bits and the mask at p = 0.25; C_out = 40 and 7 (padding columns written as zeros)."""
    sparse = gnntf.sparse
    g = world["T"]["g"]
    n = 300
    for C_out, act in ((40, "leaky"), (7, "relu"), (40, "none")):
        rng = np.random.default_rng(40 + C_out)
        x = rng.standard_normal((n, C_out))
        r = 1.0 / np.linalg.norm(x, axis=1, keepdims=True)
        y32 = (x * r).astype(np.float32)
        r32 = r.astype(np.float32).reshape(-1).copy()
        r32[5] = -np.float32(1e6)                              # a clamped row: out = 1e6 x, the derivative is r itself
        up = rng.standard_normal((n, C_out)).astype(np.float32)
        W = (C_out + 31) // 32
        words = rng.integers(0, 2 ** 32, size=(n, 2 * W), dtype=np.uint64).astype(np.uint32)
        bit1, bit2 = nref.unpack_gate(words, C_out)
        for normalize in (True, False):
            for p in (0.0, 0.25):
                mask = None if p == 0 else keep_mask(SEED, STREAM, p, n, C_out)
                G1, G2 = sparse._ngcf_back_gate(g, dev(up), dev(y32) if normalize else None, dev(r32) if normalize else None,
                                                dev(words.view(np.int32)) if act != "none" else None, act, None if p == 0 else (p, SEED, STREAM))
                assert G1.stride(0) == (C_out + 3) // 4 * 4
                f = dict(y=y32.astype(np.float64), r=np.abs(r32.astype(np.float64)).reshape(-1, 1), e_y=np.zeros((n, C_out)),
                         e_x=np.zeros((n, C_out)), clamped=(r32 < 0).reshape(-1, 1))
                w1, e1, w2, e2 = nref.back_gate_ref(f, up, bit1, bit2, act, normalize, p, mask)
                for got, want, bound in ((G1, w1, e1), (G2, w2, e2)):
                    worst = nref.ratio(host(got), want, bound)
                    print(f"back gate C_out={C_out} {act} normalize={normalize} p={p}: error / bound = {worst:.3f}")
                    assert worst <= 1
                    storage = host(torch.as_strided(got, (n, got.stride(0)), (got.stride(0), 1)))
                    assert not storage[:, C_out:].any()      # the padding: zeros
                if mask is not None:
                    assert not host(G1)[~mask].any() and host(G1)[mask].any()


GRADIENT_CASES = [("T", 64, 64), ("T", 64, 7), ("T", 16, 16), ("S", 32, 32)]


@pytest.mark.parametrize("regime, C_in, C_out", GRADIENT_CASES)
def test_autograd_against_float64(gnntf, world, regime, C_in, C_out):
    sparse = gnntf.sparse
    w = world[regime]
    g, n = w["g"], w["n"]
    op = operands(n, C_in, C_out)
    names = ("X", "W1", "b1", "W2", "b2")
    for act in (("leaky", "relu") if regime == "T" and C_out == 7 else ("leaky",)):
        for mask in (None, (0.5, SEED, STREAM)):
            for normalize in (True, False):
                where = f"{regime} {C_in}->{C_out} {act} mask={mask is not None} normalize={normalize}"
                leaves = [dev(op[k]).requires_grad_() for k in names]
                out = gnntf.ngcf_step(w["adj"], *leaves, activation=act, dropout=mask, normalize=normalize)
                assert g.last_kernel() == fused_name(C_in, mask is not None, normalize), where
                out.backward(dev(op["g"]))
                p = 0.0 if mask is None else mask[0]
                keep = None if mask is None else keep_mask(SEED, STREAM, p, n, C_out)
                f = reference(w, op, act, True, normalize, p, keep)
                assert nref.ratio(host(out), f["out"], f["out_bound"]) <= 1, where
                gate = launch(sparse, w, op, act, True, normalize, keep=True, dropout=mask)[2]
                bit1, bit2 = nref.unpack_gate(host(gate), C_out)       # the bits the kernel reported (judged on their own above)
                gated = nref.back_gate_ref(f, op["g"], bit1, bit2, act, normalize, p, keep)
                want = nref.backward_ref(w["A"], f, op["X"], op["W1"], op["W2"], *gated, L=w["L"])
                for name, key, leaf in zip(names, ("dX", "dW1", "db1", "dW2", "db2"), leaves):
                    got = host(leaf.grad)
                    worst = nref.ratio(got.reshape(1, -1) if got.ndim == 1 else got, want[key].reshape(-1, got.shape[-1]),
                                       want[key + "_bound"].reshape(-1, got.shape[-1]))
                    print(f"{where} {key}: error / bound = {worst:.3g}")
                    assert worst <= 1 and float(np.abs(got).max()) > 0, (where, key)


# ---- 6. the model ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_sided():
    """300 users and 200 items, about 2 400 user-item pairs without duplicates, stored in both directions; 16-wide features."""
    import networkx as nx
    rng = np.random.default_rng(31)
    n_u, n_i = 300, 200
    pairs = np.unique(np.stack([rng.integers(0, n_u, size=2400), n_u + rng.integers(0, n_i, size=2400)], axis=1), axis=0)
    coo = np.concatenate([pairs, pairs[:, ::-1]]).astype(np.int64)
    G = nx.Graph(); G.add_nodes_from(range(n_u + n_i)); G.add_edges_from((int(u), int(v)) for u, v in pairs)
    X = rng.standard_normal((n_u + n_i, 16)).astype(np.float32)
    return dict(coo=coo, vals=np.ones(len(coo), dtype=np.float32), shape=(n_u + n_i, n_u + n_i), X=X, G=G, pairs=pairs)


def make_model(gnntf, data, width=16, X=None, **option):
    gnntf.set_seed(11)
    torch.manual_seed(3)
    model = gnntf.NGCF(gnntf.SparseCOO(data["coo"], data["vals"], data["shape"]), data["X"] if X is None else X, num_classes=width, **option)
    model.reset()
    return model


class CountingLibrary:
    """The loaded library with every access to one of the new entries counted."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if "ngcf" in name:
            self.calls.append(name)
        return getattr(self.real, name)


def test_model_eval_against_the_oracle_per_layer(gnntf, two_sided, monkeypatch):
    from oracle import gnntf_oracle as orc
    nat = gnntf.sparse.nat
    counting = CountingLibrary(nat.lib())
    monkeypatch.setattr(nat, "lib", lambda: counting)
    fused, default = make_model(gnntf, two_sided, ngcf_layer="fused"), make_model(gnntf, two_sided)
    assert default.ngcf_layer == "composed" and fused.ngcf_layer == "fused"
    outs = dict()
    for name, model in (("fused", fused), ("default", default)):
        counting.calls.clear()
        model.training_mode(False)
        with torch.no_grad():
            outs[name] = model(model.features)
        layers = [l for l in model.layers() if isinstance(l, gnntf.NGCFLayer)]
        assert len(layers) == 3 and all(tuple(l.W1.shape) == (16, 16) for l in layers)
        if name == "fused":
            assert counting.calls == ["gnx_ngcf_step"] * 3 and model.graph.last_kernel() == fused_name(16, hubs=False)
        else:                                               # without the keyword: no call of the new entries
            assert counting.calls == []
    n = two_sided["shape"][0]
    # the default model is today's path, op for op
    with torch.no_grad():
        H, rows = default.features, []
        for l in [l for l in default.layers() if isinstance(l, gnntf.NGCFLayer)]:
            agg = gnntf.sparse.spmm(l.adjacency, H)
            H = torch.nn.functional.normalize(l.activation(gnntf.blocks.affine(H * agg, l.W1, l.b1)) + l.activation(gnntf.blocks.affine(agg, l.W2, l.b2)),
                                              dim=1, eps=1e-12)
            rows.append(H)
        assert torch.equal(outs["default"], torch.cat(rows, dim=0))
    # every fused layer against the oracle in float64 over the layer's own float32 input, within the bound (the oracle normalises the
    # adjacency in float64: the float32 weights' own rounding enters the bound as e_A)
    layers = [l for l in fused.layers() if isinstance(l, gnntf.NGCFLayer)]
    g = fused.graph
    A32 = weights_csr(g, layers[0].adjacency.vals)
    ai, av = orc.get_adjacency(two_sided["coo"], two_sided["vals"], two_sided["shape"], normalized="bipartite", training=False, dtype=np.float64)
    A64 = sp.csr_matrix((av, (ai[:, 0], ai[:, 1])), shape=two_sided["shape"])
    e_A = sp.csr_matrix(abs(A32 - A64))
    H = two_sided["X"]
    for k, l in enumerate(layers):
        W1, b1, W2, b2 = (host(t) for t in (l.W1, l.b1, l.W2, l.b2))
        want = orc.ngcf_layer_eval(two_sided["coo"], two_sided["vals"], two_sided["shape"], H, W1, b1.reshape(-1), W2, b2.reshape(-1))
        bound = nref.forward_ref(A32, H, W1, b1, W2, b2, "leaky", L=g.long_row_threshold, e_A=e_A)["out_bound"]
        got = host(outs["fused"][k * n:(k + 1) * n])
        worst = nref.ratio(got, want, bound)
        print(f"layer {k}: error / bound against the oracle = {worst:.3f}")
        assert worst <= 1
        H = got


def test_width_128_keeps_the_composed_path(gnntf, two_sided, monkeypatch):
    nat = gnntf.sparse.nat
    counting = CountingLibrary(nat.lib())
    monkeypatch.setattr(nat, "lib", lambda: counting)
    X = np.random.default_rng(5).standard_normal((two_sided["shape"][0], 128)).astype(np.float32)
    wide = make_model(gnntf, two_sided, width=128, X=X, ngcf_layer="fused")
    wide.training_mode(False)
    with torch.no_grad():
        out = wide(wide.features)
    layers = [l for l in wide.layers() if isinstance(l, gnntf.NGCFLayer)]
    assert counting.calls == [] and out.shape == (3 * two_sided["shape"][0], 128)
    assert not any(l._fused_ngcf(wide, wide.features) for l in layers) and "ngcf" not in wide.graph.last_kernel()


def matched_edges(data, count=90):
    """(edges, labels) in the layout of gnntf.negative_sampling -- a positive pair, then one negative pair of the same user -- in which
    every user stands in one positive pair and every item in one pair at all: the backward of the edge scores adds into the rows of its
    endpoints with float atomics, and a row that receives at most two addends has the same bits in whatever order they arrive."""
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


def test_captured_training_equals_eager(gnntf, two_sided, monkeypatch):
    """Two epochs of train(LinkPrediction, capture=True) under feature_dropout="fused", bit for bit the eager run.  The task holds one
    fixed list of positive and negative pairs (matched_edges), kept on the device: LinkPrediction uploads a host edge list at every
    call of its loss and a sampler draws new edges on the host at every call, neither of which a device graph can replay --
    train(capture=True) refuses both (tests/test_gpu_training.py pins the refusal), fused layer or not -- and the edge scores' backward
    is order-dependent where an endpoint repeats more than twice.  The loss is LinkPrediction's own pairwise loss."""
    import random
    nat, sparse = gnntf.sparse.nat, gnntf.sparse
    counting = CountingLibrary(nat.lib())
    monkeypatch.setattr(nat, "lib", lambda: counting)

    class DeviceEdges(sparse.DeviceIndex):
        def __len__(self):
            return self.tensor.shape[0]

    results = []
    for capture in (False, True):
        random.seed(0)
        np.random.seed(0)
        model = make_model(gnntf, two_sided, ngcf_layer="fused", feature_dropout="fused", dropout=0.25)
        edges, labels = matched_edges(two_sided)
        task = gnntf.LinkPrediction(edges, labels)
        task.edges = DeviceEdges(edges, torch.device("cuda:0"), None)
        gnntf.set_seed(11)
        torch.manual_seed(5)
        counting.calls.clear()
        model.train(train=task, epochs=2, patience=50, capture=capture,
                    optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
        assert "gnx_ngcf_step" in counting.calls and "gnx_ngcf_back_gate" in counting.calls
        results.append(([v.var.detach().clone() for v in model.vars()], model._mask_calls, edges.copy()))
    (eager, eager_masks, eager_edges), (captured, captured_masks, captured_edges) = results
    assert np.array_equal(eager_edges, captured_edges)
    assert eager_masks == captured_masks and eager_masks >= 3           # a mask stream per layer and step
    assert all(torch.equal(e, c) for e, c in zip(eager, captured))
