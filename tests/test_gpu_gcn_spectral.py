"""The fused GCNSpectralPreservingLayer on the MI355X (gnx_step_spectral_gcn, gnx_step_spectral_gcn_dropped, sparse.gcn_step_spectral,
GNN(gcn_spectral="fused")).

The forward, the gate bits and the gradients are judged against the float64 references of tests/gcn_spectral_ref.py over the very float32
weights the kernels read, with max |got - want| / bound <= 1, at regime T (n = 1547: 23 hub rows, a tile without entries, a ragged last
tile) and regime S (n = 2^15 + 11: 154 hub rows, more than one block of the row-list pass) of tests/gcnii_shapes_ref.py.  Where existing
code is the reference the comparison is bit for bit: A . X against gnx_gcn_step's, the finished value against spectral_finish's
arithmetic applied in numpy to gnx_gcn_step's act(P') -- for rows of the tile path, the hub path and the composition inside the entry
alike --, the edge-dropout entry against the plain entry over the materialised adjacency, the mask against the unmasked result."""
import functools

import numpy as np
import pytest
import torch

import gcn_spectral_ref as sref
import graphs
from test_gpu_gcn_fused import E_SEED, E_STREAM, bits, dev, dropped_world, host, weights_csr, world  # noqa: F401  (two fixtures among them)

pytestmark = pytest.mark.gpu

SEED, STREAM = 7, 2                                      # the feature mask's
FUSED = (16, 32, 64)
NONE, RELU = 0, 1


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def one_launch(C_in, C_out):
    return C_in in FUSED and C_out <= C_in


def kernel_name(C_in, C_out, p=0.0, edge=False, hubs=True):
    tail = ("_edrop" if edge else "") + ("_drop" if p else "")
    if one_launch(C_in, C_out):
        return f"k_spmm_gcn_spectral<{C_in}>" + tail + ("+long" if hubs else "")
    return "spmm+dense_mfma_gcn_spectral" + tail


def roundup4(x):
    return (x + 3) // 4 * 4


def entry(gnntf, g, Xd, Wd, bd, relu, p, vals=None, edge=None, train=True, ldo=None, stream=STREAM, gate=True, rows_through="auto"):
    """gnx_step_spectral_gcn (``edge`` = (D, p, seed, stream): gnx_step_spectral_gcn_dropped) itself, into poisoned buffers: out is NaN
    in rows of stride ``ldo`` (default: roundup4(C_out) + 4, so that columns exist beyond C_out - 1), A . X is NaN and every gate word is
    all ones.  ``train``: d_agg and (relu) d_gate are given; else d_work where rows pass through memory.  Returns (rc, out [n, ldo],
    agg or None, gate as int32 or None)."""
    nat = gnntf.sparse.nat
    n, C_in = Xd.shape
    C_out = Wd.shape[1]
    ldo = roundup4(C_out) + 4 if ldo is None else ldo
    out = torch.full((n, ldo), float("nan"), device="cuda")
    rows = torch.full((n, C_in), float("nan"), device="cuda")
    agg, work = (rows, None) if train else (None, rows if rows_through == "auto" else None)
    words = torch.full((n, sref.gate_words(C_out)), -1, dtype=torch.int32, device="cuda") if train and relu and gate else None
    layer = (nat.ptr(Xd), Xd.stride(0), C_in, nat.ptr(Wd), Wd.stride(0), C_out, nat.ptr(bd), RELU if relu else NONE, float(p), SEED, stream,
             nat.ptr(out), ldo, nat.ptr(agg), nat.ptr(words), nat.ptr(work), nat.current_stream())
    if edge is not None:
        D, e_p, e_seed, e_stream = edge
        rc = nat.lib().gnx_step_spectral_gcn_dropped(g.handle, nat.ptr(D), e_p, e_seed, e_stream, *layer)
    else:
        rc = nat.lib().gnx_step_spectral_gcn(g.handle, nat.ptr(vals), *layer)
    torch.cuda.synchronize()
    return rc, out, agg, words


@functools.lru_cache(maxsize=None)
def operands(n, C_in, C_out):
    return sref.operands(n, C_in, C_out)


def device_operands(n, C_in, C_out):
    op = operands(n, C_in, C_out)
    return op, dev(op["X"]), dev(op["W"]), dev(op["bias"])


_REFERENCES = dict()


def reference(w, regime, C_in, C_out, relu, with_bias, p):
    """The float64 reference of a case, computed once and shared."""
    key = (regime, C_in, C_out, relu, with_bias, p)
    if key not in _REFERENCES:
        op = operands(w["n"], C_in, C_out)
        mask = sref.keep(SEED, STREAM, p, w["n"], C_out) if p else None
        _REFERENCES[key] = sref.spectral_ref(w["A"], op["X"], op["W"], op["bias"] if with_bias else None, relu, p, mask, L=w["L"])
    return _REFERENCES[key]


def row_sets(info):
    return (("all", None), ("hub", info["hub"]), ("empty", info["empty"]), ("ragged", info["ragged"]))


def finish_f32(act_P, bias, p, mask):
    """spectral_finish in numpy over the float32 act(P') another entry stored: fl(x - b), kept ? fl(. s) : +0, times 2."""
    b = np.zeros((1, act_P.shape[1]), dtype=np.float32) if bias is None else np.asarray(bias, dtype=np.float32).reshape(1, -1)
    Y = (act_P - b).astype(np.float32)
    if p:
        Y = np.where(mask, Y * sref.scale(p), np.float32(0)).astype(np.float32)
    return (np.float32(2) * Y).astype(np.float32)


# ---- 1. the forward against float64, 2. the gate bits against the float64 sign ----------------------------------------------------------
@pytest.mark.parametrize("p", sref.RATES)
@pytest.mark.parametrize("regime, C_in, C_out", sref.CASES)
def test_forward_and_gate_against_float64(gnntf, world, regime, C_in, C_out, p):
    sparse = gnntf.sparse
    w = world[regime]
    g, info, n = w["g"], w["info"], w["n"]
    op, Xd, Wd, bd = device_operands(n, C_in, C_out)
    mask = sref.keep(SEED, STREAM, p, n, C_out) if p else None
    for relu in (True, False):
        plain_agg = sparse._gcn_launch(w["adj"], Xd, Wd, bd, relu, keep_agg=True)[1]
        for with_bias in (True, False):
            where = f"{regime} {C_in}->{C_out} p={p} relu={relu} bias={with_bias}"
            want = reference(w, regime, C_in, C_out, relu, with_bias, p)
            b = bd if with_bias else None
            rc, out, agg, gate = entry(gnntf, g, Xd, Wd, b, relu, p, vals=w["adj"].vals)
            assert rc == 0, (where, sparse.nat.lib().gnx_last_error())
            assert g.last_kernel() == kernel_name(C_in, C_out, p), (where, g.last_kernel())
            got = host(out)
            assert np.isnan(got[:, C_out:]).all(), where                     # nothing is written past column C_out - 1
            got = got[:, :C_out]
            for name, rows in row_sets(info):
                assert rows is None or len(rows) > 0
                r_out = sref.ratio(got, want["out"], want["out_bound"], rows)
                r_agg = sref.ratio(host(agg), want["agg"], want["agg_bound"], rows)
                print(f"{where} {name} rows: out error / bound = {r_out:.3f}, agg error / bound = {r_agg:.3f}")
                assert r_out <= 1 and r_agg <= 1, (where, name)
            assert np.array_equal(bits(agg), bits(plain_agg)), where         # A . X is bit for bit gnx_gcn_step's
            if p:
                assert not got[~mask].any() and not np.signbit(got[~mask]).any(), where          # dropped values are +0
            # the inference form has the bits of the training form, and writes nothing else
            rc, out_i, none, none_too = entry(gnntf, g, Xd, Wd, b, relu, p, vals=w["adj"].vals, train=False)
            assert rc == 0 and none is None and none_too is None and g.last_kernel() == kernel_name(C_in, C_out, p)
            assert np.array_equal(bits(out_i)[:, :C_out], got.view(np.int32)) and np.isnan(host(out_i)[:, C_out:]).all(), where
            if not relu:
                assert gate is None
                continue
            flags, clear = sref.unpack_gate(host(gate), C_out)
            assert clear, where                                              # pad bits are 0 (the words were all ones before the call)
            if not with_bias:                                                # a NULL bias is a bias of zeros: the gate of act(P') > 0
                assert np.array_equal(flags, got != 0) if p == 0 else True
                continue
            wrong, share = sref.gate_check(flags, want["P"], want["P_bound"])
            print(f"{where}: {wrong} wrong gate bits, {share:.2e} undecided")
            assert wrong == 0 and share <= sref.AMBIGUOUS_SHARE, where
            if C_out >= 2:
                for name, rows in row_sets(info)[1:]:
                    assert flags[rows].any() and not flags[rows].all(), (where, name)
            if p:                                                            # the gate is independent of the mask
                assert np.array_equal(host(gate), host(entry(gnntf, g, Xd, Wd, b, relu, 0.0, vals=w["adj"].vals)[3])), where


def test_seven_columns_into_rows_of_seven(gnntf, world):
    """C_out = 7 with ldo = 7 (single values, a lane that straddles C_out): the [n, 7] block of the padded call, nothing else touched."""
    nat = gnntf.sparse.nat
    w = world["T"]
    n, g, pad = w["n"], w["g"], 64
    _, Xd, Wd, bd = device_operands(n, 64, 7)
    rc, wide, agg_wide, gate_wide = entry(gnntf, g, Xd, Wd, bd, True, 0.5, vals=w["adj"].vals)
    assert rc == 0
    whole = torch.full((pad + n * 7 + pad,), float("nan"), device="cuda")
    agg = torch.empty(n, 64, device="cuda")
    gate = torch.full((n, 1), -1, dtype=torch.int32, device="cuda")
    out = whole[pad:pad + n * 7]
    assert nat.lib().gnx_step_spectral_gcn(g.handle, nat.ptr(w["adj"].vals), nat.ptr(Xd), 64, 64, nat.ptr(Wd), 7, 7, nat.ptr(bd), RELU, 0.5, SEED,
                                           STREAM, nat.ptr(out), 7, nat.ptr(agg), nat.ptr(gate), None, nat.current_stream()) == 0
    torch.cuda.synchronize()
    assert g.last_kernel() == kernel_name(64, 7, 0.5)
    assert bool(whole[:pad].isnan().all()) and bool(whole[pad + n * 7:].isnan().all())
    assert np.array_equal(bits(out.view(n, 7)), bits(wide)[:, :7]) and torch.equal(gate, gate_wide) and torch.equal(agg, agg_wide)
    assert int(host(gate).view(np.uint32).max()) < 128


# ---- 3. bitwise relations ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime, C_in, C_out", sref.CASES)
def test_every_path_forms_the_finished_value_alike(gnntf, world, regime, C_in, C_out):
    """gnx_gcn_step stores act(P') of the same sums -- the tile path for short rows, the long-row kernels and the dense kernel for hub
    rows, gnx_spmm and the dense kernel for the widths without a launch of their own -- so the spectral entry's out is spectral_finish
    of it, bit for bit in every row: the store loop and the row pass share that code.  With bias = 0 (and with NULL) and p = 0 that is
    exactly twice gnx_gcn_step's out; at p = 0.5 the scale is exactly 2 and a kept value is the exact double of the p = 0 value."""
    sparse = gnntf.sparse
    w = world[regime]
    g, info, n = w["g"], w["info"], w["n"]
    op, Xd, Wd, bd = device_operands(n, C_in, C_out)
    zeros = torch.zeros_like(bd)
    mask = sref.keep(SEED, STREAM, 0.5, n, C_out)
    for relu in (True, False):
        for bias, b in ((op["bias"], bd), (np.zeros(C_out, dtype=np.float32), zeros), (None, None)):
            act_P = host(sparse._gcn_launch(w["adj"], Xd, Wd, b, relu, keep_agg=False)[0])
            outs = dict()
            for p in sref.RATES:
                rc, out, _, gate = entry(gnntf, g, Xd, Wd, b, relu, p, vals=w["adj"].vals)
                assert rc == 0
                outs[p] = host(out)[:, :C_out]
                want = finish_f32(act_P, bias, p, mask)
                differ = np.flatnonzero((outs[p].view(np.int32) != want.view(np.int32)).any(axis=1))
                assert len(differ) == 0, (regime, C_in, C_out, relu, p, differ[:8], np.isin(differ, info["hub"]).all())
                if relu:
                    assert np.array_equal(sref.unpack_gate(host(gate), C_out)[0], act_P > 0)
            if bias is None or not bias.any():
                assert np.array_equal(outs[0.0].view(np.int32), (np.float32(2) * act_P).view(np.int32))
            assert np.array_equal(outs[0.5].view(np.int32), np.where(mask, np.float32(2) * outs[0.0], np.float32(0)).view(np.int32))
    assert len(info["hub"]) > 0 and float(np.abs(outs[0.0][info["hub"]]).max()) > 0


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
    plain = gnntf.DeviceGraph(gnntf.SparseCOO(np.stack([rows, cols], axis=1).astype(np.int64), vals, (n, n)), device="cuda:0")
    moved = gnntf.DeviceGraph(gnntf.SparseCOO(np.stack([pi[rows], cols], axis=1).astype(np.int64), vals, (n, n)), device="cuda:0")
    assert plain.n_hub_rows == 0 and moved.n_hub_rows == 0 and (pi // 16 != np.arange(n) // 16).mean() > 0.9
    return plain, moved, pi


@pytest.mark.parametrize("C_in, C_out", [(16, 16), (32, 32), (64, 64), (64, 40), (64, 33), (64, 7), (32, 1), (24, 24)])
def test_rows_keep_their_bits_under_a_row_permutation(gnntf, short, C_in, C_out):
    plain, moved, pi = short
    _, Xd, Wd, bd = device_operands(N_SHORT, C_in, C_out)
    rc, out, agg, gate = entry(gnntf, plain, Xd, Wd, bd, True, 0.0)
    rc_m, out_m, agg_m, gate_m = entry(gnntf, moved, Xd, Wd, bd, True, 0.0)
    assert rc == 0 and rc_m == 0 and plain.last_kernel() == moved.last_kernel() == kernel_name(C_in, C_out, hubs=False)
    assert np.array_equal(bits(agg_m)[pi], bits(agg))
    assert np.array_equal(bits(out_m)[pi][:, :C_out], bits(out)[:, :C_out]) and np.array_equal(host(gate_m)[pi], host(gate))
    assert C_out < 8 or 0.2 < sref.unpack_gate(host(gate), C_out)[0].mean() < 0.8


@pytest.mark.parametrize("C_in, C_out", [(64, 40), (24, 24)])
def test_two_calls_agree_streams_differ_and_the_counter_shifts(gnntf, world, C_in, C_out):
    w = world["T"]
    g, n = w["g"], w["n"]
    _, Xd, Wd, bd = device_operands(n, C_in, C_out)
    run = lambda stream: entry(gnntf, g, Xd, Wd, bd, True, 0.5, vals=w["adj"].vals, stream=stream)
    first, again, other, shifted = run(STREAM), run(STREAM), run(STREAM + 1), run(STREAM + 3)
    for a_, b_ in zip(first[1:], again[1:]):
        assert np.array_equal(bits(a_), bits(b_))
    assert 0.2 < float(((first[1][:, :C_out] != 0) != (other[1][:, :C_out] != 0)).float().mean()) < 0.8
    assert torch.equal(first[3], other[3]) and torch.equal(first[2], other[2])
    counter = torch.tensor([3], dtype=torch.int64, device="cuda")
    g.set_dropout_counter(counter)                       # stream s under a counter of k is stream s + k
    try:
        got = run(STREAM)
    finally:
        g.set_dropout_counter(None)
    assert np.array_equal(bits(got[1]), bits(shifted[1])) and not np.array_equal(bits(got[1]), bits(first[1]))


# ---- 4. under edge dropout: bit for bit the plain entry over the materialised adjacency ---------------------------------------------------
@pytest.mark.parametrize("C_in, C_out", [(64, 40), (32, 7), (24, 24)])
def test_edge_dropout_equals_the_materialised_adjacency(gnntf, dropped_world, C_in, C_out):
    sparse = gnntf.sparse
    e_p = 0.6
    for name in ("t", "a", "T", "dup"):
        d = dropped_world[name]
        g, n = d["g"], d["n"]
        dropped = sparse.DroppedAdjacency(g, e_p, E_SEED, E_STREAM)
        mat = sparse.normalize(g, "symmetric", "none", e_p, E_SEED, E_STREAM)
        _, Xd, Wd, bd = device_operands(n, C_in, C_out)
        hubs = len(d["hub"]) > 0
        for relu in (True, False):
            for p in sref.RATES:
                where = f"{name} {C_in}->{C_out} relu={relu} p={p}"
                rc, out, agg, gate = entry(gnntf, g, Xd, Wd, bd, relu, p, edge=(dropped.D, e_p, E_SEED, E_STREAM))
                assert rc == 0, (where, sparse.nat.lib().gnx_last_error())
                assert g.last_kernel() == kernel_name(C_in, C_out, p, edge=True, hubs=hubs), (where, g.last_kernel())
                assert dropped._vals is None                 # no value array was materialised on the way
                rc, want_out, want_agg, want_gate = entry(gnntf, g, Xd, Wd, bd, relu, p, vals=mat.vals)
                assert rc == 0 and g.last_kernel() == kernel_name(C_in, C_out, p, hubs=hubs), where
                differ = np.flatnonzero((bits(out)[:, :C_out] != bits(want_out)[:, :C_out]).any(axis=1) | (bits(agg) != bits(want_agg)).any(axis=1))
                assert len(differ) == 0, (where, differ[:8], np.isin(differ, d["hub"]).all())
                assert np.isnan(host(out)[:, C_out:]).all()
                assert gate is None or torch.equal(gate, want_gate), where
        if name in ("a", "t"):                               # a row all of whose entries are dropped: agg = 0, P' = bias, out = 2 (act(b) - b)
            rows = d["all_dropped"]
            rc, out, agg, gate = entry(gnntf, g, Xd, Wd, bd, True, 0.0, edge=(dropped.D, e_p, E_SEED, E_STREAM))
            b = host(bd)
            assert float(agg[rows].abs().max()) == 0
            assert np.array_equal(host(out)[rows][:, :C_out], np.tile(2 * (np.maximum(b, 0) - b), (len(rows), 1)))
            assert np.array_equal(sref.unpack_gate(host(gate), C_out)[0][rows], np.tile(b > 0, (len(rows), 1)))


# ---- 5. autograd against float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("backward", ["composed", "fused"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("C_in, C_out", [(64, 40), (24, 24)])
def test_autograd_against_float64(gnntf, world, C_in, C_out, relu, backward, with_bias):
    sparse = gnntf.sparse
    w = world["T"]
    g, n, p = w["g"], w["n"], 0.5
    op = operands(n, C_in, C_out)
    mask = sref.keep(SEED, STREAM, p, n, C_out)
    leaves = [dev(op["X"]).requires_grad_(), dev(op["W"]).requires_grad_()] + ([dev(op["bias"]).reshape(1, C_out).requires_grad_()] if with_bias else [])
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        out = gnntf.gcn_step_spectral(w["adj"], *leaves, relu=relu, dropout=(p, SEED, STREAM), backward=backward)
    assert g.last_kernel() == kernel_name(C_in, C_out, p)
    assert out.grad_fn is not None and type(out.grad_fn).__name__ == "_GCNSpectralStepBackward"
    # what the node keeps: A . X, W and (relu) the gate words -- 4 C_in + C_out / 8 bytes per row; neither act(P') nor out nor a byte mask
    kept = saved + ([out.grad_fn.agg] if backward == "fused" else [])
    assert sum(t.numel() * t.element_size() for t in kept) == sref.saved_bytes(n, C_in, C_out, relu) and len(kept) == (3 if relu else 2)
    agg32 = host([t for t in kept if tuple(t.shape) == (n, C_in) and t.dtype == torch.float32 and t is not leaves[0]][0])
    rc, fwd_out, fwd_agg, fwd_gate = entry(gnntf, g, leaves[0].detach(), leaves[1].detach(), leaves[2].detach() if with_bias else None, relu, p,
                                          vals=w["adj"].vals)
    assert rc == 0 and np.array_equal(bits(out), bits(fwd_out)[:, :C_out]) and np.array_equal(agg32.view(np.int32), bits(fwd_agg))
    flags = None
    if relu:
        words = host([t for t in kept if t.dtype == torch.int32][0])
        assert np.array_equal(words, host(fwd_gate))
        flags = sref.unpack_gate(words, C_out)[0]
    out.backward(dev(op["G"]), retain_graph=backward == "fused")
    if backward == "fused":
        assert out.grad_fn.agg is None                   # A . X was let go: the node runs its backward once
        with pytest.raises(Exception, match="run the forward again"):
            out.backward(dev(op["G"]))
    G32, terms = sref.gate_pass_f32(op["G"], flags, p, mask)
    want = sref.backward_ref(w["A"], agg32, G32, terms, op["W"], L=w["L"])
    ratios = dict()
    for name, leaf in zip(("dX", "dW", "db"), leaves):
        got = host(leaf.grad)
        assert got.shape == tuple(leaf.shape)
        got = got.reshape(want[name].shape if name != "db" else (1, -1))
        if name == "db" and not relu:
            assert not got.any()                         # the identity: + bias and - bias cancel everywhere
            continue
        ratios[name] = sref.ratio(got, want[name].reshape(got.shape), want[name + "_bound"].reshape(got.shape))
        assert float(np.abs(got).max()) > 0
    print(f"autograd {C_in}->{C_out} relu={relu} {backward} bias={with_bias}: error / bound = {ratios}")
    assert all(r <= 1.0 for r in ratios.values()), ratios


def test_saved_bytes_against_the_composed_node_and_a_frozen_input(gnntf, world, monkeypatch):
    sparse = gnntf.sparse
    w = world["T"]
    n, C_in, C_out = w["n"], 64, 40
    op = operands(n, C_in, C_out)

    def saved_by(fn, X_grad=True):
        leaves = [dev(op["X"]).requires_grad_(X_grad), dev(op["W"]).requires_grad_(), dev(op["bias"]).reshape(1, C_out).requires_grad_()]
        saved = dict()
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.setdefault(t.data_ptr(), t), t)[1], lambda t: t):
            out = fn(leaves)
        mine = [t for t in saved.values() if all(t.data_ptr() != leaf.data_ptr() for leaf in leaves)]
        return sum(t.numel() * t.element_size() for t in mine), out, leaves

    fused, _, _ = saved_by(lambda l: gnntf.gcn_step_spectral(w["adj"], *l, relu=True, dropout=(0.5, SEED, STREAM)))
    torch.manual_seed(0)
    composed, _, _ = saved_by(lambda l: sparse._gcn_spectral_composed(w["adj"], *l, True, (0.5, SEED, STREAM)))
    print(f"saved per row beside the inputs: fused {fused / n:.1f} bytes, composed {composed / n:.1f} bytes")
    assert fused == n * (4 * C_in + 8) and composed >= n * (4 * C_in + 4 * C_out + C_out) > fused
    # a frozen X: no dX, and neither gnx_dense nor a transposed launch runs
    for backward in ("composed", "fused"):
        _, out, leaves = saved_by(lambda l: gnntf.gcn_step_spectral(w["adj"], *l, relu=True, dropout=(0.5, SEED, STREAM), backward=backward), X_grad=False)
        with monkeypatch.context() as m:
            for fn in ("_dense_launch", "_gcn_back_launch", "_launch"):
                m.setattr(sparse, fn, lambda *a, **k: pytest.fail("the input gradient ran"))
            out.backward(dev(op["G"]))
        assert leaves[0].grad is None and float(leaves[1].grad.abs().max()) > 0 and float(leaves[2].grad.abs().max()) > 0


# ---- 6. the model ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cora():
    coo, vals, shape, X = graphs.cora_shaped(seed=4)
    labels = np.random.default_rng(4).integers(0, 7, size=shape[0])
    return dict(coo=coo, vals=vals, shape=shape, X=X, labels=labels, train=np.arange(0, 300), valid=np.arange(300, 600))


def make_model(gnntf, cora, **option):
    gnntf.set_seed(11)
    torch.manual_seed(3)
    model = gnntf.GCN(gnntf.SparseCOO(cora["coo"], cora["vals"], cora["shape"]), cora["X"], 7, latent_dims=[64, 64],
                      layer_type=gnntf.GCNSpectralPreservingLayer, **option)
    model.reset()
    rng = np.random.default_rng(12)
    for layer in model.layers():                            # (the biases start at zero: give them values)
        layer.b.data.copy_(dev(rng.uniform(-0.3, 0.3, size=tuple(layer.b.shape)).astype(np.float32)))
    return model


def record_calls(monkeypatch, sparse, graph):
    """Every (function, kernel name) after a call of sparse.spmm / sparse.dense / sparse._gcn_launch, in order."""
    seen = []
    for fn in ("spmm", "dense", "_gcn_launch"):
        def wrapped(*args, _inner=getattr(sparse, fn), _fn=fn, **kwargs):
            result = _inner(*args, **kwargs)
            seen.append((_fn, graph.last_kernel()))
            return result
        monkeypatch.setattr(sparse, fn, wrapped)
    return seen


def test_model_eval_logits_against_float64(gnntf, cora, monkeypatch):
    fused, default = make_model(gnntf, cora, gcn_spectral="fused"), make_model(gnntf, cora)
    assert default.gcn_spectral == "composed" and fused.gcn_spectral == "fused"
    logits = dict()
    for name, model in (("fused", fused), ("default", default)):
        seen = record_calls(monkeypatch, gnntf.sparse, model.graph)
        model.training_mode(False)
        with torch.no_grad():
            logits[name] = host(model(model.features))
        monkeypatch.undo()
        if name == "fused":                                 # the first layer gathers at the feature width: today's two launches
            assert [fn for fn, _ in seen] == ["spmm", "dense", "_gcn_launch", "_gcn_launch"]
            assert [k for _, k in seen[2:]] == [kernel_name(64, 64, hubs=False)] * 2
        else:                                               # without the keyword: today's calls, layer by layer
            assert [fn for fn, _ in seen] == ["spmm", "dense"] * 3 and not any("gcn" in k for _, k in seen)
            default_seen = seen
    for option in (dict(gcn_spectral="composed"), dict(gcn_layer="fused", gcn_backward="fused")):      # today's calls and bits
        named = make_model(gnntf, cora, **option)
        seen = record_calls(monkeypatch, gnntf.sparse, named.graph)
        named.training_mode(False)
        with torch.no_grad():
            assert np.array_equal(host(named(named.features)), logits["default"])
        monkeypatch.undo()
        assert seen == default_seen
    # float64 with the same weights, the bound propagated layer by layer: E_l = 2 (|A| E_(l-1)) |W_l| + the layer's own bound
    g = fused.graph
    A = weights_csr(g, fused.get_adjacency(0).vals)
    H, E = cora["X"].astype(np.float64), np.zeros(cora["X"].shape)
    for layer in [l for l in fused.layers() if isinstance(l, gnntf.GCNSpectralPreservingLayer)]:
        Wl, bl = host(layer.W), host(layer.b).reshape(-1)
        own = sref.spectral_ref(A, H, Wl, bl, True, L=g.long_row_threshold)
        H, E = own["out"], 2 * ((abs(A) @ E) @ np.abs(Wl.astype(np.float64))) + own["out_bound"]
    for name in ("fused", "default"):
        worst = sref.ratio(logits[name], H, E)
        print(f"{name}: eval logits error / propagated bound = {worst:.3f}")
        assert worst <= 1
    assert float(np.abs(H).max()) > 0


def three_steps(gnntf, cora, model):
    task = gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]])
    losses, grads, kernels = [], [], set()
    first = model._mask_calls
    torch.manual_seed(9)
    for _ in range(3):
        with model:
            for v in model.vars():
                v.var.grad = None
            loss = task.loss(model(model.features))
            kernels.add(model.graph.last_kernel())
            loss.backward()
        losses.append(float(loss.detach()))
        grads.append([v.var.grad.clone() for v in model.vars()])
        with torch.no_grad():
            for v in model.vars():
                v.var -= 0.05 * v.var.grad
    return losses, grads, model._mask_calls - first, kernels


@pytest.mark.parametrize("backward", ["composed", "fused"])
def test_model_training_is_reproducible_from_the_seed(gnntf, cora, backward):
    option = dict(gcn_spectral="fused", gcn_backward=backward)
    one = three_steps(gnntf, cora, make_model(gnntf, cora, **option))
    two = three_steps(gnntf, cora, make_model(gnntf, cora, **option))
    # per step: the adjacencies of the two latent layers, and the mask of the second (the first, at the feature width, keeps torch's)
    assert one[2] == two[2] == 3 * 3
    assert one[0] == two[0] and all(np.isfinite(one[0])) and len(set(one[0])) == 3
    for step_one, step_two in zip(one[1], two[1]):
        assert len(step_one) == 6 and all(torch.equal(a_, b_) for a_, b_ in zip(step_one, step_two))
        assert all(float(a_.abs().max()) > 0 for a_ in step_one)
    assert one[3] == {kernel_name(64, 7, hubs=False)}       # the last layer: no edge dropout, no mask
    model = make_model(gnntf, cora, **option)
    gnntf.set_seed(12)                                      # the same parameters, other masks
    assert three_steps(gnntf, cora, model)[0] != one[0]
    composed = three_steps(gnntf, cora, make_model(gnntf, cora))
    assert composed[2] == 3 * 2 and not any("gcn" in k for k in composed[3])


def test_captured_training_equals_eager(gnntf, cora, monkeypatch):
    """train(capture=True) for 3 epochs, bit for bit the eager run (the pattern of tests/test_gpu_gcn_fused.py)."""
    from gnntf import training
    observed, observe = [], training._BestSoFar.observe
    monkeypatch.setattr(training._BestSoFar, "observe", lambda self, loss: (observed[-1].append(loss), observe(self, loss))[1])
    results = []
    for capture in (False, True):
        observed.append([])
        model = make_model(gnntf, cora, gcn_spectral="fused")
        # (every layer's dropout from the counter RNG: the first layer's, at the feature width, is torch's -- none of it under capture)
        layers = [l for l in model.layers() if isinstance(l, gnntf.GCNLayer)]
        layers[0].dropout = 0
        gnntf.set_seed(11)
        torch.manual_seed(5)
        valid = gnntf.NodeClassification(cora["valid"], cora["labels"][cora["valid"]])
        model.train(train=gnntf.NodeClassification(cora["train"], cora["labels"][cora["train"]]), valid=valid, epochs=3, patience=50,
                    capture=capture, optimizer=lambda params: torch.optim.Adam(params, lr=0.01, eps=1e-7, capturable=True))
        results.append(([v.var.detach().clone() for v in model.vars()], float(model.loss(valid)), model._mask_calls))
    (eager, eager_loss, eager_masks), (captured, captured_loss, captured_masks) = results
    assert eager_masks == captured_masks == 3 * 3
    assert all(torch.equal(e, c) for e, c in zip(eager, captured))
    assert eager_loss == captured_loss
    assert len(observed[0]) == len(observed[1]) == 3 and observed[0] == observed[1] and len(set(observed[0])) == 3


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_write_nothing(gnntf, world):
    nat = gnntf.sparse.nat
    lib = nat.lib()
    w = world["T"]
    g, n = w["g"], w["n"]
    _, Xd, Wd, bd = device_operands(n, 64, 40)
    SENTINEL = 1234.5
    out, agg, work = (torch.full(shape, SENTINEL, device="cuda") for shape in ((n, 40), (n, 64), (n, 64)))
    gate = torch.full((n, 2), 77, dtype=torch.int32, device="cuda")

    def step(X=Xd, W=Wd, b=bd, out_=out, ldo=40, agg_=agg, gate_=gate, work_=None, act=RELU, rate=0.5, C_in=64, C_out=40):
        return lib.gnx_step_spectral_gcn(g.handle, nat.ptr(w["adj"].vals), nat.ptr(X), X.stride(0), C_in, nat.ptr(W), W.stride(0), C_out, nat.ptr(b),
                                         act, rate, SEED, STREAM, nat.ptr(out_), ldo, nat.ptr(agg_), nat.ptr(gate_), nat.ptr(work_),
                                         nat.current_stream())

    def refused(rc, *causes, name=b"gnx_step_spectral_gcn"):
        message = lib.gnx_last_error()
        assert rc == -1 and name in message and all(c in message for c in causes), message
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in (out, agg, work)) and bool((gate == 77).all())

    refused(step(gate_=None), b"relu with d_agg (training) needs d_gate")
    refused(step(gate_=agg), b"d_gate must be a buffer of its own")
    refused(step(gate_=out), b"d_gate must be a buffer of its own")
    refused(step(gate_=Xd), b"d_gate must be a buffer of its own")
    refused(step(gate_=work, work_=work), b"d_gate must be a buffer of its own")
    refused(step(out_=Xd, ldo=64), b"out must not alias an input")
    refused(step(agg_=Xd), b"d_agg must be a buffer of its own")
    refused(step(agg_=out), b"d_agg must be a buffer of its own")
    refused(step(work_=agg), b"d_work must be a buffer of its own")
    refused(step(ldo=39), b"ldo 39 < C_out 40")
    refused(step(rate=1.0), b"dropout rate 1 outside [0, 1)")
    refused(step(act=2), b"invalid activation 2")
    # a missing d_agg / d_work where rows pass through memory: the message says which case needs it
    refused(step(agg_=None, gate_=None), b"needs d_agg or d_work", b"hub rows")
    op24, X24, W24, b24 = device_operands(n, 24, 24)
    out24 = torch.full((n, 24), SENTINEL, device="cuda")
    refused(step(X=X24, W=W24, b=b24, out_=out24, ldo=24, agg_=None, gate_=None, C_in=24, C_out=24), b"needs d_agg or d_work", b"C_in is not 16, 32 or 64")
    assert bool((out24 == SENTINEL).all())
    _, X16, W16, b16 = device_operands(n, 16, 32)
    out32 = torch.full((n, 32), SENTINEL, device="cuda")
    refused(step(X=X16, W=W16, b=b16, out_=out32, ldo=32, agg_=None, gate_=None, C_in=16, C_out=32), b"needs d_agg or d_work", b"C_out > C_in")
    assert bool((out32 == SENTINEL).all())
    D = torch.ones(n, device="cuda")

    def dropped_step(edge_p=0.5, D_=D, gate_=gate):
        return lib.gnx_step_spectral_gcn_dropped(g.handle, nat.ptr(D_), edge_p, E_SEED, E_STREAM, nat.ptr(Xd), 64, 64, nat.ptr(Wd), 40, 40, nat.ptr(bd),
                                                 RELU, 0.0, SEED, STREAM, nat.ptr(out), 40, nat.ptr(agg), nat.ptr(gate_), None, nat.current_stream())

    refused(dropped_step(edge_p=1.0), b"outside [0, 1)", name=b"gnx_step_spectral_gcn_dropped")
    refused(dropped_step(D_=None), b"NULL degree scales", name=b"gnx_step_spectral_gcn_dropped")
    refused(dropped_step(gate_=None), b"needs d_gate", name=b"gnx_step_spectral_gcn_dropped")
    assert step() == 0 and dropped_step() == 0           # the calls themselves are well formed
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any()) and not bool((agg == SENTINEL).any()) and not bool((gate == 77).all())
    # the identity has no gate: d_gate is not looked at, and inference with d_work alone is enough
    assert step(act=NONE, gate_=None) == 0 and step(agg_=None, gate_=None, work_=work) == 0
