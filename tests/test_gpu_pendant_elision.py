"""Pendant elision of the K loop on the MI355X (gnx_graph_set_pendant_elision, gnx_graph_pendant_elision): a row whose one entry points
at a row that alone points back is launched in the last iteration only, and its neighbour forms the iterates between from H0, the
entry's value and its own row of two iterations ago -- with the operations the row's own launch ran.  So every comparison here is
torch.equal on the int32 views of the float32 results against the same handle with elision off."""
import numpy as np
import pytest
import torch

import graphs
import pendant_graphs as pg

pytestmark = pytest.mark.gpu

A = 0.1
COLD = np.int32(-2 ** 31)


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def expected_hints(rowptr, colidx, hot_rows):
    degree = np.diff(rowptr)
    order = np.lexsort((np.arange(len(degree)), -degree))
    hot = np.zeros(len(degree), dtype=bool)
    hot[order[:hot_rows]] = True
    return np.where(hot[colidx], colidx, colidx | COLD).astype(np.int32)


def special_features(n, C, seed, pendants, neighbours, hubs):
    """U(-1, 1) with rows of +0 and of -0 (a pendant, the neighbour of a pendant and a hub each), and one NaN and one Inf in a pendant
    and in a hub."""
    H0 = np.random.default_rng(seed).uniform(-1, 1, size=(n, C)).astype(np.float32)
    H0[[pendants[0], neighbours[1], hubs[0]]] = 0.0
    H0[[pendants[2], neighbours[3], hubs[-1]]] = -0.0
    H0[pendants[4], 1] = np.nan
    H0[pendants[5], C - 1] = np.inf
    H0[hubs[0], 2] = np.nan
    H0[hubs[-1], 3] = np.inf
    return H0


@pytest.fixture(scope="module")
def cases(gnntf):
    """name -> the handle, its values, the sorted CSR on the host, the elidable rows restated in numpy, and features per width.
    "rmat": 40 000 vertices, hub rows above 128 entries in the short rows' launch.  "hand": pendant_graphs.hand_built_csr in 2^20
    vertices, short rows and hub chunks in launches of their own."""
    out = {}
    coo, vals, shape = graphs.rmat_symmetric_coo(40000, 300000, seed=3)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    adj = gnntf.normalize(g, "symmetric")
    assert g.n_hub_rows > 0 and g.long_row_threshold == 128
    rowptr, colidx, _ = (t.cpu().numpy() for t in g.csr_arrays())
    out["rmat"] = dict(g=g, vals=adj.vals, rowptr=rowptr, colidx=colidx, merged=True)
    rowptr, colidx, vals, shape, named = pg.hand_built_csr()
    g = gnntf.DeviceGraph(csr=(dev(rowptr), dev(colidx), dev(vals), shape))
    assert g.n_hub_rows == 1 and g.long_row_threshold == 512
    out["hand"] = dict(g=g, vals=dev(vals), rowptr=rowptr, colidx=colidx, merged=False, named=named)
    for case in out.values():
        rowptr, colidx = case["rowptr"], case["colidx"]
        n = len(rowptr) - 1
        degree = np.diff(rowptr)
        case["n"] = n
        case["elidable"] = pg.elidable_rows(rowptr, colidx)
        pendants = np.flatnonzero(case["elidable"])
        neighbours = colidx[rowptr[pendants]]
        hubs = np.flatnonzero(degree > case["g"].long_row_threshold)
        assert len(pendants) >= 6 and len(hubs) >= 1
        case["H0"] = {C: dev(special_features(n, C, C, pendants, neighbours, hubs)) for C in (256, 128, 64, 8)}
    assert np.array_equal(out["hand"]["elidable"], pg.expected_elidable(out["hand"]["named"], out["hand"]["n"]))
    return out


def propagate(gnntf, case, C, K, relu):
    """gnx_appnp_propagate_act straight, `out` and `work` full of NaN beforehand; (out, work)"""
    nat = gnntf.sparse.nat
    H0 = case["H0"][C]
    out = torch.full_like(H0, float("nan"))
    work = torch.full_like(H0, float("nan"))
    nat.check(nat.lib().gnx_appnp_propagate_act(case["g"].handle, nat.ptr(case["vals"]), None, nat.ptr(H0), A, K, C,
                                                nat.ACT_RELU if relu else nat.ACT_NONE, nat.ptr(out), nat.ptr(work), nat.current_stream()))
    torch.cuda.synchronize()
    return out, work


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", ["rmat", "hand"])
def test_plan_is_the_numpy_restatement_and_the_hints_keep_their_array(gnntf, cases, name):
    case = cases[name]
    g = case["g"]
    g.set_gather_hints(64)
    g.set_pendant_elision(1)
    rows, last = g.pendant_elision()
    assert rows is not None and not last
    assert np.array_equal(rows.cpu().numpy(), case["elidable"]) and case["elidable"].sum() > 0
    propagate(gnntf, case, 128, 3, False)
    assert g.pendant_elision()[1]
    cols, hot = g.gather_hints()
    assert hot == 64 and np.array_equal(cols.cpu().numpy(), expected_hints(case["rowptr"], case["colidx"], 64))
    rowptr, colidx, _ = (t.cpu().numpy() for t in g.csr_arrays())
    assert np.array_equal(rowptr, case["rowptr"]) and np.array_equal(colidx, case["colidx"])
    g.set_pendant_elision(0)
    g.set_gather_hints(0)


@pytest.mark.parametrize("C", [128, 64])
@pytest.mark.parametrize("name", ["rmat", "hand"])
def test_k_loop_is_bitwise_the_one_without_elision(gnntf, cases, name, C):
    case = cases[name]
    g, n = case["g"], case["n"]
    elidable = dev(case["elidable"])
    for hot_rows in (1, 64, n):
        g.set_gather_hints(hot_rows)
        for K in (1, 2, 3, 4):
            for relu in (False, True):
                what = (name, C, hot_rows, K, relu)
                g.set_pendant_elision(0)
                want, _ = propagate(gnntf, case, C, K, relu)
                plain = g.last_kernel()
                assert not g.pendant_elision()[1] and g.last_launch_hot_rows() == hot_rows, what
                g.set_pendant_elision(1)
                got, work = propagate(gnntf, case, C, K, relu)
                assert g.pendant_elision()[1] == (K >= 2), what
                assert g.last_kernel() == plain and ("+chunks" in plain) == case["merged"] and g.last_launch_hot_rows() == hot_rows, what
                assert same_bits(got, want), what
                if K >= 2:      # no buffer between receives an elidable row
                    assert bool(torch.isnan(work[elidable]).all()), what
                if K == 4 and not relu:
                    assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any()) and bool(torch.isfinite(want).any()), what
    g.set_pendant_elision(0)
    g.set_gather_hints(0)


@pytest.mark.parametrize("C", [256, 8])
@pytest.mark.parametrize("name", ["rmat", "hand"])
def test_other_widths_keep_their_kernels(gnntf, cases, name, C):
    case = cases[name]
    g = case["g"]
    g.set_gather_hints(64)
    g.set_pendant_elision(0)
    want, _ = propagate(gnntf, case, C, 3, False)
    plain = g.last_kernel()
    g.set_pendant_elision(1)
    got, _ = propagate(gnntf, case, C, 3, False)
    assert not g.pendant_elision()[1] and g.last_kernel() == plain
    assert same_bits(got, want)
    g.set_pendant_elision(0)
    g.set_gather_hints(0)


def test_layer_path_is_bitwise_the_c_entry(gnntf, cases):
    """APPNP's K PPRIteration layers, run by the container's loop in eval mode, with elision on: the C entry's bits."""
    case = cases["rmat"]
    n, C, K = case["n"], 128, 4
    coo, vals, shape = graphs.rmat_symmetric_coo(40000, 300000, seed=3)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    gnntf.set_seed(0)
    model = gnntf.APPNP(g, torch.zeros(n, 1, device="cuda"), num_classes=C, latent_dims=[], iterations=K, a=A)
    model.training_mode(False)
    first = len(model.layers()) - K
    H0 = case["H0"][C]
    model.layers()[first - 1].value = H0
    adj = model.get_adjacency(0.5)
    g.set_gather_hints(64)
    g.set_pendant_elision(1)
    with torch.no_grad():
        model.run(H0, first=first)
    got = model.layers()[-1].value
    assert g.pendant_elision()[1]
    direct, _ = propagate(gnntf, dict(g=g, vals=adj.vals, H0={C: H0}), C, K, False)
    assert g.pendant_elision()[1] and same_bits(got, direct)
    g.set_pendant_elision(0)
    want, _ = propagate(gnntf, dict(g=g, vals=adj.vals, H0={C: H0}), C, K, False)
    assert not g.pendant_elision()[1] and same_bits(got, want)
