"""Gather hints of the wide float32 eval launches on the MI355X (gnx_graph_set_gather_hints, gnx_graph_gather_hints,
GNX_RESERVE_GATHER_HINTS): per entry the column with bit 31 set where the column is not one of the hot rows, and kernels that gather
such a row with a non-temporal load.  A hint changes which cache lines survive, never a value: same entries, same order, same fused
multiply-adds, so every comparison of results here is torch.equal on float32 bits against the unhinted launch."""
import numpy as np
import pytest
import torch

import graphs

pytestmark = pytest.mark.gpu

COLD = np.int32(-2 ** 31)
WIDTHS = (256, 128, 64)           # one wave per row; 32-lane groups; 16-lane groups
A = 0.1


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def expected_hints(g, hot_rows):
    """colidx | sign for every column outside the hot_rows rows with the most stored entries, ties to the smaller id"""
    rowptr, colidx, _ = (t.cpu().numpy() for t in g.csr_arrays())
    degree = np.diff(rowptr)
    order = np.lexsort((np.arange(len(degree)), -degree))
    hot = np.zeros(len(degree), dtype=bool)
    hot[order[:hot_rows]] = True
    return np.where(hot[colidx], colidx, colidx | COLD).astype(np.int32)


@pytest.fixture(scope="module")
def rmat(gnntf):
    """Symmetric R-MAT of 40 000 vertices (between 2^15 and 2^20 rows: rows above 128 entries are cut into chunks that share the short
    rows' launch), its normalised adjacency, and per width the unhinted propagation: made once, never changed."""
    coo, vals, shape = graphs.rmat_symmetric_coo(40000, 300000, seed=3)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    assert g.n_hub_rows > 0 and g.long_row_threshold == 128
    adj = gnntf.normalize(g, "symmetric")
    g.set_gather_hints(0)
    want, names = {}, {}
    for C in WIDTHS:
        H0 = dev(np.random.default_rng(C).uniform(-1, 1, size=(shape[0], C)).astype(np.float32))
        want[C] = (H0, gnntf.appnp_propagate(adj, H0, a=A, iterations=3))
        names[C] = g.last_kernel()
        # (the sub-wave kernels take the chunks into the short rows' launch and say so; one wave per row leaves them to the chunk kernels)
        assert g.last_launch_hot_rows() == 0 and ("+chunks" in names[C]) == (C <= 128)
    return dict(g=g, adj=adj, want=want, names=names, n=shape[0])


def test_hinted_array_is_colidx_with_the_cold_bit(rmat):
    g = rmat["g"]
    g.set_gather_hints(0)
    assert g.gather_hints() == (None, 0)
    g.set_gather_hints(64)
    cols, hot = g.gather_hints()
    assert hot == 64 and cols.dtype == torch.int32
    want = expected_hints(g, 64)
    assert np.array_equal(cols.cpu().numpy(), want)
    assert 0 < int((want >= 0).sum()) < len(want)                  # both kinds occur
    g.set_gather_hints(0)
    assert g.gather_hints() == (None, 0)


@pytest.mark.parametrize("C", WIDTHS)
def test_propagation_is_bitwise_the_unhinted_one(gnntf, rmat, C):
    g, adj = rmat["g"], rmat["adj"]
    H0, want = rmat["want"][C]
    for hot_rows in (0, 64, rmat["n"]):
        g.set_gather_hints(hot_rows)
        got = gnntf.appnp_propagate(adj, H0, a=A, iterations=3)
        name = g.last_kernel()
        assert torch.equal(got, want), (C, hot_rows)
        assert name == rmat["names"][C], name                      # the class keeps its name; the handle says what the launch took
        assert g.last_launch_hot_rows() == hot_rows
    g.set_gather_hints(0)
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0


def test_another_hot_rows_marks_the_same_array_again(gnntf, rmat):
    g = rmat["g"]
    g.set_gather_hints(0)
    g.set_gather_hints(100)
    cols, hot = g.gather_hints()
    assert hot == 100 and np.array_equal(cols.cpu().numpy(), expected_hints(g, 100))
    g.set_gather_hints(7)
    cols, hot = g.gather_hints()
    assert hot == 7 and np.array_equal(cols.cpu().numpy(), expected_hints(g, 7))
    g.set_gather_hints(0)


def test_fused_dropout_launch_keeps_the_plain_columns(gnntf, rmat):
    """gnx_spmm_dropped hashes the column of every entry: it must never see a hinted one."""
    g = rmat["g"]
    D = gnntf.sparse.dropped_degree_scales(g, 0.5, 0x5EED, 3, 1)
    H0, _ = rmat["want"][128]
    outs = []
    for hot_rows in (0, 64):
        g.set_gather_hints(hot_rows)
        adj = gnntf.sparse.DroppedAdjacency(g, 0.5, 0x5EED, 3, D=D[0])
        outs.append(gnntf.sparse._launch(adj, H0, H0, 1.0 - A, A, gnntf.sparse.nat.ACT_NONE))
        assert "_drop" in g.last_kernel() and g.last_launch_hot_rows() == 0
    g.set_gather_hints(0)
    assert torch.equal(outs[0], outs[1]) and float(outs[0].abs().max()) > 0


def hand_built_csr():
    """1 024 vertices; the 64 vertices 0, 8, ..., 504 have the longest rows (130 ... 193 entries) and are the hot ones at hot_rows =
    64.  Their rows, and the test rows below, list columns 0, 1, 8, 9, 16, 17, ...: hot and cold alternate inside every batch of four.
    Test rows (all at cold vertices): lengths 1, 2, 3, 5, 7 starting hot and starting cold, 129 (32 whole batches and one entry), and
    three consecutive rows of six entries that are all hot, all cold, all hot -- rows of one length are neighbours in the launch
    order, so two of them share a wave whichever way the pairs fall."""
    n = 1024
    alternating = np.array([[8 * i, 8 * i + 1] for i in range(64)]).ravel()            # 128 columns, hot first
    rows = {}
    for k in range(64):
        rows[8 * k] = np.concatenate([alternating, 600 + np.arange(2 + k)])              # 130 + k entries
    vertex = 515
    for length in (1, 2, 3, 5, 7):
        rows[vertex] = alternating[:length]; vertex += 2                                 # starts hot
        rows[vertex] = alternating[1:1 + length]; vertex += 2                            # starts cold
    rows[vertex] = np.concatenate([alternating, [700]])                                  # 129 entries
    rows[601], rows[602], rows[603] = 8 * np.arange(6), 1 + np.arange(6), 8 * np.arange(6, 12)
    lengths = np.array([len(rows.get(r, ())) for r in range(n)])
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    colidx = np.concatenate([np.sort(rows[r]) for r in sorted(rows)]).astype(np.int32)
    vals = np.random.default_rng(5).uniform(0.5, 1.5, size=len(colidx)).astype(np.float32)
    return rowptr, colidx, vals, (n, n), lengths


@pytest.mark.parametrize("C", WIDTHS)
def test_hand_built_rows(gnntf, C):
    rowptr, colidx, vals, shape, lengths = hand_built_csr()
    g = gnntf.DeviceGraph(csr=(dev(rowptr), dev(colidx), dev(vals), shape))
    adj = gnntf.sparse.Adjacency(g, dev(vals))
    rng = np.random.default_rng(C)
    X, H0 = dev(rng.standard_normal((shape[0], C)).astype(np.float32)), dev(rng.standard_normal((shape[0], C)).astype(np.float32))
    g.set_gather_hints(0)
    want = gnntf.sparse._launch(adj, X, H0, 1.0 - A, A, gnntf.sparse.nat.ACT_NONE)
    plain = g.last_kernel()
    g.set_gather_hints(64)
    cols, hot = g.gather_hints()
    hinted = cols.cpu().numpy()
    assert hot == 64 and np.array_equal(hinted, expected_hints(g, 64))
    assert np.array_equal(hinted < 0, (colidx % 8 != 0) | (colidx >= 512))     # exactly the multiples of 8 below 512 are hot
    got = gnntf.sparse._launch(adj, X, H0, 1.0 - A, A, gnntf.sparse.nat.ACT_NONE)
    assert g.last_kernel() == plain and g.last_launch_hot_rows() == 64
    assert torch.equal(got, want)
    # and against float64: the unhinted launch is what it should be (one row per test length)
    ref = np.zeros((shape[0], C))
    Xh = X.cpu().numpy().astype(np.float64)
    for r in np.flatnonzero(lengths):
        sl = slice(rowptr[r], rowptr[r + 1])
        ref[r] = vals[sl].astype(np.float64) @ Xh[colidx[sl]]
    ref = (1.0 - A) * ref + A * H0.cpu().numpy()
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-4, atol=1e-4)


def test_big_structure_plan_and_the_automatic_rule_below_its_size(gnntf):
    """2^20 + 1000 rows / 10M entries: the big-structure plan (hub rows in launches of their own).  The automatic rule is off
    below 2^25 rows; hints that are asked for apply."""
    n = (1 << 20) + 1000
    coo, vals, shape = graphs.rmat_symmetric_coo(n, 5_000_000, seed=11)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    adj = gnntf.normalize(g, "symmetric")
    C = 128
    H0 = dev(np.random.default_rng(1).uniform(-1, 1, size=(n, C)).astype(np.float32))
    g.set_gather_hints(0)
    want = gnntf.appnp_propagate(adj, H0, a=A, iterations=2)
    plain = g.last_kernel()
    assert g.n_hub_rows > 0 and g.long_row_threshold == 512 and "+chunks" not in plain
    g.set_gather_hints(-1)
    g.reserve(C, gather_hints=True)
    assert torch.equal(gnntf.appnp_propagate(adj, H0, a=A, iterations=2), want)
    assert g.last_kernel() == plain and g.gather_hints() == (None, 0) and g.last_launch_hot_rows() == 0
    g.set_gather_hints(4096)
    got = gnntf.appnp_propagate(adj, H0, a=A, iterations=2)
    assert g.last_kernel() == plain and g.last_launch_hot_rows() == 4096
    assert torch.equal(got, want)
    cols, hot = g.gather_hints()
    assert hot == 4096 and np.array_equal(cols.cpu().numpy(), expected_hints(g, hot))
    narrow = dev(np.random.default_rng(2).uniform(-1, 1, size=(n, 32)).astype(np.float32))
    gnntf.appnp_propagate(adj, narrow, a=A, iterations=1)          # rows of 128 bytes: never hinted
    assert g.last_launch_hot_rows() == 0


def test_automatic_rule_from_2_25_rows(gnntf):
    """2^25 + 8 rows of one entry each (made on the device): the automatic rule is on, the rows that fill 256 MiB at the width of the
    call are hot -- all rows have one entry, so those are the smallest ids -- built by the first launch or by reserve."""
    n, C = (1 << 25) + 8, 64
    rowptr = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    colidx = ((torch.arange(n, dtype=torch.int64, device="cuda") * 7919 + 13) % n).to(torch.int32)
    vals = torch.full((n,), 0.5, dtype=torch.float32, device="cuda")
    g = gnntf.DeviceGraph(csr=(rowptr, colidx, vals, (n, n)))
    adj = gnntf.sparse.Adjacency(g, vals)
    H0 = torch.rand(n, C, device="cuda") * 2 - 1
    g.set_gather_hints(0)
    want = gnntf.appnp_propagate(adj, H0, a=A, iterations=1)
    plain = g.last_kernel()
    g.set_gather_hints(-1)
    assert g.gather_hints() == (None, 0)                           # automatic: nothing is built before a launch or reserve asks
    g.reserve(C, gather_hints=True)
    cols, hot = g.gather_hints()
    assert hot == (256 << 20) // (4 * C) == 1 << 20
    assert torch.equal(cols, torch.where(colidx < hot, colidx, colidx | torch.tensor(-2 ** 31, dtype=torch.int32, device="cuda")))
    got = gnntf.appnp_propagate(adj, H0, a=A, iterations=1)
    assert g.last_kernel() == plain and g.last_launch_hot_rows() == hot
    assert torch.equal(got, want) and float(want.abs().max()) > 0


def test_non_square_handles_and_vertex_blocks_get_no_array(gnntf):
    nat = gnntf.sparse.nat
    coo, vals, shape = graphs.random_coo(100, 200, 900, seed=1)
    rect = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    rect.set_gather_hints(8)
    assert rect.gather_hints() == (None, 0)
    X = dev(np.random.default_rng(0).standard_normal((200, 64)).astype(np.float32))
    gnntf.spmm(gnntf.sparse.Adjacency(rect, None), X)
    assert rect.last_launch_hot_rows() == 0
    coo, vals, shape = graphs.random_coo(300, 300, 3000, seed=2)
    block = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    block.set_gather_hints(8)
    assert block.gather_hints()[1] == 8
    gid = torch.arange(300, dtype=torch.int32, device="cuda")
    nat.check(nat.lib().gnx_graph_set_block(block.handle, 0, 0, nat.ptr(gid), nat.current_stream()))
    assert block.gather_hints() == (None, 0)
    X = dev(np.random.default_rng(0).standard_normal((300, 64)).astype(np.float32))
    gnntf.spmm(gnntf.sparse.Adjacency(block, None), X)
    assert block.last_launch_hot_rows() == 0
