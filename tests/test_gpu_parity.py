"""Parity of the HIP path (through the C ABI) against the CPU oracle, on the GPU box.
Tolerance: float32 logits within rtol 1e-4 (BASELINE.json north_star) + atol 1e-5 for sums that
cancel; argmax identical on every row; integer structure (CSR) bit-exact."""
import os

import numpy as np
import pytest
import torch

import graphs
from oracle import gnntf_oracle as orc

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def make_graph(gnntf, coo, vals, shape):
    return gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")


# ---- A0: COO -> coalesced CSR is bit-exact ------------------------------------------------------
@pytest.mark.parametrize("shape,nnz", [((1, 1), 1), ((7, 5), 23), ((300, 300), 5000), ((2000, 1500), 60000)])
def test_csr_structure_bit_exact(gnntf, shape, nnz):
    coo, vals, shape = graphs.random_coo(shape[0], shape[1], nnz, seed=nnz, weighted=True, dup_frac=0.3)
    g = make_graph(gnntf, coo, vals, shape)
    rowptr, colidx, cvals, rows = g.csr_arrays(with_rows=True)
    wr, wc, wv = orc.coo_to_csr_coalesced(coo, vals, shape)
    assert g.nnz_entries == len(vals) and g.nnz == len(wc)
    np.testing.assert_array_equal(rowptr.cpu().numpy(), wr)
    np.testing.assert_array_equal(colidx.cpu().numpy(), wc)
    np.testing.assert_array_equal(cvals.cpu().numpy(), wv)     # duplicates summed in input order: same float32 bits
    np.testing.assert_array_equal(rows.cpu().numpy(), np.repeat(np.arange(shape[0]), np.diff(wr)))


def test_empty_and_invalid_graphs(gnntf):
    g = make_graph(gnntf, np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.float32), (5, 5))
    assert g.nnz == 0
    adj = gnntf.normalize(g, "symmetric")
    H = torch.ones(5, 3, device="cuda")
    assert float(gnntf.spmm(adj, H).abs().sum()) == 0
    out = gnntf.appnp_propagate(adj, H, a=0.25, iterations=3)
    np.testing.assert_allclose(out.cpu().numpy(), 0.25 * np.ones((5, 3)), rtol=1e-7)
    with pytest.raises(Exception, match="outside the 4 x 4 shape"):
        make_graph(gnntf, np.array([[0, 1], [4, 0]]), np.ones(2, dtype=np.float32), (4, 4))
    with pytest.raises(Exception, match="Invalid matrix normalization"):
        gnntf.normalize(g, "row")
    with pytest.raises(Exception, match="expects 5"):
        gnntf.spmm(adj, torch.ones(6, 3, device="cuda"))


def test_c_abi_argument_errors_on_device(gnntf):
    """Error convention of the boundary: int status + thread-local message, never a crash."""
    from ctypes import byref, c_void_p
    from gnntf import _native as nat
    lib = nat.lib()
    coo, vals, shape = graphs.random_coo(50, 50, 300, seed=2)
    g = make_graph(gnntf, coo, vals, shape)
    X = torch.rand(50, 16, device="cuda"); out = torch.empty_like(X)
    s = nat.current_stream()
    call = lambda *a: lib.gnx_spmm(g.handle, None, None, *a)
    assert call(nat.ptr(X), 16, 16, None, 0, 1.0, 0.0, 0, nat.ptr(X), 16, s) == -1 and b"alias" in lib.gnx_last_error()
    assert call(nat.ptr(X), 8, 16, None, 0, 1.0, 0.0, 0, nat.ptr(out), 16, s) == -1 and b"leading dimension" in lib.gnx_last_error()
    assert call(nat.ptr(X), 16, 0, None, 0, 1.0, 0.0, 0, nat.ptr(out), 16, s) == -1 and b"feature width" in lib.gnx_last_error()
    assert call(nat.ptr(X), 16, 16, None, 0, 1.0, 0.0, 7, nat.ptr(out), 16, s) == -1 and b"activation" in lib.gnx_last_error()
    assert call(None, 16, 16, None, 0, 1.0, 0.0, 0, nat.ptr(out), 16, s) == -1 and b"NULL" in lib.gnx_last_error()
    assert lib.gnx_appnp_propagate(g.handle, None, None, nat.ptr(X), 0.1, 3, 16, nat.ptr(X), nat.ptr(out), s) == -1
    assert b"distinct" in lib.gnx_last_error()
    assert lib.gnx_graph_normalize(g.handle, 1, 0, 1.5, 0, 0, nat.ptr(out), None, s) == -1 and b"dropout rate" in lib.gnx_last_error()
    assert lib.gnx_graph_normalize(g.handle, 1, 2, 0.0, 0, 0, nat.ptr(out), None, s) == -1 and b"d_diag_out" in lib.gnx_last_error()
    rect = make_graph(gnntf, *graphs.random_coo(20, 30, 100, seed=3))
    assert lib.gnx_graph_normalize(rect.handle, 1, 0, 0.0, 0, 0, nat.ptr(out), None, s) == -1 and b"square" in lib.gnx_last_error()
    bad = c_void_p()
    rp = torch.tensor([0, 2, 1, 3], device="cuda"); ci = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda"); v = torch.ones(3, device="cuda")
    assert lib.gnx_graph_create_csr(3, 3, 3, nat.ptr(rp), nat.ptr(ci), nat.ptr(v), s, byref(bad)) == -1 and b"valid sorted CSR" in lib.gnx_last_error()
    # round-2 entry points
    from ctypes import c_float
    D = torch.ones(50, device="cuda")
    gid = torch.arange(30, dtype=torch.int32, device="cuda")
    assert lib.gnx_graph_set_block(rect.handle, 0, 15, nat.ptr(gid), s) == -1 and b"do not fit" in lib.gnx_last_error()      # 20 rows behind column 15 of 30
    assert lib.gnx_graph_set_block(rect.handle, 100, 5, nat.ptr(gid), s) == 0 and lib.gnx_graph_set_block(rect.handle, 0, 0, None, s) == 0
    assert lib.gnx_spmm_dropped(rect.handle, nat.ptr(D), 0.5, 1, 1, 0, nat.ptr(X), 16, 16, None, 0, 1.0, 0.0, 0, nat.ptr(out), 16, s) == -1
    assert b"square graph or a vertex block" in lib.gnx_last_error()
    dup = make_graph(gnntf, np.concatenate([coo, coo[:5]]), np.concatenate([vals, vals[:5]]), shape)
    assert lib.gnx_spmm_dropped_chained(dup.handle, nat.ptr(D), 0.5, 1, 1, 0, None, nat.ptr(X), 16, 16, None, 0, 1.0, 0.0, 0, nat.ptr(out), 16,
                                        s) == -4 and b"duplicate" in lib.gnx_last_error()                                          # GNX_ERR_UNSUPPORTED
    assert lib.gnx_spmm_dropped_chained(g.handle, None, 0.5, 1, 1, 0, None, nat.ptr(X), 16, 16, None, 0, 1.0, 0.0, 0, nat.ptr(out), 16, s) == -1
    ptrs, coefs = (c_void_p * 1)(X.data_ptr()), (c_float * 1)(1.0)
    assert lib.gnx_linear_combination(0, ptrs, coefs, 16, nat.ptr(out), s) == -1 and b"1 to 16 terms" in lib.gnx_last_error()
    assert lib.gnx_linear_combination(17, ptrs, coefs, 16, nat.ptr(out), s) == -1
    assert lib.gnx_linear_combination(1, (c_void_p * 1)(X.data_ptr() + 4), coefs, 16, nat.ptr(out), s) == -1 and b"unaligned" in lib.gnx_last_error()
    idx64 = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert lib.gnx_gather_rows(nat.ptr(X), 16, nat.ptr(idx64), 1 << 26, 16, nat.ptr(out), 16, s) == -1 and b"2^26" in lib.gnx_last_error()
    # the library still works after the failed calls
    assert call(nat.ptr(X), 16, 16, None, 0, 1.0, 0.0, 0, nat.ptr(out), 16, s) == 0
    want = orc.sparse_dense_matmul(coo, vals, shape, X.cpu().numpy())
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=RTOL, atol=ATOL)
    # relu epilogue (GCN's default activation, gcn.py:78) and beta/alpha scaling
    H0 = torch.rand(50, 16, device="cuda") - 0.5
    assert call(nat.ptr(X), 16, 16, nat.ptr(H0), 16, -0.5, 2.0, 1, nat.ptr(out), 16, s) == 0
    np.testing.assert_allclose(out.cpu().numpy(), np.maximum(-0.5 * want + 2.0 * H0.cpu().numpy(), 0), rtol=RTOL, atol=ATOL)


def test_c_client_of_the_abi(tmp_path):
    """include/gnx.h + libgnx.so from a plain C program (no Python, no torch in the process)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "c_abi_smoke")
    lib = os.path.join(root, "gnn-tf_amd", "lib")
    subprocess.check_call(["gcc", "-std=c11", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "c_abi_smoke.c"), "-L", lib, "-lgnx", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "C ABI OK" in res.stdout, res.stdout + res.stderr


def test_random_shapes_against_oracle(gnntf):
    """Seeded fuzz over shapes, widths, leading dimensions, duplicates and empty rows (all dispatch classes)."""
    rng = np.random.default_rng(2024)
    kernels = set()
    for case in range(60):
        n_rows, n_cols = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        nnz = int(rng.integers(0, 4000))
        C = int(rng.choice([1, 2, 3, 4, 5, 8, 12, 17, 31, 32, 33, 48, 64, 65, 96, 128, 129, 160, 256, 300]))
        pad = int(rng.choice([0, 0, 1, 4, 7]))
        idx = np.stack([rng.integers(n_rows, size=nnz), rng.integers(n_cols, size=nnz)], axis=1).astype(np.int64)
        if nnz and rng.random() < 0.5:                                   # a heavy row now and then
            idx[: nnz // 2, 0] = int(rng.integers(n_rows))
        vals = rng.standard_normal(nnz).astype(np.float32)
        g = make_graph(gnntf, idx, vals, (n_rows, n_cols))
        X = rng.standard_normal((n_cols, C + pad)).astype(np.float32)
        H0 = rng.standard_normal((n_rows, C + pad)).astype(np.float32)
        Xd, H0d = dev(X)[:, :C], dev(H0)[:, :C]
        from gnntf.sparse import _launch
        got = _launch(gnntf.Adjacency(g), Xd, H0d, 0.75, 0.25, 1 if case % 3 == 0 else 0).cpu().numpy()
        want = orc.sparse_dense_matmul(idx, vals.astype(np.float64), (n_rows, n_cols), X[:, :C].astype(np.float64)) * 0.75 + 0.25 * H0[:, :C]
        if case % 3 == 0:
            want = np.maximum(want, 0)
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=1e-4, err_msg=f"case {case}: {n_rows}x{n_cols} nnz={nnz} C={C} pad={pad}")
        kernels.add(g.last_kernel())
    assert {k.split("+")[0] for k in kernels} >= {"spmm_wave", "spmm_group32", "spmm_group16", "spmm_group8"}      # (8 lanes per row is the narrowest group)


# ---- A2: get_adjacency -------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["symmetric", "bipartite", "none"])
@pytest.mark.parametrize("eye", ["none", "before", "after"])
def test_normalize_options(gnntf, norm, eye):
    coo, vals, shape = graphs.random_coo(257, 257, 3000, seed=21, weighted=True, dup_frac=0.25)
    g = make_graph(gnntf, coo, vals, shape)
    adj = gnntf.normalize(g, norm, eye)
    H = np.random.default_rng(1).standard_normal((257, 12)).astype(np.float32)
    ai, av = orc.get_adjacency(coo, vals, shape, normalized=norm, add_eye=eye, dtype=np.float64)
    want = orc.sparse_dense_matmul(ai, av, shape, H.astype(np.float64))
    np.testing.assert_allclose(gnntf.spmm(adj, dev(H)).cpu().numpy(), want, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("norm", ["symmetric", "bipartite", "none"])
@pytest.mark.parametrize("eye", ["none", "before", "after"])
def test_normalize_options_with_edge_dropout(gnntf, norm, eye):
    """Training mode: dropout first, then +I / scaling on the DROPPED values (gnn.py:37-49), duplicates included."""
    coo, vals, shape = graphs.random_coo(200, 200, 2500, seed=33, weighted=True, dup_frac=0.3)
    g = make_graph(gnntf, coo, vals, shape)
    adj = gnntf.normalize(g, norm, eye, dropout=0.3, seed=11, stream_id=5)
    ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=0.3, normalized=norm, add_eye=eye, training=True, seed=11, stream=5,
                               dtype=np.float64)
    H = np.random.default_rng(2).standard_normal((200, 9)).astype(np.float32)
    want = orc.sparse_dense_matmul(ai, av, shape, H.astype(np.float64))
    np.testing.assert_allclose(gnntf.spmm(adj, dev(H)).cpu().numpy(), want, rtol=RTOL, atol=ATOL)


def test_nan_semantics_match(gnntf):
    """Negative column sums: sqrt gives NaN in TensorFlow and here alike (no silent clamping); zero sums give 0."""
    idx = np.array([[0, 1], [1, 0], [1, 2], [2, 1], [3, 3]])
    vals = np.array([1.0, 1.0, -3.0, -3.0, 0.0], dtype=np.float32)       # column sums: 1, -2, -3, 0
    g = make_graph(gnntf, idx, vals, (4, 4))
    got = gnntf.normalize(g, "symmetric").vals.cpu().numpy()
    with np.errstate(invalid="ignore"):
        _, want = orc.get_adjacency(idx, vals, (4, 4))
    _, _, want = orc.coo_to_csr_coalesced(idx, want, (4, 4))
    assert np.isnan(got).tolist() == np.isnan(want).tolist() and np.isnan(got).any()
    assert got[-1] == 0 and want[-1] == 0                                 # divide_no_nan(1, 0) = 0 on the zero column


def test_k_loop_skips_settled_empty_rows_bitwise(gnntf):
    """gnx_appnp_propagate leaves rows without entries alone once both ping-pong buffers hold their a * H0 (GNX_ACT_SKIP_EMPTY):
    the result must equal, bit for bit, K separate full steps -- also when an EMPTY row's column is read by other rows
    (directed pattern) and for every parity of K."""
    rng = np.random.default_rng(12)
    n = 4000
    rows = rng.integers(0, n // 2, size=30000)                  # rows n/2 .. n-1 have no entries ...
    cols = rng.integers(0, n, size=30000)                       # ... but their columns are referenced
    coo = np.unique(np.stack([rows, cols], 1), axis=0)
    vals = (rng.random(len(coo)) + 0.5).astype(np.float32)
    g = make_graph(gnntf, coo, vals, (n, n))
    adj = gnntf.normalize(g, "none")
    for C in (8, 64, 256):
        H0 = dev(rng.standard_normal((n, C)).astype(np.float32))
        for K in (1, 2, 3, 6, 7):
            H = H0
            for _ in range(K):
                H = gnntf.ppr_step(adj, H, H0, 0.2)
            got = gnntf.appnp_propagate(adj, H0, a=0.2, iterations=K)
            assert torch.equal(got, H), (C, K)
            assert torch.equal(got[n // 2:], H0[n // 2:] * 0.2)
    eye = gnntf.normalize(g, "none", "after")                   # a diagonal term makes empty rows depend on the iterate: nothing is skipped
    H0 = dev(rng.standard_normal((n, 16)).astype(np.float32))
    H = H0
    for _ in range(5):
        H = gnntf.ppr_step(eye, H, H0, 0.2)
    assert torch.equal(gnntf.appnp_propagate(eye, H0, a=0.2, iterations=5), H)


def test_k_loop_never_writes_unreferenced_empty_rows_into_work_buffers(gnntf):
    """Symmetric patterns: a row without entries is referenced by nobody, so the K loop writes it into the RESULT only (the first time
    the result buffer is a destination) and never into the work buffer -- same bits as K full steps for every parity of K, and
    nothing ever reads the rows it left untouched (work and result buffers poisoned with NaN beforehand)."""
    from gnntf import _native as nat
    coo, vals, shape = graphs.rmat_symmetric_coo(6000, 9000, seed=5)               # sparse enough to leave isolated vertices
    n = shape[0]
    isolated = np.setdiff1d(np.arange(n), coo[:, 0])
    assert len(isolated) > 100
    g = make_graph(gnntf, coo, vals, shape)
    adj = gnntf.normalize(g, "symmetric")
    for C in (8, 64, 256):
        H0 = dev(np.random.default_rng(C).standard_normal((n, C)).astype(np.float32))
        for K in (1, 2, 3, 6, 7):
            H = H0
            for _ in range(K):
                H = gnntf.ppr_step(adj, H, H0, 0.2)
            out = torch.full_like(H0, float("nan"))
            work = torch.full_like(H0, float("nan"))
            nat.check(nat.lib().gnx_appnp_propagate(g.handle, nat.ptr(adj.vals), None, nat.ptr(H0), 0.2, K, C, nat.ptr(out), nat.ptr(work),
                                                    nat.current_stream()))
            assert torch.equal(out, H), (C, K)
            assert torch.equal(out[isolated], H0[isolated] * 0.2)
            if K >= 2:                                                        # the work buffer never received them
                assert bool(torch.isnan(work[isolated]).all()), (C, K)


def test_k_loop_on_the_relabelled_copy_for_narrow_widths(gnntf):
    """gnx_appnp_propagate at C <= 16 on a large graph runs on the degree-relabelled copy of the matrix (H0 permuted in, the last
    iteration scattered back): same result as K plain steps up to float32 rounding (the columns of a row are summed in another
    order), for every K parity, unaligned widths, weighted directed patterns and empty rows; C > 16 keeps the plain path bitwise."""
    n = 1_200_000
    gen = torch.Generator(device="cuda").manual_seed(5)
    rows = (torch.rand(6_000_000, device="cuda", generator=gen) ** 3 * (n * 0.7)).long()          # skewed; rows above 0.7 n stay empty
    cols = (torch.rand(6_000_000, device="cuda", generator=gen) ** 2 * n).long().clamp_(max=n - 1)
    idx = torch.unique(torch.stack([rows, cols], 1), dim=0)
    vals = torch.rand(idx.shape[0], device="cuda", generator=gen) + 0.5
    g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, vals, (n, n)), device="cuda:0")
    adj = gnntf.normalize(g, "symmetric")
    for C in (7, 8, 16, 24, 32, 40):
        H0 = torch.rand(n, C, device="cuda", generator=gen) * 2 - 1
        for K in (1, 2, 3, 10):
            H = H0
            for _ in range(K):
                H = gnntf.ppr_step(adj, H, H0, 0.15)
            got = gnntf.appnp_propagate(adj, H0, a=0.15, iterations=K)
            if C > 16:
                assert torch.equal(got, H)
            else:
                assert torch.allclose(got, H, rtol=2e-5, atol=2e-6), (C, K, float((got - H).abs().max()))
                assert torch.equal(got[int(n * 0.75):], H[int(n * 0.75):])           # rows without entries: exactly a * H0
        if C <= 16:       # the same loop with relu in every iteration's epilogue (gnx_appnp_propagate_act), on the relabelled copy
            from gnntf import _native as nat
            for K in (2, 5):
                H = H0
                for _ in range(K):
                    H = gnntf.sparse._launch(adj, H, H0, 0.85, 0.15, nat.ACT_RELU)
                got = gnntf.appnp_propagate(adj, H0, a=0.15, iterations=K, relu=True)
                assert torch.allclose(got, H, rtol=2e-5, atol=2e-6), (C, K, float((got - H).abs().max()))
                assert torch.equal(got[int(n * 0.75):], torch.relu(H0[int(n * 0.75):] * 0.15)) and float(got.min()) >= 0
    del g, adj
    # the same pattern made symmetric: rows without entries are referenced by nobody, and the loop then writes them by its last
    # (scattering) iteration only -- never into a work buffer
    sym = torch.unique(torch.cat([idx, idx.flip(1)]), dim=0)
    sym = sym[sym[:, 0] < int(n * 0.7)]
    sym = torch.unique(torch.cat([sym, sym.flip(1)]), dim=0)
    sym = sym[(sym[:, 0] < int(n * 0.7)) & (sym[:, 1] < int(n * 0.7))]
    g = gnntf.DeviceGraph(gnntf.SparseCOO(sym, torch.ones(sym.shape[0], device="cuda"), (n, n)), device="cuda:0")
    adj = gnntf.normalize(g, "symmetric")
    for C, K in ((8, 1), (8, 2), (16, 5)):
        H0 = torch.rand(n, C, device="cuda", generator=gen) * 2 - 1
        H = H0
        for _ in range(K):
            H = gnntf.ppr_step(adj, H, H0, 0.15)
        got = gnntf.appnp_propagate(adj, H0, a=0.15, iterations=K)
        assert torch.allclose(got, H, rtol=2e-5, atol=2e-6), (C, K, float((got - H).abs().max()))
        assert torch.equal(got[int(n * 0.75):], H0[int(n * 0.75):] * 0.15)
    del g, adj


def test_hand_graphs(gnntf):
    """KAT-2 on the device: isolated nodes -> a*H0; doubled COO == single COO; directed column-sum rule."""
    idx, vals, shape = orc.graph2adj(range(8), [(0, i) for i in range(1, 6)])
    adj = gnntf.normalize(make_graph(gnntf, idx, vals, shape), "symmetric")
    H0 = np.arange(16, dtype=np.float32).reshape(8, 2)
    out = gnntf.appnp_propagate(adj, dev(H0), a=0.25, iterations=3).cpu().numpy()
    np.testing.assert_allclose(out, orc.appnp_propagate(idx, vals, shape, H0, a=0.25, iterations=3), rtol=1e-6)
    np.testing.assert_array_equal(out[6:], np.float32(0.25) * H0[6:])
    und = [(0, 1), (1, 2), (2, 0), (2, 3)]
    i1, v1, s4 = orc.graph2adj(range(4), und)
    i2, v2, _ = orc.graph2adj(range(4), und + [(v, u) for u, v in und])
    a1, a2 = gnntf.normalize(make_graph(gnntf, i1, v1, s4)), gnntf.normalize(make_graph(gnntf, i2, v2, s4))
    np.testing.assert_allclose(a1.vals.cpu().numpy(), a2.vals.cpu().numpy(), rtol=1e-7)
    i3, v3, s3 = orc.graph2adj(range(3), [(0, 1), (0, 2), (1, 2)], weights=[2.0, 3.0, 4.0], directed=True)
    a3 = gnntf.normalize(make_graph(gnntf, i3, v3, s3))
    _, want = orc.get_adjacency(i3, v3, s3)
    np.testing.assert_allclose(a3.vals.cpu().numpy(), want, rtol=1e-7)   # row 0 scales by colsum 0 -> all zero
    assert float(a3.vals[:2].abs().sum()) == 0


# ---- A3/A4: SpMM + fused mix over every dispatch class ----------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 7, 8, 16, 40, 64, 100, 128, 192, 256, 260, 512, 1030])
def test_ppr_step_all_widths(gnntf, C):
    coo, vals, shape = graphs.rmat_symmetric_coo(3000, 30000, seed=C)
    g = make_graph(gnntf, coo, vals, shape)
    adj = gnntf.normalize(g, "symmetric")
    rng = np.random.default_rng(C)
    H = rng.uniform(-1, 1, size=(3000, C)).astype(np.float32)
    H0 = rng.uniform(-1, 1, size=(3000, C)).astype(np.float32)
    ai, av = orc.get_adjacency(coo, vals, shape)
    want = orc.ppr_iteration(ai, av, shape, H, H0, a=0.1)
    got = gnntf.ppr_step(adj, dev(H), dev(H0), 0.1).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gnntf.spmm(adj, dev(H)).cpu().numpy(), orc.sparse_dense_matmul(ai, av, shape, H), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("n_rows", [700, 40000])
@pytest.mark.parametrize("C", [7, 64, 256])
def test_long_rows_and_ragged(gnntf, C, n_rows):
    """Hub rows far above the long-row threshold (512 entries; 128 for structures of 2^15 ... 2^20 rows -- n_rows = 40000 --, where
    the 513- and 512-entry rows are cut into 128-entry chunks too), empty rows, a rectangular matrix, ragged tails."""
    rng = np.random.default_rng(C)
    n_cols = 5000
    hub = np.stack([np.zeros(4999, dtype=np.int64), rng.permutation(n_cols)[:4999]], axis=1)      # one 4999-entry row
    hub2 = np.stack([np.full(513, 3, dtype=np.int64), rng.permutation(n_cols)[:513]], axis=1)      # just over the threshold
    edge = np.stack([np.full(512, 5, dtype=np.int64), rng.permutation(n_cols)[:512]], axis=1)      # exactly at it
    rest = np.stack([rng.integers(10, n_rows, size=6000), rng.integers(n_cols, size=6000)], axis=1)
    coo = np.concatenate([hub, hub2, edge, rest])
    vals = rng.uniform(0.5, 1.5, size=len(coo)).astype(np.float32)
    g = make_graph(gnntf, coo, vals, (n_rows, n_cols))
    X = rng.uniform(-1, 1, size=(n_cols, C)).astype(np.float32)
    H0 = rng.uniform(-1, 1, size=(n_rows, C)).astype(np.float32)
    adj = gnntf.Adjacency(g)            # raw values
    want = orc.sparse_dense_matmul(coo, vals.astype(np.float64), (n_rows, n_cols), X.astype(np.float64))
    got = gnntf.spmm(adj, dev(X)).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=1e-4)
    assert (got[1] == 0).all()          # empty row
    # few hub chunks: the sub-wave kernels take the short rows and the chunks in ONE launch (k_spmm_group_and_chunks)
    assert g.last_kernel() == {7: "spmm_group8+chunks", 64: "spmm_group16+chunks", 256: "spmm_wave"}[C]
    # transposed product exercises long COLUMNS of the same matrix
    G = rng.uniform(-1, 1, size=(n_rows, C)).astype(np.float32)
    from gnntf.sparse import _launch
    got_t = _launch(adj, dev(G), None, 1.0, 0.0, 0, transposed=True).cpu().numpy()
    want_t = orc.sparse_dense_matmul(coo[:, ::-1], vals.astype(np.float64), (n_cols, n_rows), G.astype(np.float64))
    np.testing.assert_allclose(got_t, want_t, rtol=RTOL, atol=1e-4)


def test_reproducible_bitwise(gnntf):
    coo, vals, shape = graphs.rmat_symmetric_coo(5000, 80000, seed=3)
    adj = gnntf.normalize(make_graph(gnntf, coo, vals, shape))
    H0 = dev(np.random.default_rng(0).uniform(-1, 1, size=(5000, 256)).astype(np.float32))
    a = gnntf.appnp_propagate(adj, H0, 0.1, 10)
    b = gnntf.appnp_propagate(adj, H0, 0.1, 10)
    assert torch.equal(a, b)
    step = H0
    for _ in range(10):
        step = gnntf.ppr_step(adj, step, H0, 0.1)
    assert torch.equal(a, step)          # the fused K loop == K single steps


def test_closed_form_on_device(gnntf):
    coo, vals, shape = graphs.random_coo(150, 150, 1200, seed=5, weighted=True)
    H0 = np.random.default_rng(0).standard_normal((150, 5)).astype(np.float32)
    A = orc.to_dense(coo, vals, shape)
    d = A.sum(axis=0)
    D = np.where(d > 0, 1 / np.sqrt(np.where(d > 0, d, 1)), 0)
    want = orc.appnp_closed_form(D[:, None] * A * D[None, :], H0, 0.1, 10)
    adj = gnntf.normalize(make_graph(gnntf, coo, vals, shape))
    np.testing.assert_allclose(gnntf.appnp_propagate(adj, dev(H0), 0.1, 10).cpu().numpy(), want, rtol=RTOL, atol=ATOL)


def test_handles_release_their_memory(gnntf):
    """gnx_graph_destroy frees everything a handle allocated (CSR, transposed structure, plans, partial slab)."""
    import gc
    coo, vals, shape = graphs.rmat_symmetric_coo(20000, 400000, seed=6)
    X = torch.rand(20000, 64, device="cuda")

    def cycle():
        g = make_graph(gnntf, coo, vals, shape)
        adj = gnntf.normalize(g, "symmetric", "after", dropout=0.5, seed=1, stream_id=2)
        out = gnntf.spmm(adj, X.requires_grad_())
        out.sum().backward()                       # builds the transposed structure as well
        del g, adj, out
        gc.collect()

    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(25):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 8 * 2 ** 20, f"leaked {(free0 - free1) / 2 ** 20:.1f} MiB over 25 create/destroy cycles"


LEAK_BOUND = 8 * 2 ** 20            # as above.  The graphs below are sized so that ONE int32 [n_rows] array lost per cycle exceeds it twice


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


_LAZY_GRAPHS = {}


def lazy_part_graphs(n):
    """Device COOs of a symmetric R-MAT with about 8 entries per row, made once per n: (without duplicates, with a quarter of the
    entries listed twice, shape)."""
    if n not in _LAZY_GRAPHS:
        coo, vals, shape = graphs.rmat_symmetric_coo(n, 4 * n, seed=31)
        assert len(coo) >= 6 * n
        idx, val = dev(coo), dev(vals)
        q = len(coo) // 4
        _LAZY_GRAPHS[n] = ((idx, val), (torch.cat([idx, idx[:q]]), torch.cat([val, val[:q]])), shape)
    return _LAZY_GRAPHS[n]


def fused_training_step(gnntf, g, C, gather_order):
    """Forward and backward of a K = 2 loop over fused dropped adjacencies; the degree scales of its two streams come from ONE
    gnx_graph_colsum_streams call (on a handle without duplicates that allocates the keep-bit scratch, t_mask)."""
    sparse = gnntf.sparse
    scales = sparse.dropped_degree_scales(g, 0.5, 77, 3, 2)
    make_adj = lambda k, bwd=False: sparse.dropped_adjacency(g, 0.5, 77, 3 + k, D=scales[k])
    H0 = torch.ones((g.n_rows, C), device="cuda").requires_grad_(True)
    out = sparse.ppr_loop(make_adj, H0, 0.1, 2, gather_order=gather_order)
    out.backward(torch.ones_like(out))
    assert torch.isfinite(H0.grad).all()


@pytest.mark.parametrize("n,cycles,C,k_loop", [(2 ** 18, 25, 64, False), (2 ** 20 + 3, 5, 8, True)])
def test_handles_release_every_lazy_part(gnntf, n, cycles, C, k_loop):
    """Create / destroy with EVERY lazily built part of a handle present: transposed structure, keep-bit scratch, gather order and
    gather columns, entry-dropout tables, long-row slab, a row window set and taken back (plans rebuilt, gather order dropped), a
    vertex block set and reset -- and, from 2^20 rows at C <= 16, the relabelled copy and its feature scratch.  One int32 [n] array
    lost per cycle is 4 * n * cycles = 25 MiB (20 MiB at 2^20 + 3 rows) against the bound of 8.  Arrays sized by the number of LONG
    rows or chunks are too small for mem_get_info to see at any size a test can afford: what covers them is that the handle holds
    no raw owned pointer at all (gnx_internal.h)."""
    import gc
    nat = gnntf.sparse.nat
    plain, doubled, shape = lazy_part_graphs(n)
    gid = torch.arange(n, dtype=torch.int32, device="cuda")

    def cycle():
        g = gnntf.DeviceGraph(gnntf.SparseCOO(*plain, shape), device="cuda:0")
        assert g.nnz == g.nnz_entries
        g.reserve(C, transposed=True, train_gather=True, k_loop=k_loop)
        order, rank = g.gather_order()
        assert order.shape == rank.shape == (n,)
        fused_training_step(gnntf, g, C, "relabelled")
        g.set_row_window(4096)
        g.set_row_window(0)
        d = gnntf.DeviceGraph(gnntf.SparseCOO(*doubled, shape), device="cuda:0")
        assert d.nnz < d.nnz_entries
        d.enable_entry_dropout()
        fused_training_step(gnntf, d, C, "caller")
        b = gnntf.DeviceGraph(gnntf.SparseCOO(*plain, shape), device="cuda:0")
        nat.check(nat.lib().gnx_graph_set_block(b.handle, 0, 0, nat.ptr(gid), nat.current_stream()))
        nat.check(nat.lib().gnx_graph_set_block(b.handle, 0, 0, None, nat.current_stream()))
        nat.check(nat.lib().gnx_graph_set_block(b.handle, 0, 0, nat.ptr(gid), nat.current_stream()))   # destroyed as a block
        torch.cuda.synchronize()
        del g, d, b, order, rank
        gc.collect()

    cycle()
    free0 = free_bytes()
    for _ in range(cycles):
        cycle()
    lost = free0 - free_bytes()
    print(f"n = {n}: {lost / 2 ** 20:.2f} MiB less free after {cycles} cycles")
    assert lost < LEAK_BOUND, f"leaked {lost / 2 ** 20:.1f} MiB over {cycles} create/destroy cycles"


def test_row_window_toggles_on_a_live_handle_release_their_memory(gnntf):
    """One handle of 2^18 rows with the transposed structure and the train-gather tables: 30 times a row window is set (two sizes
    in turn) and taken back.  Every set frees and rebuilds both plans and drops the gather order and the gather columns, which the
    gnx_spmm_dropped_chained_ord launch after every toggle rebuilds.  One int32 [n] array lost per toggle is 30 MiB.  The f32 SpMM
    at C = 7 and C = 64 gives the same bits afterwards: the row order decides which rows share a launch, never a row's sum."""
    sparse = gnntf.sparse
    n = 2 ** 18
    plain, _, shape = lazy_part_graphs(n)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(*plain, shape), device="cuda:0")
    g.reserve(64, transposed=True, train_gather=True)
    adj = gnntf.normalize(g, "symmetric")
    X = {C: torch.randn((n, C), device="cuda", generator=torch.Generator(device="cuda").manual_seed(C)) for C in (7, 64)}
    before = {C: gnntf.spmm(adj, X[C]) for C in X}
    scales = sparse.dropped_degree_scales(g, 0.5, 77, 3, 2)
    dropped = sparse.dropped_adjacency(g, 0.5, 77, 3, D=scales[0])
    H0 = torch.ones((n, 8), device="cuda")

    def toggle(window):
        g.set_row_window(window)
        assert torch.equal(gnntf.spmm(adj, X[7]), before[7])                # under the window as well
        g.set_row_window(0)
        sparse._launch_chained(dropped, H0, H0, 0.9, 0.1, False, scales[1], order=sparse.nat.ORD_OUT)
        assert g.last_kernel().endswith("_ord"), g.last_kernel()

    toggle(4096)
    toggle(1000)
    free0 = free_bytes()
    for i in range(30):
        toggle((4096, 1000)[i % 2])
    lost = free0 - free_bytes()
    print(f"{lost / 2 ** 20:.2f} MiB less free after 30 toggles")
    for C in X:
        assert torch.equal(gnntf.spmm(adj, X[C]), before[C]), C
    assert lost < LEAK_BOUND, f"leaked {lost / 2 ** 20:.1f} MiB over 30 row-window toggles"


def test_refused_row_window_rolls_back(gnntf):
    """A window whose count does not fit the 32-bit order key is refused and the handle is as it was.  2^22 rows (a few hundred
    entries: most rows are empty) are cut at LONG_ROW = 512 entries, so the degree bins take bits_for(513) = 10 bits of the key, and
    windows of ONE row need bits_for(2^22 + 1) = 23 more: 33.  The ABI has no getter for the window; what reads it back is
    gnx_graph_gather_order, which is refused exactly while a window is set.  The refused call frees the plan and rebuilds the
    previous one: one int32 [n] array lost per call is 16 MiB, ten calls 160."""
    nat = gnntf.sparse.nat
    n = 2 ** 22
    rng = np.random.default_rng(4)
    pairs = np.unique(rng.integers(0, n, size=(300, 2)), axis=0)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    coo = np.unique(np.concatenate([pairs, pairs[:, ::-1]]), axis=0)
    vals = rng.uniform(0.5, 1.5, size=len(coo)).astype(np.float32)
    g = make_graph(gnntf, coo, vals, (n, n))
    adj = gnntf.normalize(g, "symmetric")
    X = torch.randn((n, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    before = gnntf.spmm(adj, X)
    assert float(before.abs().max()) > 0

    def refused():
        rc = nat.lib().gnx_graph_set_row_window(g.handle, 1, nat.current_stream())
        message = nat.lib().gnx_last_error().decode()
        assert rc == -1 and "windows" in message and "order key" in message, (rc, message)      # GNX_ERR_INVALID

    refused()
    nat.check(nat.lib().gnx_graph_gather_order(g.handle, None, None))       # the window is still 0
    assert torch.equal(gnntf.spmm(adj, X), before)
    free0 = free_bytes()
    for _ in range(10):
        refused()
    lost = free0 - free_bytes()
    print(f"{lost / 2 ** 20:.2f} MiB less free after 10 refused calls")
    assert torch.equal(gnntf.spmm(adj, X), before)
    assert lost < LEAK_BOUND, f"leaked {lost / 2 ** 20:.1f} MiB over 10 refused set_row_window calls"
    g.set_row_window(4096)                                                  # 1024 windows: 11 + 10 bits
    refused()
    assert nat.lib().gnx_graph_gather_order(g.handle, None, None) == -4     # GNX_ERR_UNSUPPORTED: the window of 4096 rows is still set
    assert "row window" in nat.lib().gnx_last_error().decode()
    assert torch.equal(gnntf.spmm(adj, X), before)
    with pytest.raises(Exception, match="windows"):
        g.set_row_window(1)
    assert g.row_window == 4096


def test_scatter_output_rows(gnntf):
    """gnx_spmm_scatter: result row i lands in out[perm[i]] (all dispatch classes incl. long rows)."""
    from gnntf.sparse import _launch
    coo, vals, shape = graphs.rmat_symmetric_coo(4000, 60000, seed=12)
    adj = gnntf.normalize(make_graph(gnntf, coo, vals, shape))
    perm = torch.randperm(4000, device="cuda")
    for C in (7, 32, 256):
        X = dev(np.random.default_rng(C).standard_normal((4000, C)).astype(np.float32))
        H0 = dev(np.random.default_rng(C + 1).standard_normal((4000, C)).astype(np.float32))
        plain = _launch(adj, X, H0, 0.9, 0.1, 0)
        out = torch.full_like(plain, float("nan"))
        _launch(adj, X, H0, 0.9, 0.1, 0, out=out, out_rows=perm.to(torch.int32))
        assert torch.equal(out[perm], plain)
    with pytest.raises(Exception, match="bad output row map"):
        _launch(adj, X, H0, 0.9, 0.1, 0, out=out, out_rows=perm)          # int64 map


def test_strided_inputs_and_gather(gnntf):
    coo, vals, shape = graphs.rmat_symmetric_coo(1000, 8000, seed=8)
    adj = gnntf.normalize(make_graph(gnntf, coo, vals, shape))
    big = dev(np.random.default_rng(1).uniform(-1, 1, size=(1000, 96)).astype(np.float32))
    view = big[:, 16:80]                # leading dimension 96, width 64, 64-byte offset
    ai, av = orc.get_adjacency(coo, vals, shape)
    want = orc.sparse_dense_matmul(ai, av, shape, view.cpu().numpy())
    np.testing.assert_allclose(gnntf.spmm(adj, view).cpu().numpy(), want, rtol=RTOL, atol=ATOL)
    odd = big[:, 1:8]                   # unaligned: scalar path
    np.testing.assert_allclose(gnntf.spmm(adj, odd).cpu().numpy(), orc.sparse_dense_matmul(ai, av, shape, odd.cpu().numpy()),
                               rtol=RTOL, atol=ATOL)
    idx = torch.tensor([5, 0, 999, 5], device="cuda")
    assert torch.equal(gnntf.gather_rows(big, idx), big[idx])
    assert torch.equal(gnntf.gather_rows(odd, idx), odd[idx])


# ---- training mode: dropout masks, renormalisation, backward ---------------------------------------------
def test_dropout_masks_match_oracle_and_golden(gnntf, golden_dir):
    z = np.load(os.path.join(golden_dir, "dropout_masks.npz"))
    coo, vals, n = z["coo"].astype(np.int64), z["vals"], int(z["n"])
    g = make_graph(gnntf, coo, vals, (n, n))
    for stream in (0, 7):
        adj = gnntf.normalize(g, "symmetric", "none", dropout=float(z["p"]), seed=int(z["seed"]), stream_id=stream)
        _, _, want = orc.coo_to_csr_coalesced(coo, z[f"adj_vals_{stream}"], (n, n))
        got = adj.vals.cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)
        assert ((got == 0) == (want == 0)).all()       # exactly the same entries dropped
        raw = gnntf.normalize(g, "none", "none", dropout=float(z["p"]), seed=int(z["seed"]), stream_id=stream)
        _, _, want_raw = orc.coo_to_csr_coalesced(coo, np.where(z[f"keep_{stream}"], vals * np.float32(2), np.float32(0)), (n, n))
        np.testing.assert_array_equal(raw.vals.cpu().numpy(), want_raw)


def test_dropout_larger_graph(gnntf):
    coo, vals, shape = graphs.cora_shaped(seed=1)[:3]
    g = make_graph(gnntf, coo, vals, shape)
    assert g.nnz_entries == 21112 and g.nnz == 10556
    adj = gnntf.normalize(g, "symmetric", "none", dropout=0.5, seed=7, stream_id=11)
    ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=0.5, training=True, seed=7, stream=11)
    H = np.random.default_rng(0).standard_normal((shape[0], 7)).astype(np.float32)
    np.testing.assert_allclose(gnntf.spmm(adj, dev(H)).cpu().numpy(), orc.sparse_dense_matmul(ai, av, shape, H), rtol=RTOL, atol=ATOL)
    # per-entry dropout on the doubled COO: coalesced multipliers are 0, 2 or 4 (x the raw 1.0)
    raw = gnntf.normalize(g, "none", "none", dropout=0.5, seed=7, stream_id=11).vals.cpu().numpy()
    assert set(np.unique(raw).tolist()) == {0.0, 2.0, 4.0}


def test_transposed_order_values(gnntf):
    """gnx_graph_normalize_t writes exactly the values gnx_graph_normalize writes, in the transposed structure's
    order; gnx_spmm_tv on them == gnx_spmm_t on the CSR-order values (bitwise), with dropout and duplicates."""
    from gnntf import _native as nat
    from gnntf.sparse import _launch
    lib = nat.lib()
    coo, vals, shape = graphs.random_coo(300, 300, 5000, seed=41, weighted=True, dup_frac=0.3)
    g = make_graph(gnntf, coo, vals, shape)
    for p in (0.0, 0.5):
        a_csr = gnntf.normalize(g, "symmetric", "after", dropout=p, seed=9, stream_id=4)
        a_t = gnntf.normalize(g, "symmetric", "after", dropout=p, seed=9, stream_id=4, transposed_only=True)
        assert torch.equal(a_csr.transposed_values(), a_t.vals_t) and torch.equal(a_csr.diag, a_t.diag)
        G = dev(np.random.default_rng(1).standard_normal((300, 24)).astype(np.float32))
        via_tv = _launch(a_t, G, None, 0.9, 0.0, 0, transposed=True)
        out = torch.empty_like(G)
        nat.check(lib.gnx_spmm_t(g.handle, nat.ptr(a_csr.vals), nat.ptr(a_csr.diag), nat.ptr(G), 24, 24, None, 0, 0.9, 0.0, 0,
                                 nat.ptr(out), 24, nat.current_stream()))
        assert torch.equal(out, via_tv)
        ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=p, add_eye="after", training=p > 0, seed=9, stream=4, dtype=np.float64)
        want = orc.sparse_dense_matmul(ai[:, ::-1], av, shape, G.cpu().numpy().astype(np.float64)) * 0.9
        np.testing.assert_allclose(out.cpu().numpy(), want, rtol=RTOL, atol=ATOL)
    with pytest.raises(Exception, match="only holds transposed-order values"):
        gnntf.spmm(a_t, G)


@pytest.mark.parametrize("C", [3, 8, 24, 64, 100, 128, 256, 300])
def test_dropped_adjacency_fused_into_spmm_bitwise(gnntf, C):
    """gnx_spmm_dropped: the dropped + re-normalised values produced inside the SpMM kernels == gnx_graph_normalize followed by
    gnx_spmm / gnx_spmm_tv, BIT FOR BIT, in every dispatch class, with hub rows (long-row kernels), forward and transposed."""
    from gnntf.sparse import _launch, DroppedAdjacency
    n = 2500
    coo, vals, shape = graphs.rmat_symmetric_coo(n, 30000, seed=7)
    hub = np.random.default_rng(1).choice(np.arange(1, n), size=1300, replace=False)            # > 2 chunks of 512
    coo = np.unique(np.concatenate([coo, np.stack([np.zeros_like(hub), hub], 1), np.stack([hub, np.zeros_like(hub)], 1)]), axis=0)
    vals = (np.random.default_rng(2).random(len(coo)) + 0.5).astype(np.float32)                 # weighted and NOT symmetric in value
    g = make_graph(gnntf, coo, vals, shape)
    assert g.nnz == g.nnz_entries
    rng = np.random.default_rng(C)
    X, H0 = dev(rng.standard_normal((n, C)).astype(np.float32)), dev(rng.standard_normal((n, C)).astype(np.float32))
    fused = gnntf.sparse.dropped_adjacency(g, 0.5, 21, 6)
    assert isinstance(fused, DroppedAdjacency)
    two_pass = gnntf.normalize(g, "symmetric", "none", dropout=0.5, seed=21, stream_id=6)
    for transposed in (False, True):
        a = _launch(fused, X, H0, 0.9, 0.1, 0, transposed=transposed)
        kernel = g.last_kernel()
        b = _launch(two_pass, X, H0, 0.9, 0.1, 0, transposed=transposed)
        assert torch.equal(a, b), (C, transposed, float((a - b).abs().max()))
        assert kernel.endswith("_drop")
    assert torch.equal(fused.vals, two_pass.vals)                       # materialised on demand for custom layers
    ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=0.5, training=True, seed=21, stream=6, dtype=np.float64)
    want = orc.sparse_dense_matmul(ai, av, shape, X.cpu().numpy().astype(np.float64)) * 0.9 + 0.1 * H0.cpu().numpy()
    np.testing.assert_allclose(_launch(fused, X, H0, 0.9, 0.1, 0).cpu().numpy(), want, rtol=RTOL, atol=ATOL)
    # duplicates in the COO: per-entry dropout needs the entry lists -> the materialised form is used
    dup = make_graph(gnntf, np.concatenate([coo, coo[:50]]), np.concatenate([vals, vals[:50]]), shape)
    assert not isinstance(gnntf.sparse.dropped_adjacency(dup, 0.5, 1, 1), DroppedAdjacency)


def test_fused_dropout_skips_dropped_entries_even_when_their_row_is_not_finite(gnntf):
    """Pins the stated precondition of gnx_spmm_dropped (gnx.h; DroppedAdjacency): a dropped entry is SKIPPED, so a non-finite row
    of X behind it does not reach the sum, while the materialised form (an explicit zero weight, as tf.nn.dropout leaves in
    G.values, layered.py:50) turns 0 * inf into NaN exactly like the oracle does.  Finite rows: the two forms stay bitwise equal."""
    from gnntf.sparse import _launch
    n, C = 600, 16
    coo, vals, shape = graphs.rmat_symmetric_coo(n, 6000, seed=12)
    g = make_graph(gnntf, coo, vals, shape)
    fused = gnntf.sparse.dropped_adjacency(g, 0.5, 5, 2)
    two_pass = gnntf.normalize(g, "symmetric", "none", dropout=0.5, seed=5, stream_id=2)
    rowptr, colidx, _ = (t.cpu().numpy() for t in g.csr_arrays())
    w = two_pass.vals.cpu().numpy()
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    col = int(colidx[np.nonzero(w == 0)[0][0]])                      # a column with at least one dropped entry
    X = np.random.default_rng(0).standard_normal((n, C)).astype(np.float32)
    X[col] = np.inf
    a = _launch(fused, dev(X), None, 1.0, 0.0, 0).cpu().numpy()
    b = _launch(two_pass, dev(X), None, 1.0, 0.0, 0).cpu().numpy()
    dropped_only = np.setdiff1d(rows[(colidx == col) & (w == 0)], rows[(colidx == col) & (w != 0)])      # rows that reach `col` through dropped entries only
    kept = np.unique(rows[(colidx == col) & (w != 0)])
    assert len(dropped_only) > 0
    assert np.isfinite(a[dropped_only]).all() and np.isnan(b[dropped_only]).all()      # skipped vs explicit zero times inf
    assert np.isinf(a[kept]).all() and not np.isfinite(b[kept]).any()                  # a kept entry carries the inf in both forms
    ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=0.5, training=True, seed=5, stream=2)
    with np.errstate(invalid="ignore"):
        want = orc.sparse_dense_matmul(ai, av, shape, X)
    assert np.isnan(want[dropped_only]).all()                                            # the reference's behaviour = the materialised form's
    untouched = np.setdiff1d(np.arange(n), rows[colidx == col])
    assert np.array_equal(a[untouched], b[untouched])


def test_linear_combination_accepts_unaligned_views(gnntf):
    """A contiguous view with a storage offset (a row slice that starts 4 bytes into an allocation) is a legal gradient for the K-loop
    backward; gnx_linear_combination itself wants 16-byte aligned pointers, so such terms are copied first."""
    base = torch.arange(4 * 7 + 1, dtype=torch.float32, device="cuda")
    t = base[1:].reshape(4, 7)
    assert t.is_contiguous() and t.data_ptr() % 16 != 0
    u = torch.ones(4, 7, device="cuda")
    out = gnntf.sparse.linear_combination([(t, 2.0), (u, -1.0), (t, 0.5)])
    assert torch.equal(out, t * 2.0 - u + t * 0.5)


def test_degree_scales_of_k_streams_in_one_pass(gnntf):
    """gnx_graph_colsum_streams: the column sums of K dropout streams from one pass over the structure == K separate
    gnx_graph_colsum calls, bit for bit (hub columns included; duplicates take the per-stream path), and against the oracle."""
    from gnntf import _native as nat
    n = 3000
    coo, vals, shape = graphs.rmat_symmetric_coo(n, 25000, seed=3)
    hub = np.random.default_rng(4).choice(np.arange(1, n), size=1500, replace=False)
    coo = np.unique(np.concatenate([coo, np.stack([hub, np.zeros_like(hub)], 1)]), axis=0)       # column 0: > 512 entries
    vals = (np.random.default_rng(5).random(len(coo)) + 0.5).astype(np.float32)
    for with_dups in (False, True):
        c, v = (np.concatenate([coo, coo[:40]]), np.concatenate([vals, vals[:40]])) if with_dups else (coo, vals)
        g = make_graph(gnntf, c, v, shape)
        for K in (1, 3, 10, 13, 20):
            got = torch.empty((K, n), device="cuda")
            nat.check(nat.lib().gnx_graph_colsum_streams(g.handle, 0.5, 99, 7, K, nat.ptr(got), nat.current_stream()))
            for k in range(K):
                one = torch.empty(n, device="cuda")
                nat.check(nat.lib().gnx_graph_colsum(g.handle, 0.5, 99, 7 + k, nat.ptr(one), nat.current_stream()))
                assert torch.equal(got[k], one), (with_dups, K, k)
        keep = orc.keep_mask(c, 0.5, 99, 8)
        want = orc.sparse_reduce_sum_axis0(c, np.where(keep, v * np.float32(2), np.float32(0)).astype(np.float64), shape)
        np.testing.assert_allclose(got[1].cpu().numpy(), want, rtol=1e-5, atol=1e-5)
    D = gnntf.sparse.dropped_degree_scales(make_graph(gnntf, coo, vals, shape), 0.5, 99, 7, 4)
    assert D.shape == (4, n) and bool(torch.isfinite(D).all())


@pytest.mark.parametrize("C", [7, 64])
def test_backward_matches_oracle(gnntf, C):
    coo, vals, shape = graphs.random_coo(400, 400, 5000, seed=31, weighted=True)
    g = make_graph(gnntf, coo, vals, shape)
    adj = gnntf.normalize(g, "symmetric", "none", dropout=0.5, seed=3, stream_id=2)      # dropped => asymmetric A_hat
    ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=0.5, training=True, seed=3, stream=2)
    rng = np.random.default_rng(C)
    H = dev(rng.standard_normal((400, C)).astype(np.float32)).requires_grad_()
    H0 = dev(rng.standard_normal((400, C)).astype(np.float32)).requires_grad_()
    gout = rng.standard_normal((400, C)).astype(np.float32)
    out = gnntf.ppr_step(adj, H, H0, 0.1)
    out.backward(dev(gout))
    wantH, wantH0 = orc.ppr_iteration_backward(ai, av, shape, gout, a=0.1)
    np.testing.assert_allclose(H.grad.cpu().numpy(), wantH, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(H0.grad.cpu().numpy(), wantH0, rtol=1e-6)
    X = dev(rng.standard_normal((400, C)).astype(np.float32)).requires_grad_()
    gnntf.spmm(adj, X).backward(dev(gout))
    np.testing.assert_allclose(X.grad.cpu().numpy(), wantH / np.float32(0.9), rtol=RTOL, atol=ATOL)


# ---- golden fixtures: full models through the layer API ------------------------------------------------------
def test_golden_cora_appnp_layer_api(gnntf, golden_dir):
    from test_oracle_kat import load_cora
    z, coo, vals, shape, X, weights = load_cora(golden_dir)
    model = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7)
    dense = [l for l in model.layers() if isinstance(l, gnntf.Dense)]
    for layer, (W, b) in zip(dense, weights):
        layer.W.data.copy_(dev(W)); layer.b.data.copy_(dev(b))
    model.training_mode(False)
    with torch.no_grad():
        logits = model(model.features).cpu().numpy()
    np.testing.assert_allclose(dense[-1].value.cpu().numpy(), z["H0"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(logits, z["logits32"], rtol=RTOL, atol=1e-6)
    np.testing.assert_allclose(logits, z["logits64"], rtol=RTOL, atol=1e-6)
    assert (logits.argmax(1) == z["argmax"]).all()           # identical labels on ALL 2708 rows
    pred = model.predict(gnntf.NodeClassification(list(range(1708, 2708))))
    assert pred.cpu().numpy().tolist() == z["argmax"][1708:].tolist()
    assert model.graph.last_kernel().split("+")[0] == "spmm_group8"


def test_golden_arxiv_gcn_layer_api(gnntf, golden_dir):
    z = np.load(os.path.join(golden_dir, "arxiv_mini_gcn.npz"))
    coo, n = z["coo"].astype(np.int64), int(z["n"])
    model = gnntf.GCN(gnntf.SparseCOO(coo, np.ones(len(coo), dtype=np.float32), (n, n)), z["X"].astype(np.float32), num_classes=40)
    layers = model.layers()
    layers[0].W.data.copy_(dev(z["W1"].astype(np.float32))); layers[0].b.data.copy_(dev(z["b1"].astype(np.float32)))
    layers[1].W.data.copy_(dev(z["W2"].astype(np.float32))); layers[1].b.data.copy_(dev(z["b2"].astype(np.float32)))
    model.training_mode(False)
    with torch.no_grad():
        out = model(model.features).cpu().numpy()
    np.testing.assert_allclose(out, z["out32"], rtol=RTOL, atol=ATOL)
    assert (out >= 0).all()


def test_gcn_transform_first(gnntf, golden_dir):
    """GCN(transform_first=True): A.(X.W) with bias + relu in the SpMM epilogue == the reference order (A.X).W
    within the float32 tolerance, forward and backward."""
    z = np.load(os.path.join(golden_dir, "arxiv_mini_gcn.npz"))
    coo, n = z["coo"].astype(np.int64), int(z["n"])
    outs, grads = [], []
    for tf_first in (False, True):
        model = gnntf.GCN(gnntf.SparseCOO(coo, np.ones(len(coo), dtype=np.float32), (n, n)), z["X"].astype(np.float32), num_classes=40,
                          transform_first=tf_first)
        layers = model.layers()
        assert [l.transform_first for l in layers] == [tf_first, tf_first]
        layers[0].W.data.copy_(dev(z["W1"].astype(np.float32))); layers[0].b.data.copy_(dev(z["b1"].astype(np.float32)))
        layers[1].W.data.copy_(dev(z["W2"].astype(np.float32))); layers[1].b.data.copy_(dev(z["b2"].astype(np.float32)))
        model.training_mode(False)
        out = model(model.features)
        (out * dev(np.random.default_rng(0).standard_normal((n, 40)).astype(np.float32))).sum().backward()
        outs.append(out.detach().cpu().numpy())
        grads.append([layers[0].W.grad.cpu().numpy(), layers[0].b.grad.cpu().numpy(), layers[1].W.grad.cpu().numpy()])
    np.testing.assert_allclose(outs[1], z["out32"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(outs[1], outs[0], rtol=RTOL, atol=ATOL)
    for a, b in zip(*grads):
        np.testing.assert_allclose(b, a, rtol=1e-3, atol=1e-3)
    assert model.graph.last_kernel().split("+")[0] in ("spmm_group16", "spmm_group32")


@pytest.mark.parametrize("how", ["degree", "locality"])
def test_model_level_degree_reorder(gnntf, golden_dir, how):
    """GNN(reorder="degree" / "locality"): same logits (float32 rounding) and the same labels in the caller's node order."""
    from test_oracle_kat import load_cora
    z, coo, vals, shape, X, weights = load_cora(golden_dir)
    logits = []
    for reorder in (None, how):
        model = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7, reorder=reorder)
        for layer, (W, b) in zip([l for l in model.layers() if isinstance(l, gnntf.Dense)], weights):
            layer.W.data.copy_(dev(W)); layer.b.data.copy_(dev(b))
        model.training_mode(False)
        with torch.no_grad():
            logits.append(model(model.features).cpu().numpy())
            again = model(dev(X)).cpu().numpy()                # features handed over in the caller's order
        np.testing.assert_allclose(again, logits[-1], rtol=1e-6, atol=1e-7)
        pred = model.predict(gnntf.NodeClassification(list(range(1708, 2708))))
        assert pred.cpu().numpy().tolist() == z["argmax"][1708:].tolist()
    np.testing.assert_allclose(logits[1], logits[0], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(logits[1], z["logits32"], rtol=RTOL, atol=1e-6)
    # training still works end to end on the reordered model
    labels = z["argmax"].astype(np.int64)
    model.train(train=gnntf.NodeClassification(list(range(300)), labels[:300]), epochs=3, patience=3)
    with pytest.raises(Exception, match="Invalid reorder option"):
        gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7, reorder="rcm")
    # the Cora-shaped stand-in is smaller than one window (and random): nothing to find -- the model says so and keeps the default
    # order; forced through, the window order must still give the same logits
    assert model.reorder_used == ("degree" if how == "degree" else None) and getattr(model.graph, "row_window", 0) == 0
    if how == "locality":
        assert model.locality_share is not None and not gnntf.ordering.found_communities(model.locality_share, shape[0], gnntf.ordering.LOCALITY_WINDOW)
        import unittest.mock
        with unittest.mock.patch.object(gnntf.ordering, "found_communities", lambda *a, **k: True), \
                unittest.mock.patch.object(gnntf.ordering, "LOCALITY_WINDOW", 256):
            forced = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7, reorder="locality")
        assert forced.reorder_used == "locality" and forced.graph.row_window == 256
        for layer, (W, b) in zip([l for l in forced.layers() if isinstance(l, gnntf.Dense)], weights):
            layer.W.data.copy_(dev(W)); layer.b.data.copy_(dev(b))
        forced.training_mode(False)
        with torch.no_grad():
            np.testing.assert_allclose(forced(forced.features).cpu().numpy(), logits[0], rtol=1e-5, atol=1e-6)


def test_locality_reorder_on_a_graph_with_communities(gnntf):
    """GNN(reorder="locality") on a planted-partition graph with shuffled labels: the order is taken (communities found), the
    library runs on row windows, predictions and logits are those of the unordered model."""
    rng = np.random.default_rng(3)
    n, k, size = 200000, 500, 400
    members = rng.permutation(n).reshape(k, size)
    comm = np.empty(n, dtype=np.int64)
    for c in range(k):
        comm[members[c]] = c
    m = 1500000
    src = rng.integers(n, size=m)
    dst = np.where(rng.random(m) < 0.85, members[comm[src], rng.integers(size, size=m)], rng.integers(n, size=m))
    coo = np.concatenate([np.stack([src, dst], 1), np.stack([dst, src], 1)])
    vals = np.ones(len(coo), dtype=np.float32)
    X = rng.standard_normal((n, 16)).astype(np.float32)
    outs = []
    for reorder in (None, "locality"):
        gnntf.set_seed(0); torch.manual_seed(0)
        model = gnntf.APPNP(gnntf.SparseCOO(coo, vals, (n, n)), X, num_classes=40, latent_dims=[], reorder=reorder)
        model.reset()
        model.training_mode(False)
        with torch.no_grad():
            outs.append(model(model.features))
    assert model.reorder_used == "locality" and model.locality_share > 0.3 and model.graph.row_window == gnntf.ordering.LOCALITY_WINDOW
    np.testing.assert_allclose(outs[1].cpu().numpy(), outs[0].cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert float((outs[1].argmax(1) == outs[0].argmax(1)).float().mean()) > 0.9999       # (random weights: near-ties may flip on rounding)
    # an R-MAT graph of the same size has no communities: the same request keeps the default order
    rcoo, rvals, rshape = graphs.rmat_symmetric_coo(n, 2 * m, seed=4)
    plain = gnntf.APPNP(gnntf.SparseCOO(rcoo, rvals, rshape), X, num_classes=8, latent_dims=[], reorder="locality")
    assert plain.reorder_used is None and getattr(plain.graph, "row_window", 0) == 0          # (its hubs are close in ANY degree-aware order)


def test_workgroups_are_dealt_round_robin_over_the_xcds(gnntf, capsys):
    """The speed assumption of the row-window launch order (xcd_block): workgroups b and b + 8 run on the same XCD.  Recorded, and
    asserted for a grid that fits the chip in one wave of workgroups; results never depend on it."""
    from gnntf import _native as nat
    out = torch.full((4096,), -1, dtype=torch.int32, device="cuda:0")
    nat.check(nat.lib().gnx_probe_block_xcd(4096, nat.ptr(out), nat.current_stream()))
    xcd = out.cpu().numpy()
    assert xcd.min() >= 0 and xcd.max() <= 7
    same = float((xcd[8:] == xcd[:-8]).mean())
    groups = [sorted(set(xcd[r::8].tolist())) for r in range(8)]
    with capsys.disabled():
        print(f"\n[xcd placement] blocks b and b + 8 on the same XCD: {same:.4f} of 4088 pairs; XCDs seen per residue class of blockIdx % 8: {groups}")
    assert same > 0.99 and len(set(xcd[:8].tolist())) == 8


@pytest.mark.parametrize("n,entries", [(3000, 30000), (40000, 500000)])
def test_row_window_changes_the_launch_order_not_the_sums(gnntf, n, entries):
    """gnx_graph_set_row_window: rows taken in windows of the caller's numbering (degree-binned inside a window).  Every row's sum
    runs over the same entries in the same order, so a single launch, its transposed form, the K loop, a training launch and the
    GCNII launch are bitwise what the default order gives; 0 restores the default; the oracle agrees."""
    coo, vals, shape = graphs.rmat_symmetric_coo(n, entries, seed=6)
    coo = np.concatenate([coo, np.stack([np.full(900, 7), np.arange(900) + 11], 1), np.stack([np.arange(900) + 11, np.full(900, 7)], 1)])   # a long row / column
    vals = np.concatenate([vals, np.ones(1800, dtype=np.float32)])
    rng = np.random.default_rng(0)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device="cuda:0")
    adj = gnntf.normalize(g, "symmetric")
    M = dev((0.5 * np.eye(32) + rng.standard_normal((32, 32)) * 0.2).astype(np.float32))

    def everything():
        out = {}
        for C in (7, 8, 40, 64, 256):
            H0 = dev(np.random.default_rng(C).standard_normal((n, C)).astype(np.float32))
            out[C, "step"] = gnntf.ppr_step(adj, H0, H0, 0.1)
            out[C, "loop"] = gnntf.appnp_propagate(adj, H0, 0.1, 4)
            out[C, "t"] = gnntf.sparse._launch(adj, H0, None, 1.0, 0.0, 0, transposed=True)
            out[C, "drop"] = gnntf.sparse._launch(gnntf.sparse.dropped_adjacency(g, 0.5, 3, 1), H0, H0, 0.9, 0.1, 0)
        H = dev(np.random.default_rng(1).standard_normal((n, 32)).astype(np.float32))
        with torch.no_grad():
            out["gcnii"] = gnntf.gcnii_step(adj, H, H, 0.1, M, relu=True)
        return out
    base = everything()
    for window in (64, 1000, n + 5):
        g.set_row_window(window)
        got = everything()
        for key in base:
            assert torch.equal(got[key], base[key]), (window, key, float((got[key] - base[key]).abs().max()))
    H0 = np.random.default_rng(8).standard_normal((n, 8)).astype(np.float32)
    want = orc.appnp_propagate(coo, vals, shape, H0, a=0.1, iterations=4)
    np.testing.assert_allclose(gnntf.appnp_propagate(adj, dev(H0), 0.1, 4).cpu().numpy(), want, rtol=RTOL, atol=ATOL)
    g.set_row_window(0)
    again = everything()
    assert all(torch.equal(again[key], base[key]) for key in base)
    with pytest.raises(Exception, match="negative window"):
        g.set_row_window(-1)


@pytest.mark.parametrize("n", [20011, 70001])
def test_row_window_remaps_the_group_kernels_bitwise(gnntf, n):
    """what reorder="locality" ships at narrow widths is k_spmm_group with the XCD-chunked block remap (xcd_block) over a
    PADDED grid, reached through launch_rows -- a graph without long rows (launch_rows_and_chunks bypasses the remap) and with at
    least 64 windows of non-empty rows.  Every row holds 3 ... 40 entries here, n is prime (the grid is no multiple of 8 chunks), and
    window = 64 / 96 must return bit for bit what the default order returns at every sub-wave width (group8 ... group32), for a
    single step, the K loop with settled rows trimmed, the transposed launch and a training launch."""
    rng = np.random.default_rng(n)
    deg = rng.integers(3, 41, size=n)
    deg[rng.integers(0, n, size=n // 10)] = 0                               # rows without entries (trimmed slots, padded blocks)
    rows = np.repeat(np.arange(n), deg)
    cols = rng.integers(0, n, size=rows.size)
    coo = np.stack([rows, cols], 1).astype(np.int64)
    vals = (rng.random(rows.size) + 0.25).astype(np.float32)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, (n, n)), device="cuda:0")
    adj = gnntf.normalize(g, "symmetric")
    kernels = {}

    def everything():
        out = {}
        for C in (7, 8, 12, 40, 64, 128):
            H0 = dev(np.random.default_rng(C).standard_normal((n, C)).astype(np.float32))
            out[C, "step"] = gnntf.ppr_step(adj, H0, H0, 0.1)
            kernels[C] = g.last_kernel()
            out[C, "loop"] = gnntf.appnp_propagate(adj, H0, 0.1, 4)
            out[C, "relu_loop"] = gnntf.appnp_propagate(adj, H0, 0.1, 3, relu=True)
            out[C, "t"] = gnntf.sparse._launch(adj, H0, None, 1.0, 0.0, 0, transposed=True)
            out[C, "drop"] = gnntf.sparse._launch(gnntf.sparse.dropped_adjacency(g, 0.5, 3, 1), H0, H0, 0.9, 0.1, 0)
        return out
    base = everything()
    assert kernels == {7: "spmm_group8", 8: "spmm_group8", 12: "spmm_group8", 40: "spmm_group16", 64: "spmm_group16", 128: "spmm_group32"}, kernels
    for window in (64, 96):
        assert g.n_rows - int((deg == 0).sum()) >= 64 * window            # the remap's own gate (GNX_ROW_PIECES)
        g.set_row_window(window)
        got = everything()
        for key in base:
            assert torch.equal(got[key], base[key]), (window, key, float((got[key] - base[key]).abs().max()))
    H0 = np.random.default_rng(8).standard_normal((n, 8)).astype(np.float32)
    want = orc.appnp_propagate(coo, vals, (n, n), H0, a=0.1, iterations=4)
    np.testing.assert_allclose(gnntf.appnp_propagate(adj, dev(H0), 0.1, 4).cpu().numpy(), want, rtol=RTOL, atol=ATOL)
    g.set_row_window(0)


def test_gcnii_layer_api(gnntf):
    """GCNII reuses the fused SpMM+mix kernel (gcn.py:7-27,54-74)."""
    coo, vals, shape = graphs.rmat_symmetric_coo(1500, 12000, seed=4)
    rng = np.random.default_rng(4)
    X = rng.standard_normal((1500, 20)).astype(np.float32)
    model = gnntf.GCNII(gnntf.SparseCOO(coo, vals, shape), X, num_classes=6, latent_dims=[32], iterations=8)
    model.reset()
    convs = [l for l in model.layers() if isinstance(l, gnntf.GCNIILayer)]
    dense = [l for l in model.layers() if isinstance(l, gnntf.Dense)]
    for l in convs:      # the reference initialises W to zero (gcn.py:11); use non-trivial weights for the check
        l.W.data.copy_(dev((rng.standard_normal((32, 32)) * 0.2).astype(np.float32)))
    model.training_mode(False)
    with torch.no_grad():
        out = model(model.features).cpu().numpy()
    want = orc.gcnii_forward_eval(coo, vals, shape, X, (dense[0].W.detach().cpu().numpy(), dense[0].b.detach().cpu().numpy()),
                                  [l.W.detach().cpu().numpy() for l in convs],
                                  (dense[1].W.detach().cpu().numpy(), dense[1].b.detach().cpu().numpy()), a=0.1, l=0.5)
    np.testing.assert_allclose(out, want, rtol=RTOL, atol=ATOL)
    assert len(convs) == 8 and [l.k for l in convs] == list(range(8))


def test_fused_ppr_loop_equals_layers(gnntf):
    """APPNP(fused=True): one autograd node for the K iterations, masks regenerated in the backward --
    same outputs (bitwise) and gradients as the K separate PPRIteration layers, in training mode."""
    coo, vals, shape = graphs.cora_shaped(seed=2)[:3]
    X = np.random.default_rng(0).standard_normal((shape[0], 24)).astype(np.float32)
    outs, grads = [], []
    for fused in (False, True):
        gnntf.set_seed(5)
        model = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7, fused=fused)
        torch.manual_seed(1)
        model.reset()
        dense = [l for l in model.layers() if isinstance(l, gnntf.Dense)]
        H0 = dev(np.random.default_rng(1).standard_normal((shape[0], 7)).astype(np.float32)).requires_grad_()
        dense[-1].value = H0                                  # drive the propagation layers directly
        feats = H0
        with model:                                           # training mode: per-iteration edge dropout
            for layer in model.layers()[len(model.layers()) - (1 if fused else 10):]:
                feats = layer(model, feats)
        (feats * dev(np.random.default_rng(2).standard_normal((shape[0], 7)).astype(np.float32))).sum().backward()
        outs.append(feats.detach()); grads.append(H0.grad.clone())
    assert torch.equal(outs[0], outs[1])
    np.testing.assert_allclose(grads[0].cpu().numpy(), grads[1].cpu().numpy(), rtol=1e-4, atol=1e-5)
    # eval mode goes through the single-call library loop
    model.training_mode(False)
    with torch.no_grad():
        ev = model.layers()[-1](model, H0.detach())
    adj = model.get_adjacency(0.5)
    assert torch.equal(ev, gnntf.appnp_propagate(adj, H0.detach(), 0.1, 10))
    # what a user gets without asking: filter.py:30-35's own list (K PPRIteration layers), executed as one fused run
    default = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7)
    assert sum(isinstance(l, gnntf.PPRIteration) for l in default.layers()) == 10 and not any(isinstance(l, gnntf.PPRLoop) for l in default.layers())
    by_layer = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7, activation=gnntf.relu)
    assert sum(isinstance(l, gnntf.PPRIteration) for l in by_layer.layers()) == 10
    with pytest.raises(Exception, match="identity activation"):
        gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7, activation=gnntf.relu, fused=True)
    # predict() through the default model == the strictly layer-by-layer execution of the same list == the collapsed model with the
    # same weights (eval mode), bit for bit; the fused run is ONE library call (the kernel log says so), layer by layer is K
    collapsed = gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7, fused=True)
    for v, w in zip(default.vars(), collapsed.vars()):
        w.assign(v.identity())
    default.training_mode(False); collapsed.training_mode(False)
    with torch.no_grad():
        as_run = default(default.features)
        inner = [l.value for l in default.layers()[-10:]]                       # lazy per-iteration values, computed on demand
        default.fuse_runs = False
        by_layers = default(default.features)
        assert torch.equal(as_run, by_layers) and torch.equal(as_run, collapsed(collapsed.features))
        for lazy, layer in zip(inner, default.layers()[-10:]):
            assert torch.equal(lazy, layer.value)


@pytest.mark.parametrize("C", [7, 64, 256])
def test_giant_row_against_fp32_sequential_and_fp64(gnntf, C):
    """A row of 320,000 entries with N(0, 1) weights times N(0, 1) features -- sums that cancel -- through the long-row path
    (512-entry chunks, partials added in chunk order), pinned two ways:
      (i)  against float64: every element within 8 float32 roundings of its OWN sum of |terms| (the yardstick of the vertex-block
           tests; what commit f2794eb's fuzz tolerance only widened);
      (ii) against the oracle's C port, which adds a row's terms one after the other in float32 -- the order the reference's
           TF-CPU kernel uses (tf.sparse.sparse_dense_matmul over the COO entries, filter.py:19): on the giant row the device
           result must be at least as close to the exact sum as that sequential float32 sum is."""
    import ctypes
    import scipy.sparse as sp
    import __graft_entry__ as ge
    rng = np.random.default_rng(100 + C)
    n, hub = 400_000, 320_000
    cols_hub = rng.choice(n, size=hub, replace=False)
    other_r = rng.integers(1, n, size=300_000)
    other_c = rng.integers(0, n, size=300_000)
    idx = np.unique(np.concatenate([np.stack([np.zeros(hub, dtype=np.int64), cols_hub], 1), np.stack([other_r, other_c], 1)]), axis=0)
    vals = rng.standard_normal(idx.shape[0]).astype(np.float32)
    X = rng.standard_normal((n, C)).astype(np.float32)
    H0 = rng.standard_normal((n, C)).astype(np.float32)
    a = np.float32(0.1)
    g = make_graph(gnntf, idx, vals, (n, n))
    got = gnntf.ppr_step(gnntf.Adjacency(g, dev(vals)), dev(X), dev(H0), float(a)).cpu().numpy()
    A64 = sp.csr_matrix((vals.astype(np.float64), (idx[:, 0], idx[:, 1])), shape=(n, n))
    beta = np.float64(np.float32(1.0 - np.float64(a)))
    want = beta * (A64 @ X.astype(np.float64)) + np.float64(a) * H0.astype(np.float64)
    terms = beta * (abs(A64) @ np.abs(X).astype(np.float64)) + np.float64(a) * np.abs(H0).astype(np.float64)
    u = 2.0 ** -24
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= 8 * u * terms + 1e-30).all(), float((err / (u * terms + 1e-30)).max())
    # the float32 sequential reference (oracle/propagate_ref.c: oracle_ppr_step), rows 0 .. 0 only matter here but all are computed
    lib = ctypes.CDLL(ge.build_oracle())
    lib.oracle_ppr_step.restype = None
    lib.oracle_ppr_step.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_float, ctypes.c_int64, ctypes.c_void_p]
    rowptr, colidx, cvals = orc.coo_to_csr_coalesced(idx, vals, (n, n))
    seq = np.empty_like(X)
    lib.oracle_ppr_step(n, rowptr.ctypes.data, colidx.ctypes.data, cvals.ctypes.data, X.ctypes.data, H0.ctypes.data, float(a), C, seq.ctypes.data)
    err_seq = np.abs(seq.astype(np.float64) - want)
    rms = lambda e: float(np.sqrt((e ** 2).mean()))
    assert rms(err[0]) <= rms(err_seq[0]), (rms(err[0]), rms(err_seq[0]))          # the giant row: chunked sums beat the sequential order
    assert (np.abs(got - seq)[0] <= err_seq[0] + 8 * u * terms[0]).all()           # and differ from it by no more than ITS error + ours
    np.testing.assert_allclose(got[1:], seq[1:], rtol=1e-5, atol=1e-5)             # short rows: a handful of terms either way


def test_capture_needs_the_handle_prepared_and_reserve_prepares_it(gnntf):
    """the lazily built parts of a handle (long-row slab, transposed structure) are never allocated under
    hipGraph capture.  A launch whose slab would have to grow there fails with a message naming gnx_graph_reserve -- and leaves
    the capture intact; after DeviceGraph.reserve(widest C) the FIRST launch at that width is captured and replays correctly."""
    coo, vals, shape = graphs.rmat_symmetric_coo(40_000, 600_000, seed=4)
    g = make_graph(gnntf, coo, vals, shape)
    adj = gnntf.normalize(g, "symmetric")
    n = shape[0]
    X8, X64 = dev(np.random.default_rng(0).standard_normal((n, 8)).astype(np.float32)), dev(np.random.default_rng(1).standard_normal((n, 64)).astype(np.float32))
    gnntf.spmm(adj, X8)                                     # the slab now fits 8 columns
    if "long" not in g.last_kernel() and "chunks" not in g.last_kernel():
        pytest.skip("this graph has no long rows: no slab to grow")
    torch.cuda.synchronize()
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(Exception, match="gnx_graph_reserve"):
        with torch.cuda.graph(refused):
            gnntf.spmm(adj, X64)
    torch.cuda.synchronize()
    fresh = make_graph(gnntf, coo, vals, shape)                         # a handle nothing has used yet: no transposed structure
    with pytest.raises(Exception, match="gnx_graph_reserve"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            gnntf.sparse._launch(gnntf.Adjacency(fresh, None), X8, None, 1.0, 0.0, 0, transposed=True)
    torch.cuda.synchronize()
    g.reserve(64, transposed=True)
    recorded = torch.cuda.CUDAGraph()
    with torch.cuda.graph(recorded):
        out_f = gnntf.spmm(adj, X64)                        # first launch at the widest width: inside the capture
        out_b = gnntf.sparse._launch(adj, X64, None, 1.0, 0.0, 0, transposed=True)
    X64.mul_(2.0)                                           # replays read the buffers as they are NOW
    recorded.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_f, gnntf.spmm(adj, X64)) and torch.equal(out_b, gnntf.sparse._launch(adj, X64, None, 1.0, 0.0, 0, transposed=True))


def test_hand_built_ppr_iteration_stack_runs_fused(gnntf):
    """The usage contract of reference demos/custom_layers.py:8-13 -- ``H0 = gnn.add(Dense(...)); for _ in range(10):
    gnn.add(PPRIteration(H0, 0.1))`` -- executes as ONE fused loop (Layer.__run__) and is bit for bit what the ten layers give
    one by one: eval mode, training mode (same sequence of edge-dropout masks), gradients, and the intermediate layers' lazily
    computed ``.value``."""
    coo, vals, shape = graphs.cora_shaped(seed=3)[:3]
    X = np.random.default_rng(0).standard_normal((shape[0], 24)).astype(np.float32)

    def build():
        gnntf.set_seed(7)
        gnn = gnntf.GNN(gnntf.SparseCOO(coo, vals, shape), X)
        gnn.add(gnntf.Dense(32, activation=gnntf.relu, dropout=0.0))
        H0 = gnn.add(gnntf.Dense(7, activation=gnntf.relu, regularize=False))
        for _ in range(10):
            gnn.add(gnntf.PPRIteration(H0, 0.1))
        return gnn

    fused, plain = build(), build()
    plain.fuse_runs = False
    for v, w in zip(fused.vars(), plain.vars()):
        w.assign(v.identity())
    launches = []
    real = gnntf.sparse.ppr_step
    # eval mode: one library call instead of ten
    fused.training_mode(False); plain.training_mode(False)
    with torch.no_grad():
        gnntf.sparse.ppr_step = lambda *a, **k: (launches.append(1), real(*a, **k))[1]
        try:
            out_f = fused(fused.features)
            assert not launches                                   # no single steps were launched ...
            out_p = plain(plain.features)
            assert len(launches) == 10                            # ... the layer-by-layer container launches ten
        finally:
            gnntf.sparse.ppr_step = real
        assert torch.equal(out_f, out_p)
        its_f = [l for l in fused.layers() if isinstance(l, gnntf.PPRIteration)]
        its_p = [l for l in plain.layers() if isinstance(l, gnntf.PPRIteration)]
        assert torch.equal(its_f[-1].value, out_f)
        assert all(l.G is fused.get_adjacency(0.5) for l in its_f)          # filter.py:18: every iteration's layer keeps its adjacency in .G
        for k in (0, 4, 8):                                       # an intermediate iteration's value: computed when read
            assert its_f[k].__dict__.get("_value") is None
            assert torch.equal(its_f[k].value, its_p[k].value)
    # training mode: the same masks, outputs and gradients
    outs, grads = [], []
    for model in (fused, plain):
        gnntf.set_seed(11)
        model._mask_calls = 0
        for v in model.vars():
            v.var.grad = None
        with model:
            out = model(model.features)
            (out * out).sum().backward()
        outs.append(out.detach())
        grads.append([v.var.grad.clone() for v in model.vars() if v.trainable])
    assert torch.equal(outs[0], outs[1])
    for gf, gp in zip(grads[0], grads[1]):
        np.testing.assert_allclose(gf.cpu().numpy(), gp.cpu().numpy(), rtol=1e-4, atol=1e-5)
    # what is NOT a plain run stays layer by layer: another activation, feature dropout, a run that does not start at H0
    gnn = build()
    gnn.add(gnntf.PPRIteration(gnn.layers()[1], 0.1, activation=gnntf.relu))
    gnn.add(gnntf.PPRIteration(gnn.layers()[1], 0.2))
    gnn.training_mode(False)
    with torch.no_grad():
        got = gnn(gnn.features)
        H0v = gnn.layers()[1].value
        adj = gnn.get_adjacency(0.5)
        want = gnntf.ppr_step(adj, torch.relu(gnntf.ppr_step(adj, gnntf.appnp_propagate(adj, H0v, 0.1, 10), H0v, 0.1)), H0v, 0.2)
    assert torch.equal(got, want)


def test_appnp_layer_list_matches_the_reference_by_default(gnntf):
    """filter.py:30-35: Dropout, one Dense per latent width, the output Dense, then ``iterations`` PPRIteration layers -- what
    ``APPNP(...)`` builds without being asked (the container fuses the run at execution); ``fused=True`` is the explicit opt-in
    to the collapsed list."""
    import networkx as nx
    G = nx.path_graph(6)
    X = np.eye(6, dtype=np.float32)
    model = gnntf.APPNP(gnntf.graph2adj(G), X, num_classes=3, latent_dims=[8, 4], iterations=10)
    names = [type(l).__name__ for l in model.layers()]
    assert names == ["Dropout", "Dense", "Dense", "Dense"] + ["PPRIteration"] * 10
    its = model.layers()[4:]
    assert all(l.H0 is model.layers()[3] and l.restart_probability == 0.1 and l.graph_dropout == 0.5 for l in its)
    assert len(gnntf.APPNP(gnntf.graph2adj(G), X, num_classes=3).layers()) == 13           # the reference's defaults: 1 + 1 + 1 + 10
    collapsed = gnntf.APPNP(gnntf.graph2adj(G), X, num_classes=3, latent_dims=[8, 4], iterations=10, fused=True)
    assert [type(l).__name__ for l in collapsed.layers()] == ["Dropout", "Dense", "Dense", "Dense", "PPRLoop"]
    assert collapsed.layers()[-1].iterations == 10 and collapsed.layers()[-1].H0 is collapsed.layers()[3]
    # a trainable restart probability (a=None) raises where the reference raises: create_var() without a shape (filter.py:35)
    with pytest.raises(Exception):
        gnntf.APPNP(gnntf.graph2adj(G), X, num_classes=3, a=None)
    # run(h, first=i): the container's loop continued from a value the caller holds
    model.reset(); model.training_mode(False)
    with torch.no_grad():
        whole = model(model.features)
        assert torch.equal(model.run(model.layers()[3].value, first=4), whole)


def test_train_and_predict_end_to_end(gnntf):
    """architecture.train()/predict() on the HIP path (README.md:26-68 usage), planted-partition graph."""
    gnntf.set_seed(0)
    rng = np.random.default_rng(0)
    n, k = 1200, 4
    labels = rng.integers(0, k, size=n)
    src, dst = rng.integers(n, size=20000), rng.integers(n, size=20000)
    keep = (labels[src] == labels[dst]) | (rng.random(20000) < 0.1)
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((int(u), int(v)) for u, v in zip(src[keep], dst[keep]) if u != v)
    X = (np.eye(k)[labels] + rng.standard_normal((n, k)) * 1.5).astype(np.float32)
    train, valid, test = list(range(0, 200)), list(range(200, 500)), list(range(500, n))
    mlp_like = (X[test].argmax(1) == labels[test]).mean()
    for fused in (False, True):
        model = gnntf.APPNP(gnntf.graph2adj(G), X, num_classes=k, fused=fused)
        model.train(train=gnntf.NodeClassification(train, labels[train]), valid=gnntf.NodeClassification(valid, labels[valid]),
                    patience=60, epochs=300)
        accuracy = gnntf.acc(model.predict(gnntf.NodeClassification(test)), labels[test])
        assert accuracy > 0.7 and accuracy > mlp_like + 0.15       # propagation, not the features, does the work


# ---- full-size properties (no oracle run at this size) ---------------------------------------------------------------
def test_full_size_properties(gnntf):
    """1M-node / 10M-entry RMAT at C=256: linearity and row-stochastic invariants of the device
    path, which need no CPU reference."""
    n = 1_000_000
    gen = torch.Generator(device="cuda").manual_seed(0)
    src = torch.randint(0, n, (5_000_000,), device="cuda", generator=gen)
    dst = (src + 1 + (torch.rand(5_000_000, device="cuda", generator=gen) ** 4 * (n - 1)).long()) % n
    idx = torch.cat([torch.stack([src, dst], 1), torch.stack([dst, src], 1)])
    g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], device="cuda"), (n, n)), device="cuda:0")
    rowptr, colidx, _ = g.csr_arrays()
    assert bool((rowptr[1:] >= rowptr[:-1]).all()) and int(rowptr[-1]) == g.nnz
    bip = gnntf.normalize(g, "bipartite")
    ones = torch.ones(n, 256, device="cuda")
    rows = gnntf.spmm(bip, ones)
    deg = (rowptr[1:] - rowptr[:-1]) > 0
    assert torch.allclose(rows[deg], torch.ones_like(rows[deg]), rtol=1e-5)      # rows of D^-1 A sum to 1
    assert float(rows[~deg].abs().sum()) == 0
    sym = gnntf.normalize(g, "symmetric")
    A = torch.rand(n, 256, device="cuda", generator=gen)
    B = torch.rand(n, 256, device="cuda", generator=gen)
    lhs = gnntf.spmm(sym, 2 * A + B)
    rhs = 2 * gnntf.spmm(sym, A) + gnntf.spmm(sym, B)
    assert torch.allclose(lhs, rhs, rtol=1e-4, atol=1e-5)                          # linearity
    # <A x, y> == <x, A^T y>: the transposed kernel against the forward one
    from gnntf.sparse import _launch
    x, y = A[:, :64].contiguous(), B[:, :64].contiguous()
    l = (gnntf.spmm(sym, x).double() * y.double()).sum()
    r = (x.double() * _launch(sym, y, None, 1.0, 0.0, 0, transposed=True).double()).sum()
    assert abs(float(l - r)) <= 1e-6 * abs(float(l))


@pytest.mark.parametrize("n,k", [(7, 1), (4096, 3), (100003, 11), (65536 * 9 + 2, 16)])
def test_linear_combination_one_pass(gnntf, n, k):
    """gnx_linear_combination (the end of the K-loop backward: dH0 = g_0 + a (g_1 + ... + g_K)): sum of up to 16 scaled arrays,
    terms added in list order with fmaf -- bit for bit the same chain on the host; lengths that are not multiples of 4."""
    from gnntf.sparse import linear_combination
    rng = np.random.default_rng(n + k)
    arrays = [rng.standard_normal(n).astype(np.float32) for _ in range(k)]
    coefs = [float(np.float32(c)) for c in rng.uniform(-2, 2, size=k)]
    got = linear_combination([(dev(x), c) for x, c in zip(arrays, coefs)]).cpu().numpy()
    want = arrays[0].astype(np.float64) * np.float32(coefs[0])
    want = want.astype(np.float32)
    for x, c in zip(arrays[1:], coefs[1:]):
        want = (x.astype(np.float64) * np.float64(np.float32(c)) + want.astype(np.float64)).astype(np.float32)   # fmaf: one rounding
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)    # (double rounding of the float64 emulation aside, the same bits)
    with pytest.raises(Exception, match="1 to 16 terms"):
        linear_combination([(dev(arrays[0]), 1.0)] * 17)


@pytest.mark.parametrize("C", [7, 9, 21, 41, 56, 127])
def test_fused_loops_pad_odd_widths(gnntf, C):
    """The K-iteration loops run odd widths at a friendlier row width (power of two up to 32, multiple of 4 beyond; zero pad
    columns): same numbers as the unpadded run to float32 rounding, eval loop and training loop (forward and dH0)."""
    from gnntf import sparse
    n = 70000                                      # (graphs below 2^16 rows are launch-bound and stay unpadded)
    coo, vals, shape = graphs.rmat_symmetric_coo(n, 400000, seed=C)
    adj = gnntf.normalize(make_graph(gnntf, coo, vals, shape), "symmetric")
    rng = np.random.default_rng(C)
    H0 = dev(rng.standard_normal((n, C)).astype(np.float32))
    G = dev(rng.standard_normal((n, C)).astype(np.float32))
    assert sparse.friendly_width(C) > C and sparse.friendly_width(C) % 4 == 0 and sparse.friendly_width(6) == 6 and sparse.friendly_width(64) == 64
    assert sparse.friendly_width(C, 2708) == C
    results = []
    for pad in (True, False):
        sparse.PAD_WIDTHS = pad
        try:
            with torch.no_grad():
                ev = gnntf.appnp_propagate(adj, H0, 0.1, 10)
            Hf = H0.clone().requires_grad_(True)
            tr = sparse.ppr_loop(lambda k, bwd=False: adj, Hf, 0.1, 10)
            tr.backward(G)
            results.append((ev, tr.detach(), Hf.grad))
        finally:
            sparse.PAD_WIDTHS = True
    for x, y in zip(*results):
        assert x.shape == (n, C) and x.is_contiguous()
        np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=1e-5, atol=1e-6)
    want = orc.appnp_propagate(coo, vals, shape, H0.cpu().numpy(), a=0.1, iterations=10)
    np.testing.assert_allclose(results[0][0].cpu().numpy(), want, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("C", [8, 64, 256])
def test_chained_training_forward_equals_step_loop(gnntf, C):
    """gnx_spmm_dropped_chained: in the fused training loop every epilogue hands the next iteration its column scale with the row
    (no per-entry scale gather from the second iteration on).  Same masks, same value as K separate gnx_spmm_dropped steps up to
    float32 rounding -- hub rows, isolated vertices (their scale is 0) and a weighted, value-asymmetric matrix included."""
    from gnntf import sparse
    from gnntf.sparse import _launch
    n, K, a, p_drop, seed, first = 2500, 5, 0.1, 0.5, 9, 4
    coo, vals, shape = graphs.rmat_symmetric_coo(n, 30000, seed=11)
    hub = np.random.default_rng(1).choice(np.arange(1, n), size=1300, replace=False)
    coo = np.unique(np.concatenate([coo, np.stack([np.zeros_like(hub), hub], 1), np.stack([hub, np.zeros_like(hub)], 1)]), axis=0)
    vals = (np.random.default_rng(2).random(len(coo)) + 0.5).astype(np.float32)
    g = make_graph(gnntf, coo, vals, shape)
    H0 = dev(np.random.default_rng(C).standard_normal((n, C)).astype(np.float32))
    D = sparse.dropped_degree_scales(g, p_drop, seed, first, K)
    make = lambda k, bwd=False: sparse.dropped_adjacency(g, p_drop, seed, first + k, D=D[k])
    with torch.no_grad():
        got = sparse.ppr_loop(make, H0, a, K)
        want = H0
        for k in range(K):
            want = _launch(make(k), want, H0, 1.0 - a, a, 0)
    assert g.last_kernel().endswith("_drop")
    scale = want.abs().max(dim=1, keepdim=True).values.clamp_min(1e-3)
    assert ((got - want).abs() / scale).max().item() < 2e-5
    adjs = [orc.get_adjacency(coo, vals, shape, graph_dropout=p_drop, training=True, seed=seed, stream=first + k, dtype=np.float64) for k in range(K)]
    ref = H0.cpu().numpy().astype(np.float64)
    for ai, av in adjs:
        ref = orc.ppr_iteration(ai, av, shape, ref, H0.cpu().numpy().astype(np.float64), a)
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=RTOL, atol=1e-4)


@pytest.mark.parametrize("C", [7, 16, 64])
def test_chained_training_backward_equals_step_loop(gnntf, C):
    """gnx_spmm_dropped_back: the backward of the fused training loop as K launches that each add their g_k to the running sum
    dH0 = g_0 + a (g_1 + ... + g_K) and hand the next launch its operand pre-scaled (no kept gradients, no per-entry scale gather,
    no summation pass).  Same value as K un-chained transposed launches (gnx_spmm_dropped) followed by the explicit sum, up to
    float32 rounding, and as the float64 oracle through the dropped adjacencies -- hub rows, isolated vertices (scale 0: their
    pre-scaled rows are zero and never gathered), a weighted value-asymmetric matrix, and autograd through ppr_loop."""
    from gnntf import sparse
    from gnntf.sparse import _launch
    n, K, a, p_drop, seed, first = 2500, 5, 0.1, 0.5, 9, 4
    coo, vals, shape = graphs.rmat_symmetric_coo(n, 30000, seed=11)
    hub = np.random.default_rng(1).choice(np.arange(1, n), size=1300, replace=False)
    coo = np.unique(np.concatenate([coo, np.stack([np.zeros_like(hub), hub], 1), np.stack([hub, np.zeros_like(hub)], 1)]), axis=0)
    vals = (np.random.default_rng(2).random(len(coo)) + 0.5).astype(np.float32)
    g = make_graph(gnntf, coo, vals, shape)
    up = dev(np.random.default_rng(C).standard_normal((n, C)).astype(np.float32))
    D = sparse.dropped_degree_scales(g, p_drop, seed, first, K)
    adjs = [sparse.dropped_adjacency(g, p_drop, seed, first + k, D=D[k]) for k in range(K)]
    got = sparse._backward_chained(adjs, up, a)
    assert g.last_kernel().endswith("_drop")
    gk, want = up, up * a
    for k in range(K - 1, -1, -1):
        gk = _launch(adjs[k], gk, None, 1.0 - a, 0.0, 0, transposed=True)
        want = want + gk * (a if k >= 1 else 1.0)
    scale = want.abs().max(dim=1, keepdim=True).values.clamp_min(1e-3)
    assert ((got - want).abs() / scale).max().item() < 2e-5
    # float64 oracle: g_k = (1-a) A_k^T g_{k+1} through the materialised dropped adjacencies
    ref_g = up.cpu().numpy().astype(np.float64)
    ref = a * ref_g
    import scipy.sparse as sp
    for k in range(K - 1, -1, -1):
        ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=p_drop, training=True, seed=seed, stream=first + k, dtype=np.float64)
        A = sp.csr_matrix((av, (ai[:, 0], ai[:, 1])), shape=shape)
        ref_g = (1.0 - a) * (A.T @ ref_g)
        ref = ref + ref_g * (a if k >= 1 else 1.0)
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=RTOL, atol=1e-4)
    # and it is what autograd runs for the fused loop
    H0 = dev(np.random.default_rng(3).standard_normal((n, C)).astype(np.float32)).requires_grad_()
    make = lambda k, bwd=False: adjs[k]
    sparse.ppr_loop(make, H0, a, K).backward(up)
    Cp = sparse.friendly_width(C, n)
    if Cp == C:
        assert torch.equal(H0.grad, got)
    else:
        assert ((H0.grad - got).abs() / scale).max().item() < 2e-5


@pytest.mark.parametrize("n", [4, 4 * 1024 * 4 * 3, 4 * (1024 * 4 * 1024 * 2 + 12345), 4 * 999_983])
def test_stream_yardsticks_move_every_element(gnntf, n):
    """gnx_stream_copy / gnx_stream_read (bench.py's measured-peak yardsticks): whole tiles, ragged tails and lengths below one tile."""
    from gnntf import _native as nat
    src = torch.arange(n, dtype=torch.float32, device="cuda") % 1024
    dst = torch.full_like(src, -1.0)
    nat.check(nat.lib().gnx_stream_copy(nat.ptr(src), nat.ptr(dst), n, nat.current_stream()))
    assert torch.equal(src, dst)
    sink = torch.zeros(64, dtype=torch.float32, device="cuda")
    ones = torch.ones(n, dtype=torch.float32, device="cuda")
    nat.check(nat.lib().gnx_stream_read(nat.ptr(ones), n, nat.ptr(sink), nat.current_stream()))
    assert float(sink.double().sum()) == n                      # per-wave sums of ones are exact; the 64 slots hold them all


# ---- the K loop with the reference's per-iteration activation (filter.py:22,28,35), fused ---------------------------------
@pytest.mark.parametrize("C", [1, 7, 16, 40, 64, 256])
def test_k_loop_with_relu_in_the_epilogue(gnntf, C):
    """gnx_appnp_propagate_act(GNX_ACT_RELU): relu after EVERY iteration inside the one library call.  Against the oracle's
    K-iteration loop with activation = relu; bit for bit what K single steps with the relu flag return; rows without entries
    (relu(a * H0) after every iteration) and long rows included; K = 0, 1, 2 (the ping-pong's corner cases)."""
    from gnntf import _native as nat
    from gnntf.sparse import _launch
    n = 3000
    coo, vals, shape = graphs.random_coo(n, n, 40000, seed=C, weighted=True, dup_frac=0.1)
    coo[:9000, 0] = 17                                                     # a long row (hub)
    keep = ~np.isin(coo[:, 0], np.arange(100, 400))                        # 300 rows without entries
    coo, vals = coo[keep], vals[keep]
    g = make_graph(gnntf, coo, vals, shape)
    adj = gnntf.normalize(g, "symmetric")
    H0 = np.random.default_rng(C).standard_normal((n, C)).astype(np.float32)
    for K in (0, 1, 2, 5, 10):
        got = gnntf.appnp_propagate(adj, dev(H0), a=0.15, iterations=K, relu=True)
        want = orc.appnp_propagate(coo, vals, shape, H0, a=0.15, iterations=K, activation=orc.relu)
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=RTOL, atol=ATOL)
        H = dev(H0)
        for _ in range(K):
            H = _launch(adj, H, dev(H0), 0.85, 0.15, nat.ACT_RELU)
        assert torch.equal(got, H), (C, K)
        if K > 0:
            assert float(got.min()) >= 0.0
            empty = got[100:400].cpu().numpy()
            np.testing.assert_array_equal(empty, np.maximum(np.float32(0.15) * H0[100:400], 0))
    # with a diagonal (add_eye, gnn.py:38-39,48-49) the settled-row rule is off and the relu still applies to every row
    for eye in ("before", "after"):
        adj_eye = gnntf.normalize(g, "symmetric", eye)
        got = gnntf.appnp_propagate(adj_eye, dev(H0), a=0.15, iterations=4, relu=True)
        want = orc.appnp_propagate(coo, vals, shape, H0, a=0.15, iterations=4, add_eye=eye, activation=orc.relu)
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=RTOL, atol=ATOL)
    # and the plain loop is still the plain loop
    assert torch.equal(gnntf.appnp_propagate(adj, dev(H0), a=0.15, iterations=3), gnntf.appnp_propagate(adj, dev(H0), a=0.15, iterations=3, relu=False))
    lib = nat.lib()
    X, out, work = dev(H0), torch.empty(n, C, device="cuda"), torch.empty(n, C, device="cuda")
    assert lib.gnx_appnp_propagate_act(g.handle, nat.ptr(adj.vals), None, nat.ptr(X), 0.1, 3, C, 7, nat.ptr(out), nat.ptr(work), nat.current_stream()) == -1
    assert b"invalid activation" in lib.gnx_last_error()


def test_appnp_with_relu_activation_runs_fused(gnntf):
    """APPNP(..., activation=relu) (filter.py:28,35: the activation goes to every PPRIteration): in eval mode the K layers run as ONE
    library call and return bit for bit what the layer-by-layer container returns; in training mode the same masks and outputs, and
    gradients equal to the layer-by-layer form's."""
    coo, vals, shape = graphs.cora_shaped(seed=5)[:3]
    X = np.random.default_rng(1).standard_normal((shape[0], 24)).astype(np.float32)

    def build(act):
        gnntf.set_seed(7)
        return gnntf.APPNP(gnntf.SparseCOO(coo, vals, shape), X, num_classes=7, latent_dims=[16], activation=act)
    fused, plain = build(gnntf.relu), build(torch.nn.functional.relu)
    plain.fuse_runs = False
    for m in (fused, plain):
        m.reset()
    for v, w in zip(fused.vars(), plain.vars()):
        w.assign(v.identity())
    assert [type(l).__name__ for l in fused.layers()] == ["Dropout", "Dense", "Dense"] + ["PPRIteration"] * 10
    calls, steps = [], []
    real_loop, real_step = gnntf.sparse.appnp_propagate, gnntf.sparse.ppr_step
    fused.training_mode(False); plain.training_mode(False)
    with torch.no_grad():
        gnntf.sparse.appnp_propagate = lambda *a, **k: (calls.append(k.get("relu")), real_loop(*a, **k))[1]
        gnntf.sparse.ppr_step = lambda *a, **k: (steps.append(1), real_step(*a, **k))[1]
        try:
            out_f = fused(fused.features)
            assert calls == [True] and not steps                          # one library call, with the relu flag
            out_p = plain(plain.features)
            assert len(steps) == 10
        finally:
            gnntf.sparse.appnp_propagate, gnntf.sparse.ppr_step = real_loop, real_step
        assert torch.equal(out_f, out_p) and float(out_f.min()) >= 0.0
        its_f = [l for l in fused.layers() if isinstance(l, gnntf.PPRIteration)]
        its_p = [l for l in plain.layers() if isinstance(l, gnntf.PPRIteration)]
        for k in (0, 5):                                                   # an intermediate iteration's value: computed when read
            assert torch.equal(its_f[k].value, its_p[k].value)
    outs, grads = [], []
    for model in (fused, plain):
        gnntf.set_seed(11)
        model._mask_calls = 0
        for v in model.vars():
            v.var.grad = None
        with model:
            out = model(model.features)
            (out * out).sum().backward()
        outs.append(out.detach())
        grads.append([v.var.grad.clone() for v in model.vars() if v.trainable])
    assert torch.equal(outs[0], outs[1])
    assert any(float(gr.abs().max()) > 0 for gr in grads[0])
    for gf, gp in zip(grads[0], grads[1]):
        np.testing.assert_allclose(gf.cpu().numpy(), gp.cpu().numpy(), rtol=1e-4, atol=1e-5)
    # feature dropout (filter.py:22) acts in training mode only: an eval-mode run of layers that have it still fuses; in training
    # mode the same stack runs layer by layer (torch's generator draws the masks)
    gnntf.set_seed(7)
    drop = gnntf.GNN(gnntf.SparseCOO(coo, vals, shape), X)
    H0 = drop.add(gnntf.Dense(7, regularize=False))
    for k in range(5):
        drop.add(gnntf.PPRIteration(H0, 0.1, activation=gnntf.relu, dropout=0.3))
    drop.reset(); drop.training_mode(False)
    calls, steps = [], []
    gnntf.sparse.appnp_propagate = lambda *a, **k: (calls.append(1), real_loop(*a, **k))[1]
    gnntf.sparse.ppr_step = lambda *a, **k: (steps.append(1), real_step(*a, **k))[1]
    try:
        with torch.no_grad():
            got = drop(drop.features)
            assert calls == [1] and not steps
            drop.fuse_runs = False
            assert torch.equal(got, drop(drop.features)) and len(steps) == 5
            drop.fuse_runs = True
        steps.clear()
        with drop:
            out = drop(drop.features)
        assert len(steps) == 5 and out.shape == got.shape                  # training mode: layer by layer
    finally:
        gnntf.sparse.appnp_propagate, gnntf.sparse.ppr_step = real_loop, real_step
    # a run whose layers disagree about the activation is not ONE run: relu x 3 then identity x 3 = two fused calls
    gnntf.set_seed(7)
    mixed = gnntf.GNN(gnntf.SparseCOO(coo, vals, shape), X)
    H0 = mixed.add(gnntf.Dense(7, regularize=False))
    for k in range(6):
        mixed.add(gnntf.PPRIteration(H0, 0.1, activation=gnntf.relu if k < 3 else gnntf.linear))
    mixed.reset(); mixed.training_mode(False)
    with torch.no_grad():
        got = mixed(mixed.features)
        mixed.fuse_runs = False
        assert torch.equal(got, mixed(mixed.features))


@pytest.mark.parametrize("C,duplicates", [(7, False), (64, False), (7, True)])
def test_relu_loop_backward_against_dense_float64(gnntf, C, duplicates):
    """The training node with relu: K iterations, each with its own dropped + renormalised adjacency (layered.py:47-50, gnn.py:37-42),
    relu after each (filter.py:22).  Forward and dH0 against the same recurrence in dense float64 with the ORACLE's per-iteration
    adjacencies (autograd on the CPU)."""
    n, K, a, p, seed, first = 300, 4, 0.1, 0.5, 5, 3
    coo, vals, shape = graphs.random_coo(n, n, 4000, seed=77, weighted=True)
    if not duplicates:                                                     # every entry once: the weights are then made inside the SpMM
        _, first_at = np.unique(coo[:, 0] * n + coo[:, 1], return_index=True)
        coo, vals = coo[np.sort(first_at)], vals[np.sort(first_at)]
    g = make_graph(gnntf, coo, vals, shape)
    assert gnntf.sparse.can_fuse_dropout(g, p) == (not duplicates)
    rng = np.random.default_rng(C)
    H0np, gout = rng.standard_normal((n, C)).astype(np.float32), rng.standard_normal((n, C)).astype(np.float32)
    if gnntf.sparse.can_fuse_dropout(g, p):
        scales = gnntf.sparse.dropped_degree_scales(g, p, seed, first, K)
        make = lambda k, bwd=False: gnntf.sparse.dropped_adjacency(g, p, seed, first + k, D=scales[k])
    else:
        make = lambda k, bwd=False: gnntf.normalize(g, "symmetric", "none", p, seed, first + k, transposed_only=bwd)
    H0 = dev(H0np).requires_grad_()
    out = gnntf.ppr_loop(make, H0, a, K, relu=True)
    out.backward(dev(gout))
    H0d = torch.tensor(H0np, dtype=torch.float64, requires_grad=True)
    H = H0d
    for k in range(K):
        ai, av = orc.get_adjacency(coo, vals, shape, graph_dropout=p, training=True, seed=seed, stream=first + k, dtype=np.float64)
        A = torch.tensor(orc.to_dense(ai, av, shape))
        H = torch.relu((1 - a) * (A @ H) + a * H0d)
    H.backward(torch.tensor(gout, dtype=torch.float64))
    np.testing.assert_allclose(out.detach().cpu().numpy(), H.detach().numpy(), rtol=RTOL, atol=ATOL)
    # a gradient element differs only where a pre-activation sits within rounding of zero: none such on this seed
    np.testing.assert_allclose(H0.grad.cpu().numpy(), H0d.grad.numpy(), rtol=1e-3, atol=1e-4)
    assert float(H0.grad.abs().max()) > 0
