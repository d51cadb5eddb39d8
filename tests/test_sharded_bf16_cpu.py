"""Opt-in bf16 storage on vertex blocks, on CPU ranks (threads exchanging through shared memory, tests/thread_comm.py): the logic
of ShardedGraph.make_state(storage=torch.bfloat16) / propagate -- which buffers are bf16, where a value is rounded, what crosses the
links -- against the float64 emulations (tests/bf16_ref.py, tests/bf16_shard_ref.py), the validation paths, and the new C entries
as far as they go without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import graphs
from bf16_ref import appnp_bf16
from bf16_shard_ref import sharded_appnp_bf16
from dist_worker import OracleBackend
from gnntf import sharded
from oracle import gnntf_oracle as orc
from thread_comm import ThreadComm, run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Bf16OracleBackend(OracleBackend):
    """The checker backend with the dtype convention of NativeBackend: a bf16 operand is widened (exactly), the sums are f32, a
    bf16 destination rounds once (torch's cast: round to nearest even), bf16 buffers are packed as bf16; mixed calls raise."""

    def _product(self, g, vals, X):
        return super()._product(g, vals, X.float() if X.dtype == torch.bfloat16 else X)

    def cast_bf16(self, src, dst):
        assert dst.dtype == torch.bfloat16 and src.dtype == torch.float32
        dst.copy_(src.to(torch.bfloat16))

    def spmm_mix(self, g, vals, X, H0, beta, alpha, out, out_rows=None, rows=None, skip_empty=False):
        if X.dtype != torch.bfloat16:
            if out.dtype != torch.float32:
                raise Exception("spmm_mix: an f32 operand needs an f32 destination")
            return super().spmm_mix(g, vals, X, H0, beta, alpha, out, out_rows=out_rows, rows=rows, skip_empty=skip_empty)
        assert H0.dtype == torch.float32 and out_rows is None
        if out.dtype == torch.float32:
            return super().spmm_mix(g, vals, X.float(), H0, beta, alpha, out, rows=rows, skip_empty=skip_empty)
        wide = out.float()                                     # rows the launch leaves alone keep their bits (bf16 -> f32 -> bf16 is exact)
        super().spmm_mix(g, vals, X.float(), H0, beta, alpha, wide, rows=rows, skip_empty=skip_empty)
        out.copy_(wide.to(torch.bfloat16))

    def halo_pack(self, plan, part, buf, send):
        if buf.dtype != send.dtype:
            raise Exception("halo_pack: the feature buffer and the send buffer must both be f32 or both bf16")
        super().halo_pack(plan, part, buf, send)               # pulled rows: copies; pushed sums: f32 products, rounded by the assignment


class CountingComm(ThreadComm):
    """ThreadComm that adds up the bytes handed to exchange_pairs."""

    def __init__(self, world, rank):
        super().__init__(world, rank)
        self.sent_bytes = 0

    def exchange_pairs(self, sends, recvs):
        self.sent_bytes += sum(t.numel() * t.element_size() for _, t in sends if t is not None)
        super().exchange_pairs(sends, recvs)


def whole_graph(n, entries, seed):
    coo, vals, _ = graphs.rmat_symmetric_coo(n, entries, seed=seed)
    ai, av = orc.get_adjacency(coo, vals, (n, n))
    rowptr, colidx, nvals = orc.coo_to_csr_coalesced(ai, av, (n, n))
    return coo, vals, sp.csr_matrix((nvals.astype(np.float64), colidx, rowptr), shape=(n, n))


def block_of(coo, vals, bounds, comm, **options):
    lo, hi = bounds[comm.rank], bounds[comm.rank + 1]
    mine = (coo[:, 0] >= lo) & (coo[:, 0] < hi)
    return sharded.ShardedGraph(torch.from_numpy(coo[mine]), torch.from_numpy(vals[mine]), bounds, backend=Bf16OracleBackend(), comm=comm,
                                keep_entries=True, **options), lo, hi


def rel_fro(got, want):
    return float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want))


# Tolerance: the project's bar for a bf16 loop against its emulation (tests/test_gpu_bf16.py): relative Frobenius error <= 1e-3.
# Measured here (checker backend, f32 sums by scipy against the float64 emulation, K = 10, a = 0.1, n = 1201 / 11000 entries,
# uniform(-1, 1) features): 4e-8 ... 8.1e-6 over all the cases below -- at least a hundred times inside the bar.  What is left is the
# f32 rounding of the sums plus the few bf16 results that the f32 sum and the float64 sum round to different neighbours.
TOL = 1e-3


@pytest.mark.parametrize("C", [12, 40])
@pytest.mark.parametrize("world,cover,split", [(3, "cover", True), (4, "pull", True), (5, "cover", "always")])
def test_bf16_blocks_match_the_emulation(world, cover, split, C):
    n, a, K = 1201, 0.1, 10
    coo, vals, A = whole_graph(n, 11000, seed=3)
    H0 = np.random.default_rng(C).uniform(-1, 1, (n, C)).astype(np.float32)
    bounds = sharded.uniform_bounds(n, world)

    def body(comm):
        sg, lo, hi = block_of(coo, vals, bounds, comm, cover=cover, split_rows=split)
        outs = {}
        for chunks in (1, 2, 3):
            state = sg.make_state(torch.from_numpy(H0[lo:hi].copy()), chunks=chunks, storage=torch.bfloat16)
            assert state.storage is torch.bfloat16 and state.H0.dtype == torch.float32 and state.result.dtype == torch.float32
            assert all(b.dtype == torch.bfloat16 for pair in state.bufs for b in pair)
            assert all(s.dtype == torch.bfloat16 and s.element_size() == 2 for s in state.send)
            for early in (False, True):
                out = sg.propagate(state, a, K, early_pull=early).clone()
                assert out.dtype == torch.float32
                assert torch.equal(out, sg.propagate(state, a, K, early_pull=early))           # repeatable on a used state
                outs[(chunks, early)] = out.numpy()
            assert torch.equal(sg.propagate(state, a, 0), torch.from_numpy(H0[lo:hi]))           # K = 0: H0, untouched
        return outs, [t.numpy() for t in sg.entries], sg.stats, bool(getattr(sg, "split_rows", False))

    parts = run_ranks(world, body)
    rows, cols, nvals, pushed = (np.concatenate([p[1][i] for p in parts]) for i in range(4))
    stats = [p[2] for p in parts]
    if split == "always":
        assert any(p[3] for p in parts)                                                        # interior / boundary handles with row maps ran
    if cover == "cover":
        assert sum(s["push_rows"] for s in stats) > 0 and pushed.any()                         # the extra rounding point is exercised
        want = sharded_appnp_bf16(rows, cols, nvals, pushed, bounds, H0, a, K)
        assert rel_fro(want.astype(np.float32), appnp_bf16(A, H0, a, K)) > 0                   # ... and it does change the result
    else:
        assert sum(s["push_rows"] for s in stats) == 0 and not pushed.any()
        want = appnp_bf16(A, H0, a, K)                                                         # a pull plan IS the one-GPU bf16 loop
        np.testing.assert_array_equal(sharded_appnp_bf16(rows, cols, nvals, pushed, bounds, H0, a, K),
                                      appnp_bf16(sp.csr_matrix((nvals.astype(np.float64), (rows, cols)), shape=(n, n)), H0, a, K))
    worst = 0.0
    for key in parts[0][0]:
        got = np.concatenate([p[0][key] for p in parts])
        err = rel_fro(got, want)
        worst = max(worst, err)
        assert err <= TOL, (world, cover, C, key, err)
        if cover == "pull":                                # the chunking and the message order change nothing about a column's sums
            np.testing.assert_array_equal(got, np.concatenate([p[0][(1, False)] for p in parts]))
    f32 = orc.appnp_propagate(coo, vals, (n, n), H0, a=a, iterations=K)
    assert rel_fro(np.concatenate([p[0][(2, False)] for p in parts]), f32.astype(np.float64)) > 1e-5          # bf16 did run
    print(f"world {world} {cover} C {C}: worst relative Frobenius error against the emulation {worst:.3e}")


def test_shard_emulation_without_pushed_entries_is_the_one_gpu_emulation():
    n, C, a = 700, 9, 0.1
    coo, vals, A = whole_graph(n, 6000, seed=4)
    H0 = np.random.default_rng(0).uniform(-1, 1, (n, C)).astype(np.float32)
    A = A.tocoo()
    for K in (0, 1, 2, 7):
        for bounds in ([0, n], sharded.uniform_bounds(n, 3)):
            got = sharded_appnp_bf16(A.row, A.col, A.data, None, bounds, H0, a, K)
            np.testing.assert_array_equal(got, appnp_bf16(A.tocsr(), H0, a, K))
    # one pushed entry is one more rounding: the results differ, by no more than u * |value * H~| in that row after one iteration
    pushed = np.zeros(A.nnz, dtype=bool)
    cross = np.nonzero((A.row < n // 2) & (A.col >= n // 2))[0]
    pushed[cross[0]] = True
    one = sharded_appnp_bf16(A.row, A.col, A.data, pushed, [0, n // 2, n], H0, a, 1)
    ref = appnp_bf16(A.tocsr(), H0, a, 1)
    delta = np.abs(one - ref)
    assert delta.max() > 0 and (np.delete(delta, A.row[cross[0]], axis=0) == 0).all()
    assert delta.max() <= 2.0 ** -8 * abs(A.data[cross[0]]) * 1.0


def test_single_block_runs_the_bf16_launches():
    n, C, a, K = 900, 12, 0.1, 10
    coo, vals, A = whole_graph(n, 8000, seed=5)
    H0 = np.random.default_rng(1).uniform(-1, 1, (n, C)).astype(np.float32)

    def body(comm):
        sg, lo, hi = block_of(coo, vals, [0, n], comm)
        state = sg.make_state(torch.from_numpy(H0.copy()), storage=torch.bfloat16)
        assert all(b.dtype == torch.bfloat16 for b in state.bufs) and state.result.dtype == torch.float32
        out = sg.propagate(state, a, K).clone()
        assert torch.equal(out, sg.propagate(state, a, K))
        start = torch.from_numpy(H0[::-1].copy())
        return out.numpy(), sg.propagate(state, a, 1, start=start).clone().numpy()

    (got, stepped), = run_ranks(1, body)
    assert rel_fro(got, appnp_bf16(A, H0, a, K)) <= TOL
    from bf16_ref import bf16_round
    want = float(np.float32(0.9)) * (A @ bf16_round(H0[::-1]).astype(np.float64)) + float(np.float32(0.1)) * H0.astype(np.float64)
    assert rel_fro(stepped, want) <= 1e-5                  # start= : bf(start) is gathered, f32 H0 is mixed in


def test_bf16_halves_the_bytes_on_the_links():
    n, C, K = 1201, 40, 4
    coo, vals, _ = whole_graph(n, 11000, seed=3)
    H0 = np.random.default_rng(2).uniform(-1, 1, (n, C)).astype(np.float32)
    world = 3
    bounds = sharded.uniform_bounds(n, world)

    def body(comm):
        comm = CountingComm(comm.world, comm.rank)
        sg, lo, hi = block_of(coo, vals, bounds, comm, cover="cover", tune_overlap=False)
        counts = {}
        for storage in (torch.float32, torch.bfloat16):
            state = sg.make_state(torch.from_numpy(H0[lo:hi].copy()), storage=storage)
            assert all(s.element_size() == (2 if storage is torch.bfloat16 else 4) for s in state.send)
            for early in (False, True):
                before = comm.sent_bytes
                sg.propagate(state, 0.1, K, early_pull=early)
                counts[(storage, early)] = comm.sent_bytes - before
        return counts, sg.n_send

    for counts, n_send in run_ranks(world, body):
        assert n_send > 0
        for early in (False, True):
            assert counts[(torch.float32, early)] == K * n_send * C * 4               # every outgoing row, once per iteration
            assert 2 * counts[(torch.bfloat16, early)] == counts[(torch.float32, early)]


def test_validation():
    n = 300
    coo, vals, _ = whole_graph(n, 2000, seed=6)
    H0 = torch.zeros(n, 8)

    def body(comm):
        sg, lo, hi = block_of(coo, vals, [0, n], comm)
        with pytest.raises(Exception, match="storage must be torch.float32 or torch.bfloat16"):
            sg.make_state(H0, storage=torch.float16)
        relabelled, _, _ = block_of(coo, vals, [0, n], comm, relabel=True)
        assert relabelled.row_order is not None
        with pytest.raises(Exception, match="relabelled block"):
            relabelled.make_state(H0, storage=torch.bfloat16)
        relabelled.make_state(H0)                                                      # f32 keeps working
        training, _, _ = block_of(coo, vals, [0, n], comm, edge_dropout=True)
        with pytest.raises(Exception, match="training block"):
            training.make_state(H0, storage=torch.bfloat16)
        # a mixed call is refused by the backend convention, not rounded silently
        state = sg.make_state(H0, storage=torch.bfloat16)
        with pytest.raises(Exception, match="f32 destination"):
            sg.backend.spmm_mix(sg.graph, None, state.H0, state.H0, 0.9, 0.1, state.bufs[1])
        import gnntf
        gnntf.set_default_device(torch.device("cpu"))
        try:
            model = gnntf.Trainable(torch.zeros(n, 6))
            head = model.add(gnntf.Dense(4))
            with pytest.raises(Exception, match="inference_dtype must be torch.float32 or torch.bfloat16"):
                model.add(sharded.ShardedPPRLoop(head, sg, 0.1, 10, inference_dtype=torch.float16))
            model.add(sharded.ShardedPPRLoop(head, sg, 0.1, 10, inference_dtype=torch.bfloat16))
        finally:
            gnntf.set_default_device(None)
        return True

    assert run_ranks(1, body) == [True]


def test_native_backend_refuses_mixed_dtypes():
    """NativeBackend's dispatch rules raise before anything reaches the library."""
    from gnntf.shard_backend import NativeBackend
    be = NativeBackend()
    plan = type("Plan", (), {"n_send": 3})()
    with pytest.raises(Exception, match="both be f32 or both bf16"):
        be.halo_pack(plan, "all", torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(3, 8))
    with pytest.raises(Exception, match="both be f32 or both bf16"):
        be.halo_pack(plan, "pull", torch.zeros(4, 8), torch.zeros(3, 8, dtype=torch.bfloat16))
    with pytest.raises(Exception, match="f32 operand needs an f32 destination"):
        be.spmm_mix(None, None, torch.zeros(4, 8), torch.zeros(4, 8), 0.9, 0.1, torch.zeros(4, 8, dtype=torch.bfloat16))
    with pytest.raises(Exception, match="no scatter map"):
        be.spmm_mix(None, None, torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(4, 8), 0.9, 0.1, torch.zeros(4, 8),
                    out_rows=torch.zeros(4, dtype=torch.int32))


def test_default_state_is_the_f32_path_bit_for_bit():
    n, C, a, K = 1003, 12, 0.1, 10
    coo, vals, _ = whole_graph(n, 9000, seed=5)
    H0 = np.random.default_rng(1).uniform(-1, 1, (n, C)).astype(np.float32)
    world = 3
    bounds = sharded.uniform_bounds(n, world)

    def body(comm):
        sg, lo, hi = block_of(coo, vals, bounds, comm)
        plain = sg.make_state(torch.from_numpy(H0[lo:hi].copy()))
        assert plain.storage is torch.float32
        tensors = [plain.H0, plain.result] + [b for pair in plain.bufs for b in pair] + list(plain.send)
        assert all(t.dtype == torch.float32 for t in tensors)
        out = sg.propagate(plain, a, K).clone()
        named = sg.make_state(torch.from_numpy(H0[lo:hi].copy()), storage=torch.float32)
        assert torch.equal(out, sg.propagate(named, a, K))
        return out.numpy()

    got = np.concatenate(run_ranks(world, body))
    np.testing.assert_allclose(got, orc.appnp_propagate(coo, vals, (n, n), H0, a=a, iterations=K), rtol=1e-4, atol=1e-5)


# ---- the C entries, as far as they go without a GPU ---------------------------------------------------------------------------
def test_new_entries_are_exported_and_check_their_arguments():
    from gnntf import _native
    lib = _native.lib()
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name in ("gnx_spmm_rows_bf16", "gnx_halo_pack_bf16", "gnx_halo_exchange_bf16"):
        assert hasattr(raw, name) and name in _native.SIGNATURES
    assert lib.gnx_version() == 900 == _native.ABI_VERSION
    assert lib.gnx_halo_pack_bf16(None, _native.HALO_ALL, None, 8, 8, None, 8, None) == -1 and b"NULL plan" in lib.gnx_last_error()
    assert lib.gnx_halo_exchange_bf16(None, _native.HALO_ALL, None, None, None, 8, None) == -1 and b"NULL plan" in lib.gnx_last_error()
    assert lib.gnx_spmm_rows_bf16(None, None, None, 8, 8, None, 0, 0.9, 0.1, 0, None, None, 1, 8, None) == -1
    assert b"gnx_spmm_rows_bf16: NULL handle" in lib.gnx_last_error()
    P = 3
    arr = lambda xs: (ctypes.c_int64 * P)(*xs)
    fake_device_list = ctypes.c_void_p(4096)                     # borrowed, never read by the plan's host code
    plan = ctypes.c_void_p()
    assert lib.gnx_halo_plan_create(P, 1, 50, arr([2, 0, 1]), arr([0] * P), arr([1, 0, 3]), arr([0] * P), fake_device_list, None,
                                    ctypes.byref(plan)) == 0
    assert lib.gnx_halo_pack_bf16(plan, 99, None, 0, 0, None, 0, None) == -1 and b"gnx_halo_pack_bf16: invalid part" in lib.gnx_last_error()
    assert lib.gnx_halo_pack_bf16(plan, _native.HALO_PULL, None, 8, 8, None, 8, None) == -1 and b"NULL buffer" in lib.gnx_last_error()
    assert lib.gnx_halo_exchange_bf16(plan, 7, fake_device_list, None, None, 8, None) == -1 and b"invalid part" in lib.gnx_last_error()
    assert lib.gnx_halo_exchange_bf16(plan, _native.HALO_ALL, None, None, None, 8, None) == -1
    assert lib.gnx_halo_plan_destroy(plan) == 0
    empty = ctypes.c_void_p()
    assert lib.gnx_halo_plan_create(P, 1, 50, arr([0] * P), arr([0] * P), arr([0] * P), arr([0] * P), None, None, ctypes.byref(empty)) == 0
    for part in (_native.HALO_ALL, _native.HALO_PULL, _native.HALO_PUSH):          # nothing to send: GNX_OK before the buffers are looked at
        assert lib.gnx_halo_pack_bf16(empty, part, None, 0, 0, None, 0, None) == 0
    assert lib.gnx_halo_plan_destroy(empty) == 0
