"""Opt-in bf16 storage on vertex blocks, on the MI355X: the bf16 pack (gather + pushed sums), the bf16 row-map SpMM, the whole
propagation over all P blocks of one graph on this GPU (ranks as threads, tests/thread_comm.py) -- bitwise against the one-GPU bf16
loop for pull plans, inside the first-order bound of the f32 loop for cover plans, against the float64 emulation on a small graph --
the model-level switch, and the RCCL transport of bf16 rows from a plain C client."""
import os
import subprocess

import numpy as np
import pytest
import torch

from bf16_ref import U
from bf16_shard_ref import sharded_appnp_bf16

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = torch.device("cuda:0")


@pytest.fixture(scope="module")
def gnntf():
    import gnntf
    gnntf.set_default_device("cuda:0")
    yield gnntf
    gnntf.set_default_device(None)


def bits(t):
    return t.view(torch.int16)


def random_bf16(shape, seed):
    g = torch.Generator(device=DEVICE).manual_seed(seed)
    return (torch.rand(shape, device=DEVICE, generator=g) * 2 - 1).to(torch.bfloat16)


# ---- 1. gnx_halo_pack_bf16 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["packed", "strided", "odd_offset"])
def test_halo_pack_bf16_is_a_copy_and_one_rounding(gnntf, layout):
    """Pull half: bitwise Xb.index_select(0, src) at every unit width (16 / 8 / 4 / 2 bytes), with a strided source and with storage
    that is only 2-byte aligned.  Push half: bitwise gnx_spmm_bf16 over the push graph with out_bf16 = 1 into a separate buffer."""
    from gnntf import _native as nat
    from gnntf.shard_backend import NativeBackend, NativeHaloPlan
    from test_gpu_bf16 import hub_graph
    be = NativeBackend()
    n_local, n_pull, n_push = 5000, 3001, 700
    rng = np.random.default_rng(1)
    src = torch.from_numpy(rng.integers(0, n_local, n_pull).astype(np.int32)).to(DEVICE)
    coo, vals, shape = hub_graph(n_push, n_local, seed=2, hubs=(600, 1400))
    push_graph = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device=DEVICE)
    # rank 1 of 2: region(0) = [10 pulled | 5 pushed] rows comes first, so the local rows start at row 15 of the buffer
    plan = NativeHaloPlan(1, n_local, [10, 0], [5, 0], [n_pull, 0], [n_push, 0], src, push_graph)
    assert (plan.local_row0, plan.n_buf, plan.n_send, plan.n_send_pull) == (15, n_local + 15, n_pull + n_push, n_pull)
    for C in (1, 7, 8, 12, 40, 64, 128, 260):
        ld = C if layout != "strided" else C + 3
        off = 1 if layout == "odd_offset" else 0
        flat = random_bf16(plan.n_buf * ld + off, seed=C)
        Xb = flat[off:].view(plan.n_buf, ld)[:, :C]
        local = Xb[plan.local_row0:plan.local_row0 + n_local]
        sflat = torch.zeros(plan.n_send * C + off, dtype=torch.bfloat16, device=DEVICE)
        send = sflat[off:].view(plan.n_send, C)
        assert Xb.data_ptr() % 4 == (2 if off else 0)
        # whole pack, and the two halves one by one into a second buffer
        be.halo_pack(plan, "all", Xb, send)
        halves = torch.zeros_like(sflat)[off:].view(plan.n_send, C)
        be.halo_pack(plan, "pull", Xb, halves)
        assert torch.equal(bits(halves[n_pull:]), torch.zeros_like(bits(halves[n_pull:])))        # the pull half leaves the push half alone
        be.halo_pack(plan, "push", Xb, halves)
        assert torch.equal(bits(send), bits(halves))
        assert torch.equal(bits(send[:n_pull]), bits(local.index_select(0, src.long()))), (layout, C)
        # the push half against the plain bf16 SpMM of the same handle, written at the same place of a buffer of its own
        other = torch.zeros_like(sflat)[off:].view(plan.n_send, C)
        nat.check(nat.lib().gnx_spmm_bf16(push_graph.handle, None, None, nat.ptr(local), ld, C, None, 0, 1.0, 0.0, nat.ACT_NONE,
                                          nat.ptr(other[n_pull:]), 1, C, nat.current_stream()))
        assert torch.equal(bits(send[n_pull:]), bits(other[n_pull:])), (layout, C)
        assert push_graph.last_kernel().endswith("_bf16")
    with pytest.raises(Exception, match="both be f32 or both bf16"):
        be.halo_pack(plan, "all", Xb, torch.zeros((plan.n_send, C), device=DEVICE))


# ---- 2. gnx_spmm_rows_bf16 ----------------------------------------------------------------------------------------------------------
def test_spmm_rows_bf16_is_the_compact_launch_scattered(gnntf):
    """Bitwise gnx_spmm_bf16 on the same compacted handle followed by a scatter through ``rows`` (H0 gathered through ``rows``): f32
    and bf16 results, with and without GNX_ACT_SKIP_EMPTY, in every row class (wave, 32 / 16 / 8-lane groups, long rows through the
    chunk kernels, the merged chunks launch)."""
    from gnntf import sparse, _native as nat
    from test_gpu_bf16 import hub_graph
    m, n_cols, n_out = 3000, 3500, 4200
    coo, vals, shape = hub_graph(m, n_cols, seed=7)
    g = gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device=DEVICE)
    adj = sparse.Adjacency(g)
    rng = np.random.default_rng(3)
    rows = torch.from_numpy(np.sort(rng.choice(n_out, size=m, replace=False)).astype(np.int32)).to(DEVICE)
    empty = torch.from_numpy(np.diff(g.csr_arrays()[0].cpu().numpy()) == 0).to(DEVICE)
    assert bool(empty.any())
    names = set()
    for i, C in enumerate((1, 7, 8, 17, 40, 64, 128, 260, 512)):
        Xb = random_bf16((n_cols, C), seed=10 + i)
        H0 = torch.rand((n_out, C), device=DEVICE, generator=torch.Generator(device=DEVICE).manual_seed(i)) * 2 - 1
        for out_dtype in (torch.float32, torch.bfloat16):
            for skip in (False, True):
                act = (nat.ACT_RELU if i % 2 else nat.ACT_NONE) | (nat.ACT_SKIP_EMPTY if skip else 0)
                got = torch.full((n_out, C), 7.0, dtype=out_dtype, device=DEVICE)
                sparse.launch_rows_bf16(adj, Xb, H0, 0.9, 0.35, rows, got, act=act)
                names.add(g.last_kernel())
                compact = torch.full((m, C), 7.0, dtype=out_dtype, device=DEVICE)
                sparse._launch_bf16(adj, Xb, H0.index_select(0, rows.long()), 0.9, 0.35, act, out=compact)
                want = torch.full((n_out, C), 7.0, dtype=out_dtype, device=DEVICE)
                want[rows.long()] = compact
                view = bits if out_dtype is torch.bfloat16 else (lambda t: t.view(torch.int32))
                assert torch.equal(view(got), view(want)), (C, out_dtype, skip)
                if skip:
                    assert bool((compact[empty] == 7.0).all()) and not bool((compact[~empty] == 7.0).all())
    assert all(n.endswith("_bf16") for n in names), names
    classes = {n.split("+")[0].replace("_bf16", "") for n in names}
    assert {"spmm_wave", "spmm_group32", "spmm_group16", "spmm_group8"} <= classes, names
    assert any("+chunks_bf16" in n for n in names) and any("+long_bf16" in n for n in names), names


# ---- 3. all P blocks of one graph on this GPU -----------------------------------------------------------------------------------------
def rmat_blocks(n, entries, C, seed=1):
    from gnntf import sharded
    u, w = sharded.rmat_relabelled_pairs(n, entries // 2, seed=seed, device=DEVICE)
    H0 = torch.rand(n, C, device=DEVICE, generator=torch.Generator(device=DEVICE).manual_seed(2)) * 2 - 1
    return u, w, H0


def block_entries(u, w, lo, hi):
    mu, mw = (u >= lo) & (u < hi), (w >= lo) & (w < hi)
    return torch.cat([torch.stack([u[mu], w[mu]], 1), torch.stack([w[mw], u[mw]], 1)])


def whole_adjacency(gnntf, u, w, n):
    idx = torch.cat([torch.stack([u, w], 1), torch.stack([w, u], 1)])
    return gnntf.normalize(gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], device=DEVICE), (n, n)), device=DEVICE), "symmetric")


def test_pull_plan_is_the_one_gpu_bf16_loop_bitwise(gnntf):
    """A pull plan has no pushed rows, so it performs exactly the roundings of gnx_appnp_propagate_bf16, and every row's entries stay
    in ascending global column order: under the matching conditions of test_pull_plan_keeps_the_one_gpu_summation_order_bitwise (the
    one-GPU reference runs each 64-column chunk on its own, both structures above 2^20 rows) the K = 10 results are IDENTICAL."""
    from gnntf import sharded, sparse
    from thread_comm import run_ranks
    world, n, entries, C = 2, 4_400_000, 52_000_000, 128
    u, w, H0 = rmat_blocks(n, entries, C)
    bounds = sharded.uniform_bounds(n, world)

    def rank_body(comm, row_window=0):
        lo, hi = bounds[comm.rank], bounds[comm.rank + 1]
        idx = block_entries(u, w, lo, hi)
        sg = sharded.ShardedGraph(idx, torch.ones(idx.shape[0], device=DEVICE), bounds, comm=comm, cover="pull", chunks=2, row_window=row_window)
        state = sg.make_state(H0[lo:hi], storage=torch.bfloat16)
        assert [c1 - c0 for c0, c1 in state.cols] == [64, 64] and state.send[0].dtype == torch.bfloat16
        out = sg.propagate(state, 0.1, 10).clone()
        assert sg.graph.last_kernel().endswith("_bf16")
        assert torch.equal(out, sg.propagate(state, 0.1, 10))                        # twice the same bits
        return out

    got = torch.cat(run_ranks(world, rank_body))
    windowed = torch.cat(run_ranks(world, lambda comm: rank_body(comm, 4096)))
    assert torch.equal(windowed, got)
    whole = whole_adjacency(gnntf, u, w, n)
    want = torch.cat([sparse._appnp_propagate_bf16(whole, H0[:, c0:c0 + 64].contiguous(), 0.1, 10, False) for c0 in (0, 64)], dim=1)
    assert whole.graph.last_kernel().endswith("_bf16")
    assert torch.equal(got, want), float((got - want).abs().max())
    f32 = torch.cat([gnntf.appnp_propagate(whole, H0[:, c0:c0 + 64].contiguous(), 0.1, 10) for c0 in (0, 64)], dim=1)
    assert not torch.equal(got, f32)                                                  # bf16 did run


@pytest.mark.parametrize("world,n,entries,C", [(8, 8_000_000, 100_000_000, 128), (3, 1_000_003, 12_000_000, 40)])
def test_cover_plan_stays_inside_the_first_order_bound(gnntf, world, n, entries, C):
    """Cover plans (pushed partial sums rounded once by their senders), as in test_vertex_blocks_of_one_graph_match_one_gpu.  Per
    column ||got - f32||_2 <= 1.05 (u/a) (max_k ||H_k||_2 + max_k ||A_hat |H_k| ||_2): the first term is the bound of the one-GPU bf16
    loop (each iterate rounded once, ||A_hat||_2 <= 1 on a symmetric pattern, the geometric sum over k gives 1/a); the second bounds
    the pushed-sum roundings, |sum_q (bf(s_iq) - s_iq)| <= u (A_hat |H~_k|)_i.  f32 = the one-GPU f32 loop, H_k its iterates.
    Measured on the MI355X: worst ||got - f32|| / bound 0.0016 (world 8; argmax agreement 0.99928) and 0.0018 (world 3; 0.99958)."""
    from gnntf import sharded, sparse
    from thread_comm import run_ranks
    a, K = 0.1, 10
    u, w, H0 = rmat_blocks(n, entries, C)
    bounds = sharded.uniform_bounds(n, world)

    def rank_body(comm):
        lo, hi = bounds[comm.rank], bounds[comm.rank + 1]
        idx = block_entries(u, w, lo, hi)
        sg = sharded.ShardedGraph(idx, torch.ones(idx.shape[0], device=DEVICE), bounds, comm=comm, cover="cover", chunks=2)
        state = sg.make_state(H0[lo:hi], storage=torch.bfloat16)
        out = sg.propagate(state, a, K).clone()
        assert sg.graph.last_kernel().endswith("_bf16")
        assert torch.equal(out, sg.propagate(state, a, K))                           # deterministic
        return out, sg.stats

    parts = run_ranks(world, rank_body)
    got = torch.cat([p[0] for p in parts])
    assert sum(p[1]["push_rows"] for p in parts) > 0
    del parts
    whole = whole_adjacency(gnntf, u, w, n)
    norm_h = torch.zeros(C, dtype=torch.float64, device=DEVICE)
    norm_ah = torch.zeros(C, dtype=torch.float64, device=DEVICE)
    ref = None
    for k in range(K + 1):
        ref = gnntf.appnp_propagate(whole, H0, a, k)
        norm_h = torch.maximum(norm_h, ref.double().norm(dim=0))
        norm_ah = torch.maximum(norm_ah, gnntf.spmm(whole, ref.abs()).double().norm(dim=0))
    bound = 1.05 * (U / a) * (norm_h + norm_ah)
    delta = (got.double() - ref.double()).norm(dim=0)
    agree = (got.argmax(1) == ref.argmax(1)).float().mean().item()
    print(f"world {world} C {C}: worst ||got - f32|| / bound = {float((delta / bound).max()):.4f}, argmax agreement {agree:.6f}")
    assert bool((delta > 0).all())
    assert bool((delta <= bound).all()), (float((delta / bound).max()), "argmax agreement with the f32 result: %.6f" % agree)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("C", [40, 64])
def test_small_cover_plan_against_the_emulation(gnntf, world, C):
    """n = 4000 on the GPU kernels against tests/bf16_shard_ref.py (pushed sums rounded per sender): relative Frobenius <= 1e-3, the
    project's bar for a bf16 loop against its emulation (tests/test_gpu_bf16.py).  Measured on the MI355X: 4e-8 ... 1.1e-5."""
    import graphs
    from gnntf import sharded
    from thread_comm import run_ranks
    n, a, K = 4000, 0.1, 10
    coo, vals, _ = graphs.rmat_symmetric_coo(n, 30000, seed=C + world)
    H0 = np.random.default_rng(C).uniform(-1, 1, (n, C)).astype(np.float32)
    bounds = sharded.uniform_bounds(n, world)

    def rank_body(comm):
        lo, hi = bounds[comm.rank], bounds[comm.rank + 1]
        mine = (coo[:, 0] >= lo) & (coo[:, 0] < hi)
        sg = sharded.ShardedGraph(torch.from_numpy(coo[mine]).to(DEVICE), torch.from_numpy(vals[mine]).to(DEVICE), bounds, comm=comm,
                                  cover="cover", split_rows="always", keep_entries=True)
        state = sg.make_state(torch.from_numpy(H0[lo:hi].copy()).to(DEVICE), storage=torch.bfloat16)
        out = sg.propagate(state, a, K).clone()
        early = sg.propagate(state, a, K, early_pull=True)
        assert torch.equal(out, early)                                               # two messages per peer: the same bytes in the same places
        return out.cpu().numpy(), [t.cpu().numpy() for t in sg.entries], sg.stats["push_rows"], sg.graph.last_kernel()

    parts = run_ranks(world, rank_body)
    assert sum(p[2] for p in parts) > 0 and all(p[3].endswith("_bf16") for p in parts)
    rows, cols, nvals, pushed = (np.concatenate([p[1][i] for p in parts]) for i in range(4))
    want = sharded_appnp_bf16(rows, cols, nvals, pushed, bounds, H0, a, K)
    got = np.concatenate([p[0] for p in parts]).astype(np.float64)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"world {world} C {C}: relative Frobenius error against the shard emulation {err:.3e}")
    assert err <= 1e-3, err
    # fixed_point_error / time_compute / time_exchange run on a bf16 state (deviation of bf16 size, not 1e-5)
    def measure(comm):
        lo, hi = bounds[comm.rank], bounds[comm.rank + 1]
        mine = (coo[:, 0] >= lo) & (coo[:, 0] < hi)
        sg = sharded.ShardedGraph(torch.from_numpy(coo[mine]).to(DEVICE), torch.ones(int(mine.sum()), device=DEVICE), bounds, comm=comm)
        state = sg.make_state(torch.zeros((hi - lo, C), device=DEVICE), storage=torch.bfloat16)
        assert sg.time_exchange(state, repeats=1) >= 0 and sg.time_compute(state, repeats=1) > 0
        return sg.fixed_point_error(state, a, K)
    errs = run_ranks(world, measure)
    # elementwise |e_K| <= u sum_k (1-a)^k |A_hat|^k |H| <= (u / a) H for the positive eigenvector H (to first order)
    assert all(1e-6 < e < U / a for e in errs), errs


def test_single_block_bf16_is_the_one_gpu_loop(gnntf):
    """World size 1: no exchange, the same per-iteration bf16 launches -- bitwise gnx_appnp_propagate_bf16 on the same structure."""
    import graphs
    from gnntf import sharded, sparse
    from thread_comm import run_ranks
    n, C = 4000, 40
    coo, vals, _ = graphs.rmat_symmetric_coo(n, 30000, seed=8)
    H0 = torch.from_numpy(np.random.default_rng(8).uniform(-1, 1, (n, C)).astype(np.float32)).to(DEVICE)

    def body(comm):
        sg = sharded.ShardedGraph(torch.from_numpy(coo).to(DEVICE), torch.from_numpy(vals).to(DEVICE), [0, n], comm=comm)
        state = sg.make_state(H0, storage=torch.bfloat16)
        out = sg.propagate(state, 0.1, 10).clone()
        assert sg.graph.last_kernel().endswith("_bf16") and sg.time_compute(state, repeats=1) > 0
        return out

    got, = run_ranks(1, body)
    whole = gnntf.normalize(gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, (n, n)), device=DEVICE), "symmetric")
    assert torch.equal(got, sparse._appnp_propagate_bf16(whole, H0, 0.1, 10, False))


# ---- 4. the model level -----------------------------------------------------------------------------------------------------------------
def test_sharded_ppr_loop_inference_dtype(gnntf):
    """ShardedPPRLoop(inference_dtype=torch.bfloat16) over two thread ranks: predict() (eval, no autograd) runs the bf16 kernels; a
    forward that autograd records is bit for bit the f32 model's.  The backward of a multi-block model runs collectives inside
    autograd's single per-device worker thread, which thread ranks cannot do: the whole training step (loss + gradients) is compared
    on a one-block model, the recorded forward on two blocks."""
    import graphs
    from gnntf import sharded
    from gnntf.training import _Objective
    from thread_comm import run_ranks
    n, F, hidden, classes, K, a = 4000, 24, 16, 7, 10, 0.1
    coo, vals, _ = graphs.rmat_symmetric_coo(n, 30000, seed=12)
    rng = np.random.default_rng(12)
    X = rng.standard_normal((n, F)).astype(np.float32)
    labels = rng.integers(0, classes, size=n)

    def models(sg, lo, hi):
        out = []
        for dtype in (torch.float32, torch.bfloat16):
            model = gnntf.Trainable(torch.from_numpy(X[lo:hi]).to(DEVICE))
            model.add(gnntf.Dense(hidden, activation=gnntf.relu))
            head = model.add(gnntf.Dense(classes, regularize=False))
            model.add(sharded.ShardedPPRLoop(head, sg, a, K, inference_dtype=dtype))
            model.reset()
            out.append((model, head))
        for v32, v16 in zip(out[0][0].vars(), out[1][0].vars()):
            v16.var.data.copy_(v32.var.data)
        return out

    def body(comm):
        bounds = sharded.uniform_bounds(n, comm.size)
        lo, hi = bounds[comm.rank], bounds[comm.rank + 1]
        mine = (coo[:, 0] >= lo) & (coo[:, 0] < hi)
        sg = sharded.ShardedGraph(torch.from_numpy(coo[mine]).to(DEVICE), torch.from_numpy(vals[mine]).to(DEVICE), bounds, comm=comm)
        logits, kernels, recorded, steps, h0sq = [], [], [], [], 0.0
        for model, head in models(sg, lo, hi):
            model.training_mode(False)
            pred = model.predict(gnntf.NodeClassification(list(range(hi - lo))))
            kernels.append(sg.graph.last_kernel())
            assert pred.shape[0] == hi - lo
            with torch.no_grad():
                logits.append(model(model.features).clone())
            h0sq = float(head.value.detach().double().pow(2).sum())               # this rank's rows of the propagation's H0
            recorded.append(model(model.features).detach().clone())              # grad enabled: the autograd node, f32
            assert not sg.graph.last_kernel().endswith("_bf16")
            if comm.size == 1:
                task = gnntf.NodeClassification(np.arange(300), labels[:300])
                params = [v.var for v in model.vars() if v.trainable]
                with model:
                    loss = _Objective(model, task, 5e-4)()
                    loss.backward()
                steps.append([loss.detach().clone()] + [p.grad.clone() for p in params])
                assert not sg.graph.last_kernel().endswith("_bf16")
        return logits, kernels, recorded, steps, h0sq

    for world in (2, 1):
        parts = run_ranks(world, body)
        # ||bf16 - f32||_F <= 1.05 (u/a) (max_k ||H_k|| + max_k ||A_hat |H_k| ||) <= 1.05 (2u/a) ||H0||_F: ||A_hat||_2 <= 1 and
        # ||H_{k+1}|| <= (1-a) ||H_k|| + a ||H0|| <= ||H0|| (all ranks' rows together; bf16 must also have changed something)
        diff = sum(float((p[0][0].double() - p[0][1].double()).pow(2).sum()) for p in parts) ** 0.5
        assert 0 < diff <= 1.05 * (2 * U / a) * sum(p[4] for p in parts) ** 0.5, diff
        for logits, kernels, recorded, steps, _ in parts:
            assert not kernels[0].endswith("_bf16") and kernels[1].endswith("_bf16"), kernels
            assert torch.equal(recorded[0], recorded[1]) and torch.equal(recorded[0], logits[0])
            if world == 1:
                assert len(steps) == 2 and len(steps[0]) == len(steps[1]) > 1
                for x, y in zip(*steps):
                    assert torch.equal(x, y)


# ---- 5. bf16 rows over RCCL ---------------------------------------------------------------------------------------------------------------
def test_bf16_halo_exchange_over_rccl_loop_back(tmp_path):
    """tests/c_abi_rccl_bf16.c: pulled bf16 rows and rounded pushed sums through ncclSend / ncclRecv of ncclBfloat16 elements (one
    rank listing itself as peer; one group, then two groups with bound entry points): received regions == packed send slices."""
    exe = str(tmp_path / "c_abi_rccl_bf16")
    lib = os.path.join(ROOT, "gnn-tf_amd", "lib")
    subprocess.check_call(["gcc", "-std=c11", "-D_DEFAULT_SOURCE", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_abi_rccl_bf16.c"), "-L", lib, "-lgnx", "-L/opt/rocm/lib", "-lamdhip64", "-lrccl", "-lm",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0 and "RCCL bf16 loop-back OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
