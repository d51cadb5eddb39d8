#!/usr/bin/env python3
"""ONE rank's block of the config-5 graph (tools/sim_blocks.py: the block bench.py --gpus P would build, loop-back communicator) with
f32 and with bf16 storage (ShardedGraph.make_state(storage=torch.bfloat16)), on one GPU: the three launches of an iteration --
the block's own SpMM (interior + boundary rows, every column chunk), the pull pack (a gather) and the push pack (the SpMM over the
push graph) -- timed one by one, f32 and bf16 interleaved in one process, and the halo bytes an iteration puts on the links.

    python tools/halo_bf16_bench.py [--worlds 8 4 2] [--feats 128] [--chunks 2] [--reps 20] [--warm 5]

Every world size runs in a child process of its own under `timeout -k 10` (no retry: the first child that fails ends the run).  Per
launch: `warm` warm-ups of each storage, then `reps` rounds of one f32 and one bf16 call, each between device events; reported: median
and quartiles, the ratio of the medians, and `bf16_slower` = the bf16 lower quartile is above the f32 upper quartile (slower by more
than the spread of the repetitions).  The yardstick is the f32 block's launch in the same process.
This is ONE rank's block on ONE GPU: no multi-GPU step is measured, and the halving of the link bytes is by construction (2-byte
rows in the same plan), not a measured speed-up.  Prints one JSON record."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnn-tf_amd"), os.path.join(ROOT, "tools")]


def quartiles(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]
    return dict(median_ms=round(q(0.5), 4), p25_ms=round(q(0.25), 4), p75_ms=round(q(0.75), 4))


def child(a):
    import torch
    import gnntf
    from gnntf import sharded
    from sim_blocks import LoopbackComm, SimGraph
    dev = torch.device("cuda:0")
    gnntf.set_default_device(dev)
    P, r, N, C = a.world, a.rank, a.nodes, a.feats
    u, w = sharded.rmat_relabelled_pairs(N, a.entries // 2, seed=1, device=dev)
    degrees = (torch.bincount(u, minlength=N) + torch.bincount(w, minlength=N)).float()
    bounds = sharded.uniform_bounds(N, P)
    lo, hi = bounds[r], bounds[r + 1]
    mu, mw = (u >= lo) & (u < hi), (w >= lo) & (w < hi)
    idx = torch.cat([torch.stack([u[mu], w[mu]], 1), torch.stack([w[mw], u[mw]], 1)])
    del u, w, mu, mw
    comm = LoopbackComm(P, r, degrees, "copy")
    sg = SimGraph(idx, torch.ones(idx.shape[0], dtype=torch.float32, device=dev), bounds, comm=comm, cover=a.cover, chunks=a.chunks,
                  keep_entries=True)
    sg.entries = None
    del idx, comm.mirrored
    torch.cuda.empty_cache()
    H0 = torch.rand(sg.n_local, C, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) * 2 - 1
    states = {"f32": sg.make_state(H0), "bf16": sg.make_state(H0, storage=torch.bfloat16)}
    kernels = {}
    for name, state in states.items():                      # real iterates in both ping-pong buffers and both send buffers
        sg.propagate(state, 0.1, 3)
        kernels[name] = sg.graph.last_kernel()
    every = range(len(states["f32"].cols))

    def launches(state):
        src = lambda c: state.bufs[c][0]
        dst = lambda c: sg.local_view(state.bufs[c][1])

        def main_spmm():                                    # a steady-state iteration (rows without entries settled)
            for c in every:
                sg._compute(state, c, src(c), dst(c), 0.1, interior=True, skip_empty=True)
                sg._compute(state, c, src(c), dst(c), 0.1, interior=False, skip_empty=True)
        return {"main_spmm": main_spmm,
                "pull_pack": lambda: [sg._pack(state, c, state.bufs[c][1], "pull") for c in every],
                "push_pack": lambda: [sg._pack(state, c, state.bufs[c][1], "push") for c in every]}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    fns = {name: launches(state) for name, state in states.items()}
    rec = {}
    for key in ("main_spmm", "pull_pack", "push_pack"):
        for _ in range(a.warm):
            for name in fns:
                fns[name][key]()
        times = {name: [] for name in fns}
        for _ in range(a.reps):
            for name in fns:
                times[name].append(timed(fns[name][key]))
        q32, q16 = quartiles(times["f32"]), quartiles(times["bf16"])
        rec[key] = dict(f32=q32, bf16=q16, f32_over_bf16=round(q32["median_ms"] / max(q16["median_ms"], 1e-9), 4),
                        bf16_slower=bool(q16["p25_ms"] > q32["p75_ms"]))
    st = sg.stats
    halo_rows = st["pull_rows"] + st["push_rows"]
    print(json.dumps(dict(world=P, rank=r, cover=a.cover, chunks=a.chunks, features=C, local_rows=sg.n_local, local_entries=sg.nnz_local,
                          split_rows=bool(sg.split_rows), stats=st, kernels=kernels, launches_ms_per_iteration=rec,
                          halo_bytes_per_iteration=dict(f32=halo_rows * C * 4, bf16=halo_rows * C * 2),
                          busiest_link_bytes_per_iteration=dict(f32=st["busiest_link_rows"] * C * 4, bf16=st["busiest_link_rows"] * C * 2))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, nargs="+", default=[8])
    ap.add_argument("--world", type=int, default=0, help="(child) the one world size this process measures")
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--nodes", type=int, default=80_000_000)
    ap.add_argument("--entries", type=int, default=1_000_000_000)
    ap.add_argument("--feats", type=int, default=128)
    ap.add_argument("--chunks", type=int, default=2)
    ap.add_argument("--cover", default="cover")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=420, help="seconds one world size may take")
    a = ap.parse_args()
    if a.world:
        return child(a)
    if a.reps < 20 or a.warm < 3:
        print("note: fewer than 20 repetitions / 3 warm-ups: not a record", file=sys.stderr)
    out = dict(what=f"one rank's block of the R-MAT graph ({a.nodes} vertices, {a.entries} entries) on ONE GPU, C = {a.feats}, {a.chunks} chunks; "
                    f"f32 and bf16 storage interleaved in one process per world size, {a.warm} warm-ups, {a.reps} repetitions, device events; "
                    "no multi-GPU step measured: the halo bytes are the plan's, halved by construction", blocks=[])
    for P in a.worlds:
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--world", str(P), "--rank", str(a.rank),
               "--nodes", str(a.nodes), "--entries", str(a.entries), "--feats", str(a.feats), "--chunks", str(a.chunks), "--cover", a.cover,
               "--reps", str(a.reps), "--warm", str(a.warm)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:                              # nothing more is started on the GPU after a failure
            out["failed"] = dict(world=P, returncode=res.returncode, stderr=res.stderr[-2000:])
            break
        out["blocks"].append(json.loads(res.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
