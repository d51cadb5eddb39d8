#!/usr/bin/env python3
"""The link task around the NGCF layers, on the config-4 graph (symmetric R-MAT, 10M vertices / 100M entries) BIPARTITE-normalised, C = 64,
one GPU, for `--pairs` positive pairs (default 10^6 and 10^7) and one negative each:

  1. the link head's backward: gnx_edge_scores_backward (float atomics) against gnx_edge_plan + gnx_edge_scores_backward_sorted, the plan
     alone, and the sorted backward of a fixed list whose plan is kept -- each into a d_grad_F that the timed call zero-fills;
  2. gnx_sample_negatives, the launch alone.  The host sampler (gnntf.negative_sampling, a Python loop over networkx) runs for seconds at
     10^5 pairs already: it is timed ONCE, at `--host-pairs` pairs on an R-MAT small enough to build in networkx (`--host-n` vertices) --
     another size and another graph than the device rows, stated as such;
  3. the training step of the 3-layer NGCF(num_classes=64, ngcf_layer="fused", feature_dropout="fused") with LinkPrediction's pairwise loss:
     a fixed device list with atomics (what tools/ngcf_fused_bench.py times as "fused"), the same list with the sorted backward (plan kept),
     and device_negative_sampling with the sorted backward (a draw and a plan per step).

    python tools/link_head_bench.py [--pairs 1000000,10000000] [--reps 20] [--warm 5]

The variants of a cell are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one call of each, each between
device events.  Reported: median and quartiles in ms per variant and, against the first variant of the cell, the ratio of the medians and
`slower` = the variant's lower quartile is above the first one's upper quartile.  Prints one JSON record."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnn-tf_amd")]


def quartiles(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]
    return dict(median_ms=round(q(0.5), 4), p25_ms=round(q(0.25), 4), p75_ms=round(q(0.75), 4))


def main():
    import numpy as np
    import torch
    import gnntf
    from gnntf import rmat, sparse
    nat = sparse.nat
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--pairs", default="1000000,10000000")
    ap.add_argument("--host-pairs", type=int, default=100_000)
    ap.add_argument("--host-n", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("link_head_bench: needs a GPU")
    if a.reps < 20 or a.warm < 5:
        print("note: fewer than 20 repetitions / 5 warm-ups: not a record", file=sys.stderr)
    device = torch.device("cuda:0")
    gnntf.set_default_device(device)
    C = 64

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def interleaved(variants):
        """{name: call} -> {name: quartiles (+ the comparison with the first variant)}"""
        for _ in range(a.warm):
            for fn in variants.values():
                fn()
        times = {name: [] for name in variants}
        for _ in range(a.reps):
            for name, fn in variants.items():
                times[name].append(timed(fn))
        out = {name: quartiles(ms) for name, ms in times.items()}
        base = out[next(iter(variants))]
        for name, q in list(out.items())[1:]:
            q["over_first"] = round(q["median_ms"] / max(base["median_ms"], 1e-9), 4)
            q["slower"] = bool(q["p25_ms"] > base["p75_ms"])
        return out

    u, v = rmat.rmat_relabelled_pairs(a.n, a.entries // 2, seed=1, device=device)
    idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
    most = max(int(p) for p in a.pairs.split(","))
    all_positives = torch.stack([u[:most], v[:most]], 1).contiguous()
    del u, v
    g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], dtype=torch.float32, device=device), (a.n, a.n)), device=device)
    del idx
    torch.cuda.empty_cache()
    X = torch.empty((a.n, C), dtype=torch.float32, device=device).uniform_(-1, 1, generator=torch.Generator(device).manual_seed(5))

    record = dict()
    for pairs in (int(p) for p in a.pairs.split(",")):
        positives = all_positives[:pairs].contiguous()
        row = dict()
        # ---- 2. the sampler launch alone (its buffer is the fixed list of the other cells)
        edges = torch.empty((2 * pairs, 2), dtype=torch.int64, device=device)
        fallbacks = torch.zeros(1, dtype=torch.int64, device=device)
        streams = iter(range(1 << 30))
        row["sampler"] = interleaved(dict(gnx_sample_negatives=lambda: sparse.sample_negatives(g, positives, 1, None, 3, next(streams), out=edges,
                                                                                              fallbacks=fallbacks)))
        row["sampler_fallbacks_per_call"] = float(fallbacks.item()) / (a.warm + a.reps)
        # ---- 1. the backward of the head
        m = edges.shape[0]
        grad_out = torch.empty(m, dtype=torch.float32, device=device).uniform_(-1, 1, generator=torch.Generator(device).manual_seed(7))
        gF = torch.empty((a.n, C), dtype=torch.float32, device=device)
        work = torch.empty(int(nat.lib().gnx_edge_sorted_work_floats(m, C)), dtype=torch.float32, device=device)
        kept = sparse.EdgePlan(edges, a.n)

        def atomic():
            gF.zero_()
            nat.check(nat.lib().gnx_edge_scores_backward(nat.ptr(X), C, a.n, C, nat.ptr(edges), m, None, nat.ptr(grad_out), nat.ptr(gF), C,
                                                         nat.current_stream()))

        def sorted_with(plan):
            gF.zero_()
            nat.check(nat.lib().gnx_edge_scores_backward_sorted(nat.ptr(X), C, a.n, C, nat.ptr(edges), m, None, nat.ptr(grad_out), nat.ptr(gF), C,
                                                                nat.ptr(plan.keys), nat.ptr(plan.pos), nat.ptr(plan.chunks), nat.ptr(work),
                                                                work.numel(), nat.current_stream()))

        row["backward"] = interleaved(dict(atomic=atomic, plan_and_sorted=lambda: sorted_with(sparse.EdgePlan(edges, a.n)),
                                           plan_alone=lambda: sparse.EdgePlan(edges, a.n), sorted_plan_kept=lambda: sorted_with(kept)))
        atomic()
        reference = gF.clone()
        sorted_with(kept)
        row["backward_max_abs_difference"], row["backward_max_abs"] = float((gF - reference).abs().max()), float(reference.abs().max())
        row["chunks"], row["named_nodes"] = int(kept.chunks[0]), int(torch.unique(edges).numel())
        del reference, gF, work, kept, grad_out
        torch.cuda.empty_cache()
        # ---- 3. the training step
        models, tasks = dict(), dict()
        for how in ("fixed_atomic", "fixed_sorted", "sampler_sorted"):
            gnntf.set_seed(3)
            torch.manual_seed(3)
            model = gnntf.NGCF(g, X, num_classes=C, ngcf_layer="fused", feature_dropout="fused")
            model.reset()
            if how == "sampler_sorted":
                tasks[how] = gnntf.LinkPrediction(gnntf.device_negative_sampling(positives, model))
            else:
                tasks[how] = gnntf.LinkPrediction(sparse.DeviceIndex(edges, device), np.tile([1, 0], pairs),
                                                  edge_backward="sorted" if how == "fixed_sorted" else "atomic")
            models[how] = model

        def step(how):
            model = models[how]
            model.training_mode(True)
            for var in model.vars():
                var.var.grad = None
            with model:
                tasks[how].loss(model(model.features)).backward()

        row["train_step"] = interleaved({how: (lambda how=how: step(how)) for how in models})
        record[str(pairs)] = row
        del models, tasks, edges
        torch.cuda.empty_cache()

    # the host sampler, once, on a graph that networkx can hold
    host = None
    if a.host_pairs > 0:
        import networkx as nx
        hu, hv = rmat.rmat_relabelled_pairs(a.host_n, 5 * a.host_n, seed=1, device=device)
        pairs_host = torch.stack([hu, hv], 1).cpu().numpy()
        G = nx.Graph()
        G.add_nodes_from(range(a.host_n))
        G.add_edges_from(map(tuple, pairs_host.tolist()))
        listed = [list(e) for e in pairs_host[:a.host_pairs].tolist()]
        t0 = time.perf_counter()
        sampler = gnntf.negative_sampling(listed, G)
        t1 = time.perf_counter()
        sampler()
        t2 = time.perf_counter()
        host = dict(vertices=a.host_n, edges=G.number_of_edges(), pairs=len(listed), construct_s=round(t1 - t0, 3), call_s=round(t2 - t1, 3))
    print(json.dumps(dict(what=f"link task, R-MAT ({a.n} vertices, {g.nnz} entries), C = {C}, samples = 1: variants of a cell interleaved in one "
                               f"process, {a.warm} warm-ups, {a.reps} repetitions, device events; train_step is NGCF(num_classes=64, "
                               f"ngcf_layer='fused', feature_dropout='fused') + LinkPrediction's pairwise loss",
                          pairs=record, host_sampler_once=host)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
