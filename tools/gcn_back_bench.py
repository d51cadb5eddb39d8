#!/usr/bin/env python3
"""The backward of the fused GCNLayer as today's kernels (GNN(gcn_backward="composed"), the default: gnx_dense writes G' W^T [n, C_in], the
transposed SpMM reads it back and gathers it at the input width) against the one launch that gathers G' at the OUTPUT width
(gcn_backward="fused": gnx_gcn_step_back / gnx_gcn_step_back_dropped), on the config-4 graph (symmetric R-MAT, 10M vertices / 100M
entries), one GPU:

  * single layers C_in -> C_out (64->64, 64->40, 64->7, 32->32) with bias and relu, over the constant adjacency and under edge dropout 0.5
    (a DroppedAdjacency with edge_dropout="fused"): `backward` is out.backward(g) of sparse.gcn_step(..., backward=how) -- the gate, the
    weight gradient and the column sums, which both variants share, and the input gradient; `input_gradient` is the input gradient alone,
    gnx_dense + the transposed SpMM against sparse.gcn_step_back over the same gated gradient;
  * the training step (forward, loss, backward) and its peak memory of GCN(latent_dims=[64, 64, 64], num_classes=40) and of the reference's
    default GCN(latent_dims=[64], num_classes=7), both with gcn_layer="fused", feature_dropout="fused", graph_dropout = 0.5 and
    dropout = 0.5 over `--features` (128) input columns.  The first layer gathers at that width and needs no input gradient; the layers
    behind it are the ones the keyword reaches.

    python tools/gcn_back_bench.py [--shapes 64x64,64x40,64x7,32x32] [--reps 20] [--warm 5]

The two are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one "composed" and one "fused" call, each between
device events (a single layer's forward runs before the first event).  Reported: median and quartiles in ms, the ratio of the medians,
`fused_slower` = the fused lower quartile is above the composed upper quartile, the peak of torch's allocator over one backward / one
training step (above what was allocated before it), and the largest difference of the two input gradients (float32 rounding: the
products associate differently).  The yardstick is the "composed" call of the same process.  Prints one JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnn-tf_amd")]

HOWS = ("composed", "fused")
E_SEED, E_STREAM = 5, 3


def quartiles(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]
    return dict(median_ms=round(q(0.5), 4), p25_ms=round(q(0.25), 4), p75_ms=round(q(0.75), 4))


def compare(tc, tf):
    qc, qf = quartiles(tc), quartiles(tf)
    return dict(composed=qc, fused=qf, composed_over_fused=round(qc["median_ms"] / max(qf["median_ms"], 1e-9), 4),
                fused_slower=bool(qf["p25_ms"] > qc["p75_ms"]))


def main():
    import numpy as np
    import torch
    import gnntf
    from gnntf import rmat, sparse
    nat = sparse.nat
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--shapes", default="64x64,64x40,64x7,32x32")
    ap.add_argument("--features", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gcn_back_bench: needs a GPU")
    if a.reps < 20 or a.warm < 5:
        print("note: fewer than 20 repetitions / 5 warm-ups: not a record", file=sys.stderr)
    device = torch.device("cuda:0")
    gnntf.set_default_device(device)
    u, v = rmat.rmat_relabelled_pairs(a.n, a.entries // 2, seed=1, device=device)
    idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
    del u, v
    g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], dtype=torch.float32, device=device), (a.n, a.n)), device=device)
    del idx
    torch.cuda.empty_cache()
    if g.nnz_entries > g.nnz:
        g.enable_entry_dropout()
    adjacencies = dict(constant=gnntf.normalize(g, "symmetric"), edge_dropout=sparse.DroppedAdjacency(g, 0.5, E_SEED, E_STREAM))
    adjacencies["constant"].transposed_values()                    # (permuted once and kept, as a constant adjacency does)

    def timed(fn, before=None):
        state = before() if before is not None else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn() if before is None else fn(state)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def interleaved(composed, fused, before_composed=None, before_fused=None):
        for _ in range(a.warm):
            timed(composed, before_composed), timed(fused, before_fused)
        tc, tf = [], []
        for _ in range(a.reps):
            tc.append(timed(composed, before_composed))
            tf.append(timed(fused, before_fused))
        return compare(tc, tf)

    def peak_of(fn, before=None):
        state = before() if before is not None else None
        torch.cuda.synchronize()
        start = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn() if before is None else fn(state)
        torch.cuda.synchronize()
        return round((torch.cuda.max_memory_allocated() - start) / 2 ** 20, 1)

    layers = dict()
    for shape in a.shapes.split(","):
        C_in, C_out = (int(c) for c in shape.split("x"))
        seeded = torch.Generator(device).manual_seed(1000 * C_in + C_out)
        X = torch.empty((a.n, C_in), dtype=torch.float32, device=device).uniform_(-1, 1, generator=seeded).requires_grad_()
        W = torch.empty((C_in, C_out), dtype=torch.float32, device=device).uniform_(-1 / 8, 1 / 8, generator=seeded).requires_grad_()
        b = torch.empty((1, C_out), dtype=torch.float32, device=device).uniform_(-0.2, 0.2, generator=seeded).requires_grad_()
        up = torch.empty((a.n, C_out), dtype=torch.float32, device=device).uniform_(-1, 1, generator=seeded)
        for name, adj in adjacencies.items():
            def forward(how, adj=adj):
                X.grad = W.grad = b.grad = None
                return sparse.gcn_step(adj, X, W, b, relu=True, edge_dropout="fused", backward=how)

            row = dict(backward=interleaved(lambda out: out.backward(up), lambda out: out.backward(up),
                                            lambda: forward("composed"), lambda: forward("fused")))
            row["kernel"] = g.last_kernel()
            row["backward_peak_mib"] = {how: peak_of(lambda out: out.backward(up), lambda how=how: forward(how)) for how in HOWS}
            X.grad = W.grad = b.grad = None
            with torch.no_grad():                                   # the input gradient alone, over one gated gradient in padded rows
                G = sparse._padded_rows(a.n, C_out, device)
                G.copy_(up)
                Wt = W.detach().t().contiguous()
                fused_edge = name == "edge_dropout"
                composed = lambda: sparse._launch(adj, sparse._dense_launch(G, Wt, None, False), None, 1.0, 0.0, nat.ACT_NONE, transposed=True)
                fused = lambda: sparse._gcn_back_launch(adj, G, Wt, fused_edge)
                row["input_gradient"] = interleaved(composed, fused)
                dX_f = fused()
                row["input_gradient_kernel"] = g.last_kernel()
                dX_c = composed()
                row["max_abs_difference"], row["max_abs"] = float((dX_c - dX_f).abs().max()), float(dX_c.abs().max())
                del G, dX_c, dX_f
            layers[f"{C_in}->{C_out} {name}"] = row
            torch.cuda.empty_cache()
        del X, W, b, up
        torch.cuda.empty_cache()

    rng = np.random.default_rng(0)
    nodes = rng.permutation(a.n)[:a.n // 10]
    X = torch.empty((a.n, a.features), dtype=torch.float32, device=device).uniform_(-1, 1, generator=torch.Generator(device).manual_seed(5))
    stacks = dict()
    for latent, classes in (([64, 64, 64], 40), ([64], 7)):
        # checked and uploaded once: a host list would be range-checked and copied inside every timed step, of both variants alike
        labels = sparse.DeviceIndex(rng.integers(0, classes, size=len(nodes)), device, classes, "label")
        where = sparse.DeviceIndex(nodes, device, a.n)
        models = dict()
        for how in HOWS:
            gnntf.set_seed(3)
            torch.manual_seed(3)
            model = gnntf.GCN(g, X, classes, latent_dims=latent, gcn_layer="fused", feature_dropout="fused", gcn_backward=how)
            model.reset()
            seeded = torch.Generator(device).manual_seed(77)
            for layer in model.layers():                            # (the biases start at zero: seeded ones)
                layer.b.data.uniform_(-0.2, 0.2, generator=seeded)
            models[how] = model

        def step(how):
            model = models[how]
            model.training_mode(True)
            for var in model.vars():
                var.var.grad = None
            with model:
                gnntf.node_ce(model(model.features), where, labels).backward()

        stack = dict(train_step=interleaved(lambda: step("composed"), lambda: step("fused")))
        stack["last_kernel"] = g.last_kernel()
        peak = dict()
        for how in HOWS:                                            # the allocator's peak over one step, above what stood before it
            for var in models[how].vars():
                var.var.grad = None
            torch.cuda.empty_cache()
            peak[how] = peak_of(lambda how=how: step(how))
        stack["train_step_peak_mib"] = peak
        stacks[f"GCN(latent_dims={latent}, num_classes={classes})"] = stack
        del models
        torch.cuda.empty_cache()
    print(json.dumps(dict(what=f"GCNLayer backward, symmetric R-MAT ({a.n} vertices, {g.nnz} entries): gcn_backward \"composed\" against \"fused\", "
                               f"interleaved in one process, {a.warm} warm-ups, {a.reps} repetitions, device events; the stacks run "
                               f"gcn_layer=\"fused\", feature_dropout=\"fused\" over {a.features} input columns, graph_dropout 0.5, dropout 0.5",
                          single_layers=layers, stacks=stacks)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
