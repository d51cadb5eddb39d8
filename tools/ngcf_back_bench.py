#!/usr/bin/env python3
"""The backward of the fused NGCFLayer as today's kernels (GNN(ngcf_backward="composed"), the default: the gate pass, two copies and column
sums, a torch multiply, gnx_dense_wgrad twice, gnx_dense twice, an addcmul, the transposed SpMM, a second addcmul) against the one launch
around the transposed SpMM (ngcf_backward="fused": gnx_step_back_ngcf, then gnx_dense_wgrad twice), on the config-4 graph (symmetric
R-MAT, 10M vertices / 100M entries) BIPARTITE-normalised as the layer takes it, one GPU:

  * single layers C_in -> C_out (64x64, 32x32, 16x16, 64x16) with both biases and leaky_relu through sparse.ngcf_step(backward=how):
    `backward` is out.backward(g) alone (the forward runs before the first event), `train_step` the forward and the backward, with
    the peak memory of each;
  * the training step and its peak memory of a 3-layer NGCF(num_classes=64, ngcf_layer="fused") over 64 input columns with
    LinkPrediction's pairwise loss over `--pairs` positive pairs and one negative each (a fixed list, kept on the device), dropout 0.1,
    under both dropout forms: the mask in the launch (feature_dropout="fused") and torch's dropout and normalize behind a launch that
    stops before the norm (feature_dropout="torch").

    python tools/ngcf_back_bench.py [--shapes 64x64,32x32,16x16,64x16] [--reps 20] [--warm 5]

The two are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one "composed" and one "fused" call, each between
device events.  Reported: median and quartiles in ms, the ratio of the medians, `fused_slower` = the fused lower quartile is above the
composed upper quartile, the peak of torch's allocator over one backward / one training step (above what was allocated before it), and
the largest difference of the two input gradients (float32 rounding: one fused multiply-add where torch rounds twice).  The yardstick is
the "composed" call of the same process.  Prints one JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnn-tf_amd")]

HOWS = ("composed", "fused")


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--shapes", default="64x64,32x32,16x16,64x16")
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ngcf_back_bench: needs a GPU")
    if a.reps < 20 or a.warm < 5:
        print("note: fewer than 20 repetitions / 5 warm-ups: not a record", file=sys.stderr)
    device = torch.device("cuda:0")
    gnntf.set_default_device(device)
    u, v = rmat.rmat_relabelled_pairs(a.n, a.entries // 2, seed=1, device=device)
    idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
    positives = torch.stack([u[:a.pairs], v[:a.pairs]], 1)
    del u, v
    g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], dtype=torch.float32, device=device), (a.n, a.n)), device=device)
    del idx
    torch.cuda.empty_cache()
    adj = gnntf.normalize(g, "bipartite")
    adj.transposed_values()                                         # (permuted once and kept, as a constant adjacency does)

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
        draw = lambda shape, lo, hi: torch.empty(shape, dtype=torch.float32, device=device).uniform_(lo, hi, generator=seeded)
        X, up = draw((a.n, C_in), -1, 1), draw((a.n, C_out), -1, 1)
        W1, W2 = draw((C_in, C_out), -1 / 8, 1 / 8), draw((C_in, C_out), -1 / 8, 1 / 8)
        b1, b2 = draw((1, C_out), -0.2, 0.2), draw((1, C_out), -0.2, 0.2)
        leaves = (X, W1, b1, W2, b2)
        for t in leaves:
            t.requires_grad_(True)

        def forward(how):
            for t in leaves:
                t.grad = None
            return sparse.ngcf_step(adj, *leaves, backward=how)

        row = dict(backward=interleaved(lambda out: out.backward(up), lambda out: out.backward(up),
                                        lambda: forward("composed"), lambda: forward("fused")))
        row["backward_peak_mib"] = {how: peak_of(lambda out: out.backward(up), lambda how=how: forward(how)) for how in HOWS}
        row["train_step"] = interleaved(lambda: forward("composed").backward(up), lambda: forward("fused").backward(up))
        row["train_step_peak_mib"] = {how: peak_of(lambda how=how: forward(how).backward(up)) for how in HOWS}
        grads = dict()
        for how in HOWS:
            forward(how).backward(up)
            if how == "fused":
                row["last_kernel"] = g.last_kernel()
            grads[how] = X.grad
        row["max_abs_difference"], row["max_abs"] = float((grads["composed"] - grads["fused"]).abs().max()), float(grads["composed"].abs().max())
        layers[f"{C_in}->{C_out}"] = row
        for t in leaves:
            t.grad = None
        del X, up, W1, W2, b1, b2, leaves, grads
        torch.cuda.empty_cache()

    class DeviceEdges(sparse.DeviceIndex):                          # LinkPrediction asks its edge list for its length
        def __len__(self):
            return self.tensor.shape[0]

    # a positive pair, then one negative of the same first endpoint (the layout of gnntf.negative_sampling), checked and uploaded once
    rng = torch.Generator(device).manual_seed(9)
    negatives = torch.stack([positives[:, 0], torch.randint(0, a.n, (positives.shape[0],), device=device, generator=rng)], 1)
    edges = torch.stack([positives, negatives], 1).reshape(-1, 2)
    X = torch.empty((a.n, 64), dtype=torch.float32, device=device).uniform_(-1, 1, generator=torch.Generator(device).manual_seed(5))
    stacks = dict()
    for feature_dropout in ("fused", "torch"):
        models, tasks = dict(), dict()
        for how in HOWS:
            gnntf.set_seed(3)
            torch.manual_seed(3)
            models[how] = gnntf.NGCF(g, X, num_classes=64, ngcf_layer="fused", ngcf_backward=how, feature_dropout=feature_dropout)
            models[how].reset()
            tasks[how] = gnntf.LinkPrediction(np.zeros((2, 2), dtype=np.int64), np.array([1, 0]))
            tasks[how].edges = DeviceEdges(edges, device, None)

        def step(how):
            model = models[how]
            model.training_mode(True)
            for var in model.vars():
                var.var.grad = None
            with model:
                tasks[how].loss(model(model.features)).backward()

        stack = dict(train_step=interleaved(lambda: step("composed"), lambda: step("fused")))
        peak = dict()
        for how in HOWS:                                            # the allocator's peak over one step, above what stood before it
            for var in models[how].vars():
                var.var.grad = None
            torch.cuda.empty_cache()
            peak[how] = peak_of(lambda how=how: step(how))
        stack["train_step_peak_mib"] = peak
        stacks[f"NGCF(num_classes=64), feature_dropout={feature_dropout!r}"] = stack
        del models, tasks
        torch.cuda.empty_cache()
    print(json.dumps(dict(what=f"NGCFLayer backward, R-MAT ({a.n} vertices, {g.nnz} entries), bipartite-normalised: ngcf_backward \"composed\" "
                               f"against \"fused\", interleaved in one process, {a.warm} warm-ups, {a.reps} repetitions, device events; the "
                               f"stacks run ngcf_layer=\"fused\" over 64 input columns, dropout 0.1, LinkPrediction over {positives.shape[0]} "
                               f"positive pairs and one negative each",
                          single_layers=layers, stacks=stacks)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
