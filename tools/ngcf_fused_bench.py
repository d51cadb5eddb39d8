#!/usr/bin/env python3
"""NGCFLayer as today's ops (GNN(ngcf_layer="composed"), the default: one SpMM, a multiply, two transforms, two leaky_relu passes, an add,
the dropout and torch's normalize) against the one launch (ngcf_layer="fused": gnx_ngcf_step, its backward one gate pass and today's
kernels), on the config-4 graph (symmetric R-MAT, 10M vertices / 100M entries) BIPARTITE-normalised as the layer takes it, one GPU:

  * single layers C -> C (64, 32, 16) with both biases and leaky_relu: the eval-mode forward, and a training step (forward, a weighted
    sum as the loss, backward to X, W1, b1, W2, b2) with its peak memory;
  * the training step and its peak memory of a 3-layer NGCF(num_classes=64) over 64 input columns with LinkPrediction's pairwise loss over
    `--pairs` positive pairs and one negative each (a fixed list, kept on the device), dropout 0.1: torch's dropout in both variants, so the
    fused layers run with normalize=False and torch's dropout and normalize follow; `--feature-dropout fused` puts the mask into the launch.

    python tools/ngcf_fused_bench.py [--widths 64,32,16] [--reps 20] [--warm 5]

The two are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one "composed" and one "fused" call, each between
device events.  Reported: median and quartiles in ms, the ratio of the medians, `fused_slower` = the fused lower quartile is above the
composed upper quartile, the peak of torch's allocator over one training step (above what was allocated before the step), and the largest
difference of the two results (the same weights; float32 rounding).  The yardstick is the "composed" call of the same process.  Prints one
JSON record."""
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
    from gnntf.blocks import affine
    from gnntf.graph_model import leaky_relu
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--widths", default="64,32,16")
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--feature-dropout", default="torch", choices=("torch", "fused"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ngcf_fused_bench: needs a GPU")
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

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def interleaved(composed, fused):
        for _ in range(a.warm):
            composed(), fused()
        tc, tf = [], []
        for _ in range(a.reps):
            tc.append(timed(composed))
            tf.append(timed(fused))
        return compare(tc, tf)

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)

    def composed_layer(X, W1, b1, W2, b2):
        agg = sparse.spmm(adj, X)
        return torch.nn.functional.normalize(leaky_relu(affine(X * agg, W1, b1)) + leaky_relu(affine(agg, W2, b2)), dim=1, eps=1e-12)

    layers = dict()
    for width in (int(c) for c in a.widths.split(",")):
        seeded = torch.Generator(device).manual_seed(1000 + width)
        draw = lambda shape, lo, hi: torch.empty(shape, dtype=torch.float32, device=device).uniform_(lo, hi, generator=seeded)
        X, G = draw((a.n, width), -1, 1), draw((a.n, width), -1, 1)
        W1, W2 = draw((width, width), -1 / 8, 1 / 8), draw((width, width), -1 / 8, 1 / 8)
        b1, b2 = draw((1, width), -0.2, 0.2), draw((1, width), -0.2, 0.2)
        leaves = (X, W1, b1, W2, b2)
        fused_layer = lambda *t: sparse.ngcf_step(adj, *t)

        def step(layer):
            for t in leaves:
                t.grad = None
                t.requires_grad_(True)
            (layer(*leaves) * G).sum().backward()
            for t in leaves:
                t.requires_grad_(False)

        row = dict()
        with torch.no_grad():
            row["eval_forward"] = interleaved(lambda: composed_layer(*leaves), lambda: fused_layer(*leaves))
            out_f = fused_layer(*leaves)
            row["kernel"] = g.last_kernel()
            out_c = composed_layer(*leaves)
            row["max_abs_difference"], row["max_abs"] = float((out_c - out_f).abs().max()), float(out_c.abs().max())
            del out_c, out_f
        row["train_step"] = interleaved(lambda: step(composed_layer), lambda: step(fused_layer))
        row["train_step_peak_mib"] = dict(composed=peak_of(lambda: step(composed_layer)), fused=peak_of(lambda: step(fused_layer)))
        layers[f"{width}->{width}"] = row
        for t in leaves:
            t.grad = None
        del X, G, W1, W2, b1, b2, leaves
        torch.cuda.empty_cache()

    class DeviceEdges(sparse.DeviceIndex):                          # LinkPrediction asks its edge list for its length
        def __len__(self):
            return self.tensor.shape[0]

    # a positive pair, then one negative of the same first endpoint (the layout of gnntf.negative_sampling), checked and uploaded once
    rng = torch.Generator(device).manual_seed(9)
    negatives = torch.stack([positives[:, 0], torch.randint(0, a.n, (positives.shape[0],), device=device, generator=rng)], 1)
    edges = torch.stack([positives, negatives], 1).reshape(-1, 2)
    X = torch.empty((a.n, 64), dtype=torch.float32, device=device).uniform_(-1, 1, generator=torch.Generator(device).manual_seed(5))
    models, tasks = dict(), dict()
    for how in HOWS:
        gnntf.set_seed(3)
        torch.manual_seed(3)
        models[how] = gnntf.NGCF(g, X, num_classes=64, ngcf_layer=how, feature_dropout=a.feature_dropout)
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

    def forward(how):
        model = models[how]
        model.training_mode(False)
        with torch.no_grad():
            return model(model.features)

    stack = dict(train_step=interleaved(lambda: step("composed"), lambda: step("fused")))
    stack["train_step_peak_mib"] = {how: peak_of(lambda: step(how)) for how in HOWS}
    stack["eval_forward"] = interleaved(lambda: forward("composed"), lambda: forward("fused"))
    stack["eval_kernel"] = g.last_kernel()
    out_c, out_f = forward("composed"), forward("fused")
    stack["eval_max_abs_difference"], stack["eval_max_abs"] = float((out_c - out_f).abs().max()), float(out_c.abs().max())
    print(json.dumps(dict(what=f"NGCFLayer, R-MAT ({a.n} vertices, {g.nnz} entries), bipartite-normalised: ngcf_layer \"composed\" against "
                               f"\"fused\", interleaved in one process, {a.warm} warm-ups, {a.reps} repetitions, device events; the stack is "
                               f"NGCF(num_classes=64) over 64 input columns, dropout 0.1 (feature_dropout={a.feature_dropout!r}), "
                               f"LinkPrediction over {positives.shape[0]} positive pairs and one negative each",
                          single_layers=layers, stack=stack)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
