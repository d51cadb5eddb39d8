#!/usr/bin/env python3
"""The feature dropout of the GCNII training layer, torch's op behind the launch (GNN(feature_dropout="torch"), the default) against
the mask made inside the launch (feature_dropout="fused": gnx_gcnii_step_drop forward, gnx_feature_dropout_back backward), on the
config-4 graph (symmetric R-MAT, 10M vertices / 100M entries), one GPU: the training step (forward, loss, backward) of a `--layers` (8)
layer GCNII stack per width (64 and 32), dropout 0.6.

    python tools/gcnii_drop_bench.py [--widths 64,32] [--layers 8] [--reps 20] [--warm 5]

The two are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one "torch" and one "fused" step, each between
device events.  Reported: median and quartiles in ms, the ratio of the medians, and `fused_slower` = the fused lower quartile is above
the torch upper quartile.  The yardstick is the "torch" step of the same process.  The masks of the two differ (torch's generator
against the counter RNG), the work per element does not.  Prints one JSON record."""
import argparse
import json
import os
import sys

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
    from gnntf import graph_model, rmat, sparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--widths", default="64,32")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gcnii_drop_bench: needs a GPU")
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

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    rng = np.random.default_rng(0)
    nodes = rng.permutation(a.n)[:a.n // 10]
    # checked and uploaded once: a host list would be range-checked and copied inside every timed step, of both variants alike
    labels = sparse.DeviceIndex(rng.integers(0, 7, size=len(nodes)), device, 7, "label")
    nodes = sparse.DeviceIndex(nodes, device, a.n)
    rows = dict()
    for C in [int(c) for c in a.widths.split(",")]:
        X = torch.empty((a.n, C), dtype=torch.float32, device=device).uniform_(-1, 1, generator=torch.Generator(device).manual_seed(C))
        models = dict()
        for how in graph_model.FEATURE_DROPOUTS:
            gnntf.set_seed(3)
            torch.manual_seed(3)
            model = gnntf.GCNII(g, X, 7, latent_dims=[C], iterations=a.layers, dropout=a.dropout, feature_dropout=how)
            model.reset()
            for layer in model.layers():                            # the reference initialises W to zero: use seeded weights
                if isinstance(layer, gnntf.GCNIILayer):
                    layer.W.data.uniform_(-1 / 8, 1 / 8)
            models[how] = model

        def step(how):
            model = models[how]
            for var in model.vars():
                var.var.grad = None
            with model:
                gnntf.node_ce(model(model.features), nodes, labels).backward()

        for _ in range(a.warm):
            step("torch"), step("fused")
        tt, tf = [], []
        for _ in range(a.reps):
            tt.append(timed(lambda: step("torch")))
            tf.append(timed(lambda: step("fused")))
        qt, qf = quartiles(tt), quartiles(tf)
        with models["fused"], torch.no_grad():
            models["fused"](models["fused"].features)
        rows[str(C)] = dict(torch=qt, fused=qf, torch_over_fused=round(qt["median_ms"] / max(qf["median_ms"], 1e-9), 4),
                            fused_slower=bool(qf["p25_ms"] > qt["p75_ms"]), kernel=g.last_kernel())
        del models, X
        torch.cuda.empty_cache()
    print(json.dumps(dict(what=f"GCNII training step (forward, loss, backward), {a.layers} layers, dropout {a.dropout}, symmetric R-MAT "
                               f"({a.n} vertices, {g.nnz} entries): feature_dropout \"torch\" against \"fused\", interleaved in one "
                               f"process, {a.warm} warm-ups, {a.reps} repetitions, device events",
                          widths=rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
