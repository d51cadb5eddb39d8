#!/usr/bin/env python3
"""GCNII training with f32 and with bf16 row storage (GNN(gcnii_training_dtype=), sparse.gcnii_train_run_bf16 over
gnx_gcnii_step_train_bf16 / gnx_feature_dropout_back_bf16 / gnx_gcnii_step_back_bf16), one GPU: the training step (forward, loss,
backward) of a `--layers` (8) layer GCNII stack, dropout 0.6, per width (16, 32, 64), on

  * the config-4 graph (symmetric R-MAT, 10M vertices / 100M entries),
  * a symmetric R-MAT of 10^6 vertices / 10^7 entries,
  * the Cora-shaped graph of the tests (2 708 vertices).

    python tools/gcnii_bf16_train_bench.py [--graphs config4,1m,cora] [--widths 16,32,64] [--layers 8] [--reps 20] [--warm 5]

Both models are GCNII(feature_dropout="fused", gcnii_backward="fused"); they differ in gcnii_training_dtype alone, and the width and row
gates of the bf16 path (sparse.GCNII_BF16_TRAIN_MIN_WIDTH / _MIN_ROWS: what this measurement is for) are switched off for the run.  The
two are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one f32 and one bf16 step, each between device
events.  Reported: median and quartiles in ms, the ratio of the medians, `bf16_slower` = the bf16 lower quartile is above the f32 upper
quartile, and the kernels the two steps end on.  The yardstick is the f32 step of the same process.  Prints one JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnn-tf_amd"), os.path.join(ROOT, "tests")]


def quartiles(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]
    return dict(median_ms=round(q(0.5), 4), p25_ms=round(q(0.25), 4), p75_ms=round(q(0.75), 4))


def main():
    import numpy as np
    import torch
    import gnntf
    from gnntf import rmat, sparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="config4,1m,cora")
    ap.add_argument("--widths", default="16,32,64")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gcnii_bf16_train_bench: needs a GPU")
    if a.reps < 20 or a.warm < 5:
        print("note: fewer than 20 repetitions / 5 warm-ups: not a record", file=sys.stderr)
    device = torch.device("cuda:0")
    gnntf.set_default_device(device)
    sparse.GCNII_BF16_TRAIN_MIN_WIDTH, sparse.GCNII_BF16_TRAIN_MIN_ROWS = 0, 0          # the gates are what is being measured

    def rmat_graph(n, entries):
        u, v = rmat.rmat_relabelled_pairs(n, entries // 2, seed=1, device=device)
        idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
        return gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], dtype=torch.float32, device=device), (n, n)), device=device)

    def cora_graph():
        import graphs
        coo, vals, shape, _ = graphs.cora_shaped(seed=0)
        return gnntf.DeviceGraph(gnntf.SparseCOO(coo, vals, shape), device=device)

    makers = dict(config4=lambda: rmat_graph(10_000_000, 100_000_000), **{"1m": lambda: rmat_graph(1_000_000, 10_000_000)}, cora=cora_graph)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    record = dict()
    for name in a.graphs.split(","):
        g = makers[name]()
        torch.cuda.empty_cache()
        n = g.n_rows
        rng = np.random.default_rng(0)
        nodes = rng.permutation(n)[:max(n // 10, 1)]
        # checked and uploaded once: a host list would be range-checked and copied inside every timed step, of both variants alike
        labels = sparse.DeviceIndex(rng.integers(0, 7, size=len(nodes)), device, 7, "label")
        nodes = sparse.DeviceIndex(nodes, device, n)
        rows = dict()
        for C in [int(c) for c in a.widths.split(",")]:
            X = torch.empty((n, C), dtype=torch.float32, device=device).uniform_(-1, 1, generator=torch.Generator(device).manual_seed(C))
            models = dict()
            for how, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                gnntf.set_seed(3)
                torch.manual_seed(3)
                model = gnntf.GCNII(g, X, 7, latent_dims=[C], iterations=a.layers, dropout=a.dropout, feature_dropout="fused",
                                    gcnii_backward="fused", gcnii_training_dtype=dtype)
                model.reset()
                for layer in model.layers():                        # the reference initialises W to zero: use seeded weights
                    if isinstance(layer, gnntf.GCNIILayer):
                        layer.W.data.uniform_(-1 / 8, 1 / 8)
                models[how] = model
            kernels = dict()

            def step(how):
                model = models[how]
                for var in model.vars():
                    var.var.grad = None
                with model:
                    gnntf.node_ce(model(model.features), nodes, labels).backward()
                kernels[how] = g.last_kernel()

            for _ in range(a.warm):
                step("f32"), step("bf16")
            t32, t16 = [], []
            for _ in range(a.reps):
                t32.append(timed(lambda: step("f32")))
                t16.append(timed(lambda: step("bf16")))
            q32, q16 = quartiles(t32), quartiles(t16)
            rows[str(C)] = dict(f32=q32, bf16=q16, f32_over_bf16=round(q32["median_ms"] / max(q16["median_ms"], 1e-9), 4),
                                bf16_slower=bool(q16["p25_ms"] > q32["p75_ms"]), bf16_faster=bool(q16["p75_ms"] < q32["p25_ms"]),
                                kernels=dict(kernels))
            del models, X
            torch.cuda.empty_cache()
        record[name] = dict(vertices=n, entries=g.nnz, widths=rows)
        del g, nodes, labels
        torch.cuda.empty_cache()
    print(json.dumps(dict(what=f"GCNII training step (forward, loss, backward), {a.layers} layers, dropout {a.dropout}, feature_dropout and "
                               f"gcnii_backward \"fused\": gcnii_training_dtype f32 against bf16, interleaved in one process, {a.warm} warm-ups, "
                               f"{a.reps} repetitions, device events", graphs=record)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
