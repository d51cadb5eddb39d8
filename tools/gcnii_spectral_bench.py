#!/usr/bin/env python3
"""GCNIISpectralPreservingLayer as today's ops (GNN(gcnii_spectral="composed"), the default: SpMM+mix, the dense kernel with bias and
relu, three torch elementwise passes) against the one launch (gcnii_spectral="fused": gnx_gcnii_step_spectral forward,
gnx_gcnii_spectral_back first in the backward), on the config-4 graph (symmetric R-MAT, 10M vertices / 100M entries), one GPU: the
training step (forward, loss, backward) and the eval-mode forward of a `--layers` (8) layer spectral GCNII stack per width (64 and 32),
dropout 0.6, and the peak memory of one training step of each.

    python tools/gcnii_spectral_bench.py [--widths 64,32] [--layers 8] [--reps 20] [--warm 5]

The two are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one "composed" and one "fused" call, each between
device events.  Reported: median and quartiles in ms, the ratio of the medians, `fused_slower` = the fused lower quartile is above the
composed upper quartile, the peak of torch's allocator over one training step (above what was allocated before the step), and the largest
difference of the eval-mode logits of the two (the same weights; float32 rounding).  The yardstick is the "composed" call of the same
process.  The masks of the two differ (torch's generator against the counter RNG), the work per element does not.  Prints one JSON
record."""
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
    ap.add_argument("--widths", default="64,32")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gcnii_spectral_bench: needs a GPU")
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
        for how in HOWS:
            gnntf.set_seed(3)
            torch.manual_seed(3)
            model = gnntf.GCNII(g, X, 7, latent_dims=[C], iterations=a.layers, dropout=a.dropout,
                                layer_type=gnntf.GCNIISpectralPreservingLayer, gcnii_spectral=how)
            model.reset()
            seeded = torch.Generator(device).manual_seed(100 + C)
            for layer in model.layers():                            # the reference initialises W and the bias to zero: use seeded ones
                if isinstance(layer, gnntf.GCNIISpectralPreservingLayer):
                    layer.W.data.uniform_(-1 / 8, 1 / 8, generator=seeded)
                    layer.bias.data.uniform_(-0.2, 0.2, generator=seeded)
            models[how] = model

        def step(how):
            model = models[how]
            model.training_mode(True)
            for var in model.vars():
                var.var.grad = None
            with model:
                gnntf.node_ce(model(model.features), nodes, labels).backward()

        def forward(how):
            model = models[how]
            model.training_mode(False)
            with torch.no_grad():
                return model(model.features)

        for _ in range(a.warm):
            step("composed"), step("fused")
        tc, tf = [], []
        for _ in range(a.reps):
            tc.append(timed(lambda: step("composed")))
            tf.append(timed(lambda: step("fused")))
        row = dict(train_step=compare(tc, tf))
        with models["fused"], torch.no_grad():
            models["fused"](models["fused"].features)
        row["train_kernel"] = g.last_kernel()
        peak = dict()
        for how in HOWS:                                           # the allocator's peak over one step, above what stood before it
            for var in models[how].vars():
                var.var.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(how)
            torch.cuda.synchronize()
            peak[how] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)
        row["train_step_peak_mib"] = peak
        for _ in range(a.warm):
            forward("composed"), forward("fused")
        tc, tf = [], []
        for _ in range(a.reps):
            tc.append(timed(lambda: forward("composed")))
            tf.append(timed(lambda: forward("fused")))
        row["eval_forward"] = compare(tc, tf)
        row["eval_kernel"] = g.last_kernel()
        out_c, out_f = forward("composed"), forward("fused")
        row["eval_logits_max_abs_difference"] = float((out_c - out_f).abs().max())
        row["eval_logits_max_abs"] = float(out_c.abs().max())
        rows[str(C)] = row
        del models, X, out_c, out_f
        torch.cuda.empty_cache()
    print(json.dumps(dict(what=f"GCNIISpectralPreservingLayer stack, {a.layers} layers, dropout {a.dropout}, symmetric R-MAT ({a.n} vertices, "
                               f"{g.nnz} entries): gcnii_spectral \"composed\" against \"fused\", interleaved in one process, {a.warm} "
                               f"warm-ups, {a.reps} repetitions, device events",
                          widths=rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
