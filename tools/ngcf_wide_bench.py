#!/usr/bin/env python3
"""NGCFLayer at input width 128 -- the width of the reference's library_recommendation demo -- three ways, on the config-4 graph (symmetric
R-MAT, 10M vertices / 100M entries) BIPARTITE-normalised as the layer takes it, one GPU:

  (a) "torch"     the composition a model runs at this width by default: one SpMM, a multiply, two transforms, two leaky_relu passes, an
                  add, the dropout and torch's normalize as passes of their own;
  (b) "entry"     sparse.ngcf_step as it is without the keyword: gnx_ngcf_step's in-entry composition (the SpMM, a product pass, the
                  dense kernel twice, a row pass);
  (c) "wide"      sparse.ngcf_step(wide="fused"): gnx_step_wide_ngcf, the SpMM and one row-local launch.

  * single layers 128 -> 128 and 128 -> 64 with both biases and leaky_relu: the eval-mode forward, a training step (forward, a weighted
    sum as the loss, backward to X, W1, b1, W2, b2) with its peak memory, and the SpMM alone beside them;
  * the training step, its peak memory and the eval forward of the 3-layer NGCF(num_classes=128) over Structural(dims=128) and features
    without columns, with LinkPrediction's pairwise loss over `--pairs` positive pairs and one negative each (a fixed list on the device),
    dropout 0.1, under torch's dropout and under feature_dropout="fused": (a) against (c) -- GNN has no keyword for (b).

    python tools/ngcf_wide_bench.py [--outputs 128,64] [--reps 20] [--warm 5]

The forms are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one call of each, each between device events.
Reported: median and quartiles in ms, the ratios of the medians to (c), the peak of torch's allocator over one training step (above what
was allocated before the step), and the largest difference of the results (the same weights; float32 rounding).  The yardsticks are (a) and
(b) of the same process.  Prints one JSON record."""
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


def compare(times):
    """times: {form: [ms]}, the new form under "wide"."""
    out = {form: quartiles(ms) for form, ms in times.items()}
    for form in times:
        if form != "wide":
            out[form + "_over_wide"] = round(out[form]["median_ms"] / max(out["wide"]["median_ms"], 1e-9), 4)
            out["wide_slower_than_" + form] = bool(out["wide"]["p25_ms"] > out[form]["p75_ms"])
    return out


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
    ap.add_argument("--outputs", default="128,64")
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--no-stack", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ngcf_wide_bench: needs a GPU")
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

    def interleaved(forms):
        for _ in range(a.warm):
            for fn in forms.values():
                fn()
        times = {form: [] for form in forms}
        for _ in range(a.reps):
            for form, fn in forms.items():
                times[form].append(timed(fn))
        return compare(times)

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)

    def torch_layer(X, W1, b1, W2, b2):
        agg = sparse.spmm(adj, X)
        return torch.nn.functional.normalize(leaky_relu(affine(X * agg, W1, b1)) + leaky_relu(affine(agg, W2, b2)), dim=1, eps=1e-12)

    layers_of = dict(torch=torch_layer, entry=lambda *t: sparse.ngcf_step(adj, *t), wide=lambda *t: sparse.ngcf_step(adj, *t, wide="fused"))
    layers = dict()
    for C_out in (int(c) for c in a.outputs.split(",")):
        seeded = torch.Generator(device).manual_seed(1000 + C_out)
        draw = lambda shape, lo, hi: torch.empty(shape, dtype=torch.float32, device=device).uniform_(lo, hi, generator=seeded)
        X, G = draw((a.n, 128), -1, 1), draw((a.n, C_out), -1, 1)
        W1, W2 = draw((128, C_out), -1 / 11, 1 / 11), draw((128, C_out), -1 / 11, 1 / 11)
        b1, b2 = draw((1, C_out), -0.2, 0.2), draw((1, C_out), -0.2, 0.2)
        leaves = (X, W1, b1, W2, b2)

        def step(layer):
            for t in leaves:
                t.grad = None
                t.requires_grad_(True)
            (layer(*leaves) * G).sum().backward()
            for t in leaves:
                t.requires_grad_(False)

        row = dict()
        with torch.no_grad():
            row["spmm_alone"] = quartiles([timed(lambda: sparse.spmm(adj, X)) for _ in range(a.warm + a.reps)][a.warm:])
            row["eval_forward"] = interleaved({form: (lambda f=f: f(*leaves)) for form, f in layers_of.items()})
            outs = dict()
            for form, f in layers_of.items():
                outs[form] = f(*leaves)
                row["kernel_" + form] = g.last_kernel()
            row["max_abs_difference"] = {form: float((outs[form] - outs["torch"]).abs().max()) for form in ("entry", "wide")}
            row["max_abs"] = float(outs["torch"].abs().max())
            del outs
        row["train_step"] = interleaved({form: (lambda f=f: step(f)) for form, f in layers_of.items()})
        row["train_step_peak_mib"] = {form: peak_of(lambda f=f: step(f)) for form, f in layers_of.items()}
        layers[f"128->{C_out}"] = row
        for t in leaves:
            t.grad = None
        del X, G, W1, W2, b1, b2, leaves
        torch.cuda.empty_cache()

    stacks = dict()
    if not a.no_stack:
        class DeviceEdges(sparse.DeviceIndex):                      # LinkPrediction asks its edge list for its length
            def __len__(self):
                return self.tensor.shape[0]

        rng = torch.Generator(device).manual_seed(9)
        negatives = torch.stack([positives[:, 0], torch.randint(0, a.n, (positives.shape[0],), device=device, generator=rng)], 1)
        edges = torch.stack([positives, negatives], 1).reshape(-1, 2)
        options = dict(torch=dict(), wide=dict(ngcf_layer="fused", ngcf_wide="fused"))
        for dropout in ("torch", "fused"):
            models, tasks = dict(), dict()
            for form, option in options.items():
                gnntf.set_seed(3)
                torch.manual_seed(3)
                models[form] = gnntf.NGCF(g, np.zeros((a.n, 0), dtype=np.float32), num_classes=128,
                                          preprocessor=gnntf.Structural(dims=128, regularize=0, bipartite=a.n // 2), feature_dropout=dropout, **option)
                models[form].reset()
                tasks[form] = gnntf.LinkPrediction(np.zeros((2, 2), dtype=np.int64), np.array([1, 0]))
                tasks[form].edges = DeviceEdges(edges, device, None)

            def step(form):
                model = models[form]
                model.training_mode(True)
                for var in model.vars():
                    var.var.grad = None
                with model:
                    tasks[form].loss(model(model.features)).backward()

            def forward(form):
                model = models[form]
                model.training_mode(False)
                with torch.no_grad():
                    return model(model.features)

            stack = dict(train_step=interleaved({form: (lambda form=form: step(form)) for form in options}))
            stack["train_step_peak_mib"] = {form: peak_of(lambda form=form: step(form)) for form in options}
            stack["eval_forward"] = interleaved({form: (lambda form=form: forward(form)) for form in options})
            stack["eval_kernel"] = g.last_kernel()
            out_t, out_w = forward("torch"), forward("wide")
            stack["eval_max_abs_difference"], stack["eval_max_abs"] = float((out_t - out_w).abs().max()), float(out_t.abs().max())
            del out_t, out_w
            for model in models.values():
                for var in model.vars():
                    var.var.grad = None
            del models, tasks
            torch.cuda.empty_cache()
            stacks["feature_dropout=" + dropout] = stack
    print(json.dumps(dict(what=f"NGCFLayer at input width 128, R-MAT ({a.n} vertices, {g.nnz} entries), bipartite-normalised: the torch "
                               f"composition (a), sparse.ngcf_step as it is (b) and sparse.ngcf_step(wide=\"fused\") (c), interleaved in one "
                               f"process, {a.warm} warm-ups, {a.reps} repetitions, device events; the stack is NGCF(num_classes=128) over "
                               f"Structural(dims=128), dropout 0.1, LinkPrediction over {positives.shape[0]} positive pairs and one negative each",
                          single_layers=layers, stacks=stacks)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
