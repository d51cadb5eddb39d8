#!/usr/bin/env python3
"""The NGCF layer's backward at input width 128 -- the width of the reference's library_recommendation demo -- two ways, on the config-4
graph (symmetric R-MAT, 10M vertices / 100M entries) BIPARTITE-normalised as the layer takes it, one GPU; the forward is
sparse.ngcf_step(wide="fused") (gnx_step_wide_ngcf) both times:

  "composed"   the node's backward as it is at this width: gnx_ngcf_back_gate, two column sums, a torch multiply, gnx_dense_wgrad
               twice, two transposed weight copies, gnx_dense twice, addcmul, the transposed SpMM, addcmul;
  "fused"      sparse.ngcf_step(wide_backward="fused"): gnx_step_back_wide_ngcf (the gate pass with the slab-ordered bias sums, one
               row-local launch, the transposed SpMM with Q1 * A mixed in) and gnx_dense_wgrad twice.

  * single layers 128 -> 128 and 128 -> 64 with both biases and leaky_relu: the backward alone (to X, W1, b1, W2, b2 over a retained
    graph) with its peak memory, the training step (forward, a weighted sum as the loss, backward) with its peak memory, and the
    transposed SpMM alone beside them;
  * the training step and its peak memory of the 3-layer NGCF(num_classes=128) over Structural(dims=128) and features without columns,
    with LinkPrediction's pairwise loss over `--pairs` positive pairs and one negative each (a fixed list on the device), dropout 0.1,
    under feature_dropout="fused" and under torch's dropout, ngcf_layer="fused" and ngcf_wide="fused" both times.

    python tools/ngcf_wide_back_bench.py [--outputs 128,64] [--reps 20] [--warm 5] [--out profiles/notes/ngcf_wide_back_bench.json]

The forms are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one call of each, each between device events.
Reported: median and quartiles in ms, the ratio of the medians, the peak of torch's allocator over one call (above what was allocated
before it), and the largest difference of the gradients (the same weights; float32 rounding).  The yardstick is "composed" of the same
process.  Prints one JSON record, and writes it to `--out` where that is given."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnn-tf_amd")]

FORMS = ("composed", "fused")


def quartiles(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]
    return dict(median_ms=round(q(0.5), 4), p25_ms=round(q(0.25), 4), p75_ms=round(q(0.75), 4))


def compare(times):
    out = {form: quartiles(ms) for form, ms in times.items()}
    out["composed_over_fused"] = round(out["composed"]["median_ms"] / max(out["fused"]["median_ms"], 1e-9), 4)
    out["fused_slower_than_composed"] = bool(out["fused"]["p25_ms"] > out["composed"]["p75_ms"])
    return out


def main():
    import numpy as np
    import torch
    import gnntf
    from gnntf import rmat, sparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--outputs", default="128,64")
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--no-stack", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ngcf_wide_back_bench: needs a GPU")
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
    note = lambda text: print("ngcf_wide_back_bench: " + text, file=sys.stderr, flush=True)
    note(f"the graph is built: {g.nnz} entries")

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

    layer_of = {form: (lambda *t, form=form: sparse.ngcf_step(adj, *t, wide="fused", wide_backward=form)) for form in FORMS}
    layers = dict()
    for C_out in (int(c) for c in a.outputs.split(",")):
        seeded = torch.Generator(device).manual_seed(1000 + C_out)
        draw = lambda shape, lo, hi: torch.empty(shape, dtype=torch.float32, device=device).uniform_(lo, hi, generator=seeded)
        X, G = draw((a.n, 128), -1, 1), draw((a.n, C_out), -1, 1)
        W1, W2 = draw((128, C_out), -1 / 11, 1 / 11), draw((128, C_out), -1 / 11, 1 / 11)
        b1, b2 = draw((1, C_out), -0.2, 0.2), draw((1, C_out), -0.2, 0.2)
        leaves = (X, W1, b1, W2, b2)

        def step(form):
            for t in leaves:
                t.grad = None
                t.requires_grad_(True)
            (layer_of[form](*leaves) * G).sum().backward()
            for t in leaves:
                t.requires_grad_(False)

        row = dict()
        with torch.no_grad():
            row["spmm_tv_alone"] = quartiles([timed(lambda: sparse._launch(adj, X, None, 1.0, 0.0, sparse.nat.ACT_NONE, transposed=True)) for _ in range(a.warm + a.reps)][a.warm:])
        # the backward alone: one retained graph per form, the gradients of all five leaves asked of it again and again
        for t in leaves:
            t.requires_grad_(True)
        outs = {form: layer_of[form](*leaves) for form in FORMS}
        back = {form: (lambda form=form: torch.autograd.grad(outs[form], leaves, G, retain_graph=True)) for form in FORMS}
        row["backward"] = interleaved(back)
        row["backward_peak_mib"] = {form: peak_of(back[form]) for form in FORMS}
        grads = dict()
        for form in FORMS:
            grads[form] = back[form]()
            row["kernel_" + form] = g.last_kernel()
        row["max_abs_difference"] = {name: float((c - f).abs().max()) for name, c, f in zip(("dX", "dW1", "db1", "dW2", "db2"), grads["composed"], grads["fused"])}
        row["max_abs"] = {name: float(c.abs().max()) for name, c in zip(("dX", "dW1", "db1", "dW2", "db2"), grads["composed"])}
        del outs, back, grads
        for t in leaves:
            t.requires_grad_(False)
        torch.cuda.empty_cache()
        row["train_step"] = interleaved({form: (lambda form=form: step(form)) for form in FORMS})
        row["train_step_peak_mib"] = {form: peak_of(lambda form=form: step(form)) for form in FORMS}
        layers[f"128->{C_out}"] = row
        note(f"128->{C_out}: " + json.dumps(row))
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
        for dropout in ("fused", "torch"):
            models, tasks = dict(), dict()
            for form in FORMS:
                gnntf.set_seed(3)
                torch.manual_seed(3)
                models[form] = gnntf.NGCF(g, np.zeros((a.n, 0), dtype=np.float32), num_classes=128,
                                          preprocessor=gnntf.Structural(dims=128, regularize=0, bipartite=a.n // 2), feature_dropout=dropout,
                                          ngcf_layer="fused", ngcf_wide="fused", ngcf_wide_backward=form)
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

            stack = dict(train_step=interleaved({form: (lambda form=form: step(form)) for form in FORMS}))
            stack["train_step_peak_mib"] = {form: peak_of(lambda form=form: step(form)) for form in FORMS}
            stack["last_kernel"] = g.last_kernel()
            for model in models.values():
                for var in model.vars():
                    var.var.grad = None
            del models, tasks
            torch.cuda.empty_cache()
            stacks["feature_dropout=" + dropout] = stack
            note(f"the stack under feature_dropout={dropout}: " + json.dumps(stack))
    record = dict(what=f"NGCFLayer backward at input width 128, R-MAT ({a.n} vertices, {g.nnz} entries), bipartite-normalised, after "
                       f"sparse.ngcf_step(wide=\"fused\"): the composed backward against wide_backward=\"fused\", interleaved in one process, "
                       f"{a.warm} warm-ups, {a.reps} repetitions, device events; the stack is NGCF(num_classes=128) over Structural(dims=128), "
                       f"dropout 0.1, LinkPrediction over {positives.shape[0]} positive pairs and one negative each",
                  single_layers=layers, stacks=stacks)
    text = json.dumps(record)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(record, indent=1) + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
