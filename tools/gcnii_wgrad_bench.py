#!/usr/bin/env python3
"""GCNII training with the mixed rows T stored, and with the weight gradient that makes them again (GNN(gcnii_weight_gradient=),
sparse.gcnii_wgrad over gnx_gcnii_wgrad / gnx_gcnii_wgrad_bf16), one GPU: the training step (forward, loss, backward) of a `--layers` (8)
layer GCNII stack, dropout 0.6, per width (16, 32, 64), with f32 and with bf16 rows, on the config-4 graph (symmetric R-MAT, 10M vertices
/ 100M entries; `--graphs 1m` for 10^6 / 10^7).

    python tools/gcnii_wgrad_bench.py [--graphs config4] [--widths 16,32,64] [--layers 8] [--reps 20] [--warm 5]

Three forms of the step, all GCNII(feature_dropout="fused", gcnii_backward="fused"):
  stored      gcnii_weight_gradient="stored": the forward writes T, it is saved, dM = T^T G through gnx_dense_wgrad (the default)
  recomputed  gcnii_weight_gradient="recomputed": no T; dM from the one launch that makes T again in LDS
  composed    the recomputation composed HERE from existing public calls, no new kernel: the "recomputed" model with its weight gradient
              replaced by the plain SpMM + mix into one scratch [n, C] (gnx_spmm / gnx_spmm_bf16) and gnx_dense_wgrad over it -- what the
              fused launch has to beat to be worth having
For either dtype the three are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one step of each, each between
device events.  Reported per form: median and quartiles in ms, the ratio against "stored", the step's peak above what is allocated
before it (torch.cuda.max_memory_allocated, no model holding anything of an earlier step), and the deepest stack of that width the form
could hold on this card: (the card's memory - what the step holds beside its layers) / (the bytes a layer adds), both taken from two
measured depths (`--layers` and half of it).  The width and row gates of the bf16 path are switched off
for the run.  Prints one JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnn-tf_amd"), os.path.join(ROOT, "tests")]

FORMS = ("stored", "recomputed", "composed")


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
    ap.add_argument("--graphs", default="config4")
    ap.add_argument("--widths", default="16,32,64")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gcnii_wgrad_bench: needs a GPU")
    if a.reps < 20 or a.warm < 5:
        print("note: fewer than 20 repetitions / 5 warm-ups: not a record", file=sys.stderr)
    device = torch.device("cuda:0")
    gnntf.set_default_device(device)
    sparse.GCNII_BF16_TRAIN_MIN_WIDTH, sparse.GCNII_BF16_TRAIN_MIN_ROWS = 0, 0

    def rmat_graph(n, entries):
        u, v = rmat.rmat_relabelled_pairs(n, entries // 2, seed=1, device=device)
        idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
        return gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], dtype=torch.float32, device=device), (n, n)), device=device)

    makers = dict(config4=lambda: rmat_graph(10_000_000, 100_000_000), **{"1m": lambda: rmat_graph(1_000_000, 10_000_000)})

    fused_wgrad = sparse.gcnii_wgrad
    scratch = dict()

    def composed_wgrad(adj, H, H0, a_mix, G, hub_rows=None):
        """T by the plain SpMM + mix into one scratch, then gnx_dense_wgrad: existing calls only."""
        key = tuple(H.shape)
        if key not in scratch:
            scratch.clear()
            scratch[key] = torch.empty(H.shape, dtype=torch.float32, device=H.device)
        beta = 1.0 - float(a_mix)
        if H.dtype == torch.bfloat16:
            T = sparse._launch_bf16(adj, H, H0, beta, float(a_mix), nat.ACT_NONE, out_bf16=False, out=scratch[key])
        else:
            T = sparse._launch(adj, H, H0, beta, float(a_mix), nat.ACT_NONE, out=scratch[key])
        return sparse._dense_wgrad(T, G)

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
        labels = sparse.DeviceIndex(rng.integers(0, 7, size=len(nodes)), device, 7, "label")
        nodes = sparse.DeviceIndex(nodes, device, n)
        rows = dict()
        for C in [int(c) for c in a.widths.split(",")]:
            X = torch.empty((n, C), dtype=torch.float32, device=device).uniform_(-1, 1, generator=torch.Generator(device).manual_seed(C))

            def make(dtype, form, layers):
                gnntf.set_seed(3)
                torch.manual_seed(3)
                model = gnntf.GCNII(g, X, 7, latent_dims=[C], iterations=layers, dropout=a.dropout, feature_dropout="fused",
                                    gcnii_backward="fused", gcnii_training_dtype=dtype,
                                    gcnii_weight_gradient="stored" if form == "stored" else "recomputed")
                model.reset()
                for layer in model.layers():                        # the reference initialises W to zero: use seeded weights
                    if isinstance(layer, gnntf.GCNIILayer):
                        layer.W.data.uniform_(-1 / 8, 1 / 8)
                return model

            kernels = dict()

            def step(model, form):
                sparse.gcnii_wgrad = composed_wgrad if form == "composed" else fused_wgrad
                for var in model.vars():
                    var.var.grad = None
                with model:
                    gnntf.node_ce(model(model.features), nodes, labels).backward()
                kernels[form] = g.last_kernel()
                sparse.gcnii_wgrad = fused_wgrad

            def release(model):
                """What a model keeps between steps: its layers' values (every layer's output) and its gradients."""
                for layer in model.layers():
                    layer.value = None
                for var in model.vars():
                    var.var.grad = None

            def peak(model, form, others):
                """The step's peak ABOVE what is allocated before it, with nothing of any model's last step left on the device."""
                for other in list(others) + [model]:
                    release(other)
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                step(model, form)
                torch.cuda.synchronize()
                return torch.cuda.max_memory_allocated() - before

            per_dtype = dict()
            for how, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                models = {form: make(dtype, form, a.layers) for form in FORMS}
                for _ in range(a.warm):
                    for form in FORMS:
                        step(models[form], form)
                times = {form: [] for form in FORMS}
                for _ in range(a.reps):
                    for form in FORMS:
                        times[form].append(timed(lambda: step(models[form], form)))
                q = {form: quartiles(times[form]) for form in FORMS}
                out = dict()
                for form in FORMS:
                    full = peak(models[form], form, models.values())
                    half_layers = max(a.layers // 2, 1)
                    half_model = make(dtype, form, half_layers)
                    step(half_model, form)                          # (its lazy allocations: the adjacency, the sparse input rows)
                    half = peak(half_model, form, models.values())
                    release(half_model)
                    del half_model
                    per_layer = (full - half) / max(a.layers - half_layers, 1)
                    fixed = torch.cuda.memory_allocated() + full - a.layers * per_layer      # the graph, the features, the step's other buffers
                    room = torch.cuda.mem_get_info()[1] - fixed
                    out[form] = dict(q[form], over_stored=round(q[form]["median_ms"] / max(q["stored"]["median_ms"], 1e-9), 4),
                                     peak_bytes=int(full), bytes_per_layer=int(per_layer),
                                     bytes_per_element_and_layer=round(per_layer / (n * C), 3),
                                     deepest_stack_at_this_width=int(room // per_layer) if per_layer > 0 else None,
                                     last_kernel=kernels.get(form))
                out["recomputed_over_composed"] = round(q["recomputed"]["median_ms"] / max(q["composed"]["median_ms"], 1e-9), 4)
                out["recomputed_faster_than_composed"] = bool(q["recomputed"]["p75_ms"] < q["composed"]["p25_ms"])
                out["recomputed_slower_than_composed"] = bool(q["recomputed"]["p25_ms"] > q["composed"]["p75_ms"])
                per_dtype[how] = out
                del models
                scratch.clear()
                torch.cuda.empty_cache()
            rows[str(C)] = per_dtype
            del X
            torch.cuda.empty_cache()
        record[name] = dict(vertices=n, entries=g.nnz, hub_rows=g.n_hub_rows, device_bytes=int(torch.cuda.mem_get_info()[1]), widths=rows)
        del g, nodes, labels
        torch.cuda.empty_cache()
    print(json.dumps(dict(what=f"GCNII training step (forward, loss, backward), {a.layers} layers, dropout {a.dropout}, feature_dropout and "
                               f"gcnii_backward \"fused\": the weight gradient over stored rows, recomputed in one launch, and recomputed by "
                               f"composition (SpMM + mix into a scratch, then gnx_dense_wgrad), interleaved in one process, {a.warm} warm-ups, "
                               f"{a.reps} repetitions, device events; deepest stack = (device memory - the step's fixed part) / (bytes a layer "
                               f"adds), both from the peaks measured at {a.layers} and {max(a.layers // 2, 1)} layers", graphs=record)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
