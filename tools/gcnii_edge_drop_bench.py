#!/usr/bin/env python3
"""A GCNIILayer stack UNDER EDGE DROPOUT (the reference's default, graph_dropout=0.5) in three forms, on the config-4 graph (symmetric
R-MAT, 10M vertices / 100M entries), one GPU: the training step (forward, loss, backward) of a `--layers` (8) layer
GCNIILayer(graph_dropout=0.5, dropout=0.6) stack behind one Dense layer, per width (64 and 32), and the peak memory of one step of each.

    python tools/gcnii_edge_drop_bench.py [--widths 64,32] [--layers 8] [--reps 20] [--warm 5] [--feature-dropout fused] [--backward fused]

  composed   GNN(gcnii_edge_dropout="composed"), the default: per layer the dropped SpMM + mix, the dense kernel, the mask as a pass of
             its own; in the backward the gate, gnx_dense_wgrad, gnx_dense and the transposed dropped SpMM
  fused      GNN(gcnii_edge_dropout="fused"): gnx_gcnii_step_dropped, and with --backward fused gnx_gcnii_step_back_dropped
  vals       the existing fused launch of a constant adjacency over ``adj.vals``: every layer materialises the nnz-sized value array of
             its dropped adjacency (gnx_graph_normalize) and, in the backward, the array in transposed order -- the other route there
             is today

The three are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one call of each, each between device events.
Reported: median and quartiles in ms, the ratios of the medians against "composed" (the yardstick is the "composed" call of the same
process), `slower` = the form's lower quartile is above the composed upper quartile, and the peak of torch's allocator over one training
step (above what was allocated before the step).  The three draw the same masks (the counter RNG, the same seeds and streams).  Prints
one JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnn-tf_amd")]

HOWS = ("composed", "fused", "vals")


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
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--widths", default="64,32")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.6)
    ap.add_argument("--graph-dropout", type=float, default=0.5)
    ap.add_argument("--feature-dropout", default="fused", choices=("torch", "fused"))
    ap.add_argument("--backward", default="fused", choices=("composed", "fused"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gcnii_edge_drop_bench: needs a GPU")
    if a.reps < 20 or a.warm < 5:
        print("note: fewer than 20 repetitions / 5 warm-ups: not a record", file=sys.stderr)
    device = torch.device("cuda:0")
    gnntf.set_default_device(device)
    u, v = rmat.rmat_relabelled_pairs(a.n, a.entries // 2, seed=1, device=device)
    idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
    del u, v
    g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], dtype=torch.float32, device=device), (a.n, a.n)), device=device)
    del idx
    if g.nnz_entries != g.nnz:
        g.enable_entry_dropout()
    g.reserve(max(int(c) for c in a.widths.split(",")), transposed=True)
    torch.cuda.empty_cache()

    class ValsLayer(gnntf.GCNIILayer):
        """GCNIILayer over the MATERIALISED values of its dropped adjacency: the existing fused launch of a constant adjacency."""

        def __forward__(self, gcn, features):
            adjacency = gcn.get_adjacency(self.graph_dropout)
            if isinstance(adjacency, sparse.DroppedAdjacency):
                adjacency = sparse.Adjacency(adjacency.graph, adjacency.vals)
            option = dict(relu=True, backward=gcn.gcnii_backward)
            if gcn.feature_dropout == "fused" and gcn.is_training():
                return sparse.gcnii_step(adjacency, features, self.H0.value, self.a, self._transform(), dropout=(self.dropout,) + tuple(gcn._next_mask_stream()),
                                         **option)
            return gcn.dropout(sparse.gcnii_step(adjacency, features, self.H0.value, self.a, self._transform(), **option), self.dropout)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    rng = np.random.default_rng(0)
    nodes = rng.permutation(a.n)[:a.n // 10]
    # checked and uploaded once: a host list would be range-checked and copied inside every timed step, of every form alike
    labels = sparse.DeviceIndex(rng.integers(0, 7, size=len(nodes)), device, 7, "label")
    nodes = sparse.DeviceIndex(nodes, device, a.n)
    rows = dict()
    for C in [int(c) for c in a.widths.split(",")]:
        X = torch.empty((a.n, C), dtype=torch.float32, device=device).uniform_(-1, 1, generator=torch.Generator(device).manual_seed(C))
        models = dict()
        for how in HOWS:
            gnntf.set_seed(3)
            torch.manual_seed(3)
            model = gnntf.GNN(g, X, feature_dropout=a.feature_dropout, gcnii_backward=a.backward,
                              gcnii_edge_dropout="fused" if how == "fused" else "composed")
            model.add(gnntf.Dense(C, dropout=0, activation=gnntf.relu))
            H0 = model.top_layer()
            layer_type = ValsLayer if how == "vals" else gnntf.GCNIILayer
            for k in range(a.layers):
                model.add(layer_type(H0, 0.1, 0.5, k, activation=gnntf.relu, dropout=a.dropout, graph_dropout=a.graph_dropout))
            model.add(gnntf.Dense(7, dropout=0, regularize=False))
            model.reset()
            seeded = torch.Generator(device).manual_seed(100 + C)
            for layer in model.layers():                            # the reference initialises W to zero: use seeded ones
                if isinstance(layer, gnntf.GCNIILayer):
                    layer.W.data.uniform_(-1 / 8, 1 / 8, generator=seeded)
            models[how] = model

        kernels = dict()

        def step(how):
            model = models[how]
            model.training_mode(True)
            for var in model.vars():
                var.var.grad = None
            with model:
                logits = model(model.features)
                kernels[how] = g.last_kernel()
                gnntf.node_ce(logits, nodes, labels).backward()

        for _ in range(a.warm):
            for how in HOWS:
                step(how)
        times = {how: [] for how in HOWS}
        for _ in range(a.reps):
            for how in HOWS:
                times[how].append(timed(lambda: step(how)))
        q = {how: quartiles(times[how]) for how in HOWS}
        row = dict(train_step=q, forward_kernel=dict(kernels))
        for how in HOWS[1:]:
            row[f"composed_over_{how}"] = round(q["composed"]["median_ms"] / max(q[how]["median_ms"], 1e-9), 4)
            row[f"{how}_slower"] = bool(q[how]["p25_ms"] > q["composed"]["p75_ms"])
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
        rows[str(C)] = row
        del models, X
        torch.cuda.empty_cache()
    print(json.dumps(dict(what=f"GCNIILayer stack, {a.layers} layers, graph_dropout {a.graph_dropout}, dropout {a.dropout}, feature_dropout "
                               f"{a.feature_dropout!r}, gcnii_backward {a.backward!r}, symmetric R-MAT ({a.n} vertices, {g.nnz} entries, "
                               f"{g.nnz_entries} stored): gcnii_edge_dropout \"composed\" against \"fused\" and against the fused launch over "
                               f"materialised values, interleaved in one process, {a.warm} warm-ups, {a.reps} repetitions, device events",
                          widths=rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
