#!/usr/bin/env python3
"""The backward of the GCNII layer, composed (gnx_dense, the transposed gnx_spmm, a scaling) against fused (ONE launch,
gnx_gcnii_step_back), on the config-4 graph (symmetric R-MAT, 10M vertices / 100M entries), one GPU:

  * the backward of ONE sparse.gcnii_step (relu): the relu mask, gnx_dense_wgrad and the rest, i.e. torch.autograd.grad of the layer's
    output with respect to H, H0 and M, per width;
  * the training step (forward, loss, backward) of a `--layers` (64) layer GCNII at C = 64 both ways.  A stack of 64 layers keeps two
    [n, C] arrays per layer for its backward, which at 10M vertices is more than a card holds: the step runs on a symmetric R-MAT of
    `--model-n` vertices (1M) and `--model-entries` entries (10M), and the record says so.

    python tools/gcnii_back_bench.py [--widths 16,32,64] [--layers 64] [--reps 20] [--warm 5]

Composed and fused are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one composed and one fused call, each
between device events.  Reported: median and quartiles in ms, the ratio of the medians, and `fused_slower` = the fused lower quartile
is above the composed upper quartile.  The yardstick is the composed call of the same process.  Prints one JSON record."""
import argparse
import json
import math
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
    from gnntf import rmat, sparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--widths", default="16,32,64")
    ap.add_argument("--layers", type=int, default=64)
    ap.add_argument("--model-n", type=int, default=1_000_000)
    ap.add_argument("--model-entries", type=int, default=10_000_000)
    ap.add_argument("--a", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gcnii_back_bench: needs a GPU")
    if a.reps < 20 or a.warm < 5:
        print("note: fewer than 20 repetitions / 5 warm-ups: not a record", file=sys.stderr)
    device = torch.device("cuda:0")
    gnntf.set_default_device(device)

    def rmat_graph(n, entries):
        u, v = rmat.rmat_relabelled_pairs(n, entries // 2, seed=1, device=device)
        idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
        del u, v
        return gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], dtype=torch.float32, device=device), (n, n)), device=device)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def compare(composed, fused):
        for _ in range(a.warm):
            composed(), fused()
        tc, tf = [], []
        for _ in range(a.reps):
            tc.append(timed(composed))
            tf.append(timed(fused))
        qc, qf = quartiles(tc), quartiles(tf)
        return dict(composed=qc, fused=qf, composed_over_fused=round(qc["median_ms"] / max(qf["median_ms"], 1e-9), 4),
                    fused_slower=bool(qf["p25_ms"] > qc["p75_ms"]))

    rows = dict()
    g = rmat_graph(a.n, a.entries)
    adj = gnntf.normalize(g, "symmetric")
    adj.transposed_values()
    g.reserve(max(int(c) for c in a.widths.split(",")), transposed=True)
    torch.cuda.synchronize()
    for C in [int(c) for c in a.widths.split(",")]:
        gen = torch.Generator(device).manual_seed(C)
        rand = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device).uniform_(-1, 1, generator=gen)
        H, H0, up = rand(a.n, C).requires_grad_(), rand(a.n, C).requires_grad_(), rand(a.n, C)
        b = math.log1p(0.5)
        M = ((1 - b) * torch.eye(C, device=device) + b * rand(C, C) / math.sqrt(C)).requires_grad_()
        outs = {how: sparse.gcnii_step(adj, H, H0, a.a, M, relu=True, backward=how) for how in sparse.GCNII_BACKWARDS}
        back = lambda how: torch.autograd.grad(outs[how], (H, H0, M), up, retain_graph=True)
        rec = dict(layer_backward=compare(lambda: back("composed"), lambda: back("fused")))
        gc, gf = back("composed"), back("fused")
        rec["kernel"] = g.last_kernel()
        rec["rel_frobenius"] = dict(dH=float(torch.linalg.norm(gf[0] - gc[0]) / torch.linalg.norm(gc[0])),
                                    dH0=float(torch.linalg.norm(gf[1] - gc[1]) / torch.linalg.norm(gc[1])))
        rows[str(C)] = rec
        del H, H0, up, M, outs, gc, gf
        torch.cuda.empty_cache()
    del g, adj
    torch.cuda.empty_cache()

    # the training step of the deepest model, both ways, over one device graph
    C = 64
    mg = rmat_graph(a.model_n, a.model_entries)
    rng = np.random.default_rng(0)
    X = torch.empty((a.model_n, C), dtype=torch.float32, device=device).uniform_(-1, 1, generator=torch.Generator(device).manual_seed(1))
    nodes = rng.permutation(a.model_n)[:a.model_n // 10]
    labels = rng.integers(0, 7, size=len(nodes))
    models = dict()
    for how in sparse.GCNII_BACKWARDS:
        gnntf.set_seed(3)
        torch.manual_seed(3)
        model = gnntf.GCNII(mg, X, 7, latent_dims=[C], iterations=a.layers, gcnii_backward=how)
        model.reset()
        for layer in model.layers():                                # the reference initialises W to zero: use seeded weights
            if isinstance(layer, gnntf.GCNIILayer):
                layer.W.data.uniform_(-1 / 8, 1 / 8)
        models[how] = model

    def step(how):
        model = models[how]
        for v in model.vars():
            v.var.grad = None
        with model:
            gnntf.node_ce(model(model.features), nodes, labels).backward()

    model_rec = compare(lambda: step("composed"), lambda: step("fused"))
    step("fused")
    model_rec["kernel"] = mg.last_kernel()
    print(json.dumps(dict(what=f"backward of the GCNII layer, symmetric R-MAT ({a.n} vertices, {a.entries} drawn entries), relu: "
                               "torch.autograd.grad of one gcnii_step with respect to H, H0 and M (mask, wgrad, the rest); composed and "
                               f"fused interleaved in one process, {a.warm} warm-ups, {a.reps} repetitions, device events",
                          widths=rows,
                          model=dict(what=f"GCNII training step (forward, loss, backward), {a.layers} layers, C = {C}, symmetric R-MAT "
                                          f"({a.model_n} vertices, {mg.nnz} entries), dropout 0.6", **model_rec))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
