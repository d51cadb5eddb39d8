#!/usr/bin/env python3
"""Node signals at width 1 (csrc/gnx_signal.hip) against the compositions they replace, one GPU, the symmetric R-MAT (10M vertices /
100M entries):

  (a) sweep        PPRSweep's ten iterations as the composition does them today -- sparse.appnp_propagate over an [n, C] matrix of
                   ones, then the division -- against sparse.sweep (signal_ppr at width 1, then the division), at C = 64 and C = 7;
  (b) smoothness   FastReg's quotient, forward + backward at C = 64 (dX and dw): smoothness(fused=False) -- spmm at width 1, its
                   gnx_spmm_tv backward, torch sums -- against fused=True;
  (c) step         the training step of GCNIIReg(iterations=8, latent_dims=[64]) over `--features` dense feature columns with and
                   without its FastReg layer (what the regulariser costs a step);
  (d) groups       with GNX_LIBRARY pointing at a tuning build (make TUNING=1): signal_ppr and the smoothness forward + backward with 8
                   and with 4 lanes per short row (GNX_SIGNAL_LANES), interleaved like everything else.

    python tools/signal_bench.py [--n 10000000] [--entries 100000000] [--reps 20] [--warm 5] [--only sweep,smoothness,step,groups]
                                 [--widths 64,7]

The variants of a cell are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one call of each, each between
device events.  Reported: median and quartiles in ms, the ratio of the medians, `fused_slower` = the fused lower quartile is above the
composition's upper quartile, and how far the two results are apart.  A cell that loses is reported as such.  Prints one JSON record."""
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


def compare(times, base, new):
    cell = {name: quartiles(ms) for name, ms in times.items()}
    cell[f"{base}_over_{new}"] = round(cell[base]["median_ms"] / max(cell[new]["median_ms"], 1e-9), 4)
    cell[f"{new}_slower"] = bool(cell[new]["p25_ms"] > cell[base]["p75_ms"])
    return cell


def main():
    import numpy as np
    import torch
    import gnntf
    from gnntf import rmat, sparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--only", default="sweep,smoothness,step")
    ap.add_argument("--widths", default="64,7", help="feature widths of the sweep cell")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("signal_bench: needs a GPU")
    if a.reps < 20 or a.warm < 5:
        print("note: fewer than 20 repetitions / 5 warm-ups: not a record", file=sys.stderr)
    only = set(a.only.split(","))
    device = torch.device("cuda:0")
    gnntf.set_default_device(device)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def interleaved(calls, base, new):
        for _ in range(a.warm):
            for fn in calls.values():
                fn()
        times = {name: [] for name in calls}
        for _ in range(a.reps):
            for name, fn in calls.items():
                times[name].append(timed(fn))
        return compare(times, base, new)

    u, v = rmat.rmat_relabelled_pairs(a.n, a.entries // 2, seed=1, device=device)
    idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
    del u, v
    g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], dtype=torch.float32, device=device), (a.n, a.n)), device=device)
    del idx
    torch.cuda.empty_cache()
    g.reserve(1, transposed=True)
    adj = gnntf.normalize(g, "symmetric")
    raw = gnntf.normalize(g, "none")
    record = dict(what=f"node signals at width 1 against their compositions, symmetric R-MAT ({a.n} vertices, {g.nnz} entries, {g.n_hub_rows} hub "
                       f"rows), interleaved in one process, {a.warm} warm-ups, {a.reps} repetitions, device events",
                  library=os.environ.get("GNX_LIBRARY", ""))
    seeded = torch.Generator(device).manual_seed(5)

    if "sweep" in only:
        cells = dict()
        with torch.no_grad():
            for C in (int(c) for c in a.widths.split(",")):
                X = torch.empty((a.n, C), dtype=torch.float32, device=device).uniform_(-1, 1, generator=seeded)
                # (the width-1 form spelled out: sparse.sweep itself takes the composition where that measured faster)
                calls = dict(composed=lambda: X / sparse.appnp_propagate(adj, torch.ones_like(X), 0.1, 10),
                             fused=lambda: X / sparse.signal_ppr(adj, None, 0.1, 10)[:, None])
                cell = interleaved(calls, "composed", "fused")
                one, two = calls["composed"](), calls["fused"]()
                cell["max_relative_difference"] = float(((one - two).abs() / two.abs().clamp_min(1e-30)).max())
                cell["kernel"] = g.last_kernel()
                cells[f"C={C}"] = cell
                del X, one, two
                torch.cuda.empty_cache()
        record["sweep_ten_iterations"] = cells

    if "smoothness" in only or "groups" in only:
        X = torch.empty((a.n, 64), dtype=torch.float32, device=device).uniform_(-1, 1, generator=seeded).requires_grad_()
        w = torch.empty((64, 1), dtype=torch.float32, device=device).uniform_(-1, 1, generator=seeded).requires_grad_()
        D = sparse.signal_colsum(raw)

        def both_ways(fused):
            def run():
                X.grad = w.grad = None
                (-sparse.smoothness(raw, X, w, colsum=D, fused=fused)).backward()
            return run

    if "smoothness" in only:
        calls = dict(composed=both_ways(False), fused=both_ways(True))
        cell = interleaved(calls, "composed", "fused")
        grads = dict()
        for name, fn in calls.items():
            fn()
            grads[name] = (X.grad.clone(), w.grad.clone())
        cell["max_difference_dX_over_max_dX"] = float((grads["composed"][0] - grads["fused"][0]).abs().max() / grads["fused"][0].abs().max())
        cell["max_difference_dw_over_max_dw"] = float((grads["composed"][1] - grads["fused"][1]).abs().max() / grads["fused"][1].abs().max())
        cell["kernel"] = g.last_kernel()
        record["smoothness_forward_backward_C64"] = cell
        del grads

    if "groups" in only:
        if "tune" not in os.environ.get("GNX_LIBRARY", ""):
            raise SystemExit("signal_bench --only groups: needs GNX_LIBRARY pointing at a tuning build (make -C gnn-tf_amd/csrc TUNING=1)")

        def with_lanes(lanes, fn):
            def run():
                os.environ["GNX_SIGNAL_LANES"] = str(lanes)
                fn()
            return run

        with torch.no_grad():
            ppr = lambda: sparse.signal_ppr(adj, None, 0.1, 10)
            record["groups_signal_ppr"] = interleaved(dict(lanes8=with_lanes(8, ppr), lanes4=with_lanes(4, ppr)), "lanes8", "lanes4")
        record["groups_smoothness_forward_backward"] = interleaved(dict(lanes8=with_lanes(8, both_ways(True)), lanes4=with_lanes(4, both_ways(True))),
                                                                   "lanes8", "lanes4")
        os.environ["GNX_SIGNAL_LANES"] = "8"

    if "smoothness" in only or "groups" in only:
        X.grad = w.grad = None
        del X, w, D
        torch.cuda.empty_cache()

    if "step" in only:
        rng = np.random.default_rng(0)
        nodes = rng.permutation(a.n)[:a.n // 10]
        labels = sparse.DeviceIndex(rng.integers(0, 40, size=len(nodes)), device, 40, "label")
        nodes = sparse.DeviceIndex(nodes, device, a.n)
        feats = torch.empty((a.n, a.features), dtype=torch.float32, device=device).uniform_(-1, 1, generator=seeded)

        def make(regularised):
            gnntf.set_seed(3)
            torch.manual_seed(3)
            if regularised:
                model = gnntf.GCNIIReg(g, feats, 40, latent_dims=[64], iterations=8)
            else:                                       # the same constructor without the FastReg layer
                model = gnntf.GNN(g, feats)
                model.add(gnntf.Dropout(0.6))
                model.add(gnntf.Dense(64, dropout=0.6, activation=gnntf.relu))
                H0 = model.top_layer()
                for k in range(8):
                    model.add(gnntf.GCNIILayer(H0, 0.1, 0.5, k, activation=gnntf.relu, dropout=0.6, graph_dropout=0))
                model.add(gnntf.Dense(40, dropout=0, regularize=False))
            model.reset()
            return model

        def step(model):
            def run():
                for var in model.vars():
                    var.var.grad = None
                with model:
                    total = gnntf.node_ce(model(model.features), nodes, labels)
                    for layer in model.layers():
                        if layer.output_regularize != 0:
                            total = total + layer.loss()
                    total.backward()
            return run

        models = dict(without=make(False), with_fastreg=make(True))
        cell = interleaved({name: step(model) for name, model in models.items()}, "without", "with_fastreg")
        record["gcniireg_iterations8_training_step"] = cell

    print(json.dumps(record))
    return 0


if __name__ == "__main__":
    sys.exit(main())
