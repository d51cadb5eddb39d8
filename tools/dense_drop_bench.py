#!/usr/bin/env python3
"""Dropout around the dense transform -- the front of APPNP and GCNII: Dropout(p_in), then Dense(O, relu, dropout=p_out) -- three ways,
one GPU:

  (a) torch     today's path: torch.nn.functional.dropout, sparse.dense, torch.nn.functional.dropout
  (b) passes    the counter-RNG passes around the same kernel: sparse.feature_dropout, sparse.dense, sparse.feature_dropout
  (c) fused     sparse.dense_step: both masks made inside the dense kernels' launch (gnx_dense_drop), the weight gradient making the
                input mask again (gnx_dense_wgrad_drop)

  * per shape n x F -> O (10M x 256 -> 64, 10M x 128 -> 64, 10M x 64 -> 64; rates 0.5 / 0.6): the forward, forward + backward with a
    constant X (dW and db; no dX), and the allocator's peak over one forward + backward of each;
  * the training step and its peak memory of APPNP(latent_dims=[64], num_classes=40) on the symmetric R-MAT (10M vertices / 100M
    entries) over `--features` (256) dense feature columns, GNN(dense_dropout="torch") against "fused".

    python tools/dense_drop_bench.py [--shapes 256x64,128x64,64x64] [--reps 20] [--warm 5] [--no-model] [--forward-only]

The variants are interleaved in one process: `warm` warm-ups of each, then `reps` rounds of one call of each, each between device
events.  Reported: median and quartiles in ms, the ratios of the medians to (a), `fused_slower` = the fused lower quartile is above
torch's upper quartile, peaks in MiB above what was allocated before the call, and -- (b) and (c) draw the same masks -- whether their
results are the same bits.  (a) is the yardstick: the path of a model without the keyword.  A cell that loses is reported as such.
With GNX_LIBRARY pointing at a tuning build, GNX_DENSE_WREG=0 / GNX_DENSE_RING=0 take kernels out of the dispatch: `kernel_choice`
names what the environment asked for.  Prints one JSON record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnn-tf_amd")]

VARIANTS = ("torch", "passes", "fused")


def quartiles(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]
    return dict(median_ms=round(q(0.5), 4), p25_ms=round(q(0.25), 4), p75_ms=round(q(0.75), 4))


def compare(times):
    """times: variant -> list of ms"""
    cell = {name: quartiles(ms) for name, ms in times.items()}
    base = cell["torch"]["median_ms"]
    for name in times:
        if name != "torch":
            cell[f"torch_over_{name}"] = round(base / max(cell[name]["median_ms"], 1e-9), 4)
    cell["fused_slower"] = bool(cell["fused"]["p25_ms"] > cell["torch"]["p75_ms"])
    return cell


def main():
    import numpy as np
    import torch
    import gnntf
    from gnntf import rmat, sparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--shapes", default="256x64,128x64,64x64")
    ap.add_argument("--rates", default="0.5,0.6")
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--forward-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_drop_bench: needs a GPU")
    if a.reps < 20 or a.warm < 5:
        print("note: fewer than 20 repetitions / 5 warm-ups: not a record", file=sys.stderr)
    device = torch.device("cuda:0")
    gnntf.set_default_device(device)
    p_in, p_out = (float(r) for r in a.rates.split(","))
    handle = gnntf.DeviceGraph(gnntf.SparseCOO(torch.tensor([[0, 1], [1, 0]], device=device), torch.ones(2, device=device), (2, 2)), device=device)
    IN, OUT = (p_in, 3, 0), (p_out, 3, 1)
    drop = torch.nn.functional.dropout

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def interleaved(calls):
        for _ in range(a.warm):
            for fn in calls.values():
                fn()
        times = {name: [] for name in calls}
        for _ in range(a.reps):
            for name, fn in calls.items():
                times[name].append(timed(fn))
        return compare(times)

    def peak_of(fn):                                                # the allocator's peak over one call, above what stood before it
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)

    shapes = dict()
    for shape in a.shapes.split(","):
        F, O = (int(c) for c in shape.split("x"))
        seeded = torch.Generator(device).manual_seed(1000 * F + O)
        X = torch.empty((a.n, F), dtype=torch.float32, device=device).uniform_(-1, 1, generator=seeded)
        W = torch.empty((F, O), dtype=torch.float32, device=device).uniform_(-1 / 8, 1 / 8, generator=seeded).requires_grad_()
        b = torch.empty((1, O), dtype=torch.float32, device=device).uniform_(-0.2, 0.2, generator=seeded).requires_grad_()
        up = torch.empty((a.n, O), dtype=torch.float32, device=device).uniform_(-1, 1, generator=seeded)
        forwards = dict(torch=lambda: drop(sparse.dense(drop(X, p_in), W, b, relu=True), p_out),
                        passes=lambda: sparse.feature_dropout(handle, sparse.dense(sparse.feature_dropout(handle, X, *IN), W, b, relu=True), *OUT),
                        fused=lambda: sparse.dense_step(handle, X, W, b, relu=True, in_dropout=IN, out_dropout=OUT))

        def both_ways(forward):
            def run():
                W.grad = b.grad = None
                forward().backward(up)
            return run

        with torch.no_grad():
            row = dict(forward=interleaved(forwards))
            row["passes_and_fused_same_bits"] = bool(torch.equal(forwards["passes"](), forwards["fused"]()))
        if not a.forward_only:
            steps = {name: both_ways(fn) for name, fn in forwards.items()}
            row["forward_backward_constant_X"] = interleaved(steps)
            row["peak_mib_forward_backward"] = {name: peak_of(fn) for name, fn in steps.items()}
            grads = dict()
            for name in ("passes", "fused"):
                steps[name]()
                grads[name] = (W.grad.clone(), b.grad.clone())
            row["passes_and_fused_same_gradient_bits"] = bool(all(torch.equal(x, y) for x, y in zip(grads["passes"], grads["fused"])))
            del grads
        W.grad = b.grad = None
        shapes[f"{a.n}x{F}->{O}"] = row
        del X, W, b, up, forwards
        torch.cuda.empty_cache()

    model_cells = None
    if not a.no_model and not a.forward_only:
        u, v = rmat.rmat_relabelled_pairs(a.n, a.entries // 2, seed=1, device=device)
        idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
        del u, v
        g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], dtype=torch.float32, device=device), (a.n, a.n)), device=device)
        del idx
        torch.cuda.empty_cache()
        rng = np.random.default_rng(0)
        nodes = rng.permutation(a.n)[:a.n // 10]
        labels = sparse.DeviceIndex(rng.integers(0, 40, size=len(nodes)), device, 40, "label")
        nodes = sparse.DeviceIndex(nodes, device, a.n)
        X = torch.empty((a.n, a.features), dtype=torch.float32, device=device).uniform_(-1, 1, generator=torch.Generator(device).manual_seed(5))

        def make(how):
            gnntf.set_seed(3)
            torch.manual_seed(3)
            model = gnntf.APPNP(g, X, 40, latent_dims=[64], dense_dropout=how)
            model.reset()
            return model

        def step(model):
            model.training_mode(True)
            for var in model.vars():
                var.var.grad = None
            with model:
                gnntf.node_ce(model(model.features), nodes, labels).backward()

        models = dict(torch=make("torch"), fused=make("fused"))
        for _ in range(a.warm):
            for model in models.values():
                step(model)
        times = {name: [] for name in models}
        for _ in range(a.reps):
            for name, model in models.items():
                times[name].append(timed(lambda: step(model)))
        cell = {name: quartiles(ms) for name, ms in times.items()}
        cell["torch_over_fused"] = round(cell["torch"]["median_ms"] / max(cell["fused"]["median_ms"], 1e-9), 4)
        cell["fused_slower"] = bool(cell["fused"]["p25_ms"] > cell["torch"]["p75_ms"])
        cell["peak_mib"] = {name: peak_of(lambda: step(model)) for name, model in models.items()}
        model_cells = dict(what=f"APPNP(latent_dims=[64], num_classes=40), symmetric R-MAT ({a.n} vertices, {g.nnz} entries), {a.features} dense "
                                f"feature columns: one training step (forward, loss, backward)", train_step=cell)
    print(json.dumps(dict(what=f"dropout({p_in}) -> dense(relu) -> dropout({p_out}): torch's dropout, the counter-RNG passes and dense_step, interleaved "
                               f"in one process, {a.warm} warm-ups, {a.reps} repetitions, device events",
                          kernel_choice={k: os.environ.get(k, "") for k in ("GNX_LIBRARY", "GNX_DENSE_WREG", "GNX_DENSE_RING")},
                          shapes=shapes, model=model_cells)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
