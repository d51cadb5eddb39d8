"""A training step with edge dropout on a graph whose COO stores every entry twice (what graph2adj makes of a graph that already
holds both directions), with and without the fused entry dropout (DeviceGraph.enable_entry_dropout).

Graph: the config-4 R-MAT graph (WORKLOADS["config4"]: 10M vertices, 100M entries), then every entry stored twice (200M entries,
100M slots).  Step: K = 10 PPR iterations with per-iteration edge dropout 0.5 + renormalisation, forward + backward through ppr_loop
with dropped_degree_scales, as bench_secondary.training_step times it.  Variants:
  a  the graph without duplicates, fused (the reference point)
  b  the doubled graph, not enabled: every iteration materialises its values (gnx_graph_normalize), forward and backward
  c  the doubled graph, enabled: the weights are made inside the SpMM from the entry tables
Prints one JSON record.  Bitwise checks at the timed size: the timed step's output and dH0 of b and c at every width, the K
degree-scale vectors of b and c, one forward and one transposed fused launch of c against normalize + spmm on the same handle, and
a K-iteration relu loop (forward + dH0) of b and c.

    python tools/entry_dropout_bench.py [--widths 7 64] [--variants a b c] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gnn-tf_amd"))

from bench_device import median_ms            # noqa: E402
from bench_record import WORKLOADS            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    n4, e4, _ = WORKLOADS["config4"]
    ap.add_argument("--nodes", type=int, default=n4)
    ap.add_argument("--entries", type=int, default=e4, help="entries of the graph WITHOUT duplicates (stored twice in b and c)")
    ap.add_argument("--widths", type=int, nargs="+", default=[7, 64])
    ap.add_argument("--variants", nargs="+", default=["a", "b", "c"])
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-check", action="store_true", help="skip the bitwise checks (profiling runs)")
    args = ap.parse_args()

    import torch
    import gnntf
    from gnntf import sharded, sparse
    device = torch.device("cuda:0")
    K, a, p, seed = args.iterations, 0.1, 0.5, 1
    n = args.nodes
    t0 = time.time()
    u, v = sharded.rmat_relabelled_pairs(n, args.entries // 2, seed=1, device=device)
    idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
    del u, v
    graphs = {}
    if "a" in args.variants:
        graphs["a"] = gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], device=device), (n, n)), device=device)
    if "b" in args.variants or "c" in args.variants:
        idx2 = torch.cat([idx, idx])
        for name in ("b", "c"):
            if name in args.variants:
                graphs[name] = gnntf.DeviceGraph(gnntf.SparseCOO(idx2, torch.ones(idx2.shape[0], device=device), (n, n)), device=device)
        del idx2
    del idx
    torch.cuda.empty_cache()
    t1 = time.time()
    if "c" in graphs:
        graphs["c"].enable_entry_dropout()
    torch.cuda.synchronize()
    t_enable = time.time() - t1
    for name, g in graphs.items():
        assert sparse.can_fuse_dropout(g, p) == (name != "b"), name
    out = dict(what=f"training step, K = {K} iterations, edge dropout {p}, forward + backward (ppr_loop with dropped_degree_scales); "
                    "a: config-4 R-MAT graph, fused; b: every entry stored twice, materialised per iteration; c: the same, "
                    "enable_entry_dropout (fused)",
               nodes=n, slots={k: g.nnz for k, g in graphs.items()}, entries={k: g.nnz_entries for k, g in graphs.items()},
               build_s=round(t1 - t0, 2), enable_entry_dropout_s=round(t_enable, 3), steps={}, degree_scales_ms={}, kernels={})

    def make_for(name, g, first=0):
        if name == "b":                         # what _propagation_run does on a large graph it cannot fuse
            return lambda k, bwd=False: sparse.normalize(g, "symmetric", "none", p, seed, first + k, transposed_only=bwd)
        scales = sparse.dropped_degree_scales(g, p, seed, first, K)
        return lambda k, bwd=False: sparse.dropped_adjacency(g, p, seed, first + k, D=scales[k])

    for name, g in graphs.items():
        out["degree_scales_ms"][name] = median_ms(lambda: sparse.dropped_degree_scales(g, p, seed, 0, K), reps=args.reps, warm=1)
    for C in args.widths:
        gen = torch.Generator(device=device).manual_seed(C)
        H0 = (torch.rand(n, C, device=device, generator=gen) * 2 - 1).requires_grad_()
        gout = torch.rand(n, C, device=device, generator=gen)
        results = {}
        for name, g in graphs.items():
            def step():
                H0.grad = None
                res = gnntf.ppr_loop(make_for(name, g), H0, a, K)
                res.backward(gout)
                return res
            out["steps"][f"{name}_C{C}_ms"] = median_ms(step, reps=args.reps, warm=1)
            out["kernels"][f"{name}_C{C}"] = g.last_kernel()
            if not args.no_check and name in ("b", "c"):
                res = step()
                results[name] = (res.detach().clone(), H0.grad.clone())
                del res
            torch.cuda.empty_cache()
        if "a" in graphs and "c" in graphs:
            out["steps"][f"c_over_a_C{C}"] = out["steps"][f"c_C{C}_ms"] / out["steps"][f"a_C{C}_ms"]
        if "b" in graphs and "c" in graphs:
            out["steps"][f"c_over_b_C{C}"] = out["steps"][f"c_C{C}_ms"] / out["steps"][f"b_C{C}_ms"]
        if len(results) == 2:
            (ob, gb), (oc, gc) = results["b"], results["c"]
            out.setdefault("bitwise_b_vs_c", {})[f"step_C{C}_forward_and_dH0"] = bool(torch.equal(oc, ob) and torch.equal(gc, gb))
        del H0, gout, results
        torch.cuda.empty_cache()

    if not args.no_check and "b" in graphs and "c" in graphs:
        gb, gc = graphs["b"], graphs["c"]
        checks = {}
        Db, Dc = sparse.dropped_degree_scales(gb, p, seed, 0, K), sparse.dropped_degree_scales(gc, p, seed, 0, K)
        checks["degree_scales_bitwise"] = bool(torch.equal(Db, Dc))
        C = min(args.widths)
        gen = torch.Generator(device=device).manual_seed(1)
        X, H0 = torch.rand(n, C, device=device, generator=gen), torch.rand(n, C, device=device, generator=gen)
        fused = sparse.dropped_adjacency(gc, p, seed, 3, D=Dc[3])
        two_pass = sparse.normalize(gc, "symmetric", "none", p, seed, 3)
        for transposed in (False, True):
            x = sparse._launch(fused, X, H0, 1 - a, a, 0, transposed=transposed)
            y = sparse._launch(two_pass, X, H0, 1 - a, a, 0, transposed=transposed)
            checks[f"launch_{'transposed' if transposed else 'forward'}_bitwise"] = bool(torch.equal(x, y))
        del X, fused, two_pass, x, y
        torch.cuda.empty_cache()
        H0 = (torch.rand(n, C, device=device, generator=gen) * 2 - 1)
        gout = torch.rand(n, C, device=device, generator=gen)
        relu = []
        for name, g in (("b", gb), ("c", gc)):
            Hr = H0.clone().requires_grad_()
            res = gnntf.ppr_loop(make_for(name, g), Hr, a, K, relu=True)
            res.backward(gout)
            relu.append((res.detach(), Hr.grad))
            del res, Hr
        checks[f"relu_loop_C{C}_forward_bitwise"] = bool(torch.equal(relu[0][0], relu[1][0]))
        checks[f"relu_loop_C{C}_dH0_bitwise"] = bool(torch.equal(relu[0][1], relu[1][1]))
        out.setdefault("bitwise_b_vs_c", {}).update(checks)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
