"""The K = 10 training step (forward + backward through ppr_loop, edge dropout 0.5) with the iterate in the caller's order, in the
library's gather order (ppr_loop(gather_order="relabelled"): gnx_spmm_dropped_chained_ord / gnx_spmm_dropped_back_ord) and, as a
yardstick, on a graph renumbered by descending degree (what a GNN(reorder="degree") model's loop runs) -- one process, interleaved.

Graph: R-MAT, 10 entries per vertex, at every size of --nodes (default 10^6 and the config-4 graph, 10^7 / 10^8).  Per width: `warm`
warm-up steps of each variant, then `reps` rounds of one step of each, timed with device events; per variant the median and the
quartiles of the step, and the medians of a middle forward launch and a middle backward launch.  `gains` = the relabelled step's
upper quartile is below the caller step's lower quartile: faster by more than the spread of the two medians, the rule
sparse.TRAIN_GATHER_MAX_WIDTH / TRAIN_GATHER_MIN_ROWS are set by.  "caller" is the default path, bit for bit and kernel for kernel the
step of the commit before this option existed: it is the baseline of every ratio.  Prints one table, then one JSON record.

    python tools/train_gather_bench.py [--nodes 1000000 10000000] [--widths 7 8 16 32 40 64] [--reps 20] [--warm 5]
    python tools/train_gather_bench.py --variants caller --nodes 10000000 --widths 7 64     (a library chosen with GNX_LIBRARY: the
                                                                                             regression guard against another build)
    rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -d DIR -- python tools/train_gather_bench.py --forward-only relabelled --nodes 10000000
        (a pass of its own per variant: the forward launches of one K = 10 loop at C = 8 and nothing else after the set-up)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gnn-tf_amd"))

VARIANTS = ("caller", "relabelled", "degree")


def quartiles(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]
    return dict(median_ms=round(q(0.5), 4), p25_ms=round(q(0.25), 4), p75_ms=round(q(0.75), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--degree", type=int, default=10, help="stored entries per vertex")
    ap.add_argument("--widths", type=int, nargs="+", default=[7, 8, 16, 32, 40, 64])
    ap.add_argument("--variants", nargs="+", default=list(VARIANTS), choices=VARIANTS)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--forward-only", choices=VARIANTS[:2], default=None,
                    help="run the forward launches of one loop at C = 8 for this variant and leave (for a counter pass)")
    args = ap.parse_args()
    if args.reps < 20 or args.warm < 5:
        print("note: fewer than 20 timed steps / 5 warm-ups: not a record", file=sys.stderr)

    import torch
    import gnntf
    from gnntf import sharded, sparse
    device = torch.device("cuda:0")
    K, a, p, seed = args.iterations, 0.1, 0.5, 1
    out = dict(what=f"training step, K = {K}, edge dropout {p}, forward + backward through ppr_loop; variants interleaved in one process, "
                    f"{args.warm} warm-ups, {args.reps} timed steps each, device events",
               library=sparse.nat.LIB_PATH, allowance=dict(max_width=sparse.TRAIN_GATHER_MAX_WIDTH, min_rows=sparse.TRAIN_GATHER_MIN_ROWS),
               sizes={})

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def loop_inputs(g):
        scales = sparse.dropped_degree_scales(g, p, seed, 0, K)
        adjs = [sparse.dropped_adjacency(g, p, seed, k, D=scales[k]) for k in range(K)]
        return adjs, (lambda k, bwd=False: adjs[k])

    rows = []
    for n in args.nodes:
        t0 = time.time()
        u, v = sharded.rmat_relabelled_pairs(n, n * args.degree // 2, seed=1, device=device)
        idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
        del u, v
        ones = torch.ones(idx.shape[0], device=device)
        graphs = {"caller": gnntf.DeviceGraph(gnntf.SparseCOO(idx, ones, (n, n)), device=device)}
        graphs["relabelled"] = graphs["caller"]
        if args.forward_only is not None:
            g = graphs["caller"]
            adjs, make = loop_inputs(g)
            g.reserve(8, train_gather=True)
            H0 = torch.rand(n, 8, device=device) * 2 - 1
            torch.cuda.synchronize()
            with torch.no_grad():
                gnntf.ppr_loop(make, H0, a, K, gather_order=args.forward_only)
            torch.cuda.synchronize()
            print(json.dumps(dict(forward_only=args.forward_only, nodes=n, slots=g.nnz, kernel=g.last_kernel())))
            return
        if "degree" in args.variants:       # GNN(reorder="degree"): stable order of descending entry count, the graph renumbered
            order = torch.argsort(torch.bincount(idx[:, 0], minlength=n), descending=True, stable=True)
            newid = torch.empty_like(order)
            newid[order] = torch.arange(n, device=device)
            graphs["degree"] = gnntf.DeviceGraph(gnntf.SparseCOO(newid[idx], ones, (n, n)), device=device)
            del order, newid
        del idx, ones
        torch.cuda.empty_cache()
        loops = {name: loop_inputs(graphs[name]) for name in set(args.variants) - {"relabelled"} | ({"caller"} if "relabelled" in args.variants else set())}
        if "relabelled" in args.variants:
            loops["relabelled"] = loops["caller"]
            graphs["caller"].reserve(max(args.widths), train_gather=True)
        rec = dict(slots=graphs["caller"].nnz, build_s=round(time.time() - t0, 2), widths={})
        for C in args.widths:
            gen = torch.Generator(device=device).manual_seed(C)
            H0 = (torch.rand(n, C, device=device, generator=gen) * 2 - 1).requires_grad_()
            gout = torch.rand(n, C, device=device, generator=gen)
            mode = lambda name: "relabelled" if name == "relabelled" else "caller"

            def step(name):
                H0.grad = None
                gnntf.ppr_loop(loops[name][1], H0, a, K, gather_order=mode(name)).backward(gout)

            kernels = {}
            for _ in range(args.warm):
                for name in args.variants:
                    step(name)
                    kernels[name] = graphs[name].last_kernel()
            times = {name: [] for name in args.variants}
            for _ in range(args.reps):
                for name in args.variants:
                    times[name].append(timed(lambda: step(name)))
            # per launch: a middle iteration (pre-scaled operand in, pre-scaled result out) of each loop
            launches = {}
            with torch.no_grad():
                k = min(5, K - 1)
                Hf = sparse._padded(H0.detach(), sparse.friendly_width(C, n))
                S, Y = Hf.clone(), torch.empty_like(Hf)
                fns = {}
                for name in args.variants:
                    adjs = loops[name][0]
                    nxt = adjs[(k + 1) % K].D
                    order = (sparse.nat.ORD_X | sparse.nat.ORD_OUT) if name == "relabelled" else None
                    fns[name, "forward"] = lambda adjs=adjs, nxt=nxt, order=order: sparse._launch_chained(
                        adjs[k], Hf, Hf, 1 - a, a, True, nxt, skip_empty=True, order=order)
                    fns[name, "backward"] = lambda adjs=adjs, nxt=nxt, order=order: sparse._launch_back(
                        adjs[k], Hf, True, nxt, S, 1.0, a * (1 - a), S, 1 - a, Y, skip_empty=True, order=order)
                for fn in fns.values():
                    for _ in range(3):
                        fn()
                lt = {key: [] for key in fns}
                for _ in range(args.reps):
                    for key, fn in fns.items():
                        lt[key].append(timed(fn))
                for (name, which), val in lt.items():
                    launches.setdefault(name, {})[which + "_ms"] = quartiles(val)["median_ms"]
                del Hf, S, Y
            q = {name: quartiles(times[name]) for name in args.variants}
            entry = dict(launch_width=sparse.friendly_width(C, n), steps=q, launches=launches, kernels=kernels)
            if "caller" in q and "relabelled" in q:
                entry["caller_over_relabelled"] = round(q["caller"]["median_ms"] / q["relabelled"]["median_ms"], 4)
                entry["gains"] = bool(q["relabelled"]["p75_ms"] < q["caller"]["p25_ms"])
            rec["widths"][f"C{C}"] = entry
            for name in args.variants:
                rows.append((n, C, entry["launch_width"], name, q[name]["median_ms"], q[name]["p25_ms"], q[name]["p75_ms"],
                             launches[name]["forward_ms"], launches[name]["backward_ms"],
                             entry.get("caller_over_relabelled") if name == "relabelled" else None,
                             entry.get("gains") if name == "relabelled" else None))
            del H0, gout
            torch.cuda.empty_cache()
        out["sizes"][str(n)] = rec
        del graphs, loops
        torch.cuda.empty_cache()

    print("| vertices | C | launched as | variant | step median ms | p25 | p75 | forward launch ms | backward launch ms | caller / relabelled | gains |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for n, C, Cw, name, med, p25, p75, fwd, bwd, ratio, gains in rows:
        print(f"| {n} | {C} | {Cw} | {name} | {med:.3f} | {p25:.3f} | {p75:.3f} | {fwd:.3f} | {bwd:.3f} | "
              f"{'' if ratio is None else f'{ratio:.3f}'} | {'' if gains is None else ('yes' if gains else 'no')} |")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
