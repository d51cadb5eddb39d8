"""The K = 10 training step (forward + backward through ppr_loop, edge dropout 0.5) with f32 and with bf16 feature storage
(ppr_loop(storage=torch.bfloat16): gnx_spmm_dropped_chained_bf16 / gnx_spmm_dropped_back_bf16), same process, interleaved.

Graph: the config-4 R-MAT graph (WORKLOADS["config4"]: 10M vertices, 100M entries); with --doubled also the same graph with every
entry stored twice (enable_entry_dropout) at the widths of --doubled-widths.  Per width: `warm` warm-up steps of each storage, then
`reps` rounds of one f32 step and one bf16 step, each timed with device events; reported: median, quartiles, the ratio of the medians
and `pays` = the bf16 step's upper quartile is below the f32 step's lower quartile (faster by more than the run-to-run spread of the
two medians: the rule sparse.BF16_TRAIN_MIN_WIDTH is set by).  Also per-launch times (a middle forward iteration and a middle backward
call of each storage, device events).  The allowance is switched off for the run (BF16_TRAIN_MIN_WIDTH = 1, BF16_TRAIN_MIN_ROWS = 0) so that every
width and every graph size (--nodes / --entries) is measured.  Prints one JSON record.

    python tools/bf16_train_bench.py [--widths 7 8 16 40 64 128] [--doubled] [--reps 20] [--warm 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gnn-tf_amd"))

from bench_record import WORKLOADS            # noqa: E402


def quartiles(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]
    return dict(median_ms=round(q(0.5), 4), p25_ms=round(q(0.25), 4), p75_ms=round(q(0.75), 4))


def main():
    ap = argparse.ArgumentParser()
    n4, e4, _ = WORKLOADS["config4"]
    ap.add_argument("--nodes", type=int, default=n4)
    ap.add_argument("--entries", type=int, default=e4)
    ap.add_argument("--widths", type=int, nargs="+", default=[7, 8, 16, 40, 64, 128])
    ap.add_argument("--doubled", action="store_true", help="also the graph with every entry stored twice")
    ap.add_argument("--doubled-widths", type=int, nargs="+", default=[7, 64])
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 20 or args.warm < 5:
        print("note: fewer than 20 timed steps / 5 warm-ups: not a record", file=sys.stderr)

    import torch
    import gnntf
    from gnntf import sharded, sparse
    shipped = sparse.BF16_TRAIN_MIN_WIDTH
    sparse.BF16_TRAIN_MIN_WIDTH, sparse.BF16_TRAIN_MIN_ROWS = 1, 0     # measure every width and size
    device = torch.device("cuda:0")
    K, a, p, seed = args.iterations, 0.1, 0.5, 1
    n = args.nodes
    t0 = time.time()
    u, v = sharded.rmat_relabelled_pairs(n, args.entries // 2, seed=1, device=device)
    idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
    del u, v
    out = dict(what=f"training step, K = {K}, edge dropout {p}, forward + backward through ppr_loop; f32 and bf16 storage interleaved "
                    f"in one process, {args.warm} warm-ups, {args.reps} timed steps each, device events",
               nodes=n, graphs={}, min_width_shipped=shipped)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(name, g):
        rec = dict(slots=g.nnz, entries=g.nnz_entries, steps={}, launches={}, kernels={})
        scales = sparse.dropped_degree_scales(g, p, seed, 0, K)
        adjs = [sparse.dropped_adjacency(g, p, seed, k, D=scales[k]) for k in range(K)]
        make = lambda k, bwd=False: adjs[k]
        for C in (args.widths if name == "config4" else args.doubled_widths):
            gen = torch.Generator(device=device).manual_seed(C)
            H0 = (torch.rand(n, C, device=device, generator=gen) * 2 - 1).requires_grad_()
            gout = torch.rand(n, C, device=device, generator=gen)

            def step(storage):
                H0.grad = None
                gnntf.ppr_loop(make, H0, a, K, storage=storage).backward(gout)

            for _ in range(args.warm):
                step(torch.float32)
                step(torch.bfloat16)
            rec["kernels"][f"C{C}"] = g.last_kernel()
            t32, t16 = [], []
            for _ in range(args.reps):
                t32.append(timed(lambda: step(torch.float32)))
                t16.append(timed(lambda: step(torch.bfloat16)))
            q32, q16 = quartiles(t32), quartiles(t16)
            rec["steps"][f"C{C}"] = dict(f32=q32, bf16=q16, f32_over_bf16=round(q32["median_ms"] / q16["median_ms"], 4),
                                         pays=bool(q16["p75_ms"] < q32["p25_ms"]))
            # per launch: a middle iteration (k = 5: pre-scaled operand, pre-scaled result) of each loop
            with torch.no_grad():
                k = min(5, K - 1)
                Hd = H0.detach()
                Cf, Cb = sparse.friendly_width(C, n), sparse.friendly_width_bf16(C, n)
                Hf, Hb = sparse._padded(Hd, Cf), sparse._padded(Hd, Cb)
                Xb = sparse.to_bf16(Hb)
                Sf, Sb = Hf.clone(), Hb.clone()
                Yf, Yb = torch.empty_like(Hf), torch.empty_like(Xb)
                nxt = adjs[(k + 1) % K].D
                launches = {
                    "forward_f32": lambda: sparse._launch_chained(adjs[k], Hf, Hf, 1 - a, a, True, nxt, skip_empty=True),
                    "forward_bf16": lambda: sparse._launch_chained_bf16(adjs[k], Xb, Hb, 1 - a, a, True, nxt, skip_empty=True, out_bf16=True),
                    "backward_f32": lambda: sparse._launch_back(adjs[k], Hf, True, nxt, Sf, 1.0, a * (1 - a), Sf, 1 - a, Yf, skip_empty=True),
                    "backward_bf16": lambda: sparse._launch_back_bf16(adjs[k], Xb, True, nxt, Sb, 1.0, a * (1 - a), Sb, 1 - a, Yb,
                                                                      skip_empty=True),
                }
                for fn in launches.values():
                    for _ in range(3):
                        fn()
                times = {key: [] for key in launches}
                for _ in range(args.reps):
                    for key, fn in launches.items():
                        times[key].append(timed(fn))
                rec["launches"][f"C{C}"] = {key: quartiles(val)["median_ms"] for key, val in times.items()}
                del Hf, Hb, Xb, Sf, Sb, Yf, Yb
            del H0, gout
            torch.cuda.empty_cache()
        return rec

    g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], device=device), (n, n)), device=device)
    out["build_s"] = round(time.time() - t0, 2)
    out["graphs"]["config4"] = measure("config4", g)
    if args.doubled:
        del g
        torch.cuda.empty_cache()
        idx2 = torch.cat([idx, idx])
        g2 = gnntf.DeviceGraph(gnntf.SparseCOO(idx2, torch.ones(idx2.shape[0], device=device), (n, n)), device=device)
        del idx2
        g2.enable_entry_dropout()
        out["graphs"]["doubled"] = measure("doubled", g2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
