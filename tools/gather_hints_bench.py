#!/usr/bin/env python3
"""Interleaved A/B of the gather hints in ONE process: gnx_appnp_propagate, K iterations, on one R-MAT graph at several widths, with
hints off (the kernels as they were) and with each hot-row count of --hot-rows, the variants alternating inside every round.

    python tools/gather_hints_bench.py --nodes 80000000 --entries 1000000000 --feats 128
    python tools/gather_hints_bench.py --nodes 10000000 --entries 100000000 --feats 256,128,64

Prints one JSON line per (width, variant): median / min / max ms per propagation over the rounds, and per width the spread of the
unhinted runs (`off` is timed twice per round: the distance of those two medians, and their per-round spread, is what a difference
between variants has to beat).  Every hinted result is compared with the unhinted one bit for bit.  With --share, also the share of
all gathers that goes to the n rows with the most entries (one cumulative degree sum on the device)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnn-tf_amd")]
import torch

import bench_device
import gnntf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--feats", type=str, default="128")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--hot-rows", type=str, default="4096,8192,16384,131072,262144,524288", help="-1 = the automatic rule (write --hot-rows=-1,...)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--share", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gnntf.set_default_device(dev)
    g, adj, prep = bench_device.build_single(a, dev)
    n = g.n_rows
    print(json.dumps({"graph": {"rows": n, "entries": g.nnz, **prep}}), flush=True)
    sets = [int(v) for v in a.hot_rows.split(",")]
    if a.share:
        rowptr = g.csr_arrays()[0]
        degree = (rowptr[1:] - rowptr[:-1]).sort(descending=True).values
        del rowptr
        cum = degree.cumsum(0)
        share = {h: float(cum[min(h, n) - 1]) / g.nnz for h in sorted(set(abs(h) for h in sets) | {2048, 4096, 8192, 16384})}
        print(json.dumps({"gather_share_of_top_rows": share}), flush=True)
        del degree, cum
        torch.cuda.empty_cache()
    variants = [("off", 0)] + [("hot%d" % h if h > 0 else "auto", h) for h in sets] + [("off_again", 0)]
    for C in (int(c) for c in a.feats.split(",")):
        gen = torch.Generator(device=dev).manual_seed(2)
        H0 = torch.rand(n, C, device=dev, generator=gen) * 2 - 1
        times, names, ref = {v: [] for v, _ in variants}, {}, None
        for r in range(a.rounds + 1):                     # round 0 warms up, builds the hints and checks the bits
            for v, hot in variants:
                g.set_gather_hints(hot)
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                out = gnntf.appnp_propagate(adj, H0, a=0.1, iterations=a.iterations)
                e.record()
                torch.cuda.synchronize()
                if r == 0:
                    names[v] = g.last_kernel() + " hot_rows=%d" % g.last_launch_hot_rows()
                    if ref is None:
                        ref = out
                    else:
                        assert torch.equal(ref, out), f"{v} changes the result at C = {C}"
                else:
                    times[v].append(s.elapsed_time(e))
                del out
        g.set_gather_hints(0)
        med = {v: sorted(t)[len(t) // 2] for v, t in times.items()}
        base = 0.5 * (med["off"] + med["off_again"])
        spread = max(abs(med["off"] - med["off_again"]), max(times["off"]) - min(times["off"]), max(times["off_again"]) - min(times["off_again"]))
        print(json.dumps({"C": C, "K": a.iterations, "off_median_ms": round(base, 3), "spread_ms": round(spread, 3)}), flush=True)
        for v, _ in variants:
            t = times[v]
            print(json.dumps({"C": C, "variant": v, "kernel": names[v], "median_ms": round(med[v], 3), "min_ms": round(min(t), 3),
                              "max_ms": round(max(t), 3), "vs_off_pct": round(100.0 * (med[v] / base - 1.0), 2),
                              "gain_over_spread": round((base - med[v]) / spread, 1) if spread > 0 else None}), flush=True)
        del H0, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
