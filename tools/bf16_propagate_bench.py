"""f32 against bf16 feature storage for the eval-mode K loop (appnp_propagate) on the R-MAT bench graph, in one process.

Per width C: H0 uniform in [-1, 1]; the f32 loop (sparse.appnp_propagate, today's path: line-friendly padding, the relabelled copy at
narrow widths) and the bf16 loop (the gnx_appnp_propagate_bf16 kernels at every width, bf16 line-friendly padding) are timed
ALTERNATELY with device events after a warm-up; medians of --reps calls each.  Prints one JSON line: ms per iteration, speed-up,
the algorithmic bytes per iteration of both (gathered rows + (col, val) per entry; H0 read, result written and row pointer per row),
and the K-loop's relative Frobenius error of bf16 against f32.

    python tools/bf16_propagate_bench.py [--n 10000000 --entries 100000000 --K 10 --widths 7,8,16,40,64,128,256 --reps 10]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnn-tf_amd"))

import torch  # noqa: E402

import gnntf  # noqa: E402
from gnntf import rmat, sparse  # noqa: E402


def byte_model(n, nnz, C, elem):
    """Algorithmic bytes of one iteration: per entry one gathered row (elem * C) + int32 column + f32 value; per row the f32 H0 row,
    the written row (bf16 between iterations, f32 in the f32 loop) and the int64 row pointer."""
    return nnz * (elem * C + 8) + n * (4 * C + elem * C + 8)


def timed(fn, reps_done):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    end.synchronize()
    reps_done.append(start.elapsed_time(end))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--a", type=float, default=0.1)
    ap.add_argument("--widths", default="7,8,16,40,64,128,256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bf16_propagate_bench: needs a GPU")
    device = torch.device("cuda:0")
    gnntf.set_default_device(device)
    u, v = rmat.rmat_relabelled_pairs(args.n, args.entries // 2, seed=1, device=device)
    idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
    del u, v
    g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], dtype=torch.float32, device=device), (args.n, args.n)),
                          device=device)
    del idx
    adj = gnntf.normalize(g, "symmetric")
    torch.cuda.synchronize()
    rows = dict()
    for C in [int(c) for c in args.widths.split(",")]:
        H0 = torch.empty((args.n, C), dtype=torch.float32, device=device).uniform_(-1, 1, generator=torch.Generator(device).manual_seed(C))
        f32 = lambda: sparse.appnp_propagate(adj, H0, args.a, args.K)
        bf16 = lambda: sparse._appnp_propagate_bf16(adj, H0, args.a, args.K, False)
        for _ in range(args.warmup):
            f32(), bf16()
        names = dict()
        t32, t16 = [], []
        for _ in range(args.reps):
            ref = timed(f32, t32)
            names["f32"] = g.last_kernel()
            got = timed(bf16, t16)
            names["bf16"] = g.last_kernel()
        err = float((got.double() - ref.double()).norm() / ref.double().norm())
        ms32, ms16 = statistics.median(t32) / args.K, statistics.median(t16) / args.K
        C32, C16 = sparse.friendly_width(C, args.n), sparse.friendly_width_bf16(C, args.n)
        b32, b16 = byte_model(args.n, g.nnz, C32, 4), byte_model(args.n, g.nnz, C16, 2)
        rows[C] = dict(f32_ms_per_iter=round(ms32, 4), bf16_ms_per_iter=round(ms16, 4), speedup=round(ms32 / ms16, 3),
                       f32_width=C32, bf16_width=C16, f32_GB_per_iter=round(b32 / 1e9, 2), bf16_GB_per_iter=round(b16 / 1e9, 2),
                       byte_ratio=round(b32 / b16, 3), f32_TBps=round(b32 / ms32 / 1e9, 2), bf16_TBps=round(b16 / ms16 / 1e9, 2),
                       rel_fro_err=float(f"{err:.3e}"), kernels=names,
                       f32_spread_ms=[round(min(t32) / args.K, 4), round(max(t32) / args.K, 4)],
                       bf16_spread_ms=[round(min(t16) / args.K, 4), round(max(t16) / args.K, 4)])
        del H0, ref, got
        torch.cuda.empty_cache()
        print(json.dumps({"C": C, **rows[C]}), file=sys.stderr, flush=True)
    print(json.dumps(dict(bench="bf16_propagate", n=args.n, nnz=g.nnz, K=args.K, a=args.a, reps=args.reps, widths=rows)))


if __name__ == "__main__":
    main()
