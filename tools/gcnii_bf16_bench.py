#!/usr/bin/env python3
"""The fused GCNII layer with f32 and with bf16 feature storage (sparse.gcnii_step(storage=) / sparse.gcnii_chain_bf16 over
gnx_gcnii_step_bf16) on the config-4 graph (symmetric R-MAT, 10M vertices / 100M entries), one GPU, eval mode:

  * ONE layer launch: f32 rows in, f32 rows out against bf16 rows in, bf16 rows out (what an inner layer of a stack does), into buffers
    that exist already;
  * a stack of `--layers` (64) layers as the model runs it: the f32 gcnii_step chain against the bf16 chain (input cast once, bf16
    between the layers, f32 out of the last; its three work buffers allocated inside, as the model does).

    python tools/gcnii_bf16_bench.py [--widths 16,32,64,128] [--layers 64] [--reps 20] [--warm 3]

f32 and bf16 are interleaved in one process: per width `warm` warm-ups of each, then `reps` rounds of one f32 and one bf16 call, each
between device events.  Reported: median and quartiles in ms, the ratio of the medians, and `bf16_slower` = the bf16 lower quartile is
above the f32 upper quartile.  The yardstick is the f32 call of the same process.  Prints one JSON record."""
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
    import torch
    import gnntf
    from gnntf import rmat, sparse
    nat = sparse.nat
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--entries", type=int, default=100_000_000)
    ap.add_argument("--widths", default="16,32,64,128")
    ap.add_argument("--layers", type=int, default=64)
    ap.add_argument("--a", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gcnii_bf16_bench: needs a GPU")
    if a.reps < 20 or a.warm < 3:
        print("note: fewer than 20 repetitions / 3 warm-ups: not a record", file=sys.stderr)
    device = torch.device("cuda:0")
    gnntf.set_default_device(device)
    u, v = rmat.rmat_relabelled_pairs(a.n, a.entries // 2, seed=1, device=device)
    idx = torch.cat([torch.stack([u, v], 1), torch.stack([v, u], 1)])
    del u, v
    g = gnntf.DeviceGraph(gnntf.SparseCOO(idx, torch.ones(idx.shape[0], dtype=torch.float32, device=device), (a.n, a.n)), device=device)
    del idx
    adj = gnntf.normalize(g, "symmetric")
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def compare(f32, bf16):
        for _ in range(a.warm):
            f32(), bf16()
        t32, t16 = [], []
        for _ in range(a.reps):
            t32.append(timed(f32))
            t16.append(timed(bf16))
        q32, q16 = quartiles(t32), quartiles(t16)
        return dict(f32=q32, bf16=q16, f32_over_bf16=round(q32["median_ms"] / max(q16["median_ms"], 1e-9), 4),
                    bf16_slower=bool(q16["p25_ms"] > q32["p75_ms"]))

    rows = dict()
    with torch.no_grad():
        for C in [int(c) for c in a.widths.split(",")]:
            gen = torch.Generator(device).manual_seed(C)
            H = torch.empty((a.n, C), dtype=torch.float32, device=device).uniform_(-1, 1, generator=gen)
            H0 = torch.empty((a.n, C), dtype=torch.float32, device=device).uniform_(-1, 1, generator=gen)
            W = torch.empty((C, C), dtype=torch.float32, device=device).uniform_(-1, 1, generator=gen) / math.sqrt(C)
            Ms = [(1 - b) * torch.eye(C, device=device) + b * W for b in (math.log1p(0.5 / (k + 1)) for k in range(a.layers))]
            Hb = sparse.to_bf16(H)
            out32, mixed = torch.empty_like(H), (None if C in (16, 32, 64) else torch.empty_like(H))
            out16, work = torch.empty_like(Hb), torch.empty_like(H)

            def layer_f32():
                nat.check(nat.lib().gnx_gcnii_step(g.handle, nat.ptr(adj.vals), nat.ptr(H), nat.ptr(H0), a.a, C, nat.ptr(Ms[0]), C,
                                                   nat.ACT_RELU, nat.ptr(out32), nat.ptr(mixed), nat.current_stream()))

            def layer_bf16():
                sparse._gcnii_launch_bf16(adj, Hb, H0, a.a, Ms[0], True, True, out=out16, work=work)

            rec = dict(layer=compare(layer_f32, layer_bf16))
            rec["kernels"] = dict(f32=(layer_f32(), g.last_kernel())[1], bf16=(layer_bf16(), g.last_kernel())[1])
            del out32, mixed, out16, work, Hb

            def stack_f32():
                X = H
                for M in Ms:
                    X = sparse.gcnii_step(adj, X, H0, a.a, M, relu=True)
                return X

            def stack_bf16():
                return sparse.gcnii_chain_bf16(adj, H, [(H0, a.a, M, True) for M in Ms])

            rec["stack"] = compare(stack_f32, stack_bf16)
            x32, x16 = stack_f32(), stack_bf16()
            rec["stack_rel_frobenius"] = float(torch.linalg.norm(x16 - x32) / torch.linalg.norm(x32))
            rows[str(C)] = rec
            del H, H0, x32, x16
            torch.cuda.empty_cache()
    print(json.dumps(dict(what=f"GCNII layer, symmetric R-MAT ({a.n} vertices, {g.nnz} entries), eval mode, relu; one launch and a stack of "
                               f"{a.layers} layers; f32 and bf16 storage interleaved in one process, {a.warm} warm-ups, {a.reps} repetitions, "
                               "device events", widths=rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
