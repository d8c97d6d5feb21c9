#!/usr/bin/env python3
"""Times the coarse network's input-gradient kernel (NerfHEngine.mlp_coarse_points_backward, dfn_mlp_coarse_points_backward) beside the
fine network's (mlp_fine_points_backward) on the same 2 048 x 64 points, in exact fp32 and split-f16.  Device events after a warm-up, the
candidates alternating inside one process; per candidate the median over the repetitions and the run-to-run spread (min .. max).

The coarse chain runs 9 forward + 9 backward layers of the fine kernel's 16 + 15, and the fine call also writes its per-row bias table
first; a coarse time at or above the fine time would be a finding.  Nothing is gated on these numbers (LABBOOK).

Usage:  python tools/gpu_coarse_points_grad_timing.py [--rows 2048] [--N 64] [--reps 7] [--inner 10] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dfnet_amd import engine as eng, synthetic as syn  # noqa: E402

DEV = "cuda:0"


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_coarse_points_grad_timing: needs a GPU (a CPU run says nothing about these kernels)")
    cw, fw, ea, et = syn.nerfh_weights(0)
    E = eng.NerfHEngine().load_numpy(cw, fw, ea, et)
    rows, N = args.rows, args.N
    gen = torch.Generator().manual_seed(rows * 1000 + N)
    pts = (torch.rand(rows, N, 3, generator=gen) * 3 - 1.5).to(DEV)
    v = torch.randn(rows, 3, generator=gen)
    v = (v / v.norm(dim=-1, keepdim=True)).to(DEV)
    hist = torch.from_numpy(syn.HIST_IDX)[None].float().to(DEV)
    G = torch.randn(rows, N, generator=gen).to(DEV)
    graw = torch.zeros(rows, N, 9, device=DEV)
    graw[..., 3] = G
    cands = {}
    for prec in ("f32", "f16x3"):
        cands[f"coarse points gradient {prec}"] = lambda p=prec: E.mlp_coarse_points_backward(pts, G, precision=p)
        cands[f"fine points gradient {prec}"] = lambda p=prec: E.mlp_fine_points_backward(pts, v, hist, graw, precision=p)
    for fn in cands.values():      # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(args.reps):
        for k, fn in cands.items():      # alternating
            times[k].append(timed(fn, args.inner))
    out = []
    for k, t in times.items():
        med = statistics.median(t)
        out.append(dict(what=k, rows=rows, N=N, us=med * 1e6, us_min=min(t) * 1e6, us_max=max(t) * 1e6,
                        ns_per_point=med * 1e9 / (rows * N)))
        print(f"{rows} x {N}  {k:32s} {med * 1e6:9.1f} us  ({min(t) * 1e6:.1f} .. {max(t) * 1e6:.1f})  "
              f"{med * 1e9 / (rows * N):6.2f} ns per point")
    for prec in ("f32", "f16x3"):
        c = statistics.median(times[f"coarse points gradient {prec}"])
        f = statistics.median(times[f"fine points gradient {prec}"])
        print(f"{prec}: coarse / fine = {c / f:.3f}")
    if args.json:
        with open(args.json, "w") as fjson:
            json.dump(out, fjson, indent=1)


if __name__ == "__main__":
    main()
