#!/usr/bin/env python3
"""Times the public compositor (engine.raw2outputs / raw2outputs_backward, dfn_raw2outputs*) on the GPU against the two things a caller
had before it: the oracle's torch expressions under torch autograd on the same device tensors, and - for d L/d raw alone in the
9-channel mode - composite_fine_backward_maps.  Device events after a warm-up, the candidates alternating inside one process; per
candidate the median over the repetitions, the run-to-run spread (min .. max) and algorithmic bytes / time against the 8 TB/s of the
project's HBM tables.  Nothing is gated on these numbers (LABBOOK).

Algorithmic bytes per ray of N samples (fp32; what the algorithm must read and write once, upstream gradients on every output):
  9 channels  forward  raw 9N + z N -> weights N + rgb 3, disp, acc, depth, beta              = 4 (11N + 7)
              backward raw 9N + z N + g_weights N + 7 -> grad_raw 9N + grad_z N               = 4 (21N + 7)
              backward, grad_raw alone, no g_weights (what composite_fine_backward_maps does) = 4 (19N + 7)
  4 channels  forward  raw 4N + z N -> weights N + rgb 3, disp, acc, depth                    = 4 (6N + 6)
              backward raw 4N + z N + g_weights N + 6 -> grad_raw 4N + grad_z N               = 4 (11N + 6)

Usage:  python tools/gpu_raw2outputs_timing.py [--reps 7] [--inner 20] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dfnet_amd import engine as eng  # noqa: E402
from oracle import nerfh_oracle as orc  # noqa: E402

DEV = "cuda:0"
HBM = 8e12
CASES = [("M3", 9, 32768, 192), ("M3", 9, 1536, 192), ("M2", 4, 32768, 64)]


def bytes_of(ch, n, N):
    if ch == 9:
        return dict(fwd=4 * n * (11 * N + 7), bwd=4 * n * (21 * N + 7), bwd_raw=4 * n * (19 * N + 7))
    return dict(fwd=4 * n * (6 * N + 6), bwd=4 * n * (11 * N + 6))


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_raw2outputs_timing: needs a GPU (a CPU run says nothing about these kernels)")
    rows = []
    for mode, ch, n, N in CASES:
        gen = torch.Generator().manual_seed(ch * 1000 + N)
        raw = torch.rand(n, N, ch, generator=gen) * 0.98 + 0.01
        for c in ((3, 7) if ch == 9 else (3,)):
            raw[..., c] = torch.nn.functional.softplus(torch.randn(n, N, generator=gen))
        z = torch.sort(torch.rand(n, N, generator=gen) * 2.5, -1)[0]
        raw, z = raw.to(DEV).contiguous(), z.to(DEV).contiguous()
        names = ("rgb", "disp", "acc", "weights", "depth") + (("beta",) if ch == 9 else ())
        G = {k: torch.randn((n, 3) if k == "rgb" else (n, N) if k == "weights" else (n,), device=DEV) for k in names}
        G_raw = {k: v for k, v in G.items() if k != "weights"}
        opts = dict(test_time=ch == 9, static_only=True)
        B = bytes_of(ch, n, N)

        def torch_both():
            r, zz = raw.detach().requires_grad_(True), z.detach().requires_grad_(True)
            out = orc.composite_fine(r, zz) if ch == 9 else orc.composite_coarse_train(r, zz)
            return torch.autograd.grad(sum((out[k] * G[k]).sum() for k in G), (r, zz))

        cands = {
            "hip forward": (lambda: eng.raw2outputs(raw, z, **opts), B["fwd"]),
            "hip backward (raw, z)": (lambda: eng.raw2outputs_backward(raw, z, G, **opts), B["bwd"]),
            "hip forward + backward": (lambda: (eng.raw2outputs(raw, z, **opts), eng.raw2outputs_backward(raw, z, G, **opts)),
                                       B["fwd"] + B["bwd"]),
            "torch autograd forward + backward": (torch_both, B["fwd"] + B["bwd"]),
        }
        if ch == 9:
            Gm = {("depth_static" if k == "depth" else k): v for k, v in G_raw.items()}
            cands["hip backward (raw alone)"] = (lambda: eng.raw2outputs_backward(raw, z, G_raw, want=("raw",), **opts), B["bwd_raw"])
            cands["composite_fine_backward_maps"] = (lambda: eng.composite_fine_backward_maps(raw, z, Gm), B["bwd_raw"])
        # the two routes compute the same thing at this size
        g_hip, g_t = eng.raw2outputs_backward(raw, z, G, **opts), torch_both()
        agree = [float((a - b).norm() / b.norm()) for a, b in zip(g_hip, g_t)]
        for fn, _ in cands.values():      # warm-up: code objects, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cands}
        for _ in range(args.reps):
            for k, (fn, _) in cands.items():      # alternating
                times[k].append(timed(fn, args.inner))
        for k, (_, nbytes) in cands.items():
            t = times[k]
            med = statistics.median(t)
            rows.append(dict(mode=mode, rays=n, samples=N, what=k, us=med * 1e6, us_min=min(t) * 1e6, us_max=max(t) * 1e6,
                             gbytes=nbytes / 1e9, tbps=nbytes / med / 1e12, of_hbm=nbytes / med / HBM,
                             hip_vs_torch_rel_l2=agree))
            print(f"{mode} {n} x {N}  {k:36s} {med * 1e6:9.1f} us  ({min(t) * 1e6:.1f} .. {max(t) * 1e6:.1f})  "
                  f"{nbytes / 1e6:8.1f} MB  {nbytes / med / 1e12:5.2f} TB/s = {100 * nbytes / med / HBM:4.1f} % of 8 TB/s")
        print(f"{mode} {n} x {N}  hip vs torch autograd: d raw {agree[0]:.1e}, d z {agree[1]:.1e} (relative L2)")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
