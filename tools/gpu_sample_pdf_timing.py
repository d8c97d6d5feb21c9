#!/usr/bin/env python3
"""Times the differentiable sampler (engine.sample_pdf + engine.sample_pdf_backward, dfn_sample_pdf / dfn_sample_pdf_backward) on the GPU
against what a caller had before it: the oracle's torch expressions under torch autograd on the same device tensors.  Device events
after a warm-up, the candidates alternating inside one process; per candidate the median over the repetitions, the run-to-run spread
(min .. max) and algorithmic bytes / time against the 8 TB/s of the project's HBM tables.  Nothing is gated on these numbers (LABBOOK,
DESIGN 3.2).

Algorithmic bytes per row of nb bins and Ni samples (fp32; what the algorithm must read and write once), with explicit draws u:
  forward   bins nb + weights nb-1 + u Ni -> samples Ni                                             = 4 (2 nb - 1 + 2 Ni)
  backward  bins nb + weights nb-1 + u Ni + grad_out Ni -> grad_bins nb + grad_weights nb-1 + grad_u Ni = 4 (4 nb - 2 + 3 Ni)
With the linspace draws (u = None) the u and grad_u terms drop out.

Usage:  python tools/gpu_sample_pdf_timing.py [--rows 61440] [--nb 63] [--ni 128] [--reps 7] [--inner 20] [--json out.json]
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
    ap.add_argument("--rows", type=int, default=61440)
    ap.add_argument("--nb", type=int, default=63)
    ap.add_argument("--ni", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_sample_pdf_timing: needs a GPU (a CPU run says nothing about these kernels)")
    n, nb, Ni = args.rows, args.nb, args.ni
    gen = torch.Generator().manual_seed(nb * 1000 + Ni)
    bins = torch.sort(torch.rand(n, nb, generator=gen) * 2.5, -1)[0].to(DEV).contiguous()
    weights = (torch.rand(n, nb - 1, generator=gen) * (torch.rand(n, nb - 1, generator=gen) > .5)).to(DEV).contiguous()
    u_rand = torch.rand(n, Ni, generator=gen).to(DEV).contiguous()
    G = torch.randn(n, Ni, generator=gen).to(DEV).contiguous()
    rows = []
    for draws, u in (("u given", u_rand), ("det", None)):
        has_u = u is not None
        fwd = 4 * n * (2 * nb - 1 + (2 if has_u else 1) * Ni)
        bwd = 4 * n * (4 * nb - 2 + (3 if has_u else 1) * Ni)
        want = ("bins", "weights", "u") if has_u else ("bins", "weights")

        def torch_both():
            b, w = bins.detach().requires_grad_(True), weights.detach().requires_grad_(True)
            if has_u:
                uu = u.detach().requires_grad_(True)
                return torch.autograd.grad((orc.sample_pdf(b, w, Ni, False, uu) * G).sum(), (b, w, uu))
            uu = torch.linspace(0., 1., Ni, device=DEV).expand(n, Ni)
            return torch.autograd.grad((orc.sample_pdf(b, w, Ni, True, uu) * G).sum(), (b, w))

        cands = {
            "hip forward": (lambda: eng.sample_pdf(bins, weights, Ni, u=u), fwd),
            "hip backward": (lambda: eng.sample_pdf_backward(bins, weights, Ni, G, u=u, want=want), bwd),
            "hip forward + backward": (lambda: (eng.sample_pdf(bins, weights, Ni, u=u),
                                                eng.sample_pdf_backward(bins, weights, Ni, G, u=u, want=want)), fwd + bwd),
            "torch autograd forward + backward": (torch_both, fwd + bwd),
        }
        # the two routes compute the same thing at this size (samples on a cdf knot may take another bin: relative L2, not a bound)
        g_hip, g_t = eng.sample_pdf_backward(bins, weights, Ni, G, u=u, want=want), torch_both()
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
            rows.append(dict(draws=draws, rows=n, nb=nb, Ni=Ni, what=k, us=med * 1e6, us_min=min(t) * 1e6, us_max=max(t) * 1e6,
                             gbytes=nbytes / 1e9, tbps=nbytes / med / 1e12, of_hbm=nbytes / med / HBM, hip_vs_torch_rel_l2=agree))
            print(f"{draws:8s} {n} x {nb} / {Ni}  {k:36s} {med * 1e6:9.1f} us  ({min(t) * 1e6:.1f} .. {max(t) * 1e6:.1f})  "
                  f"{nbytes / 1e6:8.1f} MB  {nbytes / med / 1e12:5.2f} TB/s = {100 * nbytes / med / HBM:4.1f} % of 8 TB/s", flush=True)
        print(f"{draws:8s} {n} x {nb} / {Ni}  hip vs torch autograd (relative L2): " +
              ", ".join(f"d {k} {e:.1e}" for k, e in zip(want, agree)), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
