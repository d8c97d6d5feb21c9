"""Cost of the point query against the ray query on the same points (LABBOOK round 13).

  python tools/gpu_point_query.py [--rounds 6] [--inner 10] [--grid 128] [--log profiles/r13_point_query.log]

A GRID^3 lattice over [-1, 1]^3 (default 128^3 = 2.1 M points) as GRID^2 rows of GRID points along x, one view direction per row.
The same points go through both entries in one process:
    mlp_fine          rays: o = the row's first point, d = (step, 0, 0), z = 0 .. GRID-1 (the kernel forms o + d z)
    mlp_fine_points   pts = fl(o + fl(d z)), formed beforehand: the kernel loads them
The two are ALTERNATED, `--rounds` times each (at least four), after a warm-up of both; each timing is `--inner` back-to-back calls
between two device events, divided by `--inner`.  Both series are printed in full, one JSON line per arithmetic mode (split-f16 and
f16), with the medians, the spread of mlp_fine's own runs (max - min) and the verdict of the A/B rule of LABBOOK: the point query is
accepted when its median is no slower than mlp_fine's by more than three times that spread.  The outputs of the two entries are
compared bit for bit on the way (the points are collinear by construction).  --log also appends the lines to a file.
The timed work includes the bias-table kernel and the allocation of raw, on both sides alike."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if args.rounds < 4:
        ap.error("--rounds must be at least 4: the spread of mlp_fine's own runs is the yardstick")
    if not torch.cuda.is_available():
        raise SystemExit("gpu_point_query.py measures on the GPU: no device found, nothing measured")
    from dfnet_amd import engine as eng, synthetic as syn
    DEV, n = "cuda:0", args.grid
    E = eng.NerfHEngine(precision="f16x3").load_numpy(*syn.nerfh_weights(0))
    ax = torch.linspace(-1., 1., n)
    yy, zz = torch.meshgrid(ax, ax, indexing="ij")
    o = torch.stack([torch.full_like(yy, -1.), yy, zz], -1).reshape(-1, 3).to(DEV)            # [n^2, 3]: the row's first point
    d = torch.tensor([2. / (n - 1), 0., 0.]).expand(n * n, 3).contiguous().to(DEV)
    z = torch.arange(n, dtype=torch.float32).expand(n * n, n).contiguous().to(DEV)
    g = torch.Generator().manual_seed(0)
    v = torch.randn(n * n, 3, generator=g)
    v = (v / v.norm(dim=-1, keepdim=True)).to(DEV)
    hist = torch.as_tensor(syn.HIST_IDX).float()[None].to(DEV)
    pts = (o[:, None] + d[:, None] * z[..., None]).contiguous()                                # two separately rounded fp32 operations
    lines = []
    for prec in ("f16x3", "f16"):
        ray = lambda: E.mlp_fine(o, d, v, hist, z, precision=prec)
        pnt = lambda: E.mlp_fine_points(pts, v, hist, precision=prec)
        same = bool(torch.equal(ray(), pnt()))
        for _ in range(3):
            ray(), pnt()
        torch.cuda.synchronize()

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / args.inner

        t_ray, t_pnt = [], []
        for _ in range(args.rounds):
            t_ray.append(timed(ray))
            t_pnt.append(timed(pnt))
        E.check_range()
        m_ray, m_pnt, spread = float(np.median(t_ray)), float(np.median(t_pnt)), max(t_ray) - min(t_ray)
        lines.append(dict(precision=prec, points=n ** 3, rows=n * n, same_bits=same, mlp_fine_ms=[round(t, 4) for t in t_ray],
                          mlp_fine_points_ms=[round(t, 4) for t in t_pnt], median_mlp_fine_ms=round(m_ray, 4),
                          median_mlp_fine_points_ms=round(m_pnt, 4), spread_mlp_fine_ms=round(spread, 4),
                          ns_per_point_points=round(m_pnt * 1e6 / n ** 3, 3), accepted=bool(m_pnt - m_ray <= 3 * spread)))
        print(json.dumps(lines[-1]), flush=True)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
