"""Cost of the mesh export on the trained fixture (tests/golden/trained_nerfh_weights.npz): the density grid and the iso-surface.

  python tools/gpu_mesh_timing.py [--sizes 256 512] [--rounds 5] [--inner 5] [--log profiles/mesh_timing.log]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_mesh_timing.py --sizes 256 --trace-only     (kernel times: a run of its own)

Per grid size N (N^3 nodes over [-0.7, 0.7]^3), after a warm-up of every shape, one JSON line with
  grid_query       mesh.density_grid (dfn_grid_points + the fine point query + the copy of channel 3, slab by slab): seconds per grid
                   and points/s, beside `point_query`: the same kernels (NerfHEngine.mlp_fine_points, split-f16) on ONE slab's points
                   formed beforehand, in the same process on the same box.  tools/gpu_point_query.py measures that entry on a 128^3
                   lattice; run it in the same job for its figure.
  count / emit     dfn_isosurface_count (count_kernel + scan_sums_kernel) and dfn_isosurface_emit at the 0.9 quantile of the grid,
                   each `--inner` back-to-back calls between two device events, `--rounds` times: median and spread.
  bytes            what each MUST move, from the shapes: count reads 4 B of sigma and writes 9 B (two prefixes and the crossing
                   bits) per node plus 8 B per scan block; the block-sum scan reads and writes 8 B per scan block; emit reads 1 B per
                   node (the bits) and writes 12 B per vertex and per triangle.  bytes / time is given as a share of HBM bandwidth,
                   against both the nominal 8 TB/s and the 6.29 TB/s a float4 copy achieves on an MI355X.  The event times include
                   the launch gaps of the two count kernels; the per-kernel times come from the kernel trace.
A size whose buffers do not fit is reported as skipped.  --trace-only runs the warm-up and `--inner` calls of each entry and prints
nothing else: for use under the profiler."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_NOMINAL, HBM_ACHIEVABLE = 8.0e12, 6.29e12   # bytes/s: the specification; a float4 copy measured on an MI355X
# isosurface.hip's kScan, repeated by hand (the comment beside kScan names this file).  Only the block-sum terms of the byte model use
# it: 24 B per 256 nodes beside 13 B per node, so a stale value moves the reported shares by under 1 %
SCAN_BLOCK = 256


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def series(fn, rounds, inner):
    t = [timed(fn, inner) for _ in range(rounds)]
    return float(np.median(t)), float(max(t) - min(t))


def measure(n, args, q, lib):
    from dfnet_amd import _lib, engine as eng, mesh
    DEV = torch.device("cuda:0")
    axes = mesh.grid_axes((-.7, -.7, -.7, .7, .7, .7), n, device=DEV)
    nodes = n ** 3
    sigma = mesh.density_grid(q, axes)                                         # warm-up of the grid query, and the volume itself
    iso = float(np.float32(float(sigma.reshape(-1).kthvalue(int(0.9 * (nodes - 1)) + 1).values)))
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    nbytes = lib.dfn_isosurface_workspace_bytes(n, n, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    totals = torch.zeros(2, dtype=torch.int64, device=DEV)
    count = lambda: _lib.check(lib.dfn_isosurface_count(P(sigma), n, n, n, iso, P(ws), nbytes, P(totals), _lib.current_stream()))
    count()
    V, F = totals.tolist()
    verts, faces = torch.empty(V, 3, device=DEV), torch.empty(F, 3, dtype=torch.int32, device=DEV)
    emit = lambda: _lib.check(lib.dfn_isosurface_emit(P(sigma), *(P(a) for a in axes), n, n, n, iso, P(ws), nbytes, P(verts), V, P(faces),
                                                      F, _lib.current_stream()))
    emit()
    planes = max(1, (1 << 20) // (n * n))
    slab = eng.grid_points(axes, 0, planes)
    view = torch.tensor([[0., 0., -1.]], device=DEV).expand(slab.shape[0], 3).contiguous()
    hist = torch.zeros(1, 10, device=DEV)
    point = lambda: q.engine.mlp_fine_points(slab, view, hist)
    point()
    torch.cuda.synchronize()
    if args.trace_only:
        for fn in (count, emit, point):
            for _ in range(args.inner):
                fn()
        mesh.density_grid(q, axes)
        torch.cuda.synchronize()
        return None
    t_grid, s_grid = series(lambda: mesh.density_grid(q, axes), args.rounds, 1)
    t_point, s_point = series(point, args.rounds, args.inner)
    t_count, s_count = series(count, args.rounds, args.inner)
    t_emit, s_emit = series(emit, args.rounds, args.inner)
    blocks = (nodes + SCAN_BLOCK - 1) // SCAN_BLOCK
    b_count = nodes * (4 + 9) + blocks * 8 + blocks * 16      # count_kernel, then the block-sum scan (8 B read + 8 B written per block)
    b_emit = nodes * 1 + (V + F) * 12
    share = lambda b, t: {"GB": round(b / 1e9, 4), "GBps": round(b / t / 1e9, 1), "share_of_8TBps": round(b / t / HBM_NOMINAL, 4),
                          "share_of_6.29TBps": round(b / t / HBM_ACHIEVABLE, 4)}
    return dict(grid=n, nodes=nodes, threshold=iso, V=V, F=F, workspace_MB=round(nbytes / 2 ** 20, 1),
                grid_query=dict(s=round(t_grid, 4), spread_s=round(s_grid, 4), points_per_s=round(nodes / t_grid)),
                point_query=dict(points=slab.shape[0] * slab.shape[1], s=round(t_point, 6), spread_s=round(s_point, 6),
                                 points_per_s=round(slab.shape[0] * slab.shape[1] / t_point)),
                count=dict(ms=round(t_count * 1e3, 4), spread_ms=round(s_count * 1e3, 4), **share(b_count, t_count)),
                emit=dict(ms=round(t_emit * 1e3, 4), spread_ms=round(s_emit * 1e3, 4), **share(b_emit, t_emit)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_mesh_timing.py measures on the GPU: no device found, nothing measured")
    from dfnet_amd import _lib, engine as eng, nerfw, synthetic as syn
    lib = _lib.load()
    q = nerfw.HipQuery(eng.NerfHEngine(precision="f16x3").load_numpy(*syn.trained_nerfh_weights()))
    lines = []
    for n in args.sizes:
        try:
            line = measure(n, args, q, lib)
        except torch.cuda.OutOfMemoryError as e:
            line = dict(grid=n, skipped=f"does not fit: {str(e).splitlines()[0]}")
            torch.cuda.empty_cache()
        if line is not None:
            line["device"] = torch.cuda.get_device_name(0)
            lines.append(line)
            print(json.dumps(line), flush=True)
    q.engine.check_range()
    if args.log and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
