#!/usr/bin/env python3
"""Measurements of the render maps' frame back-end (dfn_frame_post_maps) and of render_path(ret_maps=...).

  python tools/gpu_post_maps.py kernel [--reps 20]
      One 16-frame batch at 640 x 480, all five maps and per-frame gt: three warm-up calls, then --reps calls of
      engine.frame_post_maps, each between device events.  Prints one JSON line: bytes the three kernels move (computed from the shapes),
      median / min / max of the whole call.  For the kernels' own times run it under a kernel trace in a run of its own:
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/gpu_post_maps.py kernel
      (beta_max_kernel, frame_post_maps_kernel, frame_post_maps_finish_kernel in DIR/.../k_kernel_stats.csv).
  python tools/gpu_post_maps.py path --arm plain|maps [--frames 32] [--tree DIR]
      render_path of --frames poses at 640 x 480, 64 + 128 samples, split-f16, with a save directory and one grey ground-truth frame; a
      4-frame warm-up run first.  plain: without ret_maps; maps: ret_maps=True.  --tree: import dfnet_amd from another checkout (a build of
      the parent commit, arm plain) so that the unchanged path is compared library against library.  One JSON line with last_timing.
Alternate the arms in fresh processes and repeat: the spread between repeats of one arm is the yardstick for a difference between two."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_ACHIEVABLE = 6.3e12   # bytes / s: the achievable HBM rate the project's rooflines use (profiles/r05_roofline.md)


def kernel(reps):
    import torch
    sys.path.insert(0, ROOT)
    from dfnet_amd import engine as eng
    n, H, W = 16, 480, 640
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    maps = {m: torch.rand((n, H, W, 3) if m.startswith("rgb_") else (n, H, W), device=dev, generator=g) * 2.5 + 0.1 for m in eng.MAP_NAMES}
    gt = torch.rand(n, H, W, 3, device=dev, generator=g)
    px = n * H * W
    # per pixel: beta once for the maximum (4 B); then two depths, beta, two colours (4 + 4 + 4 + 12 + 12 = 36 B) and gt (12 B) in,
    # two uint16 + one uint8 + two 3 x uint8 (11 B) out
    moved = {"beta_max_kernel": 4 * px, "frame_post_maps_kernel": (36 + 12 + 11) * px}
    for _ in range(3):
        eng.frame_post_maps(maps, 0.0, 2.5, gt=gt)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.frame_post_maps(maps, 0.0, 2.5, gt=gt)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    total = sum(moved.values())
    med = float(np.median(ms))
    print(json.dumps({"case": "frame_post_maps, 16 x 640x480, five maps + per-frame gt", "reps": reps, "bytes_moved": moved, "bytes_total": total,
                      "call_median_ms": med, "call_min_ms": min(ms), "call_max_ms": max(ms),
                      "call_TBps_at_median": total / (med * 1e-3) / 1e12, "call_fraction_of_6.3TBps": total / (med * 1e-3) / HBM_ACHIEVABLE,
                      "note": "the call = memset + three kernels + seven output allocations; kernel times come from a kernel trace"}), flush=True)


def path(arm, frames, tree):
    import torch
    sys.path.insert(0, tree)
    from dfnet_amd import engine as eng, rendering, synthetic as syn
    from dfnet_amd.nerfw import HipQuery
    assert os.path.abspath(eng.__file__).startswith(os.path.abspath(tree) + os.sep), eng.__file__
    H, W, focal, Nc, Ni = 480, 640, 585.0, 64, 128
    E = eng.NerfHEngine(precision="f16x3").load_numpy(*syn.nerfh_weights(0))
    kw = dict(network_query_fn=HipQuery(E), perturb=False, N_importance=Ni, N_samples=Nc, use_viewdirs=True, white_bkgd=False,
              raw_noise_std=0., test_time=True, ndc=False, lindisp=False, near=0.0, far=2.5)
    gt = np.full((H, W, 3), 0.5, np.float32)
    more = {"ret_maps": True} if arm == "maps" else {}
    rec = None
    for n in (4, frames):   # the first run warms up code objects, the allocator and the PNG pool's imports
        poses = torch.stack([torch.from_numpy(syn.orbit_pose(k, n)) for k in range(n)])
        hist = torch.from_numpy(syn.HIST_IDX).repeat(n, 1)
        savedir = tempfile.mkdtemp(prefix="post_maps_png_")
        t0 = time.time()
        with torch.no_grad():
            rendering.render_path(None, poses, [H, W, focal], 32768, kw, gt_imgs=gt, savedir=savedir, single_gt_img=True, img_ids=hist, **more)
        wall = time.time() - t0
        files = os.listdir(savedir)
        png_bytes = sum(os.path.getsize(os.path.join(savedir, f)) for f in files)
        shutil.rmtree(savedir, ignore_errors=True)
        tm = rendering.render_path.last_timing
        rec = {"arm": arm, "tree": os.path.abspath(tree), "frames": n, "wall_s": wall, "render_s": tm["render_s"], "post_launch_s": tm["post_launch_s"],
               "png_tail_s": tm["png_tail_s"], "png_files": len(files), "png_bytes": png_bytes, "maps": tm.get("maps", [])}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "path"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--arm", choices=("plain", "maps"), default="plain")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.what == "kernel":
        kernel(a.reps)
    else:
        path(a.arm, a.frames, a.tree)
