"""A/B of the compositing backward: the kernel for every output (dfn_composite_fine_backward_maps) with all eight upstream gradients
and with g_rgb alone, beside the rgb-only kernel (dfn_composite_fine_backward).  n = 76 800 rays (a 240 x 320 frame), Nf = 192, 5
warm-up and 20 timed launches each, median.  Traffic: 10 floats read (raw 9, z 1) and 9 written per sample.  One JSON line.

    python tools/gpu_maps_grad_ab.py [--rays 76800] [--nf 192]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dfnet_amd import engine as eng  # noqa: E402


def median_ms(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=76800)
    ap.add_argument("--nf", type=int, default=192)
    a = ap.parse_args()
    n, Nf = a.rays, a.nf
    gen = torch.Generator(device="cuda").manual_seed(0)
    raw = torch.rand(n, Nf, 9, device="cuda", generator=gen)
    raw[..., 3] = torch.nn.functional.softplus(torch.randn(n, Nf, device="cuda", generator=gen))
    raw[..., 7] = torch.nn.functional.softplus(torch.randn(n, Nf, device="cuda", generator=gen))
    z = torch.sort(torch.rand(n, Nf, device="cuda", generator=gen) * 2.5, -1)[0].contiguous()
    G = {k: torch.randn((n, 3) if k.startswith("rgb") else (n,), device="cuda", generator=gen) for k in eng.GRAD_NAMES}
    # the wrappers allocate the [n,Nf,9] result per call (torch's caching allocator: no device allocation after the warm-up)
    t_all = median_ms(lambda: eng.composite_fine_backward_maps(raw, z, G))
    t_rgb = median_ms(lambda: eng.composite_fine_backward_maps(raw, z, dict(rgb=G["rgb"])))
    t_old = median_ms(lambda: eng.composite_fine_backward(raw, z, G["rgb"]))
    gb = n * Nf * 19 * 4 / 1e9
    print("MAPS_GRAD_AB " + json.dumps(dict(rays=n, Nf=Nf, all_eight_ms=t_all, rgb_only_new_ms=t_rgb, rgb_only_existing_ms=t_old,
                                            gbps_all_eight=gb / t_all * 1e3, gbps_rgb_only_new=gb / t_rgb * 1e3,
                                            gbps_rgb_only_existing=gb / t_old * 1e3, ratio_all_vs_existing=t_all / t_old,
                                            ratio_rgb_new_vs_existing=t_rgb / t_old)))


if __name__ == "__main__":
    main()
