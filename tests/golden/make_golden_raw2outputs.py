#!/usr/bin/env python3
"""Generate tests/golden/g17_raw2outputs.npz by running the REFERENCE's own raw2outputs_NeRFW (models/rendering.py:132-243) on the CPU,
the way tests/golden/make_golden.py does (same import path, same empty `imageio` stand-in): numbers only, nothing of its source.

n = 6 rays of N = 12 samples, raw as tests/test_gpu_maps_grad.py::stage_inputs forms it (colours and beta in (0, 1), densities
softplus(N(0,1)), z sorted in [0, 2.5]); the 1- and 4-channel modes take a sigma of BOTH signs (N(0.5, 1.5)), so that the relu matters.
Per mode the reference's 7-tuple and, from the reference under torch autograd, d/d raw and d/d z_vals of one fixed weighted sum of ALL
the outputs the mode returns (the weights G_* are stored).  raw_noise_std = 0 throughout.

  m1   typ="coarse", test_time                           raw [n,N,1]
  m2   typ="coarse", training                            raw [n,N,4]        m2w: white_bkgd
  m3   output_transient, test_time, static_only, "fine"  raw [n,N,9]        m3w: white_bkgd
  m3t  output_transient, training, "fine"

Usage:  python tests/golden/make_golden_raw2outputs.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/script"
sys.path.insert(0, REF)
sys.modules.setdefault("imageio", types.ModuleType("imageio"))

NAMES = ("rgb", "disp", "acc", "weights", "depth", "tsig", "beta")
MODES = {   # raw key, then the reference's arguments after rays_d
    "m1": ("raw1", dict(raw_noise_std=0., output_transient=False, white_bkgd=False, test_time=True, static_only=True, typ="coarse")),
    "m2": ("raw4", dict(raw_noise_std=0., output_transient=False, white_bkgd=False, test_time=False, static_only=True, typ="coarse")),
    "m2w": ("raw4", dict(raw_noise_std=0., output_transient=False, white_bkgd=True, test_time=False, static_only=True, typ="coarse")),
    "m3": ("raw9", dict(raw_noise_std=0., output_transient=True, white_bkgd=False, test_time=True, static_only=True, typ="fine")),
    "m3w": ("raw9", dict(raw_noise_std=0., output_transient=True, white_bkgd=True, test_time=True, static_only=True, typ="fine")),
    "m3t": ("raw9", dict(raw_noise_std=0., output_transient=True, white_bkgd=False, test_time=False, static_only=True, typ="fine")),
}


def main():
    from models import rendering  # the reference
    n, N = 6, 12
    gen = torch.Generator().manual_seed(1717)
    raw9 = torch.rand(n, N, 9, generator=gen) * 0.98 + 0.01
    raw9[..., 3] = torch.nn.functional.softplus(torch.randn(n, N, generator=gen))
    raw9[..., 7] = torch.nn.functional.softplus(torch.randn(n, N, generator=gen))
    z = torch.sort(torch.rand(n, N, generator=gen) * 2.5, -1)[0]
    sig = torch.randn(n, N, generator=gen) * 1.5 + 0.5
    raw4 = torch.cat([raw9[..., :3], sig[..., None]], -1)
    raw1 = sig[..., None].clone()
    rays_d = torch.randn(n, 3, generator=gen)
    G = {k: torch.randn((n, 3) if k == "rgb" else (n, N) if k in ("weights", "tsig") else (n,), generator=gen) for k in NAMES}
    out = dict(z=z, raw1=raw1, raw4=raw4, raw9=raw9, **{"G_" + k: v for k, v in G.items()})
    for tag, (rk, kw) in MODES.items():
        r = out[rk].clone().requires_grad_(True)
        zz = z.clone().requires_grad_(True)
        res = rendering.raw2outputs_NeRFW(r, zz, rays_d, beta_min=0.1, **kw)
        loss = 0.
        for k, v in zip(NAMES, res):
            if v is None:
                continue
            out[f"{tag}_{k}"] = v.detach().clone()
            if v.requires_grad:          # M2's beta is a constant
                loss = loss + (v * G[k]).sum()
        loss.backward()
        out[f"{tag}_graw"], out[f"{tag}_gz"] = r.grad.clone(), zz.grad.clone()
    path = os.path.join(HERE, "g17_raw2outputs.npz")
    np.savez_compressed(path, **{k: v.numpy() for k, v in out.items()})
    print(f"g17_raw2outputs: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
