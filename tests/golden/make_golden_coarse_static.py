#!/usr/bin/env python3
"""Generate tests/golden/g18_coarse_static.npz by running the REFERENCE's own run_network_NeRFW(..., typ='coarse', test_time=False)
(models/nerfw.py:47-60, with NeRFW.forward's output_transient=False branch, :326-343) on the CPU, the way tests/golden/make_golden.py
does (same import path, same empty `imageio` stand-in): numbers only, nothing of its source.

The coarse NeRFW(W=128) holds dfnet_amd.synthetic.nerfh_weights(0)'s coarse network.  Inputs: 3 rows x 5 points in [-1.5, 1.5]^3 and
3 unit view directions.  Stored: the inputs, the [3, 5, 4] output, the weights G of one fixed weighted sum of it and, from the
reference under torch autograd, d sum(out * G) / d points [3, 5, 3] and / d viewdirs [3, 3].

Usage:  python tests/golden/make_golden_coarse_static.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/script"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
sys.modules.setdefault("imageio", types.ModuleType("imageio"))

from dfnet_amd import synthetic as syn  # noqa: E402


def main():
    from models import nerfw  # the reference
    cw = syn.nerfh_weights(0)[0]
    coarse = nerfw.NeRFW("coarse", D=8, W=128, skips=[4], in_channels_xyz=63, in_channels_dir=27)
    missing = coarse.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in cw.items()}, strict=False)
    assert not missing.missing_keys and not missing.unexpected_keys, missing
    embed_fn, ch_xyz, _ = nerfw.get_embedder(10, 0)
    embeddirs_fn, ch_dir, _ = nerfw.get_embedder(4, 0)
    assert (ch_xyz, ch_dir) == (63, 27)
    gen = torch.Generator().manual_seed(1818)
    rows, N = 3, 5
    pts = torch.rand(rows, N, 3, generator=gen) * 3 - 1.5
    v = torch.randn(rows, 3, generator=gen)
    v = v / v.norm(dim=-1, keepdim=True)
    G = torch.randn(rows, N, 4, generator=gen)
    p, w = pts.clone().requires_grad_(True), v.clone().requires_grad_(True)
    out = nerfw.run_network_NeRFW(p, w, None, coarse, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn, typ="coarse", embedding_a=None,
                                  embedding_t=None, output_transient=False, netchunk=65536, test_time=False)
    assert tuple(out.shape) == (rows, N, 4)
    (out * G).sum().backward()
    path = os.path.join(HERE, "g18_coarse_static.npz")
    arrs = dict(pts=pts, viewdirs=v, G=G, raw4=out.detach(), g_pts=p.grad, g_viewdirs=w.grad)
    np.savez_compressed(path, **{k: t.numpy() for k, t in arrs.items()})
    print(f"g18_coarse_static: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrs)} arrays")


if __name__ == "__main__":
    main()
