"""Timing of the generic-width render gradient for an A/B of library builds (tools/gpu_ab_libs.sh, one library per process through
DFN_LIB_PATH): dfn_nerfh_generic_render_rays_backward on 4 096 rays, 64+128 samples, netwidth 32 and 256; where the library has
dfn_nerfh_generic_render_rays_backward_raw, that entry too (grad_raw NULL / given / alone).  One JSON line per (netwidth, mode): median,
min and max of AB_REPS device-event timings after three warm-up calls.  `tag` (argv[1]) labels the lines; with AB_SAVE=dir the old
entry's gradients are saved to dir/ab_<tag>_<netwidth>.pt for a bitwise comparison between builds.

  LINES_KEPT=12 tools/gpu_ab_libs.sh "python tools/gpu_generic_backward_ab.py x" libdfnet_hip_parent.so libdfnet_hip.so"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dfnet_amd import _lib  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "lib"
_probe = ctypes.CDLL(_lib.LIB_PATH)
HAS_RAW = hasattr(_probe, "dfn_nerfh_generic_render_rays_backward_raw")
for name in [k for k in _lib.SIGNATURES if not hasattr(_probe, k)]:   # an older build: bind what it exports
    _lib.SIGNATURES.pop(name)
from dfnet_amd import engine as eng, synthetic as syn  # noqa: E402
from dfnet_amd._lib import current_stream, ptr  # noqa: E402
from oracle import nerfh_oracle as orc  # noqa: E402

DEV = "cuda:0"
T = torch.from_numpy
R, Nc, Ni, REPS = 4096, 64, 128, int(os.environ.get("AB_REPS", "15"))
lib = _lib.load()
for width in (32, 256):
    cw, fw, ea, et = syn.nerfh_weights(4, W=width)
    E = eng.NerfHEngine(width=width, precision="f32").load_numpy(cw, fw, ea, et)
    rng = np.random.default_rng(11)
    ro, rd = orc.get_rays(480, 640, 585.0, T(syn.orbit_pose(3, 8))[:3, :4])
    sel = rng.choice(480 * 640, R, replace=False)
    o, d = ro.reshape(-1, 3)[sel].contiguous().to(DEV), rd.reshape(-1, 3)[sel].contiguous().to(DEV)
    hist = T(rng.integers(0, 40, (R, 10)).astype(np.float32)).to(DEV)
    G = T(rng.standard_normal((R, 3)).astype(np.float32)).to(DEV)
    Gr = T((rng.standard_normal((R, Nc + Ni, 9)) / (Nc + Ni)).astype(np.float32)).to(DEV)
    ws = torch.empty(lib.dfn_nerfh_generic_backward_workspace_bytes(E.handle, R, Nc, Ni), dtype=torch.uint8, device=DEV)
    go, gd = torch.empty(R, 3, device=DEV), torch.empty(R, 3, device=DEV)
    wsp = ctypes.c_void_p(ws.data_ptr())

    def old():
        rc = lib.dfn_nerfh_generic_render_rays_backward(E.handle, ptr(o), ptr(d), None, ptr(hist), R, R, Nc, Ni, 0., 2.5, ptr(G), ptr(go), ptr(gd),
                                                        None, wsp, ws.numel(), current_stream())
        assert rc == 0, lib.dfn_last_error()

    def new(g, gr):
        rc = lib.dfn_nerfh_generic_render_rays_backward_raw(E.handle, ptr(o), ptr(d), None, ptr(hist), R, R, Nc, Ni, 0., 2.5, ptr(g), ptr(gr),
                                                            ptr(go), ptr(gd), None, wsp, ws.numel(), current_stream())
        assert rc == 0, lib.dfn_last_error()

    modes = [("old_entry", old)]
    if HAS_RAW:
        modes += [("new_entry_null_raw", lambda: new(G, None)), ("new_entry_rgb_and_raw", lambda: new(G, Gr)), ("new_entry_raw_only", lambda: new(None, Gr))]
    for name, fn in modes:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        ts = np.array(ts)
        print(json.dumps(dict(lib=tag, width=width, mode=name, median_ms=round(float(np.median(ts)), 3), min_ms=round(float(ts.min()), 3),
                              max_ms=round(float(ts.max()), 3), reps=REPS)), flush=True)
        if name == "old_entry" and os.environ.get("AB_SAVE"):
            torch.save((go.cpu(), gd.cpu()), os.path.join(os.environ["AB_SAVE"], f"ab_{tag}_{width}.pt"))
    del E
