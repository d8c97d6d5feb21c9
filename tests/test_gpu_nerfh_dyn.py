"""The pass rule of the fused render route, under the default kernel variant.

The fused route (no raw wanted, compositing inside the fine kernel) renders from a workspace layout without a raw slot, in passes
bounded by a constant of its own (nerfh_api.hip: kMaxFusedChunkRays, carve; 327 680 rays was measured and is not a gain, so it stands
at the raw route's 65 536).  The default variant's kernels claim their tiles from device counters that are zeroed in front of every
pass and read a per-ray table that is rewritten per pass; where a call is cut into passes is scheduling only, so every output keeps
its bits.  (That the claimed tiles give the dealt tiles' bits, multi-pass calls included, is tests/test_gpu_nerfh_lean.py.)

  * one call against its passes: 65 600 rays at 16 + 16 through render_rays against render_rays on the two halves the 65 536-ray bound
    cuts it into (one pass under a larger kMaxFusedChunkRays), torch.equal on rgb / disp / acc, with one shared histogram and with one
    histogram per ray (the per-ray table's summation order follows hist_rows, never the pass: nerfh_stages.hip, ray_bias_kernel).
  * dfn_render_workspace_bytes is at least the fused layout and at least the raw layout, both summed here by carve()'s formula.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dfnet_amd import synthetic as syn  # noqa: E402
from oracle import nerfh_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
T = torch.from_numpy
MAX_CHUNK, MAX_FUSED_CHUNK = 65536, 65536   # nerfh_api.hip: kMaxChunkRays, kMaxFusedChunkRays


def rays(n, seed=3):
    """n rays of a 480 x 640 camera on the synthetic orbit, in a fixed random order"""
    ro, rd = orc.get_rays(480, 640, 585.0, T(syn.orbit_pose(2, 8))[:3, :4])
    sel = torch.randperm(480 * 640, generator=torch.Generator().manual_seed(seed))[:n]
    return ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous()


# ---------------------------------------------------------------------------------------------- one call against its old passes
@pytest.fixture(scope="module")
def engine():
    from dfnet_amd import engine as eng
    return eng.NerfHEngine(precision="f16x3").load_numpy(*syn.nerfh_weights(0))


def _old_chunk(n):
    passes = (n + MAX_CHUNK - 1) // MAX_CHUNK
    return ((n + passes - 1) // passes + 63) & ~63


@pytest.mark.parametrize("per_ray_hist", (False, True))
def test_one_call_is_its_old_passes(engine, per_ray_hist):
    n, Nc, Ni = 65600, 16, 16
    cut = _old_chunk(n)
    assert cut == 32832
    dev = "cuda:0"
    o, d = (t.to(dev) for t in rays(n, seed=7))
    if per_ray_hist:
        hist = T(np.random.default_rng(5).integers(0, 40, (n, 10)).astype(np.float32)).to(dev)
    else:
        hist = T(np.asarray(syn.HIST_IDX, dtype=np.float32)).to(dev)
    part = lambda t, lo, hi: t[lo:hi] if per_ray_hist else t
    whole = engine.render_rays(o, d, hist, Nc, Ni, 0., 2.5)
    halves = [engine.render_rays(o[lo:hi], d[lo:hi], part(hist, lo, hi), Nc, Ni, 0., 2.5) for lo, hi in ((0, cut), (cut, n))]
    assert whole[3] is None
    for i, k in enumerate(("rgb", "disp", "acc")):
        ref = torch.cat([h[i] for h in halves])
        differ = int((whole[i] != ref).sum())
        print(f"per_ray_hist={per_ray_hist} {k}: {differ} of {ref.numel()} elements differ from the two passes")
        assert whole[i].shape == ref.shape and torch.equal(whole[i], ref), (k, differ)
        assert float(ref.abs().max()) > 0 and bool(torch.isfinite(ref).all())
    assert engine.range_flags() == 0


# ---------------------------------------------------------------------------------------------- workspace
def _layout_bytes(n, Nc, Ni, fused, rec_floats=12):
    """carve() of nerfh_api.hip: every slot rounded up to 256 bytes"""
    al = lambda b: (b + 255) & ~255
    bound = MAX_FUSED_CHUNK if fused else MAX_CHUNK
    passes = (n + bound - 1) // bound
    chunk = ((n + passes - 1) // passes + 63) & ~63
    Nf = Nc + Ni
    total = 3 * al(n * 12)                                  # o, d, v
    total += al(chunk * Nc * 4) + al(chunk * Nf * 4)        # sigma, z
    if not fused:
        total += al(chunk * Nf * 9 * 4)                     # raw
    total += al(chunk * 256 * 4)                            # per-ray table: ray_bias_floats(kMaxWidth) floats
    total += al(chunk * ((Nf + 31) // 32) * rec_floats * 4)   # segment records
    return total


def test_workspace_covers_both_routes(engine):
    lib = engine.lib
    for n, Nc, Ni in ((307200, 64, 128), (65600, 16, 16), (1040, 64, 64)):
        fused, raw = _layout_bytes(n, Nc, Ni, True), _layout_bytes(n, Nc, Ni, False)
        got = lib.dfn_render_workspace_bytes(n, Nc, Ni)
        print(f"{n} rays {Nc}+{Ni}: dfn_render_workspace_bytes {got}, fused layout {fused}, raw layout {raw}")
        assert got >= fused and got >= raw
        got_maps = lib.dfn_render_maps_workspace_bytes(n, Nc, Ni)
        assert got_maps >= _layout_bytes(n, Nc, Ni, True, 16) and got_maps >= _layout_bytes(n, Nc, Ni, False, 16)
