"""Kernel variant 8 and the pass rule of the fused render route.

Variant 8 is variant 7 with the tiles of its two kernels (split-f16 16x16x32 coarse kernel, plain fused fine kernel) claimed from a
device counter instead of dealt blockIdx.x, + gridDim.x, ... (nerfh_layout.h: kDynVariant; nerfh_mlp_dyn.hip; nerfh_mlp_core.h:
Stager::claim / next, mid_sync).  The fused route (no raw wanted, compositing inside the fine kernel) renders from a workspace layout
without a raw slot, in passes bounded by a constant of its own (nerfh_api.hip: kMaxFusedChunkRays, carve; 327 680 rays was measured
and is not a gain, so it stands at the raw route's 65 536).  Both are scheduling only: the same code computes every tile from the same
inputs into the same place, so every output keeps its bits.  The variant is latched per process
(DFN_MLP_VARIANT), so each variant runs in a child:

  * variant 8 against variant 7 with torch.equal (zero elements may differ) on coarse sigma and the fused route's rgb / disp / acc, the
    range guard clean, the CU count taken from the device:
      a  64 rays at 64 + 64: fewer tiles than workgroups, nothing is ever claimed;
      b  8 (CUs + 1) rays at 16 + 16: CUs + 1 fine tiles -- exactly one claim wins a tile, every other workgroup sees more == false;
      c  1 040 rays at 64 + 64: second and third tiles per workgroup, the streamed ring wraps past the resident layers;
      d  case c a second time in the same process: the counters are zeroed again in front of every pass;
      e  2 x 65 600 rays at 16 + 16 in one call: three passes, the counters zeroed in front of each;
      f  kMaxFusedChunkRays + 64 rays at 8 + 24 in one call: two passes whatever that bound is;
    and one render_image frame at 640 x 480, 64 + 128.
  * one call against its passes: 65 600 rays at 16 + 16 through render_rays against render_rays on the two halves the 65 536-ray bound
    cuts it into (one pass under a larger kMaxFusedChunkRays), torch.equal on rgb / disp / acc, with one shared histogram and with one
    histogram per ray (the per-ray table's summation order follows hist_rows, never the pass: nerfh_stages.hip, ray_bias_kernel).
  * dfn_render_workspace_bytes is at least the fused layout and at least the raw layout, both summed here by carve()'s formula.

This file is also the child of its own bit-identity tests: python tests/test_gpu_nerfh_dyn.py <out.pt>.
"""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dfnet_amd import synthetic as syn  # noqa: E402
from oracle import nerfh_oracle as orc  # noqa: E402

T = torch.from_numpy
TAGS = ("a", "b", "c", "d", "e", "f")
KEYS = ("sigma", "rgb", "disp", "acc")
MAX_CHUNK, MAX_FUSED_CHUNK = 65536, 65536   # nerfh_api.hip: kMaxChunkRays, kMaxFusedChunkRays


def rays(n, seed=3):
    """n rays of a 480 x 640 camera on the synthetic orbit, in a fixed random order (repeated past 307 200)"""
    ro, rd = orc.get_rays(480, 640, 585.0, T(syn.orbit_pose(2, 8))[:3, :4])
    sel = torch.randperm(480 * 640, generator=torch.Generator().manual_seed(seed))
    sel = sel.repeat((n + sel.numel() - 1) // sel.numel())[:n]
    return ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous()


def ray_cases(cus):
    """{tag: (n_rays, Nc, Ni)}"""
    return {"a": (64, 64, 64), "b": (8 * (cus + 1), 16, 16), "c": (1040, 64, 64), "d": (1040, 64, 64), "e": (2 * 65600, 16, 16),
            "f": (MAX_FUSED_CHUNK + 64, 8, 24)}


def child(out_path):
    """Coarse sigma and the fused route's outputs of every case, and one frame, in this process's variant; seed-0 synthetic weights."""
    from dfnet_amd import engine as eng
    dev = "cuda:0"
    E = eng.NerfHEngine(precision="f16x3").load_numpy(*syn.nerfh_weights(0))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shared = T(np.asarray(syn.HIST_IDX, dtype=np.float32)).to(dev)
    res = {"cus": cus}
    for tag, (n, Nc, Ni) in ray_cases(cus).items():
        o, d = (t.to(dev) for t in rays(n))
        rec = dict(sigma=E.mlp_coarse(o, d, Nc, 0., 2.5).cpu())
        f = E.render_rays(o, d, shared, Nc, Ni, 0., 2.5)
        assert f[3] is None
        rec.update(rgb=f[0].cpu(), disp=f[1].cpu(), acc=f[2].cpu())
        res[tag] = rec
    c2w = T(syn.orbit_pose(0, 8)).to(dev)
    rgb, disp, acc = E.render_image(c2w, 480, 640, 585.0, shared, 64, 128, 0., 2.5)
    res["frame"] = dict(rgb=rgb.cpu(), disp=disp.cpu(), acc=acc.cpu())
    res["range_flags"] = E.range_flags()
    torch.save(res, out_path)


if __name__ == "__main__":
    child(sys.argv[1])
    sys.exit(0)

import pytest  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(variant, *argv):
    env = dict(os.environ, DFN_MLP_VARIANT=str(variant), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, *argv], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    if out.returncode < 0 or out.returncode in (134, 137, 139):   # the child died on the GPU: nothing more is started on it
        pytest.exit(f"variant {variant} child ended with status {out.returncode}: {out.stderr[-2000:]}", returncode=3)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


# ---------------------------------------------------------------------------------------------- bit identity with variant 7
@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """The child's outputs under variants 7 and 8."""
    out = {}
    for variant in (7, 8):
        path = str(tmp_path_factory.mktemp("dyn") / f"v{variant}.pt")
        _run(variant, os.path.abspath(__file__), path)
        out[variant] = torch.load(path)
    return out


@pytest.mark.parametrize("tag", TAGS)
def test_variant8_is_variant7_bit_for_bit(pair, tag):
    a, b = pair[7][tag], pair[8][tag]
    differ = {k: int((a[k] != b[k]).sum()) for k in KEYS}
    print(f"{tag} (CUs {pair[8]['cus']}): elements that differ between variants 7 and 8: {differ}")
    for k in KEYS:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, differ[k])
        assert float(a[k].abs().max()) > 0 and bool(torch.isfinite(a[k]).all()), k   # the outputs are there at all
    assert pair[7]["range_flags"] == 0 and pair[8]["range_flags"] == 0


def test_second_run_repeats_the_first(pair):
    """case d is case c again in the same process: the counters of the first run must not reach into the second"""
    for k in KEYS:
        assert torch.equal(pair[8]["c"][k], pair[8]["d"][k]), k


def test_frame_variant8_is_variant7(pair):
    a, b = pair[7]["frame"], pair[8]["frame"]
    for k in ("rgb", "disp", "acc"):
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))
    assert tuple(a["rgb"].shape) == (480, 640, 3) and float(a["acc"].max()) > 0
    assert pair[7]["range_flags"] == 0 and pair[8]["range_flags"] == 0


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
