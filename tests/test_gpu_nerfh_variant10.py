"""Kernel variant 10: the fused fine kernel's per-ray seeds stored at the accumulators' scale.

Variant 10 is variant 9 (split-f16 16x16x32 coarse kernel and plain fused fine kernel, resident layers, claimed tiles, kept encoding)
whose fused fine route has ray_bias_kernel write its per-ray table multiplied by the fine network's in_scale, once per pass, so that the
two RAYBIAS layers of the fine kernel take the loaded seeds as they are instead of multiplying them on every tile (nerfh_layout.h:
kHoistVariant; nerfh_mlp_hoist.hip; nerfh_mlp_core.h: layer(); nerfh_stages.hip: ray_bias_kernel<SCALED>).  The product is the same fp32
multiply by a power of two on the same values, moved, so every output must keep variant 9's bits.  The variant is latched per process
(DFN_MLP_VARIANT), so each variant runs in a child with a time limit, and no child is started after one fails:

  * variant 10 against variant 9 with torch.equal (zero elements may differ; finite, not all zero) on coarse sigma and the fused
    route's rgb / disp / acc, split-f16 at netwidth 128, dfn_nerfh_range_status 0 after each case:
      a  64 rays at 64 + 64: fewer tiles than workgroups;
      b  8 calls of 257 rays at 16 + 16: ragged last tiles whose points are clamped, several calls in one process;
      c  1 040 rays at 64 + 64: 260 coarse / 1 040 fine tiles on 256 workgroups, so workgroups take several tiles;
      d  case c a second time in the same process: the tile counters are re-armed;
      e  the rays of a 24 x 32 image from raygen at 64 + 128: origins and directions differ per ray, Nf = 192 as in the workload;
      f  kMaxFusedChunkRays + 64 = 65 600 rays at 16 + 16: two passes, so the scaled table is rewritten per pass;
      h  case a with one histogram row per ray: ray_bias_kernel's other summation path (per-ray embeddings, two waves per ray), the
         only input on which the scaled table is formed by other code than in the shared-histogram cases;
  * g  case a at precision f16 under DFN_MLP_VARIANT=10: the route falls back (nerfh_route.h: variant 10 outside split-f16 is variant
       4's plain kernels, as under variant 9) and gives variant 9's output there too;
  * under variant 10 the routes that must still read the UNSCALED table give variant 9's bits on 64 rows: a maps render (rgb / disp /
    acc and the five maps), a `raw` render (rgb / disp / acc / raw) and a fine point query (raw), each with the shared and with the
    per-ray histogram.

This file is also the child of its own tests: python tests/test_gpu_nerfh_variant10.py <out.pt>.
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
TAGS = ("a", "b", "c", "d", "e", "f", "g", "h")
KEYS = ("sigma", "rgb", "disp", "acc")
MAX_FUSED_CHUNK = 65536   # nerfh_api.hip: kMaxFusedChunkRays
# {tag: (calls, rays per call, Nc, Ni, precision, one histogram row per ray)}; e takes its rays from raygen
CASES = {"a": (1, 64, 64, 64, "f16x3", False), "b": (8, 257, 16, 16, "f16x3", False), "c": (1, 1040, 64, 64, "f16x3", False),
         "d": (1, 1040, 64, 64, "f16x3", False), "e": (1, 24 * 32, 64, 128, "f16x3", False),
         "f": (1, MAX_FUSED_CHUNK + 64, 16, 16, "f16x3", False), "g": (1, 64, 64, 64, "f16", False), "h": (1, 64, 64, 64, "f16x3", True)}
# the routes that keep the unscaled table: (tag, per-ray histogram)
OTHER = tuple((kind, per_ray) for kind in ("maps", "raw", "points") for per_ray in (False, True))
MAPS = ("depth", "depth_static", "beta", "rgb_static", "rgb_transient")


def rays(n, seed=3):
    """n rays of a 480 x 640 camera on the synthetic orbit, in a fixed random order"""
    ro, rd = orc.get_rays(480, 640, 585.0, T(syn.orbit_pose(2, 8))[:3, :4])
    sel = torch.randperm(480 * 640, generator=torch.Generator().manual_seed(seed))[:n]
    return ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous()


def ray_hists(n, seed=11):
    """one histogram row per ray: embedding indices drawn over the whole vocabulary, every ray its own"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1000, (n, len(syn.HIST_IDX)), generator=g).float()


def child(out_path):
    """Coarse sigma and the fused route's outputs of every case, then the maps / raw / point-query routes, in this process's variant;
    seed-0 synthetic weights."""
    from dfnet_amd import engine as eng
    dev = "cuda:0"
    E = eng.NerfHEngine(precision="f16x3").load_numpy(*syn.nerfh_weights(0))
    shared = T(np.asarray(syn.HIST_IDX, dtype=np.float32)).to(dev)
    res = {}
    for tag, (calls, n, Nc, Ni, prec, per_ray) in CASES.items():
        if tag == "e":
            o, d, _ = eng.raygen(24, 32, 29.25, T(syn.orbit_pose(1, 8)).to(dev), want_viewdirs=False)
            o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        else:
            o, d = (t.to(dev) for t in rays(calls * n))
        hists = ray_hists(calls * n).to(dev) if per_ray else None
        parts = {k: [] for k in KEYS}
        for c in range(calls):
            oc, dc = o[c * n:(c + 1) * n].contiguous(), d[c * n:(c + 1) * n].contiguous()
            hc = hists[c * n:(c + 1) * n].contiguous() if per_ray else shared
            parts["sigma"].append(E.mlp_coarse(oc, dc, Nc, 0., 2.5, precision=prec).cpu())
            f = E.render_rays(oc, dc, hc, Nc, Ni, 0., 2.5, precision=prec)
            assert f[3] is None
            for k, t in zip(("rgb", "disp", "acc"), f):
                parts[k].append(t.cpu())
        rec = {k: torch.cat(v) for k, v in parts.items()}
        rec["range_flags"] = E.range_flags()
        res[tag] = rec
    # the routes that read the unscaled table: 64 rows at 64 + 64 in split-f16
    o, d = (t.to(dev) for t in rays(64))
    v = d / d.norm(dim=-1, keepdim=True)
    z = torch.linspace(0.1, 2.4, 64, device=dev)
    pts = (o[:, None, :] + d[:, None, :] * z[None, :, None]).contiguous()
    for kind, per_ray in OTHER:
        hc = ray_hists(64).to(dev) if per_ray else shared
        if kind == "maps":
            rgb, disp, acc, raw, maps = E.render_rays_maps(o, d, hc, 64, 64, 0., 2.5, precision="f16x3")
            rec = dict(rgb=rgb, disp=disp, acc=acc, **{m: maps[m] for m in MAPS})
        elif kind == "raw":
            rgb, disp, acc, raw = E.render_rays(o, d, hc, 64, 64, 0., 2.5, retraw=True, precision="f16x3")
            rec = dict(rgb=rgb, disp=disp, acc=acc, raw=raw)
        else:
            rec = dict(raw=E.mlp_fine_points(pts, v, hc, precision="f16x3"))
        rec = {k: t.cpu() for k, t in rec.items()}
        rec["range_flags"] = E.range_flags()
        res[(kind, per_ray)] = rec
    torch.save(res, out_path)


if __name__ == "__main__":
    child(sys.argv[1])
    sys.exit(0)

import pytest  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(variant, *argv):
    env = dict(os.environ, DFN_MLP_VARIANT=str(variant), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, *argv], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    if out.returncode < 0 or out.returncode in (134, 137, 139):   # the child died on the GPU: nothing more is started on it
        pytest.exit(f"variant {variant} child ended with status {out.returncode}: {out.stderr[-2000:]}", returncode=3)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """The child's outputs under variants 9 and 10 (an exception in the first child's run leaves the second unstarted)."""
    out = {}
    for variant in (9, 10):
        path = str(tmp_path_factory.mktemp("variant10") / f"v{variant}.pt")
        _run(variant, os.path.abspath(__file__), path)
        out[variant] = torch.load(path)
    return out


def _same_bits(a, b, keys):
    differ = {k: int((a[k] != b[k]).sum()) for k in keys}
    print(f"elements that differ between variants 9 and 10: {differ}")
    for k in keys:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, differ[k])
        assert float(a[k].abs().max()) > 0 and bool(torch.isfinite(a[k]).all()) and bool(torch.isfinite(b[k]).all()), k
    assert a["range_flags"] == 0 and b["range_flags"] == 0


@pytest.mark.parametrize("tag", TAGS)
def test_variant10_is_variant9_bit_for_bit(pair, tag):
    a, b = pair[9][tag], pair[10][tag]
    calls, n, Nc, _, prec, per_ray = CASES[tag]
    print(f"{tag} ({calls} x {n} rays, {prec}, {'one histogram per ray' if per_ray else 'shared histogram'})")
    assert tuple(a["sigma"].shape) == (calls * n, Nc) and tuple(a["rgb"].shape) == (calls * n, 3)
    _same_bits(a, b, KEYS)


def test_per_ray_histograms_reach_the_output(pair):
    """case h is case a's rays with other embeddings: were the histogram rows ignored, h would test nothing a does not"""
    assert not torch.equal(pair[10]["a"]["rgb"], pair[10]["h"]["rgb"])


def test_second_run_repeats_the_first(pair):
    """case d is case c again in the same process: the counters are zeroed and the table rewritten in front of every pass"""
    for k in KEYS:
        assert torch.equal(pair[10]["c"][k], pair[10]["d"][k]), k


@pytest.mark.parametrize("kind,per_ray", OTHER)
def test_other_routes_keep_the_unscaled_table(pair, kind, per_ray):
    a, b = pair[9][(kind, per_ray)], pair[10][(kind, per_ray)]
    keys = [k for k in a if k != "range_flags"]
    assert set(keys) == set(k for k in b if k != "range_flags") and keys
    _same_bits(a, b, keys)
