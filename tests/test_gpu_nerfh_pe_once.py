"""Kernel variant 9: the positional encoding formed once per tile.

Variant 9 is variant 8 (split-f16 16x16x32 coarse kernel and plain fused fine kernel, resident layers, claimed tiles) with the 63-wide
positional encoding of a tile's points kept in registers for the skip concat in front of layer 5 instead of formed a second time there
(nerfh_layout.h: kKeptVariant; nerfh_mlp_pe.hip; nerfh_mlp_core.h: trunk(), kEncodingKept).  The kept operand is the value the second
evaluation computes from the same inputs with the same code, so every output must keep variant 8's bits.  The variant is latched per
process (DFN_MLP_VARIANT), so each variant runs in a child with a time limit, and no child is started after one fails:

  * variant 9 against variant 8 with torch.equal (zero elements may differ; finite, not all zero) on coarse sigma and the fused
    route's rgb / disp / acc, split-f16 at netwidth 128, dfn_nerfh_range_status 0 after each case:
      a  64 rays at 64 + 64: fewer tiles than workgroups;
      b  8 calls of 257 rays at 16 + 16: a ragged last tile whose points are clamped (257 x 16 and 257 x 32 are no multiples of the
         256 points of a tile), several calls in one process;
      c  1 040 rays at 64 + 64: 260 coarse / 1 040 fine tiles on 256 workgroups, so workgroups take a second and a third tile and the
         kept operand must be the new tile's;
      d  case c a second time in the same process;
      e  the rays of a 24 x 32 image from raygen at 64 + 128: origins and directions differ per ray, Nf = 192 as in the workload;
      f  kMaxFusedChunkRays + 64 rays at 16 + 16: one tile-row of rays above the pass bound, a multi-pass call;
  * g  case a at precision f16 under DFN_MLP_VARIANT=9: the route falls back (nerfh_route.h: variant 9 outside split-f16 is variant
       4's plain kernels, as under variant 8) and gives variant 8's output there too.

This file is also the child of its own tests: python tests/test_gpu_nerfh_pe_once.py <out.pt>.
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
TAGS = ("a", "b", "c", "d", "e", "f", "g")
KEYS = ("sigma", "rgb", "disp", "acc")
MAX_FUSED_CHUNK = 65536   # nerfh_api.hip: kMaxFusedChunkRays
# {tag: (calls, rays per call, Nc, Ni, precision)}; e takes its rays from raygen
CASES = {"a": (1, 64, 64, 64, "f16x3"), "b": (8, 257, 16, 16, "f16x3"), "c": (1, 1040, 64, 64, "f16x3"), "d": (1, 1040, 64, 64, "f16x3"),
         "e": (1, 24 * 32, 64, 128, "f16x3"), "f": (1, MAX_FUSED_CHUNK + 64, 16, 16, "f16x3"), "g": (1, 64, 64, 64, "f16")}


def rays(n, seed=3):
    """n rays of a 480 x 640 camera on the synthetic orbit, in a fixed random order"""
    ro, rd = orc.get_rays(480, 640, 585.0, T(syn.orbit_pose(2, 8))[:3, :4])
    sel = torch.randperm(480 * 640, generator=torch.Generator().manual_seed(seed))[:n]
    return ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous()


def child(out_path):
    """Coarse sigma and the fused route's outputs of every case in this process's variant; seed-0 synthetic weights."""
    from dfnet_amd import engine as eng
    dev = "cuda:0"
    E = eng.NerfHEngine(precision="f16x3").load_numpy(*syn.nerfh_weights(0))
    shared = T(np.asarray(syn.HIST_IDX, dtype=np.float32)).to(dev)
    res = {}
    for tag, (calls, n, Nc, Ni, prec) in CASES.items():
        if tag == "e":
            o, d, _ = eng.raygen(24, 32, 29.25, T(syn.orbit_pose(1, 8)).to(dev), want_viewdirs=False)
            o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        else:
            o, d = (t.to(dev) for t in rays(calls * n))
        parts = {k: [] for k in KEYS}
        for c in range(calls):
            oc, dc = o[c * n:(c + 1) * n].contiguous(), d[c * n:(c + 1) * n].contiguous()
            parts["sigma"].append(E.mlp_coarse(oc, dc, Nc, 0., 2.5, precision=prec).cpu())
            f = E.render_rays(oc, dc, shared, Nc, Ni, 0., 2.5, precision=prec)
            assert f[3] is None
            for k, t in zip(("rgb", "disp", "acc"), f):
                parts[k].append(t.cpu())
        rec = {k: torch.cat(v) for k, v in parts.items()}
        rec["range_flags"] = E.range_flags()
        res[tag] = rec
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
    """The child's outputs under variants 8 and 9 (an exception in the first child's run leaves the second unstarted)."""
    out = {}
    for variant in (8, 9):
        path = str(tmp_path_factory.mktemp("pe_once") / f"v{variant}.pt")
        _run(variant, os.path.abspath(__file__), path)
        out[variant] = torch.load(path)
    return out


@pytest.mark.parametrize("tag", TAGS)
def test_variant9_is_variant8_bit_for_bit(pair, tag):
    a, b = pair[8][tag], pair[9][tag]
    calls, n, Nc, _, prec = CASES[tag]
    differ = {k: int((a[k] != b[k]).sum()) for k in KEYS}
    print(f"{tag} ({calls} x {n} rays, {prec}): elements that differ between variants 8 and 9: {differ}")
    assert tuple(a["sigma"].shape) == (calls * n, Nc) and tuple(a["rgb"].shape) == (calls * n, 3)
    for k in KEYS:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, differ[k])
        assert float(a[k].abs().max()) > 0 and bool(torch.isfinite(a[k]).all()) and bool(torch.isfinite(b[k]).all()), k
    assert a["range_flags"] == 0 and b["range_flags"] == 0


def test_second_run_repeats_the_first(pair):
    """case d is case c again in the same process: what a workgroup kept for its last tile must not reach into the next launch"""
    for k in KEYS:
        assert torch.equal(pair[9]["c"][k], pair[9]["d"][k]), k
