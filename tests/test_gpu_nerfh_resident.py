"""Kernel variant 7: variant 6 with a fixed set of small layers resident in LDS in the split-f16 16x16x32 coarse kernel and plain fused
fine kernel (nerfh_layout.h: kResidentVariant, kCoarseResident, kFineResident; nerfh_mlp_res.hip; nerfh_mlp_core.h: stage_resident,
layer<..., RES>).  The resident layers are copied into LDS once per workgroup and leave the streamed unit table; the fragments, the
MFMAs and the conversion pieces are variant 6's in variant 6's order, so every output is variant 6's bit for bit.  The variant is
latched per process (DFN_MLP_VARIANT), so each variant runs in a child:

  * variant 7 against variant 6 with torch.equal (zero elements may differ) on coarse sigma, raw, rgb / disp / acc on the raw route and
    on the fused one, the five render maps and a maps render's rgb / disp / acc (the raw route's fine kernel and the maps flavour keep
    variant 6's kernels behind the new coarse kernel and must still match), for the three cases of tests/test_gpu_nerfh_halfheads.py and
    for 1 040 rays at 64 + 64: 66 560 coarse points = 260 tiles and 133 120 fine points = 520 tiles, so that on 256 CUs workgroups of
    both kernels take a second and a third tile -- the streamed ring wraps past the resident layers and the resident copy is read
    again by later tiles; the range guard clean;
  * variant 7 through the checks and bounds variant 4 is held to (the CHILD program of tests/test_gpu_nerfh_mfma16.py, imported), the
    fp32-grade raw check against the exact-fp32 kernel included: a conversion piece that reads an accumulator too early loses a
    correction product and sits 1e-6 instead of 2.4e-7 from exact fp32 (nerfh_mlp_core.h).

This file is also the child of its own bit-identity tests: python tests/test_gpu_nerfh_resident.py <out.pt>.
"""
import json
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
MAPS = ("depth", "depth_static", "beta", "rgb_static", "rgb_transient")
TAGS = ("r37_8_16", "r37_32_32", "r64_64_128", "r1040_64_64")


def ray_cases():
    """{tag: (o, d, hist, Nc, Ni)}: the first three are the half-height heads' own cases"""
    ro, rd = orc.get_rays(48, 64, 73.0, T(syn.orbit_pose(2, 8))[:3, :4])
    sel = torch.randperm(48 * 64, generator=torch.Generator().manual_seed(3))
    pick = lambda s: (ro.reshape(-1, 3)[s].contiguous(), rd.reshape(-1, 3)[s].contiguous())
    shared = T(np.asarray(syn.HIST_IDX, dtype=np.float32))
    hist64 = T(np.random.default_rng(5).integers(0, 40, (64, 10)).astype(np.float32))
    return {"r37_8_16": (*pick(sel[:37]), shared, 8, 16),
            "r37_32_32": (*pick(sel[:37]), shared, 32, 32),
            "r64_64_128": (*pick(sel[100:164]), hist64, 64, 128),
            "r1040_64_64": (*pick(sel[200:1240]), shared, 64, 64)}


def child(out_path):
    """Every output of the four cases in this process's variant, seed-0 synthetic weights."""
    from dfnet_amd import engine as eng
    E = eng.NerfHEngine(precision="f16x3").load_numpy(*syn.nerfh_weights(0))
    res = {}
    for tag, (o, d, hist, Nc, Ni) in ray_cases().items():
        o, d, hist = o.to("cuda:0"), d.to("cuda:0"), hist.to("cuda:0")
        args = (o, d, hist, Nc, Ni, 0., 2.5)
        rec = dict(sigma=E.mlp_coarse(o, d, Nc, 0., 2.5).cpu())
        rgb, disp, acc, raw = E.render_rays(*args, retraw=True)               # the raw route: separate compositor
        rec.update(raw=raw.cpu(), rgb=rgb.cpu(), disp=disp.cpu(), acc=acc.cpu())
        f = E.render_rays(*args)                                              # compositing fused where Nc + Ni is a multiple of 32
        assert f[3] is None
        rec.update(fused_rgb=f[0].cpu(), fused_disp=f[1].cpu(), fused_acc=f[2].cpu())
        m = E.render_rays_maps(*args)
        rec.update(maps_rgb=m[0].cpu(), maps_disp=m[1].cpu(), maps_acc=m[2].cpu())
        rec.update({"map_" + k: m[4][k].cpu() for k in MAPS})
        res[tag] = rec
    assert E.range_flags() == 0
    torch.save(res, out_path)


if __name__ == "__main__":
    child(sys.argv[1])
    sys.exit(0)

import pytest  # noqa: E402

from tests import test_gpu_nerfh_mfma16 as m16  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("sigma", "raw", "rgb", "disp", "acc", "fused_rgb", "fused_disp", "fused_acc", "maps_rgb", "maps_disp", "maps_acc") + \
    tuple("map_" + k for k in MAPS)


def _run(variant, *argv, code=None):
    env = dict(os.environ, DFN_MLP_VARIANT=str(variant), PYTHONPATH=ROOT)
    cmd = [sys.executable, "-c", code] if code else [sys.executable, *argv]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    if out.returncode < 0 or out.returncode in (134, 137, 139):   # the child died on the GPU: nothing more is started on it
        pytest.exit(f"variant {variant} child ended with status {out.returncode}: {out.stderr[-2000:]}", returncode=3)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


# ---------------------------------------------------------------------------------------------- bit identity with variant 6
@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """The child's outputs under variants 6 and 7."""
    out = {}
    for variant in (6, 7):
        path = str(tmp_path_factory.mktemp("resident") / f"v{variant}.pt")
        _run(variant, os.path.abspath(__file__), path)
        out[variant] = torch.load(path)
    return out


@pytest.mark.parametrize("tag", TAGS)
def test_variant7_is_variant6_bit_for_bit(pair, tag):
    a, b = pair[6][tag], pair[7][tag]
    differ = {k: int((a[k] != b[k]).sum()) for k in KEYS}
    print(f"{tag}: elements that differ between variants 6 and 7: {differ}")
    for k in KEYS:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, differ[k])
    for k in ("sigma", "raw", "fused_rgb", "map_beta"):   # the outputs are there at all
        assert float(a[k].abs().max()) > 0 and bool(torch.isfinite(a[k]).all()), k


# ---------------------------------------------------------------------------------------------- variant 4's checks and bounds
@pytest.fixture(scope="module")
def checks():
    line = [x for x in _run(7, code=m16.CHILD).splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_g7_golden_render(checks):
    assert m16._value(checks, "g7") < 2e-5


def test_fused_compositing_matches_retraw(checks):
    assert m16._value(checks, "fused") < 2e-6


def test_g6_configs(checks):
    assert m16._value(checks, "g6") < 2e-5


def test_ray_count_off_the_tile(checks):
    assert m16._value(checks, "ragged") < 2e-5


def test_raw_is_fp32_grade(checks):
    rec = m16._value(checks, "grade")
    print(f"variant 7 raw vs the exact-fp32 kernel: {rec}")
    assert rec["raw_max_rel_f16x3_vs_f32"] < 5e-7, rec
    assert rec["raw_rms_rel_f16x3_vs_f32"] < 1.5e-7, rec


def test_trained_weights_goldens(checks):
    assert m16._value(checks, "g15") == "ok"


def test_range_guard_parity_or_loud_error(checks):
    assert m16._value(checks, "guard") == "ok"
