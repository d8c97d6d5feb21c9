"""Kernel variant 4: the split-f16 render MLP on 16x16x32 MFMAs (nerfh_layout.h: PrecX3M16), held to the bounds variant 0 (the
32x32x16 kernels) is held to.  The variant is latched per process (DFN_MLP_VARIANT), so each variant runs its checks in a child; the
same checks run for variant 0 next to it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, traceback
import numpy as np, torch
from dfnet_amd import engine as eng, synthetic as syn
from oracle import nerfh_oracle as orc
from tests import test_gpu_nerfh as t
from tests.conftest import golden
import bench

T, dev, relmax = torch.from_numpy, t.dev, t.relmax
out = {}
def run(name, fn):
    try:
        out[name] = fn()
    except Exception:
        out[name] = {"error": traceback.format_exc()[-3000:]}

cw, fw, ea, et = syn.nerfh_weights(0)
E = eng.NerfHEngine().load_numpy(cw, fw, ea, et)
c, f = t.tt(cw), t.tt(fw)
hist = dev(syn.HIST_IDX)

def g7():
    g = golden("g7_render_image")
    r = E.render_image(dev(g["c2w"]), int(g["H"]), int(g["W"]), float(g["focal"]), dev(g["hist"]), int(g["Nc"]), int(g["Ni"]),
                       float(g["near"]), float(g["far"]), precision="f16x3")
    return max(relmax(x, g[k]) for x, k in zip(r, ("rgb", "disp", "acc")))

def fused():
    o, d, _ = eng.raygen(96, 128, 146.0, T(syn.orbit_pose(3, 8)).to("cuda:0"))
    a = E.render_rays(o.reshape(-1, 3), d.reshape(-1, 3), hist, 64, 128, 0., 2.5, precision="f16x3")
    b = E.render_rays(o.reshape(-1, 3), d.reshape(-1, 3), hist, 64, 128, 0., 2.5, retraw=True, precision="f16x3")
    assert a[3] is None and b[3] is not None
    return max(relmax(x, y.cpu()) for x, y in zip(a[:3], b[:3]))

def g6():
    e = 0.
    for tag in "ab":
        g = golden("g6_render_rays_" + tag)
        r = E.render_rays(dev(g["rays_o"]), dev(g["rays_d"]), dev(g["hist"]), int(g["Nc"]), int(g["Ni"]), float(g["near"]),
                          float(g["far"]), retraw=True, precision="f16x3")
        e = max([e] + [relmax(x, g[k]) for x, k in zip(r, ("rgb", "disp", "acc", "raw"))])
    return e

def ragged():
    # 37 rays: 888 (8+16) and 7104 (64+128) points, neither a multiple of the 256-point tile; fused and separate compositing
    c2w = T(syn.orbit_pose(2, 8))
    ro, rd = orc.get_rays(48, 64, 73.0, c2w[:3, :4])
    sel = torch.randperm(48 * 64, generator=torch.Generator().manual_seed(3))[:37]
    o, d = ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous()
    rows = orc.pack_ray_rows(o, d, 0., 2.5, syn.HIST_IDX)
    e = 0.
    for Nc, Ni in ((8, 16), (64, 128)):
        with torch.no_grad():
            ref = orc.render_rays(rows, c, f, T(ea), T(et), Nc, Ni)
        for retraw in (False, True):
            r = E.render_rays(o.to("cuda:0"), d.to("cuda:0"), hist, Nc, Ni, 0., 2.5, retraw=retraw, precision="f16x3")
            e = max(e, relmax(r[0], ref["rgb_map"]), relmax(r[1], ref["disp_map"]), relmax(r[2], ref["acc_map"]))
    return e

def grade():
    E3 = eng.NerfHEngine(precision="f16x3").load_numpy(cw, fw, ea, et)
    return bench.fp32_grade_check(E3, torch.device("cuda:0"), n=2048)

def g15():
    tw = np.load("tests/golden/trained_nerfh_weights.npz")
    Et = eng.NerfHEngine().load_numpy({k[7:]: tw[k] for k in tw.files if k.startswith("coarse.")},
                                      {k[5:]: tw[k] for k in tw.files if k.startswith("fine.")},
                                      tw["embedding_a.weight"], tw["embedding_t.weight"])
    t._trained_weights_render_vs_reference(Et, golden, "f16x3", 2e-5, False)
    return "ok"

def guard():
    for gain in (1.6, 3.0, 6.0, 16.0):
        t.test_range_guard_parity_or_loud_error(gain)
    return "ok"

for name, fn in (("g7", g7), ("fused", fused), ("g6", g6), ("ragged", ragged), ("grade", grade), ("g15", g15), ("guard", guard)):
    run(name, fn)
print("RESULT " + json.dumps(out))
'''


@pytest.fixture(scope="module", params=[4, 0], ids=["variant4", "variant0"])
def checks(request):
    env = dict(os.environ, DFN_MLP_VARIANT=str(request.param), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [x for x in out.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def _value(checks, name):
    v = checks[name]
    assert not (isinstance(v, dict) and "error" in v), v.get("error") if isinstance(v, dict) else v
    return v


def test_g7_golden_render(checks):
    assert _value(checks, "g7") < 2e-5


def test_fused_compositing_matches_retraw(checks):
    assert _value(checks, "fused") < 2e-6


def test_g6_configs(checks):
    """8+16 samples (segments not fused) and 64+128, raw included"""
    assert _value(checks, "g6") < 2e-5


def test_ray_count_off_the_tile(checks):
    assert _value(checks, "ragged") < 2e-5


def test_raw_is_fp32_grade(checks):
    """fine-network raw against the exact-fp32 kernel on the same samples, at test_split_f16_raw_outputs_are_fp32_grade's bounds"""
    rec = _value(checks, "grade")
    assert rec["raw_max_rel_f16x3_vs_f32"] < 5e-7, rec
    assert rec["raw_rms_rel_f16x3_vs_f32"] < 1.5e-7, rec


def test_trained_weights_goldens(checks):
    assert _value(checks, "g15") == "ok"


def test_range_guard_parity_or_loud_error(checks):
    assert _value(checks, "guard") == "ok"
