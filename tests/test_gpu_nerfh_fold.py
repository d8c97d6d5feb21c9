"""Kernel variant 5: variant 4 (split-f16 on 16x16x32 MFMAs) with xyz_encoding_final folded at commit into dir_encoding.0 and
transient_encoding.0 (nerfh_layout.h: kFineFoldSeq; nerfh_mlp_fold.hip).  The variant is latched per process (DFN_MLP_VARIANT), so
each variant runs in a child:

  * variant 5 through the checks and bounds variant 4 is held to (the CHILD program of tests/test_gpu_nerfh_mfma16.py, imported);
  * plumbing: with xyz_encoding_final = (identity, 0) the folded matrices ARE dir_encoding.0[:, :128] / transient_encoding.0[:, :128]
    and `final` is h8 bit for bit (1 x (hi + lo) is exact in fp32 and splits back into the same hi, lo), so the two variants multiply
    the same operands in the same K order: raw, rgb, disp and acc must be the same bits;
  * bias fold: the same identity with a seeded non-zero bias (|b| <= 0.5), where variant 4 adds b to h8 and variant 5 adds
    W[:, :128] b to the per-ray seeds: variant 5 must sit within 1.5 x variant 4's own distance from the oracle + 1e-7;
  * maps: a maps render's rgb / disp / acc are the plain render's bits and the five maps hold variant 4's bound against the oracle.

This file is also the child of its own plumbing / bias-fold tests: python tests/test_gpu_nerfh_fold.py <out.pt>.
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
BIAS_SEED = 11


def fold_weights(bias_seed=None):
    """The synthetic scene (seed 0) with fine.xyz_encoding_final = (identity, 0 or a seeded bias in [-0.5, 0.5])."""
    cw, fw, ea, et = syn.nerfh_weights(0)
    fw = dict(fw)
    fw["xyz_encoding_final.weight"] = np.eye(128, dtype=np.float32)
    b = np.zeros(128, np.float32) if bias_seed is None else np.random.default_rng(bias_seed).uniform(-0.5, 0.5, 128).astype(np.float32)
    fw["xyz_encoding_final.bias"] = b
    return cw, fw, ea, et


def ray_cases():
    """{tag: (o, d, hist, Nc, Ni)}: 37 rays at 8 + 16 (888 points: no multiple of the 256-point tile, separate compositor) with the
    shared histogram, and 64 rays at 64 + 128 (48 tiles, fused compositing) with a histogram per ray."""
    ro, rd = orc.get_rays(48, 64, 73.0, T(syn.orbit_pose(2, 8))[:3, :4])
    sel = torch.randperm(48 * 64, generator=torch.Generator().manual_seed(3))
    pick = lambda s: (ro.reshape(-1, 3)[s].contiguous(), rd.reshape(-1, 3)[s].contiguous())
    hist64 = T(np.random.default_rng(5).integers(0, 40, (64, 10)).astype(np.float32))
    return {"r37": (*pick(sel[:37]), T(np.asarray(syn.HIST_IDX, dtype=np.float32)), 8, 16),
            "r64": (*pick(sel[100:164]), hist64, 64, 128)}


def child(out_path):
    """Render both cases with both weight sets in this process's variant: {"plumb/r37": {raw, rgb, disp, acc, fused_*}, ...}."""
    from dfnet_amd import engine as eng
    res = {}
    for wtag, seed in (("plumb", None), ("bias", BIAS_SEED)):
        E = eng.NerfHEngine(precision="f16x3").load_numpy(*fold_weights(seed))
        for tag, (o, d, hist, Nc, Ni) in ray_cases().items():
            args = (o.to("cuda:0"), d.to("cuda:0"), hist.to("cuda:0"), Nc, Ni, 0., 2.5)
            rgb, disp, acc, raw = E.render_rays(*args, retraw=True)
            rec = dict(raw=raw.cpu(), rgb=rgb.cpu(), disp=disp.cpu(), acc=acc.cpu())
            f = E.render_rays(*args)   # 64 + 128: compositing fused into the fine kernel
            assert f[3] is None
            rec.update(fused_rgb=f[0].cpu(), fused_disp=f[1].cpu(), fused_acc=f[2].cpu())
            res[f"{wtag}/{tag}"] = rec
        assert E.range_flags() == 0
    torch.save(res, out_path)


if __name__ == "__main__":
    child(sys.argv[1])
    sys.exit(0)

import pytest  # noqa: E402

from tests import test_gpu_nerfh_mfma16 as m16  # noqa: E402
from tests import render_maps_cases as rc  # noqa: E402

gpu = pytest.mark.gpu   # per test: the oracle-only check at the end runs without a GPU
KEYS = ("raw", "rgb", "disp", "acc", "fused_rgb", "fused_disp", "fused_acc")


def _run(variant, *argv, code=None):
    env = dict(os.environ, DFN_MLP_VARIANT=str(variant), PYTHONPATH=ROOT)
    cmd = [sys.executable, "-c", code] if code else [sys.executable, *argv]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    if out.returncode < 0 or out.returncode in (134, 137, 139):   # the child died on the GPU: nothing more is started on it
        pytest.exit(f"variant {variant} child ended with status {out.returncode}: {out.stderr[-2000:]}", returncode=3)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


# ---------------------------------------------------------------------------------------------- variant 4's checks and bounds
@pytest.fixture(scope="module")
def checks():
    line = [x for x in _run(5, code=m16.CHILD).splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@gpu
def test_g7_golden_render(checks):
    assert m16._value(checks, "g7") < 2e-5


@gpu
def test_fused_compositing_matches_retraw(checks):
    assert m16._value(checks, "fused") < 2e-6


@gpu
def test_g6_configs(checks):
    assert m16._value(checks, "g6") < 2e-5


@gpu
def test_ray_count_off_the_tile(checks):
    assert m16._value(checks, "ragged") < 2e-5


@gpu
def test_raw_is_fp32_grade(checks):
    rec = m16._value(checks, "grade")
    print(f"variant 5 raw vs the exact-fp32 kernel: {rec}")
    assert rec["raw_max_rel_f16x3_vs_f32"] < 5e-7, rec
    assert rec["raw_rms_rel_f16x3_vs_f32"] < 1.5e-7, rec


@gpu
def test_trained_weights_goldens(checks):
    assert m16._value(checks, "g15") == "ok"


@gpu
def test_range_guard_parity_or_loud_error(checks):
    assert m16._value(checks, "guard") == "ok"


# ---------------------------------------------------------------------------------------------- plumbing and bias fold
@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """The child's renders under variants 4 and 5."""
    out = {}
    for variant in (4, 5):
        path = str(tmp_path_factory.mktemp("fold") / f"v{variant}.pt")
        _run(variant, os.path.abspath(__file__), path)
        out[variant] = torch.load(path)
    return out


@gpu
@pytest.mark.parametrize("tag", ["r37", "r64"])
def test_identity_final_is_bit_identical(pair, tag):
    a, b = pair[4]["plumb/" + tag], pair[5]["plumb/" + tag]
    for k in KEYS:
        diff = float((a[k].double() - b[k].double()).abs().max())
        print(f"{tag} {k}: max |variant 5 - variant 4| = {diff:.3e}")
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert float(a["raw"].abs().max()) > 0 and bool(torch.isfinite(a["raw"]).all())


def _oracle(wts, case, dtype):
    cw, fw, ea, et = wts
    o, d, hist, Nc, Ni = case
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.no_grad():
            tt = lambda dct: {k: T(v).to(dtype) for k, v in dct.items()}
            rows = orc.pack_ray_rows(o.to(dtype), d.to(dtype), 0., 2.5, hist.to(dtype))
            st = {}
            r = orc.render_rays(rows, tt(cw), tt(fw), T(ea).to(dtype), T(et).to(dtype), Nc, Ni, stages=st)
    finally:
        torch.set_default_dtype(prev)
    return dict(raw=st["raw"], rgb=r["rgb_map"], disp=r["disp_map"], acc=r["acc_map"])


def _dist(got, ref):
    """max over channels of max |delta| / max |channel| (raw: its 9 channels; rgb, disp, acc: the whole map)."""
    got, ref = got.double(), ref.double()
    if got.dim() == 3:
        return max(float((got[..., c] - ref[..., c]).abs().max() / ref[..., c].abs().max().clamp_min(1e-30)) for c in range(got.shape[-1]))
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def bias_refs():
    wts = fold_weights(BIAS_SEED)
    return {tag: _oracle(wts, case, torch.float32) for tag, case in ray_cases().items()}


@gpu
@pytest.mark.parametrize("tag", ["r37", "r64"])
def test_bias_fold_holds_variant4s_distance_to_the_oracle(pair, bias_refs, tag):
    """Variant 4 is the yardstick, not the code under test: err(variant 5) <= 1.5 x err(variant 4) + 1e-7 for raw, rgb, disp and acc
    (the form of tests/test_gpu_generic_surface.py::holds).  The oracle is well-conditioned on these inputs: its fp32 evaluation sits
    5e-7 .. 8e-7 (raw), 2e-7 .. 6e-7 (rgb, disp) from its float64 one (test_bias_fold_oracle_is_well_conditioned)."""
    ref, a, b = bias_refs[tag], pair[4]["bias/" + tag], pair[5]["bias/" + tag]
    bad = []
    for k in ("raw", "rgb", "disp", "acc"):
        e4, e5 = _dist(a[k], ref[k]), _dist(b[k], ref[k])
        print(f"{tag} {k}: variant 5 {e5:.3e} from the oracle, variant 4 {e4:.3e}")
        if not e5 <= 1.5 * e4 + 1e-7:
            bad.append((k, e5, e4))
    for k in ("rgb", "disp", "acc"):   # the fused compositor against the separate one, as for every variant
        assert _dist(b["fused_" + k], b[k]) < 2e-6, k
    assert not bad, bad
    assert float((a["raw"] - pair[4]["plumb/" + tag]["raw"]).abs().max()) > 1e-3   # the bias reaches the outputs
    # ... and by different roundings in the two variants (h8 + b against seeds + W b): the colour channels cannot agree bit for bit
    # everywhere unless variant 5 ran variant 4's kernel; static_sigma (channel 3) reads h8 alone and must
    differ = (a["raw"] != b["raw"]).reshape(-1, 9).sum(0).tolist()
    print(f"{tag}: raw elements that differ between the variants, per channel: {differ} of {a['raw'].numel() // 9}")
    assert differ[3] == 0 and sum(differ) > 0, differ


# ---------------------------------------------------------------------------------------------- maps
@gpu
def test_maps_flavour(tmp_path):
    """The G6 a/b rays and the G7 image (the smallest fused case) through the maps entries under variant 5, at variant 4's bound of
    tests/test_gpu_render_maps.py::test_fixture_maps_per_variant; rgb / disp / acc the plain entries' bits."""
    cw, fw, ea, et = syn.nerfh_weights(0)
    refs = rc.fixture_refs(({k: T(v) for k, v in cw.items()}, {k: T(v) for k, v in fw.items()}, T(ea), T(et)))
    path = str(tmp_path / "refs.pt")
    torch.save(refs, path)
    res = json.loads(_run(5, os.path.join(ROOT, "tests", "render_maps_cases.py"), path, "f16x3").split("MAPS_JSON")[-1])["f16x3"]
    print(f"variant 5 maps vs oracle: {res['errs']}")
    assert res["same"]
    assert max(res["errs"].values()) < rc.TOL["f16x3"], res["errs"]


# ---------------------------------------------------------------------------------------------- the oracle alone (no GPU)
def test_bias_fold_oracle_is_well_conditioned():
    """Fixed before any GPU run: on the bias-fold inputs the oracle's fp32 evaluation is its float64 one to fp32 round-off (measured:
    raw 5.3e-7 / 7.9e-7, rgb 1.9e-7 / 6.1e-7, disp 2.0e-7 / 5.5e-7, acc 1.2e-7 / 6.0e-8 for r37 / r64), far inside the project's
    whole-path bound for fp32-grade arithmetic (2e-5): no sample of these rays sits on a gate that a last-bit change would flip."""
    wts = fold_weights(BIAS_SEED)
    for tag, case in ray_cases().items():
        a, b = _oracle(wts, case, torch.float32), _oracle(wts, case, torch.float64)
        d = {k: _dist(a[k], b[k]) for k in a}
        print(f"{tag}: fp32 oracle vs float64 oracle {d}")
        assert max(d.values()) < 2e-5, (tag, d)
