"""Render maps (depth, depth_static, beta, rgb_static, rgb_transient: models/rendering.py:196-241) on the GPU: the stage on its own, the
fused and the non-fused routes of the whole path at every arithmetic mode and netwidth, the properties of a full frame, and
render(ret_maps=...).  Expected values come from the unedited oracle (tests/render_maps_cases.py)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dfnet_amd import _lib, engine as eng, nerfw, rendering
from dfnet_amd import synthetic as syn
from oracle import nerfh_oracle as orc
from tests import render_maps_cases as rc
from tests.render_maps_cases import MAPS, TOL, dev, relmax

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = rc.DEV
ROOT = rc.ROOT


def tt(d):
    return {k: T(v) for k, v in d.items()}


def weights(seed=0, W=128):
    cw, fw, ea, et = syn.nerfh_weights(seed, W=W)
    return (cw, fw, ea, et), (tt(cw), tt(fw), T(ea), T(et))


@pytest.fixture(scope="module")
def scene():
    raw_w, w = weights()
    return eng.NerfHEngine().load_numpy(*raw_w), w


@pytest.fixture(scope="module")
def refs(scene):
    return rc.fixture_refs(scene[1])


def kwargs(E, Nc, Ni, **over):
    kw = dict(network_query_fn=nerfw.HipQuery(E, 65536), perturb=False, N_importance=Ni, N_samples=Nc, use_viewdirs=True,
              white_bkgd=False, raw_noise_std=0., test_time=True, ndc=False, lindisp=False)
    kw.update(over)
    return kw


# ---------------------------------------------------------------------------------------------- 1. the stage
def test_stage_on_the_composite_fixture(gold):
    """dfn_composite_fine_maps on G4's raw, z against the oracle; 3e-6 is test_composite_golden_all_modes' bound for this kernel family."""
    g = gold("g4_composite")
    ref = rc.oracle_maps(T(g["raw"]), T(g["z"]))
    got = eng.composite_fine_maps(dev(g["raw"]), dev(g["z"]))
    assert set(got) == set(MAPS)
    # the three maps the reference itself recorded in G4
    assert relmax(got["depth_static"], g["depth"]) < 3e-6 and relmax(got["depth"], g["train_depth"]) < 3e-6 and relmax(got["beta"], g["beta"]) < 3e-6
    errs = {k: relmax(got[k], ref[k]) for k in MAPS}
    print(f"stage vs oracle: {errs}")
    assert max(errs.values()) < 3e-6, errs
    # a subset writes the same bits, and only what was asked for
    sub = eng.composite_fine_maps(dev(g["raw"]), dev(g["z"]), maps=("beta", "rgb_transient"))
    assert set(sub) == {"beta", "rgb_transient"} and all(torch.equal(sub[k], got[k]) for k in sub)


# ---------------------------------------------------------------------------------------------- 2. whole path, netwidth 128
@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16"])
def test_fixture_maps_vs_oracle(scene, refs, prec):
    """G6 a/b rays and the G7 image through render_rays_maps / render_image_maps (the process's kernel variant: split-f16 on 16x16x32
    MFMAs by default) under the per-mode bounds of test_render_rays_golden / test_render_image_golden; rgb / disp / acc are the plain
    entries' bits."""
    errs, same = rc.run_fixtures(scene[0], prec, refs)
    print(f"{prec}: {errs}")
    assert same, "rgb / disp / acc of the maps entries differ from the plain entries'"
    assert max(errs.values()) < TOL[prec], errs


@pytest.mark.parametrize("variant,precs", [(0, ("f16x3", "f16", "f32")), (4, ("f16x3",)), (1, ("f16",)), (3, ("f16", "f16x3"))])
def test_fixture_maps_per_variant(refs, tmp_path, variant, precs):
    """The maps flavour of every fine-kernel variant that composites in-kernel (DFN_MLP_VARIANT is latched per process: one child each)."""
    path = str(tmp_path / "refs.pt")
    torch.save(refs, path)
    env = dict(os.environ, DFN_MLP_VARIANT=str(variant), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "render_maps_cases.py"), path, *precs], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.split("MAPS_JSON")[-1])
    for prec in precs:
        print(f"variant {variant} {prec}: {res[prec]['errs']}")
        assert res[prec]["same"], (variant, prec)
        assert max(res[prec]["errs"].values()) < TOL[prec], (variant, prec, res[prec]["errs"])


# ---------------------------------------------------------------------------------------------- 3. the non-fused routes
@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16"])
def test_retraw_route_equals_fused_route(scene, prec):
    """The same rays with and without retraw: the maps of composite_fine_maps on the raw in HBM against those of the fused epilogue,
    under the fused = separate bound the project holds for rgb (2e-6, test_fused_compositing_matches_separate_compositor)."""
    E = scene[0]
    o, d, _ = eng.raygen(96, 128, 146.0, T(syn.orbit_pose(3, 8)).to(DEV))
    args = (o.reshape(-1, 3), d.reshape(-1, 3), dev(syn.HIST_IDX), 64, 128, 0., 2.5)
    a = E.render_rays_maps(*args, precision=prec)
    b = E.render_rays_maps(*args, retraw=True, precision=prec)
    assert a[3] is None and b[3] is not None
    errs = {k: relmax(a[4][k], b[4][k]) for k in MAPS}
    print(f"{prec} fused vs retraw: {errs}")
    assert max(errs.values()) < 2e-6, errs
    plain = E.render_rays(*args, retraw=True, precision=prec)
    assert all(torch.equal(x, y) for x, y in zip(plain, b[:4]))


def test_segment_misfit_route_vs_oracle(scene):
    """64 + 100 samples (164 is no multiple of a 32-sample segment): the separate compositor runs on the workspace's raw.  There is no
    fused render of these samples to compare with, so the reference is the oracle under the whole-path bound of the fp32-grade modes
    (2e-5), the maps must tie in with the plain outputs (disp = 1 / max(1e-10, depth_static / acc)), and the two non-fused routes
    (raw in the workspace, raw returned) run the same compositor on the same raw: the same bits."""
    E, w = scene
    o, d, _ = eng.raygen(12, 16, 14.6, T(syn.orbit_pose(3, 8)).to(DEV))
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    ref = rc.oracle_render_maps(orc.pack_ray_rows(o.cpu(), d.cpu(), 0., 2.5, syn.HIST_IDX), w, 64, 100)
    for prec in ("f32", "f16x3"):
        rgb, disp, acc, raw, mp = E.render_rays_maps(o, d, dev(syn.HIST_IDX), 64, 100, 0., 2.5, precision=prec)
        errs = {k: relmax(mp[k], ref[k]) for k in MAPS}
        print(f"{prec} 64+100 vs oracle: {errs}")
        assert raw is None and max(errs.values()) < 2e-5, errs
        torch.testing.assert_close(disp, 1. / torch.clamp(mp["depth_static"] / acc, min=1e-10), rtol=1e-6, atol=0)
        assert all(torch.equal(x, y) for x, y in zip(E.render_rays(o, d, dev(syn.HIST_IDX), 64, 100, 0., 2.5, precision=prec)[:3], (rgb, disp, acc)))
        kept = {k: v.clone() for k, v in mp.items()}
        with_raw = E.render_rays_maps(o, d, dev(syn.HIST_IDX), 64, 100, 0., 2.5, retraw=True, precision=prec)
        assert with_raw[3] is not None and all(torch.equal(with_raw[4][k], kept[k]) for k in MAPS)


@pytest.mark.parametrize("width", [256, 32])
def test_other_netwidths_vs_oracle(width):
    """netwidth 256 (register-resident kernels, separate compositor) and 32 (generic path) against the oracle under the bound
    tests/test_gpu_generic_surface.py holds for rgb at those widths (3e-5), with that file's weights (seed 4) and ray batch."""
    raw_w, w = weights(4, W=width)
    E = eng.NerfHEngine(width=width, precision="f32").load_numpy(*raw_w)
    rng = np.random.default_rng(11)
    ro, rd = orc.get_rays(480, 640, 585.0, T(syn.orbit_pose(3, 8))[:3, :4])
    sel = rng.choice(480 * 640, 150, replace=False)
    o, d = ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous()
    hist = T(rng.integers(0, 40, (150, 10)).astype(np.float32))
    view = d / torch.norm(d, dim=-1, keepdim=True)
    rows = torch.cat([o, d, torch.full((150, 1), 0.), torch.full((150, 1), 2.5), view, hist], 1)
    ref = rc.oracle_render_maps(rows, w, 16, 32)
    rgb, disp, acc, raw, mp = E.render_rays_maps(dev(o), dev(d), dev(hist), 16, 32, 0., 2.5)
    errs = {k: relmax(mp[k], ref[k]) for k in MAPS}
    errs.update(rgb=relmax(rgb, ref["rgb"]), disp=relmax(disp, ref["disp"]))
    print(f"netwidth {width} vs oracle: {errs}")
    assert max(errs.values()) < 3e-5, errs
    plain = E.render_rays(dev(o), dev(d), dev(hist), 16, 32, 0., 2.5)
    assert all(torch.equal(x, y) for x, y in zip(plain[:3], (rgb, disp, acc)))
    if width == 32:   # the generic path in chunks: the same bits as one pass
        E.GENERIC_CHUNK, keep = 64, E.GENERIC_CHUNK
        try:
            chunked = E.render_rays_maps(dev(o), dev(d), dev(hist), 16, 32, 0., 2.5, retraw=True)
        finally:
            E.GENERIC_CHUNK = keep
        assert chunked[3].shape == (150, 48, 9) and all(torch.equal(chunked[4][k], mp[k]) for k in MAPS)


# ---------------------------------------------------------------------------------------------- 4. a full frame
def _raw_call(E, maps_struct, c2w, H, W, focal, hist, Nc, Ni, near, far, new):
    """dfn_render_image / dfn_render_image_maps straight through ctypes."""
    lib = E.lib
    out = (torch.empty(H, W, 3, device=DEV), torch.empty(H, W, device=DEV), torch.empty(H, W, device=DEV))
    ws = torch.empty(lib.dfn_render_maps_workspace_bytes(H * W, Nc, Ni), dtype=torch.uint8, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    head = (E.handle, _lib.PRECISIONS[E.precision], vp(c2w), H, W, focal, near, far, Nc, Ni, vp(hist), *[vp(t) for t in out], vp(ws), ws.numel())
    if new:
        _lib.check(lib.dfn_render_image_maps(*head, maps_struct, _lib.current_stream()), "dfn_render_image_maps")
    else:
        _lib.check(lib.dfn_render_image(*head, _lib.current_stream()), "dfn_render_image")
    torch.cuda.synchronize()
    return out


def test_full_frame_properties(scene):
    """640 x 480, 64 + 128, the scene of tests/test_gpu_nerfh.py::test_full_frame_properties."""
    E = scene[0]
    H, W, focal, near, far = 480, 640, 585.0, 0., 2.5
    c2w = T(syn.orbit_pose(1, 8)).to(DEV)
    hist = dev(syn.HIST_IDX)
    first = E.render_image_maps(c2w, H, W, focal, hist, 64, 128, near, far)
    rgb, disp, acc, mp = first[0].clone(), first[1].clone(), first[2].clone(), {k: v.clone() for k, v in first[4].items()}
    again = E.render_image_maps(c2w, H, W, focal, hist, 64, 128, near, far)
    assert torch.equal(rgb, again[0]) and torch.equal(disp, again[1]) and torch.equal(acc, again[2])   # idempotent, bit for bit
    assert all(torch.equal(mp[k], again[4][k]) for k in MAPS)
    plain = E.render_image(c2w, H, W, focal, hist, 64, 128, near, far)
    assert torch.equal(rgb, plain[0]) and torch.equal(disp, plain[1]) and torch.equal(acc, plain[2])
    # rays are independent: a 5000-ray subset rendered alone gives the same bits for every map
    o, d, _ = eng.raygen(H, W, focal, c2w)
    sel = torch.randperm(H * W, generator=torch.Generator().manual_seed(0))[:5000].to(DEV)
    sub = E.render_rays_maps(o.reshape(-1, 3)[sel], d.reshape(-1, 3)[sel], hist, 64, 128, near, far)
    assert torch.equal(sub[0], rgb.reshape(-1, 3)[sel])
    for k in MAPS:
        assert torch.equal(sub[4][k], mp[k].reshape(H * W, *mp[k].shape[2:])[sel]), k
    # any subset of the maps gives the bits of asking for all five
    for names in (("depth",), ("rgb_static",), ("beta", "rgb_transient"), ("depth_static", "depth", "rgb_static", "rgb_transient")):
        part = E.render_image_maps(c2w, H, W, focal, hist, 64, 128, near, far, maps=names)
        assert set(part[4]) == set(names) and torch.equal(part[0], rgb) and torch.equal(part[1], disp)
        assert all(torch.equal(part[4][k], mp[k]) for k in names), names
    # five NULLs and a NULL struct are the old entry
    c3 = c2w[:3, :4].contiguous()
    old = _raw_call(E, None, c3, H, W, focal, hist, 64, 128, near, far, new=False)
    for st in (None, ctypes.byref(_lib.RenderMaps())):
        new = _raw_call(E, st, c3, H, W, focal, hist, 64, 128, near, far, new=True)
        assert all(torch.equal(a, b) for a, b in zip(old, new))
    assert all(torch.equal(a, b) for a, b in zip(old, (rgb, disp, acc)))
    # ranges
    assert all(bool(torch.isfinite(v).all()) for v in mp.values())
    assert float(mp["rgb_static"].min()) >= 0 and float(mp["rgb_static"].max()) <= 1 + 1e-5
    assert float(mp["rgb_transient"].min()) >= 0
    assert float(mp["depth"].max()) <= far * (1 + 1e-5) and float(mp["depth"].min()) >= 0
    assert float(mp["beta"].min()) >= 0.1
    torch.testing.assert_close(disp, 1. / torch.clamp(mp["depth_static"] / acc, min=1e-10), rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------- 5. the maps are not aliases
def _alias_gaps(r):
    """How far the oracle's maps are from the maps they could be mistaken for, normalised as relmax normalises."""
    return {"rgb_static - rgb": float((r["rgb_static"] - r["rgb"]).abs().max() / r["rgb_static"].abs().max()),
            "rgb_transient": float(r["rgb_transient"].abs().max() / r["rgb"].abs().max()),   # against zero, on the scale of rgb
            "depth - depth_static": float((r["depth"] - r["depth_static"]).abs().max() / r["depth"].abs().max())}


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_maps_are_not_aliases_on_the_fixtures(refs, prec):
    """From the oracle's values alone: on the fixtures of test 2 the static colour differs from the joint one, the transient colour from
    zero and the joint depth from the static one by more than 100 x the mode's tolerance, so a kernel that returned one map for another
    could not pass test 2.  Oracle figures (G6 a / G6 b / G7): rgb_static - rgb 0.082 / 0.047 / 0.048, depth - depth_static 0.77 / 0.71 /
    0.71 against 100 x 2e-5.  Against plain f16's 100 x 1e-3 the static-colour figure of these fixtures is too small (47 x .. 82 x the
    tolerance): f16 has a sharper fixture of its own below."""
    for tag, r in refs.items():
        gaps = _alias_gaps(r)
        print(f"{tag}: {gaps}")
        assert min(gaps.values()) > 100 * TOL[prec], (tag, gaps)


def test_f16_maps_on_a_sharper_scene_and_not_aliases():
    """Plain f16 on a fixture whose maps differ by more than 100 x its tolerance: the G6-b rays through the weights of seed 0 with
    every matrix x 2 (syn.nerfh_weights(0, gain=2.0); oracle: rgb_static - rgb 0.128, depth - depth_static 0.60 of the map's largest
    value, against 100 x 1e-3), held to the same 1e-3 against the oracle, the range guard clean."""
    g = rc.golden("g6_render_rays_b")
    cw, fw, ea, et = syn.nerfh_weights(0, gain=2.0)
    rows = orc.pack_ray_rows(T(g["rays_o"]), T(g["rays_d"]), float(g["near"]), float(g["far"]), g["hist"])
    ref = rc.oracle_render_maps(rows, (tt(cw), tt(fw), T(ea), T(et)), 64, 128)
    gaps = _alias_gaps(ref)
    print(f"gain 2.0: {gaps}")
    assert min(gaps.values()) > 100 * TOL["f16"], gaps
    E = eng.NerfHEngine().load_numpy(cw, fw, ea, et)
    E.range_flags()
    rgb, disp, acc, _, mp = E.render_rays_maps(dev(g["rays_o"]), dev(g["rays_d"]), dev(g["hist"]), 64, 128, 0., 2.5, precision="f16")
    assert E.range_flags() == 0
    errs = {k: relmax(mp[k], ref[k]) for k in MAPS}
    print(f"gain 2.0 f16 vs oracle: {errs}")
    assert max(errs.values()) < TOL["f16"], errs


# ---------------------------------------------------------------------------------------------- 6. render(ret_maps=...)
def test_render_keyword_on_every_test_time_branch(gold):
    """Keys, shapes and values (split-f16 engine: the fp32-grade whole-path bound, 2e-5) on the c2w, rays, c2w_staticcam and ndc
    branches with and without retraw; what the keyword refuses; and the extras of a call without it."""
    raw_w, w = weights()
    E = eng.NerfHEngine(precision="f16x3").load_numpy(*raw_w)
    g = gold("g14_render_ndc_staticcam")
    H, W, focal, Nc, Ni = int(g["H"]), int(g["W"]), float(g["focal"]), int(g["Nc"]), int(g["Ni"])
    c2w, static, hist = T(g["c2w"]).float(), T(g["c2w_staticcam"]).float(), np.asarray(g["hist"], dtype=np.float32)
    ro, rd = orc.get_rays(H, W, focal, c2w[:3, :4])
    view = rd.reshape(-1, 3) / torch.norm(rd.reshape(-1, 3), dim=-1, keepdim=True)

    def ref_of(o, d, near, far):
        rows = orc.pack_ray_rows(o.reshape(-1, 3), d.reshape(-1, 3), near, far, hist)
        rows[:, 8:11] = view
        return rc.oracle_render_maps(rows, w, Nc, Ni)

    def check(got, ref, names, lead, retraw):
        extras = got[3]
        assert set(extras) == set(names) | ({"raw"} if retraw else set())
        for k in names:
            assert extras[k].shape == tuple(lead) + ((3,) if k.startswith("rgb_") else ()), (k, extras[k].shape)
            assert relmax(extras[k].reshape(ref[k].shape), ref[k]) < 2e-5, k
        assert relmax(got[0].reshape(-1, 3), ref["rgb"]) < 2e-5
        if retraw:
            assert extras["raw"].shape == tuple(lead) + (Nc + Ni, 9)

    with torch.no_grad():
        base = ref_of(ro, rd, 0., 2.5)
        for retraw in (False, True):
            kw = kwargs(E, Nc, Ni, retraw=retraw)
            # c2w: [H,W] / [H,W,3]
            got = rendering.render(H, W, focal, c2w=dev(c2w), near=0., far=2.5, img_idx=dev(hist)[None], ret_maps=True, **kw)
            check(got, base, MAPS, (H, W), retraw)
            # rays with a leading shape of their own, a subset of the maps
            rays = (dev(ro).reshape(2, H * W // 2, 3), dev(rd).reshape(2, H * W // 2, 3))
            got = rendering.render(H, W, focal, rays=rays, near=0., far=2.5, img_idx=dev(hist)[None], ret_maps=("depth", "rgb_static"), **kw)
            check(got, base, ("depth", "rgb_static"), (2, H * W // 2), retraw)
            # c2w_staticcam
            so, sd = orc.get_rays(H, W, focal, static[:3, :4])
            got = rendering.render(H, W, focal, c2w=dev(c2w), c2w_staticcam=dev(static), near=0., far=2.5, img_idx=dev(hist)[None],
                                   ret_maps=True, **kw)
            check(got, ref_of(so, sd, 0., 2.5), MAPS, (H, W), retraw)
            # ndc
            no, nd = orc.ndc_rays(H, W, focal, 1., ro, rd)
            got = rendering.render(H, W, focal, c2w=dev(c2w), near=0., far=1., img_idx=dev(hist)[None], ret_maps=["beta"],
                                   **kwargs(E, Nc, Ni, retraw=retraw, ndc=True))
            check(got, ref_of(no, nd, 0., 1.), ("beta",), (H, W), retraw)
        # without the keyword: exactly the extras of today
        kw = kwargs(E, Nc, Ni)
        assert rendering.render(H, W, focal, c2w=dev(c2w), near=0., far=2.5, img_idx=dev(hist)[None], **kw)[3] == {}
        assert rendering.render(H, W, focal, c2w=dev(c2w), near=0., far=2.5, img_idx=dev(hist)[None], ret_maps=False, **kw)[3] == {}
        assert set(rendering.render(H, W, focal, rays=(dev(ro), dev(rd)), near=0., far=2.5, img_idx=dev(hist)[None],
                                    **kwargs(E, Nc, Ni, retraw=True))[3]) == {"raw"}
        with pytest.raises(ValueError, match="unknown render map"):
            rendering.render(H, W, focal, c2w=dev(c2w), near=0., far=2.5, img_idx=dev(hist)[None], ret_maps=("depht",), **kw)
    # the maps are not differentiable: a tracked pose, tracked rays and training kwargs are refused by name
    pose = dev(c2w)[:3, :4].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="ret_maps"):
        rendering.render(H, W, focal, c2w=pose, near=0., far=2.5, img_idx=dev(hist)[None], ret_maps=True, **kwargs(E, Nc, Ni))
    rays = torch.stack([dev(ro), dev(rd)]).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="ret_maps"):
        rendering.render(H, W, focal, rays=rays, near=0., far=2.5, img_idx=dev(hist)[None], ret_maps=("depth",), **kwargs(E, Nc, Ni))
    q = nerfw.HipQuery(E, 65536)
    q.trainer = object()   # training kwargs: refused before the trainer is touched
    with pytest.raises(NotImplementedError, match="ret_maps"):
        rendering.render(H, W, focal, c2w=dev(c2w), near=0., far=2.5, img_idx=dev(hist)[None], ret_maps=True,
                         **kwargs(E, Nc, Ni, network_query_fn=q, test_time=False, perturb=1.))
