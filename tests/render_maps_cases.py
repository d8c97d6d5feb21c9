"""Shared by tests/test_gpu_render_maps.py and the child processes it starts (DFN_MLP_VARIANT is latched per process): the oracle's
values of the five render maps and the comparison of one engine against them on the G6 a/b rays and the G7 image.

Expected values come from the unedited oracle (oracle/nerfh_oracle.py, pinned to the reference by G4 / G6):
  depth_static, beta  composite_fine(raw, z)                              rendering.py:218-228, :204-208
  depth               composite_fine(raw, z, test_time=False)["depth"]    rendering.py:241
  rgb_static          composite_fine on raw with channel 7 (sigma_t) zeroed: a = a_s, T = T_s, the transient term vanishes
  rgb_transient       composite_fine on raw with channels 0..2 (c_s) zeroed: the static term vanishes
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import nerfh_oracle as orc  # noqa: E402

T = torch.from_numpy
DEV = "cuda:0"
MAPS = ("depth", "depth_static", "beta", "rgb_static", "rgb_transient")
# the project's per-mode bounds of these fixtures (tests/test_gpu_nerfh.py::test_render_rays_golden / test_render_image_golden)
TOL = {"f32": 2e-5, "f16x3": 2e-5, "f16": 1e-3}


def relmax(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert not torch.isnan(a).any()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def dev(x):
    return torch.as_tensor(x).float().to(DEV).contiguous()


def oracle_maps(raw, z):
    """The five maps of raw [n,Nf,9], z [n,Nf] by the oracle's compositor alone (module docstring)."""
    raw, z = torch.as_tensor(raw), torch.as_tensor(z)
    base = orc.composite_fine(raw, z)
    no_t, no_s = raw.clone(), raw.clone()
    no_t[..., 7] = 0
    no_s[..., 0:3] = 0
    return dict(depth=orc.composite_fine(raw, z, test_time=False)["depth"], depth_static=base["depth"], beta=base["beta"],
                rgb_static=orc.composite_fine(no_t, z)["rgb"], rgb_transient=orc.composite_fine(no_s, z)["rgb"],
                rgb=base["rgb"], disp=base["disp"], acc=base["acc"])


def oracle_render_maps(rows, w, Nc, Ni):
    """Whole path through the oracle: rows (orc.pack_ray_rows), w = (coarse, fine, emb_a, emb_t) as tensors."""
    st = {}
    with torch.no_grad():
        orc.render_rays(rows, *w, Nc, Ni, stages=st)
        return oracle_maps(st["raw"], st["z_fine"])


def golden(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))


def fixture_cases():
    """{tag: (golden dict, oracle rows)} of the G6 a/b rays and the G7 image."""
    out = {}
    for tag in "ab":
        g = golden("g6_render_rays_" + tag)
        out["g6" + tag] = (g, orc.pack_ray_rows(T(g["rays_o"]), T(g["rays_d"]), float(g["near"]), float(g["far"]), g["hist"]))
    g = golden("g7_render_image")
    ro, rd = orc.get_rays(int(g["H"]), int(g["W"]), float(g["focal"]), T(g["c2w"]).float()[:3, :4])
    out["g7"] = (g, orc.pack_ray_rows(ro.reshape(-1, 3), rd.reshape(-1, 3), float(g["near"]), float(g["far"]), g["hist"]))
    return out


def fixture_refs(w):
    """{tag: {map: tensor}} from the oracle, for weights w."""
    return {tag: oracle_render_maps(rows, w, int(g["Nc"]), int(g["Ni"])) for tag, (g, rows) in fixture_cases().items()}


def run_fixtures(E, prec, refs):
    """Render the three fixtures through the maps entries in `prec`: {"tag/map": relmax vs the oracle} and whether rgb / disp / acc
    are the plain entries' bits."""
    errs, same = {}, True
    for tag, (g, _) in fixture_cases().items():
        Nc, Ni, near, far = int(g["Nc"]), int(g["Ni"]), float(g["near"]), float(g["far"])
        if tag == "g7":
            H, W, focal = int(g["H"]), int(g["W"]), float(g["focal"])
            plain = [t.clone() for t in E.render_image(dev(g["c2w"]), H, W, focal, dev(g["hist"]), Nc, Ni, near, far, precision=prec)]
            rgb, disp, acc, _, mp = E.render_image_maps(dev(g["c2w"]), H, W, focal, dev(g["hist"]), Nc, Ni, near, far, precision=prec)
            assert mp["depth"].shape == (H, W) and mp["rgb_static"].shape == (H, W, 3)
            mp = {k: v.reshape(H * W, *v.shape[2:]) for k, v in mp.items()}
        else:
            args = (dev(g["rays_o"]), dev(g["rays_d"]), dev(g["hist"]), Nc, Ni, near, far)
            plain = [t.clone() for t in E.render_rays(*args, precision=prec)[:3]]
            rgb, disp, acc, raw, mp = E.render_rays_maps(*args, precision=prec)
            assert raw is None
        same = same and all(torch.equal(a, b) for a, b in zip(plain, (rgb, disp, acc)))
        assert set(mp) == set(MAPS)
        for k in MAPS:
            errs[f"{tag}/{k}"] = relmax(mp[k], refs[tag][k])
    return errs, same


if __name__ == "__main__":
    # child of test_fixture_maps_per_variant: python tests/render_maps_cases.py <refs.pt> <precision>...; prints one JSON line
    from dfnet_amd import engine as eng, synthetic as syn
    refs = torch.load(sys.argv[1])
    E = eng.NerfHEngine().load_numpy(*syn.nerfh_weights(0))
    res = {}
    for prec in sys.argv[2:]:
        errs, same = run_fixtures(E, prec, refs)
        res[prec] = dict(errs=errs, same=same)
    print("MAPS_JSON " + json.dumps(res))
