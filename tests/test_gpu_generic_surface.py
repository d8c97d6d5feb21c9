"""The generic-width path (every netwidth other than 128; gradients at 256 too) under the whole render() surface:
render(retraw=True) under autograd — d L / d raw through dfn_nerfh_generic_render_rays_backward_raw — and explicit view directions
on the generic forward (dfn_nerfh_generic_render_rays_v), which test-time ndc / c2w_staticcam need (models/rendering.py:318-320,
353-400).  Every GPU call goes through the C ABI; the truth is the CPU oracle, for gradients in float64 (tests/yardstick.py)."""
import ctypes

import numpy as np
import pytest
import torch

from dfnet_amd import _lib, engine as eng, nerfw, rendering, synthetic as syn
from dfnet_amd._lib import current_stream, ptr
from oracle import nerfh_oracle as orc
from tests.yardstick import float64_default, rays_off_a_gate, rel_l2, to64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
NEAR, FAR = 0., 2.5


def relmax(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert not torch.isnan(a).any()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def dev(x):
    return torch.as_tensor(x).float().to(DEV).contiguous()


# ---------------------------------------------------------------------------------------------- the oracle half (runs without a GPU)
def weights(width, seed):
    cw, fw, ea, et = syn.nerfh_weights(seed, W=width)
    return (cw, fw, ea, et), ({k: T(v) for k, v in cw.items()}, {k: T(v) for k, v in fw.items()}, T(ea), T(et))


def ray_rows(o, d, hist, view=None):
    """The oracle's 21-float ray rows in the dtype of the rays (orc.pack_ray_rows casts to fp32; the float64 truth must not)."""
    n = o.shape[0]
    if view is None:
        view = d / torch.norm(d, dim=-1, keepdim=True)
    hist = hist.to(o.dtype).reshape(-1, hist.shape[-1])
    if hist.shape[0] != n:
        hist = hist.repeat(n, 1)
    return torch.cat([o, d, torch.full((n, 1), NEAR, dtype=o.dtype), torch.full((n, 1), FAR, dtype=o.dtype), view.to(o.dtype), hist], 1)


def oracle_render(o, d, hist, w, Nc, Ni, view=None):
    return orc.render_rays(ray_rows(o, d, hist, view), *w, Nc, Ni, retraw=True)


def oracle_loss(out, G, Gr):
    loss = 0.
    if G is not None:
        loss = loss + (out["rgb_map"] * G).sum()
    if Gr is not None:
        loss = loss + (out["raw"] * Gr).sum()
    return loss


def oracle_ray_grads(o, d, hist, w, Nc, Ni, G, Gr, f64=False):
    """(render outputs, d loss / d rays_o, d loss / d rays_d) by autograd through the oracle, in fp32 or float64."""
    if f64:
        with float64_default():
            return oracle_ray_grads(*to64((o, d, hist, w)), Nc, Ni, to64(G), to64(Gr))
    o, d = o.detach().clone().requires_grad_(True), d.detach().clone().requires_grad_(True)
    out = oracle_render(o, d, hist, w, Nc, Ni)
    oracle_loss(out, G, Gr).backward()
    return {k: v.detach() for k, v in out.items()}, o.grad, d.grad


def ray_batch(n, seed, pose=3):
    """n rays drawn from a 480 x 640 frame, one histogram vector per ray."""
    rng = np.random.default_rng(seed)
    ro, rd = orc.get_rays(480, 640, 585.0, T(syn.orbit_pose(pose, 8))[:3, :4])
    sel = rng.choice(480 * 640, n, replace=False)
    o, d = ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous()
    hist = T(rng.integers(0, 40, (n, 10)).astype(np.float32))
    return rng, o, d, hist


def ray_case(width, Nc=16, Ni=32, n=150):
    """Test 1's inputs: (numpy weights, oracle weights, o, d, hist, G, Gr)."""
    raw_w, w = weights(width, SEEDS[width])
    rng, o, d, hist = ray_batch(n, 11)
    G = T(rng.standard_normal((n, 3)).astype(np.float32))
    Gr = T((rng.standard_normal((n, Nc + Ni, 9)) / (Nc + Ni)).astype(np.float32))
    return raw_w, w, o, d, hist, G, Gr


def yardstick(got_o, got_d, o, d, hist, w, Nc, Ni, G, Gr):
    """The project's float64 criterion of a ray gradient (tests/test_gpu_train.py::test_generic_width_render_gradient_vs_oracle):
    returns dict(eo, ed, yo, yd, per_o, per_d, left_out) over the rays that rays_off_a_gate (default arguments) keeps."""
    _, ref_o, ref_d = oracle_ray_grads(o, d, hist, w, Nc, Ni, G, Gr)
    _, o64, d64 = oracle_ray_grads(o, d, hist, w, Nc, Ni, G, Gr, f64=True)
    w64, o_64, d_64, h64 = to64(w), to64(o), to64(d), to64(hist)

    def single64(i, delta):
        with float64_default():
            _, a, b = oracle_ray_grads(o_64[i:i + 1] + delta, d_64[i:i + 1], h64[i:i + 1], w64, Nc, Ni,
                                       None if G is None else to64(G)[i:i + 1], None if Gr is None else to64(Gr)[i:i + 1])
        return torch.cat([a[0], b[0]])
    got_o, got_d = got_o.detach().cpu(), got_d.detach().cpu()
    keep = rays_off_a_gate(torch.cat([got_o, got_d], -1), torch.cat([o64, d64], -1), single64)
    per = lambda g, t: float(((g.double() - t).norm(dim=1) / t.norm(dim=1).clamp_min(1e-20)).median())
    return dict(eo=rel_l2(got_o[keep], o64[keep]), ed=rel_l2(got_d[keep], d64[keep]), yo=rel_l2(ref_o[keep], o64[keep]),
                yd=rel_l2(ref_d[keep], d64[keep]), per_o=per(got_o, o64), per_d=per(got_d, d64), left_out=int((~keep).sum()),
                rays=int(keep.numel()))


def holds(y):
    """err <= 1.5 x yard + 2e-4 for d rays_o and d rays_d, the typical ray within 2e-4 (test_gpu_train.py:660)."""
    return y["eo"] <= 1.5 * y["yo"] + 2e-4 and y["ed"] <= 1.5 * y["yd"] + 2e-4 and y["per_o"] < 2e-4 and y["per_d"] < 2e-4


def show(tag, y):
    print(f"{tag} vs float64: d rays_o {y['eo']:.2e} (torch fp32: {y['yo']:.2e}), d rays_d {y['ed']:.2e} (torch fp32: {y['yd']:.2e}), "
          f"median per-ray {y['per_o']:.2e} / {y['per_d']:.2e}; rays on a gate (left out): {y['left_out']} of {y['rays']}")


# Weight seeds of the two widths: the scene of tests/test_gpu_train.py::test_generic_width_render_gradient_vs_oracle (same weights, rays
# and histograms), fixed on the oracle alone before any GPU run: the fp32 oracle's own distance from the float64 one (the yardstick) is
# finite — 8e-5 / 1e-4 for d rays_o / d rays_d at netwidth 32, 2e-3 / 2e-3 at 256 — and its median per-ray error (3e-5 .. 5e-5) is inside
# 2e-4 for both losses (LABBOOK, "Generic-width render surface").
SEEDS = {32: 4, 256: 4}


# ---------------------------------------------------------------------------------------------- engines
_ENGINES = {}


def engine(width, seed):
    if (width, seed) not in _ENGINES:
        cw, fw, ea, et = syn.nerfh_weights(seed, W=width)
        _ENGINES[width, seed] = eng.NerfHEngine(width=width, precision="f32").load_numpy(cw, fw, ea, et)
    return _ENGINES[width, seed]


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    _ENGINES.clear()


def kwargs(E, Nc, Ni, **over):
    kw = dict(network_query_fn=nerfw.HipQuery(E, 65536), perturb=False, N_importance=Ni, N_samples=Nc, use_viewdirs=True,
              white_bkgd=False, raw_noise_std=0., test_time=True, ndc=False, lindisp=False)
    kw.update(over)
    return kw


# ---------------------------------------------------------------------------------------------- 1. retraw under autograd, rays
@pytest.mark.parametrize("width", [32, 256])
def test_retraw_under_autograd_rays(width):
    """render(rays=..., retraw=True) with rays that require grad at netwidth 32 and 256: `raw` is part of the graph, a loss on rgb
    AND raw, then on raw alone (grad_rgb reaches the node as None), against the float64 oracle.
    Measured on an MI355X (LABBOOK R7.2; error vs float64 of d rays_o, d rays_d, torch fp32's own distance in brackets):
      netwidth 32:  rgb + raw 7.65e-5 (7.79e-5), 1.03e-4 (1.06e-4); raw alone 7.28e-5 (7.48e-5), 9.85e-5 (1.03e-4); 3 of 150 rays on a gate
      netwidth 256: rgb + raw 1.77e-3 (2.33e-3), 1.32e-3 (2.23e-3); raw alone 1.43e-3 (2.16e-3), 1.68e-3 (2.73e-3); 6 of 150 rays on a gate
      median per-ray error 2.7e-5 .. 3.9e-5; tracked forward vs oracle: raw 1.9e-6 / 6.6e-7, rgb 4.0e-7 / 4.1e-7."""
    Nc, Ni, n = 16, 32, 150
    _, w, o, d, hist, G, Gr = ray_case(width, Nc, Ni, n)
    E = engine(width, SEEDS[width])
    kw = kwargs(E, Nc, Ni, retraw=True)
    rendering.GRAD_FORWARD_PRECISION = "f32" if width == 256 else None
    try:
        with torch.no_grad():
            ref = oracle_render(o, d, hist, w, Nc, Ni)
        # a leading shape of its own: 150 rays as [5, 30, 3]
        rays = torch.stack([dev(o), dev(d)]).reshape(2, 5, 30, 3).requires_grad_(True)
        rgb, disp, acc, extras = rendering.render(480, 640, 585., rays=rays, near=NEAR, far=FAR, img_idx=dev(hist), **kw)
        raw = extras["raw"]
        assert raw.requires_grad and rgb.requires_grad and not disp.requires_grad and not acc.requires_grad
        assert raw.shape == (5, 30, Nc + Ni, 9) and rgb.shape == (5, 30, 3)
        e_raw, e_rgb = relmax(raw.reshape(n, Nc + Ni, 9), ref["raw"]), relmax(rgb.reshape(n, 3), ref["rgb_map"])
        print(f"netwidth {width} tracked forward vs oracle: raw {e_raw:.2e}, rgb {e_rgb:.2e}")
        assert e_raw < 3e-5 and e_rgb < 3e-5
        ((rgb.reshape(n, 3) * dev(G)).sum() + (raw.reshape(n, Nc + Ni, 9) * dev(Gr)).sum()).backward()
        both = yardstick(rays.grad[0].reshape(n, 3), rays.grad[1].reshape(n, 3), o, d, hist, w, Nc, Ni, G, Gr)
        show(f"netwidth {width} retraw under autograd, rgb + raw loss", both)
        # raw alone
        rays.grad = None
        raw = rendering.render(480, 640, 585., rays=rays, near=NEAR, far=FAR, img_idx=dev(hist), **kw)[3]["raw"]
        (raw.reshape(n, Nc + Ni, 9) * dev(Gr)).sum().backward()
        alone = yardstick(rays.grad[0].reshape(n, 3), rays.grad[1].reshape(n, 3), o, d, hist, w, Nc, Ni, None, Gr)
        show(f"netwidth {width} retraw under autograd, raw-only loss", alone)
    finally:
        rendering.GRAD_FORWARD_PRECISION = None
    assert np.isfinite([both["yo"], both["yd"], alone["yo"], alone["yd"]]).all()
    assert holds(both), both
    assert holds(alone), alone


# ---------------------------------------------------------------------------------------------- 2. the same through the pose
def test_retraw_under_autograd_pose():
    """render(c2w=pose, retraw=True) at netwidth 32 (12 x 16 frame, 64 + 128): get_rays' node in front of the ray node; pose.grad against
    the float64 oracle, within 3 x the fp32 oracle's own distance + 2e-4 (the bound of d c2w at generic width, test_gpu_train.py:680, :704).
    Measured on an MI355X (LABBOOK R7.2): d c2w 8.3e-3 of the largest entry, torch fp32 5.5e-3 (relative L2 7.1e-3 / 3.9e-3)."""
    H, W, focal, Nc, Ni = 12, 16, 14.6, 64, 128
    _, w = weights(32, SEEDS[32])
    E = engine(32, SEEDS[32])
    rng = np.random.default_rng(2)
    c2w = T(syn.orbit_pose(5, 8))[:3, :4].contiguous()
    G = T(rng.standard_normal((H * W, 3)).astype(np.float32))
    Gr = T((rng.standard_normal((H * W, Nc + Ni, 9)) / (Nc + Ni)).astype(np.float32))
    hist = T(syn.HIST_IDX.astype(np.float32))

    def oracle_pose_grad(c2w, w, G, Gr, hist):
        p = c2w.detach().clone().requires_grad_(True)
        ro, rd = orc.get_rays(H, W, focal, p)
        ro, rd = ro.to(p.dtype), rd.to(p.dtype)
        out = oracle_render(ro.reshape(-1, 3), rd.reshape(-1, 3), hist, w, Nc, Ni)
        oracle_loss(out, G, Gr).backward()
        return {k: v.detach() for k, v in out.items()}, p.grad

    ref_out, ref = oracle_pose_grad(c2w, w, G, Gr, hist)
    with float64_default():
        _, ref64 = oracle_pose_grad(*to64((c2w, w, G, Gr, hist)))
    pose = dev(c2w).requires_grad_(True)
    rgb, disp, acc, extras = rendering.render(H, W, focal, c2w=pose, near=NEAR, far=FAR, img_idx=dev(hist), **kwargs(E, Nc, Ni, retraw=True))
    raw = extras["raw"]
    assert raw.shape == (H, W, Nc + Ni, 9) and raw.requires_grad and rgb.shape == (H, W, 3)
    assert relmax(raw.reshape(-1, Nc + Ni, 9), ref_out["raw"]) < 3e-5 and relmax(rgb.reshape(-1, 3), ref_out["rgb_map"]) < 3e-5
    ((rgb.reshape(-1, 3) * dev(G)).sum() + (raw.reshape(-1, Nc + Ni, 9) * dev(Gr)).sum()).backward()
    yard, err = relmax(ref, ref64), relmax(pose.grad, ref64)
    print(f"netwidth 32 render(c2w, retraw) under autograd vs float64: d c2w {err:.2e} (torch fp32: {yard:.2e}); "
          f"relative L2 {rel_l2(pose.grad, ref64):.2e} (torch fp32: {rel_l2(ref, ref64):.2e})")
    assert np.isfinite(yard) and err <= 3 * yard + 2e-4


# ---------------------------------------------------------------------------------------------- 3. each raw channel on its own
def test_each_raw_channel_reaches_the_rays():
    """A loss on ONE raw channel at a time (32 rays, netwidth 32, E.render_rays_backward(grad_rgb=None, grad_raw=one-hot x Gr)): a wrong
    or missing channel cannot hide behind the other eight.  Same yardstick bound as the batch test.
    Measured on an MI355X (LABBOOK R7.2): d rays_o 2.3e-5 .. 4.8e-5 (torch fp32: 2.6e-5 .. 5.2e-5), d rays_d 2.4e-5 .. 6.9e-5
    (2.4e-5 .. 8.2e-5) over the nine channels; 1 of 32 rays on a gate."""
    Nc, Ni, n = 16, 32, 32
    _, w = weights(32, SEEDS[32])
    E = engine(32, SEEDS[32])
    rng, o, d, hist = ray_batch(n, 23)
    Gr = T((rng.standard_normal((n, Nc + Ni, 9)) / (Nc + Ni)).astype(np.float32))
    results = []
    for ch in range(9):
        Gc = torch.zeros_like(Gr)
        Gc[..., ch] = Gr[..., ch]
        go, gd, gv = E.render_rays_backward(dev(o), dev(d), dev(hist), Nc, Ni, NEAR, FAR, None, grad_raw=dev(Gc))
        assert gv is None
        y = yardstick(go, gd, o, d, hist, w, Nc, Ni, None, Gc)
        show(f"netwidth 32 raw channel {ch} alone", y)
        results.append(y)
    for ch, y in enumerate(results):
        assert np.isfinite([y["yo"], y["yd"]]).all() and y["eo"] <= 1.5 * y["yo"] + 2e-4 and y["ed"] <= 1.5 * y["yd"] + 2e-4, (ch, y)


# ---------------------------------------------------------------------------------------------- 4. explicit view directions
def rotated_viewdirs(d, angle=0.35):
    """Unit vectors that are NOT d / |d|: those, turned by a fixed angle about the z axis."""
    v = d / d.norm(dim=-1, keepdim=True)
    c, s = float(np.cos(angle)), float(np.sin(angle))
    return torch.stack([c * v[:, 0] - s * v[:, 1], s * v[:, 0] + c * v[:, 1], v[:, 2]], -1).contiguous()


def test_explicit_viewdirs_on_the_generic_forward():
    """E.render_rays(viewdirs=v) on the generic path with unit vectors that are not d / |d|: against the oracle with v in the ray rows at
    netwidth 32 (measured: raw 1.6e-6, rgb 4.0e-7), against the register-resident exact-fp32 kernels at netwidth 128."""
    Nc, Ni, n = 16, 32, 77
    _, w = weights(32, SEEDS[32])
    E = engine(32, SEEDS[32])
    _, o, d, hist = ray_batch(n, 5)
    v = rotated_viewdirs(d)
    with torch.no_grad():
        ref = oracle_render(o, d, hist, w, Nc, Ni, view=v)
    rgb, disp, acc, raw = E.render_rays(dev(o), dev(d), dev(hist), Nc, Ni, NEAR, FAR, viewdirs=dev(v), retraw=True, precision="generic")
    errs = dict(rgb=relmax(rgb, ref["rgb_map"]), disp=relmax(disp, ref["disp_map"]), acc=relmax(acc, ref["acc_map"]), raw=relmax(raw, ref["raw"]))
    print(f"netwidth 32 explicit viewdirs vs oracle: {errs}")
    assert max(errs.values()) < 3e-5, errs
    rgb_d = E.render_rays(dev(o), dev(d), dev(hist), Nc, Ni, NEAR, FAR, viewdirs=None, precision="generic")[0]
    assert relmax(rgb_d, rgb.cpu()) > 1e-4          # the pointer is really read
    # viewdirs = d / |d| given explicitly is the derived case
    vd = d / d.norm(dim=-1, keepdim=True)
    rgb_e = E.render_rays(dev(o), dev(d), dev(hist), Nc, Ni, NEAR, FAR, viewdirs=dev(vd), precision="generic")[0]
    assert relmax(rgb_e, rgb_d.cpu()) < 3e-5
    # netwidth 128: the generic path against the register-resident exact-fp32 kernels, same directions
    E128 = engine(128, 4)
    a = E128.render_rays(dev(o), dev(d), dev(hist), Nc, Ni, NEAR, FAR, viewdirs=dev(v), retraw=True, precision="generic")
    b = E128.render_rays(dev(o), dev(d), dev(hist), Nc, Ni, NEAR, FAR, viewdirs=dev(v), retraw=True, precision="f32")
    for x, y, name in zip(a, b, ("rgb", "disp", "acc", "raw")):
        assert rel_l2(x, y) < 1e-3, name


def test_viewdirs_need_one_row_per_ray():
    """The kernels read one view direction per ray: a shorter tensor is refused by every ray render, plain and with maps, on the
    register-resident kernels (netwidth 128) as on the generic path, before anything is launched."""
    Nc, Ni, n = 16, 32, 77
    _, o, d, hist = ray_batch(n, 5)
    args = (dev(o), dev(d), dev(hist), Nc, Ni, NEAR, FAR)
    short = dev(rotated_viewdirs(d)[:n - 1])
    for E in (engine(128, 4), engine(32, SEEDS[32])):
        for call in (E.render_rays, E.render_rays_maps, E.generic_render_rays, E.generic_render_rays_maps):
            with pytest.raises(ValueError, match=f"viewdirs must have {n} rows"):
                call(*args, viewdirs=short)


# ---------------------------------------------------------------------------------------------- 5. ndc / c2w_staticcam at test time
def test_ndc_and_staticcam_at_netwidth_32(gold):
    """render(ndc=True) and render(c2w_staticcam=...) at a generic width against orc.render on the G14 fixture's pose and intrinsics
    (the fixture's images are netwidth 128: only c2w, c2w_staticcam, H, W, focal, Nc, Ni and hist are reused)."""
    g = gold("g14_render_ndc_staticcam")
    H, W, focal, Nc, Ni = int(g["H"]), int(g["W"]), float(g["focal"]), int(g["Nc"]), int(g["Ni"])
    _, w = weights(32, SEEDS[32])
    E = engine(32, SEEDS[32])
    c2w, static, hist = T(g["c2w"]).float(), T(g["c2w_staticcam"]).float(), np.asarray(g["hist"], dtype=np.float32)
    with torch.no_grad():
        ref_ndc = orc.render(H, W, focal, 1 << 30, *w, Nc, Ni, 0., 1., hist, c2w=c2w, ndc=True)
        ref_static = orc.render(H, W, focal, 1 << 30, *w, Nc, Ni, 0., 2.5, hist, c2w=c2w, c2w_staticcam=static)
    with torch.no_grad():
        got = rendering.render(H, W, focal, c2w=dev(c2w), near=0., far=1., img_idx=dev(hist)[None], **kwargs(E, Nc, Ni, ndc=True, retraw=True))
    errs = [relmax(a, b) for a, b in zip(got[:3], ref_ndc)]
    print(f"netwidth 32 ndc vs oracle: {errs}")
    assert got[0].shape == (H, W, 3) and got[3]["raw"].shape == (H, W, Nc + Ni, 9) and max(errs) < 3e-5, errs
    with torch.no_grad():
        got = rendering.render(H, W, focal, c2w=dev(c2w), c2w_staticcam=dev(static), near=0., far=2.5, img_idx=dev(hist)[None], **kwargs(E, Nc, Ni))
    errs = [relmax(a, b) for a, b in zip(got[:3], ref_static)]
    print(f"netwidth 32 c2w_staticcam vs oracle: {errs}")
    assert got[3] == {} and max(errs) < 3e-5, errs
    # rays instead of a pose
    o, d = orc.get_rays(H, W, focal, c2w)
    with torch.no_grad():
        got = rendering.render(H, W, focal, rays=(dev(o), dev(d)), near=0., far=1., img_idx=dev(hist)[None], **kwargs(E, Nc, Ni, ndc=True))
    assert max(relmax(a, b) for a, b in zip(got[:3], ref_ndc)) < 3e-5


# ---------------------------------------------------------------------------------------------- 6. the old entries are unchanged
def _raw_calls(E, o, d, hist, Nc, Ni, G):
    """(old forward, new forward with NULL viewdirs, old backward, new backward with NULL grad_raw) straight through ctypes."""
    lib, n, Nf = E.lib, o.shape[0], Nc + Ni
    ws_f = torch.empty(lib.dfn_nerfh_generic_workspace_bytes(E.handle, n, Nc, Ni), dtype=torch.uint8, device=DEV)
    ws_b = torch.empty(lib.dfn_nerfh_generic_backward_workspace_bytes(E.handle, n, Nc, Ni), dtype=torch.uint8, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    outs = []
    for new in (False, True):
        rgb, disp, acc, raw = (torch.full(s, float("nan"), device=DEV) for s in ((n, 3), (n,), (n,), (n, Nf, 9)))
        ws_f.zero_()
        if new:
            rc = lib.dfn_nerfh_generic_render_rays_v(E.handle, ptr(o), ptr(d), None, ptr(hist), hist.shape[0], n, Nc, Ni, NEAR, FAR, ptr(rgb),
                                                     ptr(disp), ptr(acc), ptr(raw), vp(ws_f), ws_f.numel(), current_stream())
        else:
            rc = lib.dfn_nerfh_generic_render_rays(E.handle, ptr(o), ptr(d), ptr(hist), hist.shape[0], n, Nc, Ni, NEAR, FAR, ptr(rgb),
                                                   ptr(disp), ptr(acc), ptr(raw), vp(ws_f), ws_f.numel(), current_stream())
        assert rc == 0, lib.dfn_last_error()
        go, gd = torch.full((n, 3), float("nan"), device=DEV), torch.full((n, 3), float("nan"), device=DEV)
        ws_b.zero_()
        if new:
            rc = lib.dfn_nerfh_generic_render_rays_backward_raw(E.handle, ptr(o), ptr(d), None, ptr(hist), hist.shape[0], n, Nc, Ni, NEAR, FAR,
                                                                ptr(G), None, ptr(go), ptr(gd), None, vp(ws_b), ws_b.numel(), current_stream())
        else:
            rc = lib.dfn_nerfh_generic_render_rays_backward(E.handle, ptr(o), ptr(d), None, ptr(hist), hist.shape[0], n, Nc, Ni, NEAR, FAR,
                                                            ptr(G), ptr(go), ptr(gd), None, vp(ws_b), ws_b.numel(), current_stream())
        assert rc == 0, lib.dfn_last_error()
        outs.append((rgb, disp, acc, raw, go, gd))
    return outs, (ws_b, go, gd)


@pytest.mark.parametrize("width", [32, 128])
def test_old_entries_equal_the_new_ones_with_null(width):
    """dfn_nerfh_generic_render_rays / _backward against the new entries with viewdirs = NULL / grad_raw = NULL: the same bits; both
    gradients NULL is DFN_ERR_ARG under the entry's name."""
    Nc, Ni, n = 16, 32, 77
    E = engine(width, 4)
    rng, o, d, hist = ray_batch(n, 9)
    o, d, hist, G = dev(o), dev(d), dev(hist), dev(rng.standard_normal((n, 3)).astype(np.float32))
    (old, new), (ws_b, go, gd) = _raw_calls(E, o, d, hist, Nc, Ni, G)
    for a, b, name in zip(old, new, ("rgb", "disp", "acc", "raw", "grad_rays_o", "grad_rays_d")):
        assert not torch.isnan(a).any() and torch.equal(a, b), name
    # both gradients NULL: refused before any device work, and the message names the entry
    lib = E.lib
    rc = lib.dfn_nerfh_generic_render_rays_backward_raw(E.handle, ptr(o), ptr(d), None, ptr(hist), n, n, Nc, Ni, NEAR, FAR, None, None, ptr(go),
                                                        ptr(gd), None, ctypes.c_void_p(ws_b.data_ptr()), ws_b.numel(), current_stream())
    assert rc == -1 and b"dfn_nerfh_generic_render_rays_backward_raw" in lib.dfn_last_error()
    # the old entry still needs its grad_rgb
    rc = lib.dfn_nerfh_generic_render_rays_backward(E.handle, ptr(o), ptr(d), None, ptr(hist), n, n, Nc, Ni, NEAR, FAR, None, ptr(go), ptr(gd),
                                                    None, ctypes.c_void_p(ws_b.data_ptr()), ws_b.numel(), current_stream())
    assert rc == -1 and b"dfn_nerfh_generic_render_rays_backward:" in lib.dfn_last_error()
    # a zero grad_raw adds nothing: the compositor's gradient + 0
    z = torch.zeros(n, Nc + Ni, 9, device=DEV)
    go_z, gd_z, _ = E.render_rays_backward(o, d, hist, Nc, Ni, NEAR, FAR, G, precision="generic", grad_raw=z)
    assert torch.equal(go_z, old[4]) and torch.equal(gd_z, old[5])


# ---------------------------------------------------------------------------------------------- 7. chunking
@pytest.mark.parametrize("which", ["GENERIC_CHUNK", "GENERIC_GRAD_CHUNK"])
def test_chunked_calls_equal_stand_alone_ones(which):
    """More rays than one pass of the generic path takes (the forward's chunk and the gradient's), explicit view directions and
    grad_raw given: the first and the last 37 rays equal a stand-alone call on those rays, bit for bit (rays are independent)."""
    Nc, Ni = 8, 8
    E = engine(32, SEEDS[32])
    n = getattr(E, which) + 37
    gen = torch.Generator().manual_seed(3)
    _, o0, d0, _ = ray_batch(512, 13)
    idx = torch.randint(0, 512, (n,), generator=gen)
    o = (o0[idx] + 0.01 * torch.randn(n, 3, generator=gen)).contiguous()
    d = (d0[idx] + 0.01 * torch.randn(n, 3, generator=gen)).contiguous()
    hist = torch.randint(0, 40, (n, 10), generator=gen).float()
    G = torch.randn(n, 3, generator=gen)
    Gr = torch.randn(n, Nc + Ni, 9, generator=gen) / (Nc + Ni)
    v = rotated_viewdirs(d)
    o, d, hist, G, Gr, v = (dev(t) for t in (o, d, hist, G, Gr, v))
    full_f = E.render_rays(o, d, hist, Nc, Ni, NEAR, FAR, viewdirs=v, retraw=True)
    full_b = E.render_rays_backward(o, d, hist, Nc, Ni, NEAR, FAR, G, viewdirs=v, grad_raw=Gr)
    full_r = E.render_rays_backward(o, d, hist, Nc, Ni, NEAR, FAR, None, grad_raw=Gr)
    for sl in (slice(0, 37), slice(n - 37, n)):
        cut = lambda t: t[sl].contiguous()
        part_f = E.render_rays(cut(o), cut(d), cut(hist), Nc, Ni, NEAR, FAR, viewdirs=cut(v), retraw=True)
        part_b = E.render_rays_backward(cut(o), cut(d), cut(hist), Nc, Ni, NEAR, FAR, cut(G), viewdirs=cut(v), grad_raw=cut(Gr))
        part_r = E.render_rays_backward(cut(o), cut(d), cut(hist), Nc, Ni, NEAR, FAR, None, grad_raw=cut(Gr))
        for a, b in zip(full_f + full_b + full_r[:2], part_f + part_b + part_r[:2]):
            assert not torch.isnan(b).any() and torch.equal(a[sl], b)
