"""Differentiable disp, acc and render maps: the compositing backward for every output of the fine compositor
(dfn_composite_fine_backward_maps, models/rendering.py:161-243), the generic-width gradient that uses it, and render(diff_maps=True).

Truth: torch.autograd through the CPU oracle in float64 (tests/yardstick.py).  Yardstick: torch's own fp32 autograd of the same oracle.
Bound: relative L2 error <= 1.5 x yardstick + 2e-4 per tensor — the form the project applies wherever a gradient through the compositor is
held to this yardstick (tests/test_gpu_options.py:131, tests/test_gpu_generic_surface.py::holds, tests/test_gpu_train.py:643); its additive
term is the bound tests/test_gpu_grad.py::test_composite_backward_vs_autograd applies to the existing compositing backward (2e-4; that
test states no multiple of its own).  d c2w: 3 x yardstick + 2e-4 of the largest entry (tests/test_gpu_generic_surface.py:230).

Measured figures: the docstrings of the tests and LABBOOK R9.1."""

import numpy as np
import pytest
import torch

from dfnet_amd import _lib, engine as eng, rendering
from oracle import nerfh_oracle as orc
from tests import render_maps_cases as rmc
from tests import test_gpu_generic_surface as gs
from tests.yardstick import float64_default, rays_off_a_gate, rel_l2, to64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
NEAR, FAR = 0., 2.5
GRADS = ("rgb", "acc", "depth", "depth_static", "disp", "beta", "rgb_static", "rgb_transient")
MAPS = rmc.MAPS


def dev(x):
    return torch.as_tensor(x).float().to(DEV).contiguous()


def bound(yard):
    return 1.5 * yard + 2e-4


# ---------------------------------------------------------------------------------------------- the oracle half (runs without a GPU)
def stage_inputs(n, Nf, seed=0):
    """raw [n,Nf,9] with sigma_s, sigma_t = softplus(N(0,1)), colours and beta in (0,1); z sorted in [0, 2.5]."""
    gen = torch.Generator().manual_seed(1000 * seed + 10 * Nf + n)
    raw = torch.rand(n, Nf, 9, generator=gen) * 0.98 + 0.01
    raw[..., 3] = torch.nn.functional.softplus(torch.randn(n, Nf, generator=gen))
    raw[..., 7] = torch.nn.functional.softplus(torch.randn(n, Nf, generator=gen))
    z = torch.sort(torch.rand(n, Nf, generator=gen) * 2.5, -1)[0]
    return raw.contiguous(), z.contiguous(), gen


def stage_loss(m, G):
    return sum((m[k] * G[k]).sum() for k in G)


def stage_grad(raw, z, G, f64=False):
    """d sum_k (output_k * G_k) / d raw by autograd through oracle_maps (orc.composite_fine), in fp32 or float64."""
    if f64:
        with float64_default():
            return stage_grad(*to64((raw, z, G)))
    r = raw.detach().clone().requires_grad_(True)
    return torch.autograd.grad(stage_loss(rmc.oracle_maps(r, z), G), r)[0]


def one_hot(name, n):
    """A unit gradient on output `name` alone, for every ray: 1 for the [n] outputs, a one-hot channel (ray index mod 3) for the [n,3] ones."""
    if name.startswith("rgb"):
        g = torch.zeros(n, 3)
        g[torch.arange(n), torch.arange(n) % 3] = 1.
        return g
    return torch.ones(n)


def random_weights(n, gen):
    return {k: torch.randn((n, 3) if k.startswith("rgb") else (n,), generator=gen) for k in GRADS}


def scene_weights(width, seed):
    return gs.weights(width, seed)[1]


def g6_rays():
    g = rmc.golden("g6_render_rays_a")
    assert int(g["Nc"]) == 8 and int(g["Ni"]) == 16 and g["rays_o"].shape == (64, 3)
    return T(g["rays_o"]).float(), T(g["rays_d"]).float(), T(g["hist"]).float().reshape(1, -1), 8, 16


def loss_weights(n, seed):
    """Random per-ray weights on rgb, disp, acc and the five maps."""
    gen = torch.Generator().manual_seed(seed)
    return {k: torch.randn((n, 3) if k.startswith("rgb") else (n,), generator=gen) for k in ("rgb", "disp", "acc") + MAPS}


def oracle_outputs(o, d, hist, w, Nc, Ni):
    """Every output of the oracle's render of rays (o, d): rgb, disp, acc and the five maps, attached to (o, d)."""
    st = {}
    orc.render_rays(gs.ray_rows(o, d, hist), *w, Nc, Ni, stages=st)
    return rmc.oracle_maps(st["raw"], st["z_fine"])


def oracle_ray_grads(o, d, hist, w, Nc, Ni, G, f64=False):
    if f64:
        with float64_default():
            return oracle_ray_grads(*to64((o, d, hist, w)), Nc, Ni, to64(G))
    o, d = o.detach().clone().requires_grad_(True), d.detach().clone().requires_grad_(True)
    stage_loss(oracle_outputs(o, d, hist, w, Nc, Ni), G).backward()
    return o.grad, d.grad


def ray_yardstick(got_o, got_d, o, d, hist, w, Nc, Ni, G):
    """tests/test_gpu_generic_surface.py::yardstick for the loss over all outputs: the float64 criterion over the rays that
    rays_off_a_gate keeps (max_frac = 0.04: at most 4 % of the rays may be excused, and only when their float64 gradient itself moves)."""
    ref_o, ref_d = oracle_ray_grads(o, d, hist, w, Nc, Ni, G)
    o64, d64 = oracle_ray_grads(o, d, hist, w, Nc, Ni, G, f64=True)
    w64, o_64, d_64, h64, G64 = to64(w), to64(o), to64(d), to64(hist), to64(G)

    def single64(i, delta):
        with float64_default():
            a, b = oracle_ray_grads(o_64[i:i + 1] + delta, d_64[i:i + 1], h64, w64, Nc, Ni, {k: v[i:i + 1] for k, v in G64.items()})
        return torch.cat([a[0], b[0]])
    got_o, got_d = got_o.detach().cpu(), got_d.detach().cpu()
    keep = rays_off_a_gate(torch.cat([got_o, got_d], -1), torch.cat([o64, d64], -1), single64, max_frac=0.04)
    per = lambda g, t: float(((g.double() - t).norm(dim=1) / t.norm(dim=1).clamp_min(1e-20)).median())
    return dict(eo=rel_l2(got_o[keep], o64[keep]), ed=rel_l2(got_d[keep], d64[keep]), yo=rel_l2(ref_o[keep], o64[keep]),
                yd=rel_l2(ref_d[keep], d64[keep]), per_o=per(got_o, o64), per_d=per(got_d, d64), left_out=int((~keep).sum()),
                rays=int(keep.numel()))


# Weight seed per netwidth and the seed of the loss weights, fixed on the oracle alone before any GPU run (the procedure above with the fp32
# oracle's own gradient in the place of the HIP one): the yardstick is finite, the fp32 oracle's median per-ray error is inside 2e-4 and
# it needs no more than the 2 rays of 64 that max_frac = 0.04 allows.  Kept: weight seed 0 at every width, loss seed 7 (LABBOOK).
SEEDS = {128: 0, 32: 0, 256: 0}
LOSS_SEED = 7


# ---------------------------------------------------------------------------------------------- 1. the stage against the float64 oracle
SHAPES = [(n, Nf) for n in (5, 7) for Nf in (1, 24, 63, 64, 65, 128, 192, 200, 320, 512)]


@pytest.mark.parametrize("n,Nf", SHAPES)
def test_stage_vs_float64_oracle(n, Nf):
    """Each upstream gradient alone (one-hot per ray) and all eight with random weights, n not a multiple of the 4 waves of a block, Nf over
    every SPL instantiation (1, 2, 3, 4, 6, 8 samples per lane) and the lane boundaries 63 / 64 / 65.  With g_rgb alone the result also agrees
    with composite_fine_backward within the same bound.
    Measured on an MI355X (LABBOOK R9.1; relative L2 from float64, torch fp32's own in brackets), worst over the 20 shapes: rgb_static alone
    3.03e-6 (1.30e-6) at n = 7, Nf = 512; all eight 2.69e-6 (1.72e-6); g_rgb alone against the rgb-only kernel 6.6e-7.  acc alone: the true
    gradient is below fp32 on these rays (see test_stage_acc_gradient_on_rays_that_let_light_through): HIP 1.0, torch fp32 1.9e8 .. 1.2e9."""
    raw, z, gen = stage_inputs(n, Nf)
    cases = [(k, {k: one_hot(k, n)}) for k in GRADS] + [("all", random_weights(n, gen))]
    fails = []
    for tag, G in cases:
        truth, ref = stage_grad(raw, z, G, f64=True), stage_grad(raw, z, G)
        got = eng.composite_fine_backward_maps(dev(raw), dev(z), {k: dev(v) for k, v in G.items()})
        assert got.shape == (n, Nf, 9) and torch.isfinite(got).all()
        yard, e = rel_l2(ref, truth), rel_l2(got, truth)
        print(f"n={n} Nf={Nf} {tag}: HIP {e:.2e} vs float64 (torch fp32: {yard:.2e})")
        assert np.isfinite(yard)
        if not e <= bound(yard):
            fails.append((tag, e, yard))
        if tag == "rgb":
            old = eng.composite_fine_backward(dev(raw), dev(z), dev(G["rgb"]))
            e_old = rel_l2(got, old)
            print(f"n={n} Nf={Nf} rgb alone vs composite_fine_backward: {e_old:.2e}")
            if not e_old <= bound(yard):
                fails.append(("rgb vs the rgb-only kernel", e_old, yard))
    assert not fails, fails


def test_stage_null_is_zero_and_ext():
    """All NULL: DFN_ERR_ARG.  A NULL pointer is the same as a tensor of zeros, bit for bit.  grad_raw_ext alone reproduces itself; with
    upstream gradients it is added to their d L/d raw."""
    n, Nf = 7, 200
    raw, z, gen = stage_inputs(n, Nf, seed=1)
    G = {k: dev(v) for k, v in random_weights(n, gen).items()}
    rawd, zd = dev(raw), dev(z)
    with pytest.raises(_lib.DfnError, match=r"status -1"):
        eng.composite_fine_backward_maps(rawd, zd, {})
    with pytest.raises(_lib.DfnError, match=r"status -1"):
        eng.composite_fine_backward_maps(rawd, zd, {k: None for k in GRADS})
    zeros = {k: torch.zeros_like(v) for k, v in G.items()}
    for given in (("rgb",), ("disp",), ("beta", "rgb_static"), ("acc", "depth", "depth_static", "rgb_transient"), GRADS[:-1]):
        some = eng.composite_fine_backward_maps(rawd, zd, {k: G[k] for k in given})
        full = eng.composite_fine_backward_maps(rawd, zd, {k: (G[k] if k in given else zeros[k]) for k in GRADS})
        assert torch.equal(some, full), given
    ext = dev(torch.randn(n, Nf, 9, generator=gen))
    assert torch.equal(eng.composite_fine_backward_maps(rawd, zd, {}, grad_raw=ext), ext)
    both = eng.composite_fine_backward_maps(rawd, zd, G, grad_raw=ext)
    assert torch.equal(both, eng.composite_fine_backward_maps(rawd, zd, G) + ext)


def test_stage_opaque_and_static_only_rays():
    """One ray with an opaque sample (sigma_s = 50 at index 3) and one with sigma_t == 0: finite gradients, inside the bound; on the
    sigma_t == 0 ray the colour gradient of the rgb_static loss equals that of the (rgb - rgb_transient) loss (T_s = T and a_t = 0 there:
    the same products, so the two agree to the last bits — held to 1e-6 of the largest entry)."""
    n, Nf = 2, 24
    raw, z, gen = stage_inputs(n, Nf, seed=2)
    raw[0, 3, 3] = 50.
    raw[1, :, 7] = 0.
    G = random_weights(n, gen)
    truth, ref = stage_grad(raw, z, G, f64=True), stage_grad(raw, z, G)
    got = eng.composite_fine_backward_maps(dev(raw), dev(z), {k: dev(v) for k, v in G.items()})
    assert torch.isfinite(got).all()
    for i, tag in enumerate(("opaque sample", "sigma_t == 0")):
        yard, e = rel_l2(ref[i], truth[i]), rel_l2(got[i], truth[i])
        print(f"{tag}: HIP {e:.2e} vs float64 (torch fp32: {yard:.2e})")
        assert np.isfinite(yard) and e <= bound(yard), (tag, e, yard)
    g = dev(torch.randn(n, 3, generator=gen))
    a = eng.composite_fine_backward_maps(dev(raw), dev(z), dict(rgb_static=g))[1, :, 0:3]
    b = eng.composite_fine_backward_maps(dev(raw), dev(z), dict(rgb=g, rgb_transient=-g))[1, :, 0:3]
    assert torch.isfinite(a).all() and float((a - b).abs().max()) <= 1e-6 * float(a.abs().max())


@pytest.mark.parametrize("n,Nf", [(5, 24), (7, 200)])
def test_stage_acc_gradient_on_rays_that_let_light_through(n, Nf):
    """d acc / d sigma_i = delta_i x (the transmittance behind the last sample).  With sigma = softplus(N(0,1)) and a last interval of 1e2
    that is below fp32 on nearly every ray of the shapes above (float64 1e-40 and less: the kernel's closed form returns 0 there and
    torch's fp32 autograd returns round-off, 1e8 relative), so those cases cannot tell a right g_acc term from a missing one.  Here the last
    sample is nearly transparent (sigma_s, sigma_t = 1e-3, 2e-3) and the gradient is of order one: acc alone, disp alone (which reaches
    raw through acc and depth_static) and all eight, same bound.
    Measured on an MI355X (LABBOOK R9.1): acc alone 1.96e-7 (torch fp32: 9.6e-8) / 6.8e-7 (2.3e-7), disp alone 1.2e-7 / 7.8e-7, all eight
    1.2e-7 / 1.1e-6 at 5 x 24 / 7 x 200."""
    raw, z, gen = stage_inputs(n, Nf, seed=3)
    raw[:, -1, 3], raw[:, -1, 7] = 1e-3, 2e-3
    for tag, G in (("acc", dict(acc=one_hot("acc", n))), ("disp", dict(disp=one_hot("disp", n))), ("all", random_weights(n, gen))):
        truth, ref = stage_grad(raw, z, G, f64=True), stage_grad(raw, z, G)
        got = eng.composite_fine_backward_maps(dev(raw), dev(z), {k: dev(v) for k, v in G.items()})
        yard, e = rel_l2(ref, truth), rel_l2(got, truth)
        print(f"transparent last sample, n={n} Nf={Nf} {tag}: HIP {e:.2e} vs float64 (torch fp32: {yard:.2e})")
        assert np.isfinite(yard) and yard < 1e-5 and e <= bound(yard), (tag, e, yard)


# ---------------------------------------------------------------------------------------------- engines and render kwargs
@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(width):
        if width not in made:
            from dfnet_amd import synthetic as syn
            cw, fw, ea, et = syn.nerfh_weights(SEEDS[width], W=width)
            made[width] = eng.NerfHEngine(width=width, precision="f32").load_numpy(cw, fw, ea, et)
        return made[width]
    yield get
    made.clear()


class tracked_mode:
    """netwidth 128 two-pass / one-pass (rendering.GRAD_TWO_PASS) and the fp32 tracked forward of netwidth 256, restored on exit."""

    def __init__(self, width, two_pass=True):
        self.width, self.two_pass = width, two_pass

    def __enter__(self):
        self.keep = (rendering.GRAD_TWO_PASS, rendering.GRAD_FORWARD_PRECISION)
        rendering.GRAD_TWO_PASS = self.two_pass
        rendering.GRAD_FORWARD_PRECISION = "f32" if self.width == 256 else None

    def __exit__(self, *exc):
        rendering.GRAD_TWO_PASS, rendering.GRAD_FORWARD_PRECISION = self.keep


def render_all(E, rays, hist, Nc, Ni, **over):
    """render(rays, ret_maps=True, ...) -> {name: tensor} over rgb, disp, acc, the five maps (and raw)."""
    rgb, disp, acc, extras = rendering.render(480, 640, 585., rays=rays, near=NEAR, far=FAR, img_idx=hist, ret_maps=True,
                                              **gs.kwargs(E, Nc, Ni, **over))
    return dict(rgb=rgb, disp=disp, acc=acc, **extras)


# ---------------------------------------------------------------------------------------------- 2. end to end
@pytest.mark.parametrize("width,two_pass", [(128, True), (128, False), (32, True), (256, True)])
def test_ray_gradients_of_every_output(engines, width, two_pass):
    """The 64 rays of G6 a (8 + 16 samples), a loss with random per-ray weights on rgb, disp, acc and the five maps: d L/d rays_o and
    d L/d rays_d against float64 autograd through the oracle, bound and per-ray criterion of tests/test_gpu_generic_surface.py::holds.
    Measured on an MI355X (LABBOOK R9.1; d rays_o, d rays_d, torch fp32 in brackets; rays left out of 64): netwidth 128 two-pass and one-pass
    2.18e-5 (1.51e-5), 6.55e-5 (3.41e-5), 0; netwidth 32 2.38e-5 (1.92e-5), 3.97e-5 (3.32e-5), 1; netwidth 256 1.28e-4 (1.32e-4), 1.01e-4
    (1.08e-4), 2; median per-ray error 1.3e-5 .. 2.5e-5."""
    o, d, hist, Nc, Ni = g6_rays()
    n = o.shape[0]
    w = scene_weights(width, SEEDS[width])
    G = loss_weights(n, LOSS_SEED)
    E = engines(width)
    with tracked_mode(width, two_pass):
        rays = torch.stack([dev(o), dev(d)]).requires_grad_(True)
        out = render_all(E, rays, dev(hist), Nc, Ni, diff_maps=True)
        assert all(out[k].requires_grad for k in G)
        with torch.no_grad():
            ref = oracle_outputs(o, d, hist, w, Nc, Ni)
        for k in G:
            assert rmc.relmax(out[k], ref[k]) < 3e-5, k   # the tracked forward's bound (tests/test_gpu_generic_surface.py:179)
        stage_loss(out, {k: dev(v) for k, v in G.items()}).backward()
    y = ray_yardstick(rays.grad[0], rays.grad[1], o, d, hist, w, Nc, Ni, G)
    gs.show(f"netwidth {width}{'' if two_pass else ' one-pass'} diff_maps, loss on all outputs", y)
    assert np.isfinite([y["yo"], y["yd"]]).all()
    assert y["left_out"] <= int(0.04 * n)
    assert gs.holds(y), y


@pytest.mark.parametrize("width", [128, 32])
def test_pose_gradient_of_every_output(engines, width):
    """render(c2w = pose, diff_maps=True, ret_maps=True) on the 12 x 16 G7 image (64 + 128): get_rays' node in front of the ray node;
    pose.grad against the float64 oracle within 3 x the fp32 oracle's own distance + 2e-4 of the largest entry.
    Measured on an MI355X (LABBOOK R9.1): netwidth 128 2.20e-3 (torch fp32: 2.03e-3), netwidth 32 4.8e-4 (6.8e-3)."""
    g = rmc.golden("g7_render_image")
    H, W, focal, Nc, Ni = int(g["H"]), int(g["W"]), float(g["focal"]), int(g["Nc"]), int(g["Ni"])
    c2w = T(g["c2w"]).float()[:3, :4].contiguous()
    hist = T(g["hist"]).float().reshape(1, -1)
    w = scene_weights(width, SEEDS[width])
    G = loss_weights(H * W, LOSS_SEED + 1)

    def oracle_pose_grad(c2w, w, G, hist):
        p = c2w.detach().clone().requires_grad_(True)
        ro, rd = orc.get_rays(H, W, focal, p)
        stage_loss(oracle_outputs(ro.to(p.dtype).reshape(-1, 3), rd.to(p.dtype).reshape(-1, 3), hist, w, Nc, Ni), G).backward()
        return p.grad

    ref = oracle_pose_grad(c2w, w, G, hist)
    with float64_default():
        ref64 = oracle_pose_grad(*to64((c2w, w, G, hist)))
    E = engines(width)
    with tracked_mode(width):
        pose = dev(c2w).requires_grad_(True)
        rgb, disp, acc, extras = rendering.render(H, W, focal, c2w=pose, near=NEAR, far=FAR, img_idx=dev(hist), ret_maps=True, diff_maps=True,
                                                  **gs.kwargs(E, Nc, Ni))
        out = dict(rgb=rgb, disp=disp, acc=acc, **extras)
        assert rgb.shape == (H, W, 3) and disp.shape == (H, W) and extras["rgb_static"].shape == (H, W, 3) and extras["beta"].shape == (H, W)
        stage_loss({k: v.reshape(H * W, *v.shape[2:]) for k, v in out.items()}, {k: dev(v) for k, v in G.items()}).backward()
    yard, err = gs.relmax(ref, ref64), gs.relmax(pose.grad, ref64)
    print(f"netwidth {width} render(c2w, diff_maps) vs float64: d c2w {err:.2e} (torch fp32: {yard:.2e}); "
          f"relative L2 {rel_l2(pose.grad, ref64):.2e} (torch fp32: {rel_l2(ref, ref64):.2e})")
    assert np.isfinite(yard) and err <= 3 * yard + 2e-4


# ---------------------------------------------------------------------------------------------- 3. the surface
def test_opt_in_only(engines):
    """diff_maps=False: disp / acc detached and ret_maps refused under autograd, as before; training mode, ndc and render_frames refuse
    diff_maps; at netwidth 128 the register-resident route refuses grad_maps."""
    o, d, hist, Nc, Ni = g6_rays()
    E = engines(32)
    rays = torch.stack([dev(o), dev(d)]).requires_grad_(True)
    kw = gs.kwargs(E, Nc, Ni)
    rgb, disp, acc, extras = rendering.render(480, 640, 585., rays=rays, near=NEAR, far=FAR, img_idx=dev(hist), **kw)
    assert rgb.requires_grad and not disp.requires_grad and not acc.requires_grad and extras == {}
    with pytest.raises(NotImplementedError, match="ret_maps together with autograd"):
        rendering.render(480, 640, 585., rays=rays, near=NEAR, far=FAR, img_idx=dev(hist), ret_maps=True, **kw)
    with pytest.raises(NotImplementedError, match="ndc / c2w_staticcam together with autograd"):
        rendering.render(480, 640, 585., rays=rays, near=NEAR, far=FAR, img_idx=dev(hist), diff_maps=True, **dict(kw, ndc=True))
    with pytest.raises(NotImplementedError, match="diff_maps"):
        rendering.render_frames(12, 16, 14.6, dev(torch.eye(4)[None, :3]).requires_grad_(True), dev(hist), near=NEAR, far=FAR, diff_maps=True, **kw)
    rgb, disp, acc, extras = rendering.render(480, 640, 585., rays=rays, near=NEAR, far=FAR, img_idx=dev(hist), diff_maps=True, **kw)
    assert rgb.requires_grad and disp.requires_grad and acc.requires_grad and extras == {}
    with torch.no_grad():   # nothing to attach to: the plain render
        _, disp, _, _ = rendering.render(480, 640, 585., rays=rays, near=NEAR, far=FAR, img_idx=dev(hist), diff_maps=True, **kw)
    assert not disp.requires_grad
    with pytest.raises(NotImplementedError, match="grad_maps"):
        engines(128).render_rays_backward(dev(o), dev(d), dev(hist), Nc, Ni, NEAR, FAR, None, grad_maps=dict(acc=dev(torch.ones(64))))


@pytest.mark.parametrize("width", [32, 256, 128])
def test_forward_values_are_the_untracked_render(engines, width):
    """With diff_maps=True the forward values of rgb, disp, acc and the maps are the bits of the untracked render(ret_maps=True).  Netwidth 128
    tracks through the saving forward (the fine net in split-f16 with its ReLU signs recorded), which is not the arithmetic of the untracked
    render: there the values are the bits of the tracked render without diff_maps (rgb, disp, acc) and of composite_fine_maps on the saved
    state, and within 2 x 2e-5 of the untracked render (each is held to 2e-5 of the oracle, tests/render_maps_cases.py::TOL)."""
    o, d, hist, Nc, Ni = g6_rays()
    E = engines(width)
    with tracked_mode(width):
        rays = torch.stack([dev(o), dev(d)]).requires_grad_(True)
        got = render_all(E, rays, dev(hist), Nc, Ni, diff_maps=True)
        with torch.no_grad():
            plain = render_all(E, rays, dev(hist), Nc, Ni)
        assert set(got) == set(plain) == {"rgb", "disp", "acc", *MAPS}
        if width != 128:
            for k in plain:
                assert torch.equal(got[k].detach(), plain[k]), k
            return
        for k in plain:
            e = rmc.relmax(got[k], plain[k])
            print(f"netwidth 128 tracked (diff_maps) vs untracked {k}: {e:.2e}")
            assert e < 4e-5, k
        tracked = rendering.render(480, 640, 585., rays=rays, near=NEAR, far=FAR, img_idx=dev(hist), **gs.kwargs(E, Nc, Ni))
        for k, t in zip(("rgb", "disp", "acc"), tracked[:3]):
            assert torch.equal(got[k].detach(), t.detach()), k
        od, dd = dev(o), dev(d)
        _, _, _, zf, raw, _ = E.render_rays_saving(od, dd, dd / dd.norm(dim=-1, keepdim=True), dev(hist), Nc, Ni, NEAR, FAR, with_masks=True)
        mp = E.composite_fine_maps(raw, zf)
        for k in MAPS:
            assert torch.equal(got[k].detach(), mp[k]), k


@pytest.mark.parametrize("width,two_pass", [(128, True), (128, False), (32, True)])
def test_retraw_composes_with_diff_maps(engines, width, two_pass):
    """retraw + diff_maps: the gradient of (loss on the outputs) + (loss on raw) equals the sum of the two separate backward passes within
    round-off — 2e-4 relative L2, the bound of a ray gradient in fp32 (tests/test_gpu_grad.py::TOL): d L/d raw of the returned raw is added
    to the compositor's inside the kernel (grad_raw_ext), and everything behind it is linear in d L/d raw."""
    o, d, hist, Nc, Ni = g6_rays()
    n = o.shape[0]
    E = engines(width)
    G = {k: dev(v) for k, v in loss_weights(n, LOSS_SEED + 2).items()}
    Gr = dev(torch.randn(n, Nc + Ni, 9, generator=torch.Generator().manual_seed(5)) / (Nc + Ni))
    grads = []
    with tracked_mode(width, two_pass):
        for use_maps, use_raw in ((True, True), (True, False), (False, True)):
            rays = torch.stack([dev(o), dev(d)]).requires_grad_(True)
            out = render_all(E, rays, dev(hist), Nc, Ni, diff_maps=True, retraw=True)
            assert out["raw"].requires_grad and out["raw"].shape == (n, Nc + Ni, 9)
            loss = (stage_loss(out, G) if use_maps else 0.) + ((out["raw"] * Gr).sum() if use_raw else 0.)
            loss.backward()
            grads.append(rays.grad.clone())
    e = rel_l2(grads[0], grads[1] + grads[2])
    print(f"netwidth {width}{'' if two_pass else ' one-pass'} retraw + diff_maps vs the two passes apart: {e:.2e}")
    assert torch.isfinite(grads[0]).all() and e <= 2e-4


def test_generic_route_chunks(engines):
    """render_rays_backward(grad_maps=...) with GENERIC_GRAD_CHUNK = 24 (64 rays: passes of 24, 24 and 16): the bits of the one-pass call
    (rays are independent, tests/test_gpu_generic_surface.py::test_chunked_calls_equal_stand_alone_ones), for grad_maps alone, with grad_rgb
    beside it and with grad_raw."""
    o, d, hist, Nc, Ni = g6_rays()
    n = o.shape[0]
    E = engines(32)
    gen = torch.Generator().manual_seed(9)
    G = {k: dev(v) for k, v in random_weights(n, gen).items()}
    Gr = dev(torch.randn(n, Nc + Ni, 9, generator=gen) / (Nc + Ni))
    rest = {k: v for k, v in G.items() if k != "rgb"}
    calls = (lambda: E.render_rays_backward(dev(o), dev(d), dev(hist), Nc, Ni, NEAR, FAR, None, grad_maps=G),
             lambda: E.render_rays_backward(dev(o), dev(d), dev(hist), Nc, Ni, NEAR, FAR, G["rgb"], grad_maps=rest),
             lambda: E.render_rays_backward(dev(o), dev(d), dev(hist), Nc, Ni, NEAR, FAR, None, grad_maps=rest, grad_raw=Gr))
    whole = [c() for c in calls]
    assert torch.equal(whole[0][0], whole[1][0]) and torch.equal(whole[0][1], whole[1][1])   # grad_rgb stands for grad_maps['rgb']
    keep, E.GENERIC_GRAD_CHUNK = E.GENERIC_GRAD_CHUNK, 24
    try:
        parts = [c() for c in calls]
    finally:
        E.GENERIC_GRAD_CHUNK = keep
    for a, b in zip(whole, parts):
        assert torch.isfinite(b[0]).all() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="given twice"):
        E.render_rays_backward(dev(o), dev(d), dev(hist), Nc, Ni, NEAR, FAR, G["rgb"], grad_maps=G)
