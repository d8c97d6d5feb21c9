"""The acceptance test of the public compositor and sampler: a renderer composed by the caller from the point queries,
rendering.raw2outputs_NeRFW and rendering.sample_pdf (query -> composite -> sample -> sort -> query -> composite, the body of the
reference's render_rays at test time, models/rendering.py:245-337) against rendering.render on the same rays - forward, and the gradient
with respect to the rays under autograd.  G6's 64 rays at 8 + 16 samples, netwidth 128, split-f16."""
import pytest
import torch

from dfnet_amd import rendering
from tests import test_gpu_generic_surface as gs
from tests.render_maps_cases import golden, relmax
from tests.test_gpu_points import wrapped
from tests.yardstick import rel_l2

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"
NEAR, FAR = 0., 2.5


@pytest.fixture(scope="module")
def scene():
    g = golden("g6_render_rays_a")
    assert int(g["Nc"]) == 8 and int(g["Ni"]) == 16 and g["rays_o"].shape == (64, 3)
    q, mods, _ = wrapped(width=128, seed=0, precision="f16x3")
    rays = tuple(T(g[k]).float().to(DEV).contiguous() for k in ("rays_o", "rays_d"))
    return q, mods, rays, T(g["hist"]).float().reshape(1, -1).to(DEV), 8, 16


def composed(q, mods, o, d, hist, Nc, Ni):
    """The reference's test-time render_rays written out by a caller -> raw2outputs_NeRFW's 7-tuple of the fine pass."""
    coarse, fine, emb_a, emb_t = mods
    n = o.shape[0]
    viewdirs = d / torch.norm(d, dim=-1, keepdim=True)
    t = torch.linspace(0., 1., Nc, device=o.device)
    z = (NEAR * (1. - t) + FAR * t).expand(n, Nc)
    with torch.no_grad():      # the coarse query has no input gradient, and needs none: the samples drawn from it are detached
        sigma = q(o[:, None] + d[:, None] * z[..., None], viewdirs, hist, coarse, 'coarse', emb_a, emb_t, False, True)
    _, _, _, weights, _, _, _ = rendering.raw2outputs_NeRFW(sigma, z, d, 0., False, test_time=True, typ="coarse")
    z_mid = .5 * (z[:, 1:] + z[:, :-1])
    z_samples = rendering.sample_pdf(z_mid, weights[..., 1:-1], Ni, det=True)
    z_fine, _ = torch.sort(torch.cat([z, z_samples], -1), -1)
    pts = o[:, None] + d[:, None] * z_fine[..., None]      # two rounded operations, as tests/test_gpu_points.py forms its points
    raw = q(pts, viewdirs, hist, fine, 'fine', emb_a, emb_t, True, True)
    return rendering.raw2outputs_NeRFW(raw, z_fine, d, 0., True, test_time=True, typ="fine")


def test_composed_renderer_forward(scene):
    """rgb, disp, acc within 4e-5 of rendering.render(rays=...): each side is held to 2e-5 of the oracle
    (tests/render_maps_cases.py::TOL)."""
    q, mods, (o, d), hist, Nc, Ni = scene
    with torch.no_grad():
        rgb, disp, acc, w, depth, tsig, beta = composed(q, mods, o, d, hist, Nc, Ni)
        ref = rendering.render(480, 640, 585., rays=torch.stack([o, d]), near=NEAR, far=FAR, img_idx=hist, **gs.kwargs(q.engine, Nc, Ni))
    assert w.shape == (64, Nc + Ni) and tsig.shape == (64, Nc + Ni) and beta.shape == (64,) and ref[3] == {}
    for name, a, b in zip(("rgb", "disp", "acc"), (rgb, disp, acc), ref[:3]):
        e = relmax(a, b)
        print(f"composed renderer vs render(): {name} {e:.2e}")
        assert e < 4e-5, name
    assert q.engine.range_flags() == 0


def test_composed_renderer_ray_gradients(scene):
    """d L/d (rays_o, rays_d) of a random-weighted loss over rgb, disp, acc and depth through the composition against
    render(rays, diff_maps=True, ret_maps=("depth_static",)): 2e-4 relative L2, the fp32 ray-gradient bound of tests/test_gpu_grad.py::TOL.
    Both routes run the fine network's gradient kernel on the same points and differ in the compositor's round-off."""
    q, mods, (o, d), hist, Nc, Ni = scene
    gen = torch.Generator().manual_seed(17)
    G = {k: torch.randn((64, 3) if k == "rgb" else (64,), generator=gen).to(DEV) for k in ("rgb", "disp", "acc", "depth")}
    oo, dd = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    rgb, disp, acc, _, depth, _, _ = composed(q, mods, oo, dd, hist, Nc, Ni)
    assert all(t.requires_grad for t in (rgb, disp, acc, depth))
    ((rgb * G["rgb"]).sum() + (disp * G["disp"]).sum() + (acc * G["acc"]).sum() + (depth * G["depth"]).sum()).backward()
    rays = torch.stack([o, d]).requires_grad_(True)
    r_rgb, r_disp, r_acc, extras = rendering.render(480, 640, 585., rays=rays, near=NEAR, far=FAR, img_idx=hist, diff_maps=True,
                                                    ret_maps=("depth_static",), **gs.kwargs(q.engine, Nc, Ni))
    ((r_rgb * G["rgb"]).sum() + (r_disp * G["disp"]).sum() + (r_acc * G["acc"]).sum() + (extras["depth_static"] * G["depth"]).sum()).backward()
    assert torch.isfinite(oo.grad).all() and torch.isfinite(dd.grad).all() and float(oo.grad.abs().max()) > 0
    e_o, e_d = rel_l2(oo.grad, rays.grad[0]), rel_l2(dd.grad, rays.grad[1])
    print(f"composed renderer vs render(diff_maps): d rays_o {e_o:.2e}, d rays_d {e_d:.2e}")
    assert e_o <= 2e-4 and e_d <= 2e-4
