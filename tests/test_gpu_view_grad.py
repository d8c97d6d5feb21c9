"""render(ndc=True / c2w_staticcam=..., diff_view=True) under autograd and in training mode (models/rendering.py:364-376, which the
reference runs as plain tensor ops): the adjoints of ndc_rays and of viewdirs = d / |d| as stages, the render nodes with explicit view
directions on every route (netwidth 128 two-pass and one-pass, the generic route), the training step with explicit view directions in its
three modes, and the refusals that stay.

Scene: syn.nerfh_weights(0), the pose and the static pose of G14 (tests/golden/g14_render_ndc_staticcam.npz), H x W = 6 x 8, focal 7.3; NDC
renders near 0 / far 1, the static camera near 0 / far 2.5; 8 + 16 samples at test time, 16 + 24 in training mode.

Truth: torch.autograd through the CPU oracle in float64 (tests/yardstick.py).  `yard` is the distance of the SAME oracle in fp32 from it on
the same inputs, and the bound is the project's rule  error <= 3 x yard + TOL  (tests/test_gpu_train.py:321), errors relative to the largest
entry of the truth, TOL = 2e-4 per ray and 2e-3 for a pose gradient (tests/test_gpu_grad.py:28-31).  Weight gradients: relative L2 per tensor,
`exact` within 3 x yard + 2e-4, `fused` / `fused_split` within 3 x max(yard, exact) + 5e-4 (tests/test_gpu_train.py:321-323).  A ray on a ReLU
gate (yardstick.rays_off_a_gate) may be left out, at most 1 of 48, and is printed.

Measured figures: LABBOOK, "ndc and c2w_staticcam under autograd"."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dfnet_amd import engine as eng, nerf_train, nerfw, rendering
from dfnet_amd import synthetic as syn
from dfnet_amd._lib import current_stream, ptr
from oracle import nerfh_oracle as orc
from tests.yardstick import float64_default, rays_off_a_gate, rel_l2, to64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
H, W, FOCAL = 6, 8, 7.3
NC, NI = 8, 16           # test time
TNC, TNI = 16, 24        # training mode
TOL_RAY, TOL_C2W = 2e-4, 2e-3


def dev(x):
    return torch.as_tensor(x).float().to(DEV).contiguous()


def relmax(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert not torch.isnan(a).any()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------- the oracle half (runs without a GPU)
def g14():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_render_ndc_staticcam.npz")))


def weights(width=128):
    cw, fw, ea, et = syn.nerfh_weights(0, W=width)
    return (cw, fw, ea, et), ({k: T(v) for k, v in cw.items()}, {k: T(v) for k, v in fw.items()}, T(ea), T(et))


def get_rays(c2w):
    """orc.get_rays in the dtype of the pose (the oracle's casts its pose to fp32; the float64 truth must not)."""
    cx = ((torch.linspace(0, W - 1, W, dtype=c2w.dtype) - W * .5) / FOCAL)[None, :].expand(H, W)
    cy = (-(torch.linspace(0, H - 1, H, dtype=c2w.dtype) - H * .5) / FOCAL)[:, None].expand(H, W)
    cam = torch.stack([cx, cy, -torch.ones(H, W, dtype=c2w.dtype)], -1)
    rays_d = torch.sum(cam[..., None, :] * c2w[:3, :3], -1)
    return c2w[:3, 3].expand(rays_d.shape).reshape(-1, 3), rays_d.reshape(-1, 3)


def view_rows(x, hist, near, far, ndc):
    """rendering.py:364-389 on the leaves x (out of o, d, c2w, static): the oracle's 21-float ray rows [o d near far viewdir hist], in the
    dtype of the leaves (orc.pack_ray_rows has this layout but casts to fp32), with the view directions of the given rays / pose and the
    rays of the static camera and / or the NDC map."""
    o, d = get_rays(x["c2w"]) if "c2w" in x else (x["o"], x["d"])
    view = d / torch.norm(d, dim=-1, keepdim=True)
    if "static" in x:
        o, d = get_rays(x["static"])
    if ndc:
        o, d = orc.ndc_rays(H, W, FOCAL, 1., o, d)
    n = o.shape[0]
    col = lambda v: torch.full((n, 1), v, dtype=o.dtype)
    return torch.cat([o, d, col(near), col(far), view, hist.to(o.dtype).reshape(1, -1).repeat(n, 1)], 1)


def oracle_outputs(x, w, hist, Nc, Ni, near, far, ndc):
    """rgb, acc, raw and the joint depth sum w z of the test-time render, attached to the leaves."""
    st = {}
    out = orc.render_rays(view_rows(x, hist, near, far, ndc), *w, Nc, Ni, retraw=True, stages=st)
    return dict(rgb=out["rgb_map"], acc=out["acc_map"], raw=out["raw"], depth=orc.composite_fine(out["raw"], st["z_fine"], test_time=False)["depth"])


def weighted(out, G):
    return sum((out[k] * G[k].to(out[k].dtype)).sum() for k in G)


def oracle_grads(x, loss_of, f64=False):
    """{leaf: d loss_of(leaves) / d leaf} by autograd, in fp32 or float64."""
    if f64:
        with float64_default():
            return oracle_grads(to64(x), loss_of)
    x = {k: v.detach().clone().requires_grad_(True) for k, v in x.items()}
    loss_of(x).backward()
    return {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in x.items()}


def render_loss(w, hist, Nc, Ni, near, far, ndc, G):
    """x -> the loss sum_k (output_k * G_k) of the test-time render, with the weights in the dtype of the leaves."""
    def loss_of(x):
        ww = to64(w) if next(iter(x.values())).dtype == torch.float64 else w
        return weighted(oracle_outputs(x, ww, hist, Nc, Ni, near, far, ndc), G)
    return loss_of


def holds(tag, got, ref32, ref64, tol):
    """error <= 3 x yard + tol, both relative to the largest entry of the float64 truth; prints the figures first."""
    yard, e = relmax(ref32, ref64), relmax(got, ref64)
    print(f"{tag}: {e:.2e} from float64 (torch fp32: {yard:.2e}; bound {3 * yard + tol:.2e})")
    assert np.isfinite(yard) and e <= 3 * yard + tol, (tag, e, yard)


def ray_holds(tag, got, x, loss_for, tol=TOL_RAY):
    """The per-ray rule for d rays_o / d rays_d.  loss_for(rows or None) -> loss_of restricted to those rays (None: all)."""
    ref32, ref64 = oracle_grads(x, loss_for(None)), oracle_grads(x, loss_for(None), f64=True)

    def single64(i, delta):
        xi = {"o": x["o"][i:i + 1].double() + delta, "d": x["d"][i:i + 1].double()}
        with float64_default():
            g = oracle_grads(xi, loss_for(slice(i, i + 1)))
        return torch.cat([g["o"][0], g["d"][0]])
    cat = lambda g: torch.cat([g["o"].detach().cpu(), g["d"].detach().cpu()], -1)
    keep = rays_off_a_gate(cat(got), cat(ref64), single64, max_frac=1. / 48)
    assert int((~keep).sum()) <= 1
    if not bool(keep.all()):
        print(f"{tag}: ray {int((~keep).nonzero()[0])} sits on a ReLU gate (its float64 gradient itself moves) and is left out")
    for k in ("o", "d"):
        holds(f"{tag} d rays_{k}", got[k].detach().cpu()[keep], ref32[k][keep], ref64[k][keep], tol)


def loss_weights(n, Nf, seed, names=("rgb",)):
    gen = torch.Generator().manual_seed(seed)
    shape = dict(rgb=(n, 3), acc=(n,), depth=(n,), raw=(n, Nf, 9))
    return {k: torch.randn(shape[k], generator=gen) / (Nf if k == "raw" else 1) for k in names}


# ---------------------------------------------------------------------------------------------- engines
_ENGINES = {}


def engine(width):
    if width not in _ENGINES:
        _ENGINES[width] = eng.NerfHEngine(width=width, precision="f32").load_numpy(*weights(width)[0])
    return _ENGINES[width]


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    _ENGINES.clear()


@pytest.fixture()
def fp32_tracked():
    """Engine precision f32 with the split-f16 gradient kernels, as tests/test_gpu_grad.py runs its oracle comparisons."""
    rendering.GRAD_FORWARD_PRECISION = "f32"
    try:
        yield
    finally:
        rendering.GRAD_FORWARD_PRECISION = None
        rendering.GRAD_TWO_PASS = True


def kwargs(E, Nc=NC, Ni=NI, **over):
    kw = dict(network_query_fn=nerfw.HipQuery(E, 65536), perturb=False, N_importance=Ni, N_samples=Nc, use_viewdirs=True, white_bkgd=False,
              raw_noise_std=0., test_time=True, ndc=False, lindisp=False)
    kw.update(over)
    return kw


ROUTES = [(128, True), (128, False), (32, True)]   # (netwidth, GRAD_TWO_PASS): two-pass, one-pass, the generic route


# ---------------------------------------------------------------------------------------------- a. the adjoint of ndc_rays
def ndc_inputs(n, seed=3):
    g = g14()
    o, d = get_rays(T(g["c2w"]))
    gen = torch.Generator().manual_seed(seed)
    pick = torch.arange(n) % o.shape[0]
    o = o[pick] + 0.05 * torch.randn(n, 3, generator=gen)
    d = d[pick] + (0.01 * torch.randn(n, 3, generator=gen) if n > 48 else 0.)
    return o.contiguous(), d.contiguous(), torch.randn(n, 3, generator=gen), torch.randn(n, 3, generator=gen)


@pytest.mark.parametrize("n", [48, 1, 257])
def test_ndc_rays_backward_vs_float64_autograd(n):
    """dfn_ndc_rays_backward against float64 autograd of orc.ndc_rays with random upstream gradients: the 48 rays of the G14 pose with
    jittered origins, one ray, and 257 = one past a 256-thread block; both upstreams and each alone.  Bound 3 x yard + 1e-6."""
    o, d, Go, Gd = ndc_inputs(n)
    for tag, go, gd in (("both", Go, Gd), ("d L/d o' alone", Go, None), ("d L/d d' alone", None, Gd)):
        def loss_of(x):
            no, nd = orc.ndc_rays(H, W, FOCAL, 1., x["o"], x["d"])
            return (0. if go is None else (no * go.to(no.dtype)).sum()) + (0. if gd is None else (nd * gd.to(nd.dtype)).sum())
        x = dict(o=o, d=d)
        ref32, ref64 = oracle_grads(x, loss_of), oracle_grads(x, loss_of, f64=True)
        got_o, got_d = eng.ndc_rays_backward(H, W, FOCAL, 1., dev(o), dev(d), None if go is None else dev(go), None if gd is None else dev(gd))
        assert got_o.shape == (n, 3) and got_d.shape == (n, 3)
        holds(f"ndc_rays_backward n={n} {tag}: d o", got_o, ref32["o"], ref64["o"], 1e-6)
        holds(f"ndc_rays_backward n={n} {tag}: d d", got_d, ref32["d"], ref64["d"], 1e-6)
    with pytest.raises(ValueError, match="both None"):
        eng.ndc_rays_backward(H, W, FOCAL, 1., dev(o), dev(d))
    # ... and as the public function: ray_utils.ndc_rays(diff=True) attaches the same bits, diff=False stays detached
    od, dd = dev(o).requires_grad_(True), dev(d).requires_grad_(True)
    plain = rendering.ndc_rays(H, W, FOCAL, 1., od, dd)
    no, nd = rendering.ndc_rays(H, W, FOCAL, 1., od, dd, diff=True)
    assert not plain[0].requires_grad and no.requires_grad and torch.equal(no, plain[0]) and torch.equal(nd, plain[1])
    ((no * dev(Go)).sum() + (nd * dev(Gd)).sum()).backward()
    both = eng.ndc_rays_backward(H, W, FOCAL, 1., dev(o), dev(d), dev(Go), dev(Gd))
    assert torch.equal(od.grad, both[0]) and torch.equal(dd.grad, both[1])


# ---------------------------------------------------------------------------------------------- b. the adjoint of v = d / |d|
@pytest.mark.parametrize("n", [48, 1, 257])
def test_viewdirs_backward_vs_autograd(n):
    """dfn_viewdirs_backward against torch autograd of d / |d| (float64), within 1e-6 of the largest entry; accumulate adds to a buffer."""
    _, d, G, fill = ndc_inputs(n, seed=5)
    d64 = d.double().requires_grad_(True)
    ((d64 / torch.norm(d64, dim=-1, keepdim=True)) * G.double()).sum().backward()
    got = eng.viewdirs_backward(dev(d), dev(G))
    e = relmax(got, d64.grad)
    print(f"viewdirs_backward n={n}: {e:.2e} from float64 autograd")
    assert got.shape == (n, 3) and e < 1e-6
    buf = dev(fill)
    out = eng.viewdirs_backward(dev(d), dev(G), out=buf)
    assert out is buf and relmax(buf, d64.grad + fill.double()) < 1e-6


# ---------------------------------------------------------------------------------------------- c. ndc under autograd
@pytest.mark.parametrize("width,two_pass", ROUTES)
def test_ndc_render_of_rays_under_autograd(fp32_tracked, width, two_pass):
    """render(rays=..., ndc=True, diff_view=True): d loss / d rays against the float64 oracle, per ray."""
    rendering.GRAD_TWO_PASS = two_pass
    g, (_, w), E = g14(), weights(width), engine(width)
    hist = T(g["hist"])
    o, d = get_rays(T(g["c2w"]))
    G = loss_weights(48, NC + NI, 21)
    od, dd = dev(o).requires_grad_(True), dev(d).requires_grad_(True)
    rgb, disp, acc, extras = rendering.render(H, W, FOCAL, rays=(od, dd), near=0., far=1., img_idx=dev(hist)[None], diff_view=True,
                                              **kwargs(E, ndc=True))
    assert rgb.shape == (48, 3) and rgb.requires_grad and not disp.requires_grad and extras == {}
    with torch.no_grad():   # the values are those of the untracked render of the same arithmetic
        ref = orc.render(H, W, FOCAL, 1 << 30, *w, NC, NI, 0., 1., g["hist"], rays=(o, d), ndc=True)[0]
    assert relmax(rgb, ref) < 2e-5
    (rgb * dev(G["rgb"])).sum().backward()
    loss_for = lambda rows: render_loss(w, hist, NC, NI, 0., 1., True, G if rows is None else {k: v[rows] for k, v in G.items()})
    ray_holds(f"netwidth {width} two_pass={two_pass} render(rays, ndc)", dict(o=od.grad, d=dd.grad), dict(o=o, d=d), loss_for)


@pytest.mark.parametrize("width,two_pass", ROUTES)
def test_ndc_render_of_a_pose_under_autograd(fp32_tracked, gold, width, two_pass):
    """render(c2w=..., ndc=True, diff_view=True): rgb within 2e-5 of the reference's own NDC render (G14, at its 16 + 32 samples, netwidth
    128), d loss / d c2w against the float64 oracle."""
    rendering.GRAD_TWO_PASS = two_pass
    g, (_, w), E = gold("g14_render_ndc_staticcam"), weights(width), engine(width)
    hist = T(g["hist"])
    if width == 128:
        pose = dev(g["c2w"]).requires_grad_(True)
        rgb = rendering.render(H, W, FOCAL, c2w=pose, near=0., far=1., img_idx=dev(hist)[None], diff_view=True,
                               **kwargs(E, int(g["Nc"]), int(g["Ni"]), ndc=True))[0]
        e = relmax(rgb, g["rgb_ndc"])
        print(f"two_pass={two_pass} tracked ndc render vs the reference's (G14): {e:.2e}")
        assert rgb.shape == (H, W, 3) and rgb.requires_grad and e < 2e-5
    G = loss_weights(48, NC + NI, 22)
    pose = dev(g["c2w"]).requires_grad_(True)
    rgb = rendering.render(H, W, FOCAL, c2w=pose, near=0., far=1., img_idx=dev(hist)[None], diff_view=True, **kwargs(E, ndc=True))[0]
    (rgb.reshape(-1, 3) * dev(G["rgb"])).sum().backward()
    x, loss_of = dict(c2w=T(g["c2w"])), render_loss(w, hist, NC, NI, 0., 1., True, G)
    holds(f"netwidth {width} two_pass={two_pass} render(c2w, ndc): d c2w", pose.grad, oracle_grads(x, loss_of)["c2w"],
          oracle_grads(x, loss_of, f64=True)["c2w"], TOL_C2W)


# ---------------------------------------------------------------------------------------------- d. c2w_staticcam under autograd
def static_case(E, w, g, G, ndc, pose_grad, static_grad, near, far, **over):
    """One tracked render with c2w_staticcam -> (outputs, pose, static, the oracle's leaves and loss)."""
    pose, static = dev(g["c2w"]).requires_grad_(pose_grad), dev(g["c2w_staticcam"]).requires_grad_(static_grad)
    out = rendering.render(H, W, FOCAL, c2w=pose, c2w_staticcam=static, near=near, far=far, img_idx=dev(g["hist"])[None], diff_view=True,
                           **kwargs(E, ndc=ndc, **over))
    x = dict(c2w=T(g["c2w"]), static=T(g["c2w_staticcam"]))
    return out, pose, static, x, render_loss(w, T(g["hist"]), NC, NI, near, far, ndc, G)


@pytest.mark.parametrize("width,two_pass", ROUTES)
def test_static_camera_under_autograd(fp32_tracked, gold, width, two_pass):
    """render(c2w=..., c2w_staticcam=..., diff_view=True): d c2w arrives through the view directions alone (its translation column gets
    exactly nothing), d c2w_staticcam when it requires grad, a call with only c2w_staticcam requiring grad is tracked, and both options
    together (the static camera's rays through the NDC map)."""
    rendering.GRAD_TWO_PASS = two_pass
    g, (_, w), E = gold("g14_render_ndc_staticcam"), weights(width), engine(width)
    G = loss_weights(48, NC + NI, 23)
    tag = f"netwidth {width} two_pass={two_pass} c2w_staticcam"
    for ndc, near, far in ((False, 0., 2.5), (True, 0., 1.)):
        (rgb, disp, acc, extras), pose, static, x, loss_of = static_case(E, w, g, G, ndc, True, True, near, far)
        assert rgb.shape == (H, W, 3) and rgb.requires_grad and not disp.requires_grad and extras == {}
        if width == 128 and not ndc:   # (at G14's sample counts the untracked test compares; here against the oracle at 8 + 16)
            with torch.no_grad():
                ref = orc.render(H, W, FOCAL, 1 << 30, *w, NC, NI, near, far, g["hist"], c2w=T(g["c2w"]), c2w_staticcam=T(g["c2w_staticcam"]))[0]
            assert relmax(rgb, ref) < 2e-5
        (rgb.reshape(-1, 3) * dev(G["rgb"])).sum().backward()
        ref32, ref64 = oracle_grads(x, loss_of), oracle_grads(x, loss_of, f64=True)
        assert float(ref64["c2w"][:, 3].abs().max()) == 0. and float(pose.grad[:, 3].abs().max()) == 0.
        holds(f"{tag} ndc={ndc}: d c2w", pose.grad, ref32["c2w"], ref64["c2w"], TOL_C2W)
        holds(f"{tag} ndc={ndc}: d c2w_staticcam", static.grad, ref32["static"], ref64["static"], TOL_C2W)
    # only the static camera requires grad: tracked, and the same gradient (the same kernels on the same values)
    (rgb2, _, _, _), pose2, static2, _, _ = static_case(E, w, g, G, True, False, True, 0., 1.)
    assert rgb2.requires_grad and torch.equal(rgb2, rgb)
    (rgb2.reshape(-1, 3) * dev(G["rgb"])).sum().backward()
    assert pose2.grad is None and torch.equal(static2.grad, static.grad)
    # only the pose: the static camera is a constant
    (rgb3, _, _, _), pose3, static3, _, _ = static_case(E, w, g, G, True, True, False, 0., 1.)
    (rgb3.reshape(-1, 3) * dev(G["rgb"])).sum().backward()
    assert static3.grad is None and torch.equal(pose3.grad, pose.grad)


@pytest.mark.parametrize("width,two_pass", ROUTES)
def test_static_camera_with_retraw_and_diff_maps(fp32_tracked, gold, width, two_pass):
    """retraw=True with diff_maps=True, ret_maps='depth': a loss over raw, depth and acc (and rgb) reaches both poses; against the oracle
    composed from orc.render_rays and orc.composite_fine."""
    rendering.GRAD_TWO_PASS = two_pass
    g, (_, w), E = gold("g14_render_ndc_staticcam"), weights(width), engine(width)
    G = loss_weights(48, NC + NI, 24, names=("rgb", "acc", "depth", "raw"))
    (rgb, disp, acc, extras), pose, static, x, loss_of = static_case(E, w, g, G, False, True, True, 0., 2.5, retraw=True, diff_maps=True,
                                                                     ret_maps=("depth",))
    assert sorted(extras) == ["depth", "raw"] and all(t.requires_grad for t in (rgb, disp, acc, extras["depth"], extras["raw"]))
    got = dict(rgb=rgb.reshape(-1, 3), acc=acc.reshape(-1), depth=extras["depth"].reshape(-1), raw=extras["raw"].reshape(48, NC + NI, 9))
    weighted(got, {k: dev(v) for k, v in G.items()}).backward()
    ref32, ref64 = oracle_grads(x, loss_of), oracle_grads(x, loss_of, f64=True)
    tag = f"netwidth {width} two_pass={two_pass} c2w_staticcam, loss over rgb, acc, depth, raw"
    holds(f"{tag}: d c2w", pose.grad, ref32["c2w"], ref64["c2w"], TOL_C2W)
    holds(f"{tag}: d c2w_staticcam", static.grad, ref32["static"], ref64["static"], TOL_C2W)


# ---------------------------------------------------------------------------------------------- e. training mode
def modules(width):
    """(engine, [coarse, fine, emb_a, emb_t] on the GPU, trainer) with the scene's weights."""
    (cw, fw, ea, et), _ = weights(width)
    coarse = nerfw.NeRFW('coarse', D=8, W=width, skips=[4], in_channels_xyz=63, in_channels_dir=27)
    fine = nerfw.NeRFW('fine', D=8, W=width, skips=[4], in_channels_xyz=63, in_channels_dir=27, encode_appearance=True, encode_transient=True,
                       in_channels_a=50, in_channels_t=20)
    coarse.load_state_dict({k: T(v) for k, v in cw.items()})
    fine.load_state_dict({k: T(v) for k, v in fw.items()})
    emb_a, emb_t = torch.nn.Embedding(1000, 5), torch.nn.Embedding(1000, 2)
    emb_a.weight.data.copy_(T(ea))
    emb_t.weight.data.copy_(T(et))
    mods = [m.to(DEV) for m in (coarse, fine, emb_a, emb_t)]
    E = eng.NerfHEngine(width=width, precision="f32").load_numpy(cw, fw, ea, et)
    tr = nerf_train.NerfHTrainer(E, *mods)
    tr.range_check = "repeat"
    return E, mods, tr


# Seed of the target and the three draws per netwidth, fixed on the oracle alone before any GPU run (the per-ray procedure below with the
# fp32 oracle's own gradient in the place of the HIP one, seeds 31 .. 38): the first seed at which the fp32 oracle's worst ray is below the
# 1e-3 at which rays_off_a_gate starts to examine a ray, so that the one ray in 48 the rule allows is there for the code under test.  In
# training mode (40 samples through two 8-layer ReLU networks per ray) most seeds have one ray whose float64 gradient itself moves under a
# 3e-6 shift of its origin: fp32 yard 1e-2 with it, 1e-4 without.
TRAIN_SEED = {128: 33, 32: 31, "static": 32}   # "static": the pose-gradient case at netwidth 128, the seed of the smallest fp32 yard (7e-5)


def train_inputs(seed):
    g = g14()
    o, d = get_rays(T(g["c2w"]))
    gen = torch.Generator().manual_seed(seed)
    target = torch.rand(48, 3, generator=gen)
    draws = (torch.rand(48, TNC, generator=gen), torch.randn(48, TNC, generator=gen), torch.rand(48, TNI, generator=gen))
    return o.contiguous(), d.contiguous(), T(g["hist"]), target, draws


def train_loss(w, hist, target, draws, rows=None):
    """leaves (o, d and, when present, the named parameters) -> sum(NerfWLoss) of the training render of the NDC rays with the view
    directions of the given rays: orc.ndc_rays, the ray rows with rows[:, 8:11] = view, orc.render_rays_train, orc.nerfw_loss.
    rows: the loss of those rays alone, as they enter the batch's: every term of NerfWLoss is a mean over the rays, so the loss of a
    subset is scaled by its share of the 48 (the gradient of ray i alone is then row i of the batch gradient, which is what
    rays_off_a_gate compares it with; tests/test_gpu_train.py:483-491 cancels the same 1/R)."""
    sl = slice(None) if rows is None else rows
    share = 1. if rows is None else len(range(*rows.indices(48))) / 48.

    def loss_of(x):
        f64 = x["o"].dtype == torch.float64
        cast = to64 if f64 else (lambda v: v)
        cw, fw, ea, et = cast(w)
        cw = {k: x.get("coarse." + k, v) for k, v in cw.items()}
        fw = {k: x.get("fine." + k, v) for k, v in fw.items()}
        ea, et = x.get("embedding_a.weight", ea), x.get("embedding_t.weight", et)
        out = orc.render_rays_train(view_rows(x, hist, 0., 1., True), cw, fw, ea, et, TNC, TNI, *(cast(t)[sl] for t in draws), perturb=1.,
                                    raw_noise_std=0.)
        ld = orc.nerfw_loss({'rgb_fine': out['rgb_map'], 'rgb_coarse': out['rgb0'], 'beta': out['beta'],
                             'transient_sigmas': out['transient_sigmas']}, cast(target)[sl])
        return sum(ld.values()) * share
    return loss_of


def train_kwargs(E, mods, tr, **over):
    kw = dict(network_query_fn=nerfw.HipQuery(E, trainer=tr), perturb=1., N_importance=TNI, network_fine=mods[1], N_samples=TNC,
              network_fn=mods[0], use_viewdirs=True, white_bkgd=False, raw_noise_std=0., embedding_a=mods[2], embedding_t=mods[3],
              test_time=False, ndc=False, lindisp=False)
    kw.update(over)
    return kw


def device_loss(rgb, extras, target):
    ld = orc.nerfw_loss({'rgb_fine': rgb, 'rgb_coarse': extras['rgb0'], 'beta': extras['beta'], 'transient_sigmas': extras['transient_sigmas']},
                        target)
    return sum(ld.values())


def named_params(w):
    cw, fw, ea, et = w
    P = {"coarse." + k: v for k, v in cw.items()}
    P.update({"fine." + k: v for k, v in fw.items()})
    P.update({"embedding_a.weight": ea, "embedding_t.weight": et})
    return P


@pytest.fixture(scope="module")
def train128():
    """The netwidth-128 training scene and its oracle gradients (fp32 and float64), computed once."""
    E, mods, tr = modules(128)
    _, w = weights(128)
    o, d, hist, target, draws = train_inputs(TRAIN_SEED[128])
    x = dict(o=o, d=d, **named_params(w))
    loss_of = train_loss(w, hist, target, draws)
    return dict(E=E, mods=mods, tr=tr, w=w, o=o, d=d, hist=hist, target=target, draws=draws, ref32=oracle_grads(x, loss_of),
                ref64=oracle_grads(x, loss_of, f64=True))


def train_render(s, rays_grad, **over):
    o, d = dev(s["o"]).requires_grad_(rays_grad), dev(s["d"]).requires_grad_(rays_grad)
    for p in s["tr"].params:
        p.grad = None
    rgb, disp, acc, extras = rendering.render(H, W, FOCAL, rays=(o, d), near=0., far=1., img_idx=dev(s["hist"])[None],
                                              draws=tuple(dev(t) for t in s["draws"]), **train_kwargs(s["E"], s["mods"], s["tr"], **over))
    return o, d, rgb, extras


def test_training_render_with_ndc_weight_and_ray_gradients(train128):
    """render(test_time=False, ndc=True, diff_view=True), 48 rays, 16 + 24 samples, fixed draws, NerfWLoss: the weight gradients of the
    exact, fused and fused_split steps against the float64 oracle, and d rays of the exact step per ray."""
    s = train128
    tr, ref32, ref64 = s["tr"], s["ref32"], s["ref64"]
    got, err = {}, {}
    try:
        for tag, exact, split, rays_grad in (("exact", True, False, True), ("fused", False, False, False), ("fused_split", False, True, False)):
            tr.exact, tr.fused_split = exact, split
            o, d, rgb, extras = train_render(s, rays_grad, ndc=True, diff_view=True)
            assert rgb.shape == (48, 3) and rgb.requires_grad
            device_loss(rgb, extras, dev(s["target"])).backward()
            assert tr._saved["exact"] == exact and tr._saved["viewdirs_given"]
            got[tag] = {k: p.grad.detach().cpu().clone() for k, p in zip(tr.names, tr.params)}
            if rays_grad:
                rays = dict(o=o.grad, d=d.grad)
    finally:
        tr.exact, tr.fused_split = False, False
    assert s["E"].range_flags() == 0
    worst = dict(yard=0., exact=0., fused=0., fused_split=0.)
    for k in tr.names:
        if float(ref64[k].abs().max()) == 0.:   # a parameter the loss does not reach (None in torch)
            continue
        yard = rel_l2(ref32[k], ref64[k])
        e = {t: rel_l2(got[t][k], ref64[k]) for t in got}
        worst = {t: max(worst[t], v) for t, v in dict(e, yard=yard).items()}
        err[k] = (e, yard)
    print("training render with ndc, worst relative L2 from float64 over the gradient tensors:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, (e, yard) in err.items():
        assert e["exact"] <= 3. * yard + 2e-4, (k, e, yard)
        for t in ("fused", "fused_split"):
            assert e[t] <= 3. * max(yard, e["exact"]) + 5e-4, (k, t, e, yard)
    loss_for = lambda rows: train_loss(s["w"], s["hist"], s["target"], s["draws"], rows)
    ray_holds("training render with ndc (exact step)", rays, dict(o=s["o"], d=s["d"]), loss_for)


def test_training_render_with_ndc_at_netwidth_32():
    """The same on the exact step of another netwidth (32: the layer-by-layer products are the only step there)."""
    E, mods, tr = modules(32)
    _, w = weights(32)
    o, d, hist, target, draws = train_inputs(TRAIN_SEED[32])
    s = dict(E=E, mods=mods, tr=tr, o=o, d=d, hist=hist, target=target, draws=draws)
    od, dd, rgb, extras = train_render(s, True, ndc=True, diff_view=True)
    device_loss(rgb, extras, dev(target)).backward()
    assert tr._saved["exact"] and tr._saved["viewdirs_given"]
    x = dict(o=o, d=d, **named_params(w))
    loss_of = train_loss(w, hist, target, draws)
    ref32, ref64 = oracle_grads(x, loss_of), oracle_grads(x, loss_of, f64=True)
    worst = dict(yard=0., exact=0.)
    for k, p in zip(tr.names, tr.params):
        if float(ref64[k].abs().max()) == 0.:
            continue
        yard, e = rel_l2(ref32[k], ref64[k]), rel_l2(p.grad, ref64[k])
        worst = dict(yard=max(worst["yard"], yard), exact=max(worst["exact"], e))
        assert e <= 3. * yard + 2e-4, (k, e, yard)
    print("netwidth 32 training render with ndc, worst relative L2 from float64:", {k: f"{v:.2e}" for k, v in worst.items()})
    ray_holds("netwidth 32 training render with ndc", dict(o=od.grad, d=dd.grad), dict(o=o, d=d),
              lambda rows: train_loss(w, hist, target, draws, rows))


def test_training_render_with_a_static_camera(train128, gold):
    """c2w_staticcam in training mode: the pose receives its gradient through the view directions alone, the static pose through the rays;
    against the float64 oracle (d c2w rule)."""
    s, g = train128, gold("g14_render_ndc_staticcam")
    tr = s["tr"]
    _, _, _, target, draws = train_inputs(TRAIN_SEED["static"])
    pose, static = dev(g["c2w"]).requires_grad_(True), dev(g["c2w_staticcam"]).requires_grad_(True)
    for p in tr.params:
        p.grad = None
    rgb, disp, acc, extras = rendering.render(H, W, FOCAL, c2w=pose, c2w_staticcam=static, near=0., far=2.5, img_idx=dev(s["hist"])[None],
                                              draws=tuple(dev(t) for t in draws), diff_view=True, **train_kwargs(s["E"], s["mods"], tr))
    assert rgb.shape == (H, W, 3) and rgb.requires_grad
    device_loss(rgb.reshape(-1, 3), {k: v.reshape(48, *v.shape[2:]) for k, v in extras.items()}, dev(target)).backward()
    assert tr._saved["exact"] and float(pose.grad[:, 3].abs().max()) == 0. and tr.params[0].grad is not None

    def loss_of(x):
        cast = to64 if x["c2w"].dtype == torch.float64 else (lambda v: v)
        out = orc.render_rays_train(view_rows(x, s["hist"], 0., 2.5, False), *cast(s["w"]), TNC, TNI, *cast(draws), perturb=1., raw_noise_std=0.)
        return sum(orc.nerfw_loss({'rgb_fine': out['rgb_map'], 'rgb_coarse': out['rgb0'], 'beta': out['beta'],
                                   'transient_sigmas': out['transient_sigmas']}, cast(target)).values())
    x = dict(c2w=T(g["c2w"]), static=T(g["c2w_staticcam"]))
    ref32, ref64 = oracle_grads(x, loss_of), oracle_grads(x, loss_of, f64=True)
    holds("training render with c2w_staticcam: d c2w", pose.grad, ref32["c2w"], ref64["c2w"], TOL_C2W)
    holds("training render with c2w_staticcam: d c2w_staticcam", static.grad, ref32["static"], ref64["static"], TOL_C2W)


@pytest.mark.parametrize("exact", [False, True])
def test_train_forward_v_keeps_the_bits_of_train_forward(train128, gold, exact):
    """dfn_nerfh_train_forward_v with NULL view directions, and with the device's own normalised rays_d (dfn_raygen's), returns the bits of
    dfn_nerfh_train_forward: the fused chains and the exact step."""
    s, g = train128, gold("g14_render_ndc_staticcam")
    tr, E = s["tr"], s["E"]
    o, d, v = (t.reshape(-1, 3).contiguous() for t in eng.raygen(H, W, FOCAL, dev(g["c2w"])))
    hist, draws = dev(s["hist"])[None], tuple(dev(t) for t in s["draws"])
    names = ("rgb_map", "disp_map", "acc_map", "raw", "rgb0", "disp0", "acc0", "z_std", "beta")
    base = {k: t.clone() for k, t in tr.forward(o, d, hist, TNC, TNI, 0., 2.5, draws[0], draws[1], 0.5, draws[2], exact=exact).items()}
    given = tr.forward(o, d, hist, TNC, TNI, 0., 2.5, draws[0], draws[1], 0.5, draws[2], exact=exact, viewdirs=v)
    assert tr._saved["viewdirs_given"] and tr._saved["exact"] == exact
    for k in names:
        assert torch.equal(given[k], base[k]), k
    # NULL through the entry itself (the trainer calls the plain entry when it has no view directions)
    out = {k: torch.empty_like(base[k]) for k in names}
    ws = tr._workspace(48, TNC, TNI, o.device)
    tr.set_mode(exact)
    rc = tr.lib.dfn_nerfh_train_forward_v(E.handle, tr._ptr_array(tr.params), ptr(o), ptr(d), None, ptr(hist), 1, 48, TNC, TNI, 0., 2.5, ptr(draws[0]),
                                          ptr(draws[1]), 0.5, ptr(draws[2]), *(ptr(out[k]) for k in names), ctypes.c_void_p(ws.data_ptr()),
                                          ws.numel(), current_stream())
    assert rc == 0
    for k in names:
        assert torch.equal(out[k], base[k]), k
    # view directions that differ do change the render: the pointer is live
    other = tr.forward(o, d, hist, TNC, TNI, 0., 2.5, draws[0], draws[1], 0.5, draws[2], exact=exact, viewdirs=v.flip(0).contiguous())
    assert not torch.equal(other["rgb_map"], base["rgb_map"])
    assert E.range_flags() == 0


# ---------------------------------------------------------------------------------------------- f. nothing else moved
def test_without_the_keyword_everything_is_as_before(fp32_tracked, train128, gold):
    g, E = gold("g14_render_ndc_staticcam"), engine(128)
    hist = dev(g["hist"])[None]
    # the three refusals, with their texts, now naming the keyword
    pose = dev(g["c2w"]).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="autograd.*diff_view"):
        rendering.render(H, W, FOCAL, c2w=pose, near=0., far=1., img_idx=hist, **kwargs(E, ndc=True))
    o, d = get_rays(T(g["c2w"]))
    rays = torch.stack([dev(o), dev(d)]).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="ndc / c2w_staticcam together with autograd.*diff_view"):
        rendering.render(H, W, FOCAL, rays=rays, near=0., far=1., img_idx=hist, diff_maps=True, **kwargs(E, ndc=True))
    with pytest.raises(NotImplementedError, match="ndc / c2w_staticcam together with autograd.*diff_view"):
        rendering.render(H, W, FOCAL, c2w=pose, c2w_staticcam=dev(g["c2w_staticcam"]), near=0., far=2.5, img_idx=hist, **kwargs(E))
    s = train128
    with pytest.raises(NotImplementedError, match="ndc / c2w_staticcam together with training-mode rendering.*diff_view"):
        train_render(s, False, ndc=True, diff_maps=True)
    # without the keyword a static pose that requires grad does not make the call tracked
    static = dev(g["c2w_staticcam"]).requires_grad_(True)
    rgb = rendering.render(H, W, FOCAL, c2w=dev(g["c2w"]), c2w_staticcam=static, near=0., far=2.5, img_idx=hist, **kwargs(E))[0]
    assert not rgb.requires_grad
    # render_frames keeps refusing, with or without the keyword
    poses = dev(g["c2w"])[None].requires_grad_(True)
    for over in ({}, dict(diff_view=True)):
        with pytest.raises(NotImplementedError, match="ndc / c2w_staticcam together with autograd"):
            rendering.render_frames(H, W, FOCAL, poses, hist, near=0., far=1., **kwargs(E, ndc=True, **over))
    # diff_view=True without ndc / c2w_staticcam: the same bits, values and gradients, at test time ...
    G = dev(loss_weights(48, NC + NI, 25)["rgb"])
    res = []
    for over in ({}, dict(diff_view=True)):
        rr = torch.stack([dev(o), dev(d)]).requires_grad_(True)
        rgb, disp, acc, _ = rendering.render(H, W, FOCAL, rays=rr, near=0., far=2.5, img_idx=hist, **kwargs(E), **over)
        (rgb * G).sum().backward()
        pp = dev(g["c2w"]).requires_grad_(True)
        img = rendering.render(H, W, FOCAL, c2w=pp, near=0., far=2.5, img_idx=hist, **kwargs(E), **over)[0]
        (img.reshape(-1, 3) * G).sum().backward()
        res.append((rgb.detach(), disp, acc, rr.grad, img.detach(), pp.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # ... and in training mode
    res = []
    for over in ({}, dict(diff_view=True)):
        od, dd, rgb, extras = train_render(s, True, **over)
        device_loss(rgb, extras, dev(s["target"])).backward()
        res.append([rgb.detach(), extras["beta"].detach(), od.grad, dd.grad] + [p.grad.clone() for p in s["tr"].params])
    for a, b in zip(*res):
        assert torch.equal(a, b)
