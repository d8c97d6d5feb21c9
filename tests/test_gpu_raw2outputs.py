"""raw2outputs_NeRFW and sample_pdf as public device functions (dfnet_amd.rendering, dfnet_amd.engine.raw2outputs / raw2outputs_backward;
dfn_raw2outputs, dfn_raw2outputs_backward): every mode of models/rendering.py:132-243 forward, and the gradient with respect to raw AND
z_vals.

Forward bounds are the ones the project applies to these quantities: relative maximum 3e-6 (tests/test_gpu_nerfh.py::
test_composite_golden_all_modes), 2e-6 for the weights of the coarse test-time mode (test_coarse_weights_golden).
Gradients: truth is torch autograd through the oracle in float64, the yardstick torch's own fp32 autograd of the same oracle, and the HIP
result is held to relative L2 <= 1.5 x yardstick + 2e-4 per tensor (tests/raw2outputs_cases.py::bound, the bound of
tests/test_gpu_maps_grad.py).  The oracle functions are pinned to the reference by G17 (tests/test_raw2outputs_oracle_golden.py)."""
import numpy as np
import pytest
import torch

from dfnet_amd import _lib, engine as eng, rendering
from tests import raw2outputs_cases as rc
from tests.render_maps_cases import golden, relmax
from tests.yardstick import rel_l2

pytestmark = pytest.mark.gpu
T = torch.from_numpy
dev = rc.dev
SHAPES = [(n, N) for n in (5, 7) for N in (1, 2, 24, 63, 64, 65, 128, 192, 200, 320, 512)]
TOL, TOL_W1 = 3e-6, 2e-6
G17 = {"m1": "raw1", "m2": "raw4", "m2w": "raw4", "m3": "raw9", "m3w": "raw9", "m3t": "raw9"}


def tol(tag, name):
    return TOL_W1 if (rc.MODES[tag][0] == 1 and name == "weights") else TOL


def engine_forward(tag, raw, z, noise=None, std=0.):
    return eng.raw2outputs(dev(raw), dev(z), dev(noise), std, 0.1, **rc.engine_opts(tag))


def public_forward(tag, raw, z, noise=None, std=0., rays_d=None):
    """rendering.raw2outputs_NeRFW called as the reference is: positional up to raw_noise_std, the rest by keyword."""
    return rendering.raw2outputs_NeRFW(raw, z, rays_d, std, beta_min=0.1, noise=noise, **rc.MODES[tag][1])


def check_tuple(tag, res, n, N, raw):
    """The reference's 7-tuple, its shapes and its None pattern; -> {name: tensor} of the outputs the mode computes."""
    ch = rc.MODES[tag][0]
    assert isinstance(res, tuple) and len(res) == 7
    rgb, disp, acc, w, depth, tsig, beta = res
    assert acc.shape == (n,) and w.shape == (n, N)
    if ch == 1:
        assert rgb is None and disp is None and depth is None and tsig is None and beta is None
        return dict(acc=acc, weights=w)
    assert rgb.shape == (n, 3) and disp.shape == (n,) and depth.shape == (n,) and beta.shape == (n,)
    if ch == 4:
        assert tsig is None and not bool(beta.any())
        return dict(rgb=rgb, disp=disp, acc=acc, weights=w, depth=depth)
    assert torch.equal(tsig, raw[..., 7])
    return dict(rgb=rgb, disp=disp, acc=acc, weights=w, depth=depth, beta=beta)


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("tag", sorted(G17))
def test_forward_g17_the_reference_itself(tag):
    """The reference's own outputs (G17: 6 rays x 12 samples, sigma of both signs in M1 / M2), engine function and public function."""
    g = golden("g17_raw2outputs")
    raw, z = T(g[G17[tag]]), T(g["z"])
    arg = raw[..., 0] if tag == "m1" else raw
    got = engine_forward(tag, arg, z)
    pub = check_tuple(tag, public_forward(tag, dev(raw), dev(z), rays_d=dev(torch.ones(6, 3))), 6, 12, dev(raw))
    assert set(got) == set(pub) == set(rc.OUTPUTS[rc.MODES[tag][0]])
    for k in got:
        e = relmax(got[k], g[f"{tag}_{k}"])
        print(f"G17 {tag} {k}: {e:.2e}")
        assert e < tol(tag, k), (tag, k, e)
        assert torch.equal(got[k], pub[k]), k


@pytest.mark.parametrize("n,N", SHAPES)
def test_forward_vs_oracle_every_mode(n, N):
    """Every mode and flag combination (rc.MODES), without noise and with explicit noise at raw_noise_std = 0.5 in M1 / M2; n is no multiple
    of the four waves of a block, N covers every samples-per-lane instantiation and the 63 / 64 / 65 lane boundary.  The M3 outputs are
    the bits of engine.composite_fine on the same inputs."""
    fails = []
    for tag, (ch, kw) in rc.MODES.items():
        raw, z, noise, _ = rc.inputs(ch, n, N)
        for std in ((0., 0.5) if ch != 9 else (0.,)):
            ref = rc.oracle(tag, raw, z, noise * std if std else None)
            res = public_forward(tag, dev(raw), dev(z), dev(noise) if std else None, std)
            got = check_tuple(tag, res, n, N, dev(raw))
            direct = engine_forward(tag, raw[..., 0] if ch == 1 else raw, z, noise if std else None, std)
            for k in got:
                assert torch.isfinite(got[k]).all() and torch.equal(got[k], direct[k]), (tag, k)
                e = relmax(got[k], ref[k])
                if not e < tol(tag, k):
                    fails.append((tag, std, k, e))
        if ch == 9:
            old = eng.composite_fine(dev(raw), dev(z), 0.1, kw["test_time"], kw["static_only"], kw["white_bkgd"], want_aux=True)
            for k in got:
                assert torch.equal(got[k], old[k]), (tag, k)
    assert not fails, fails


def test_public_function_refusals_and_noise():
    n, N = 5, 24
    raw9, z, noise, _ = rc.inputs(9, n, N)
    raw4 = rc.inputs(4, n, N)[0]
    r9, r4, zd = dev(raw9), dev(raw4), dev(z)
    with pytest.raises(TypeError, match="NoneType"):        # the reference: deltas * None
        rendering.raw2outputs_NeRFW(r9, zd, None, 0, True, test_time=True, typ="coarse")
    with pytest.raises(NotImplementedError, match="channels"):
        rendering.raw2outputs_NeRFW(r9, zd, None, 0, False, test_time=True, typ="fine")
    with pytest.raises(NotImplementedError, match="channels"):
        rendering.raw2outputs_NeRFW(r4, zd, None, 0, True, typ="fine")
    with pytest.raises(NotImplementedError, match="channels"):
        rendering.raw2outputs_NeRFW(r9[..., :6].contiguous(), zd, None)
    with pytest.raises(ValueError, match="noise"):
        rendering.raw2outputs_NeRFW(r9, zd, None, 0.5, True, typ="fine", noise=dev(noise))
    with pytest.raises(ValueError, match="CUDA"):           # no CPU fallback
        rendering.raw2outputs_NeRFW(raw4, z, None)
    # the defaults are the reference's: typ="coarse", test_time=False, output_transient=False -> M2
    res = rendering.raw2outputs_NeRFW(r4, zd, None)
    assert res[5] is None and torch.equal(res[0], eng.raw2outputs(r4, zd)["rgb"])
    # M1 reads channel 0 of whatever raw has
    a = rendering.raw2outputs_NeRFW(r4, zd, None, test_time=True)
    b = rendering.raw2outputs_NeRFW(r4[..., :1].contiguous(), zd, None, test_time=True)
    assert a[0] is None and torch.equal(a[3], b[3]) and torch.equal(a[2], b[2])
    # raw_noise_std != 0 without noise draws torch.randn on the device: reproducible from the generator's state, and it moves the result
    torch.manual_seed(11)
    one = rendering.raw2outputs_NeRFW(r4, zd, None, 0.5)
    torch.manual_seed(11)
    drawn = torch.randn(n, N, device=zd.device)
    assert torch.equal(one[3], rendering.raw2outputs_NeRFW(r4, zd, None, 0.5, noise=drawn)[3]) and not torch.equal(one[3], res[3])
    # at std 0 nothing is drawn, and the transient mode ignores raw_noise_std as the reference does
    state = torch.cuda.get_rng_state()
    rendering.raw2outputs_NeRFW(r4, zd, None, 0.)
    t = rendering.raw2outputs_NeRFW(r9, zd, None, 0.7, True, typ="fine")
    assert torch.equal(state, torch.cuda.get_rng_state())
    assert torch.equal(t[0], rendering.raw2outputs_NeRFW(r9, zd, None, 0., True, typ="fine")[0])


# ---------------------------------------------------------------------------------------------- the sampler
def test_sample_pdf_public():
    g = golden("g5_sample_pdf")
    bins, w = dev(g["bins"]), dev(g["weights"])
    n = bins.shape[0]
    for Ni, key in ((128, "det128"), (17, "det17")):
        got = rendering.sample_pdf(bins, w, Ni, det=True)
        assert torch.equal(got, eng.sample_pdf(bins, w, Ni)) and relmax(got, g[key]) < 5e-6
    u = dev(g["u"])
    got = rendering.sample_pdf(bins, w, 40, u=u)
    assert torch.equal(got, eng.sample_pdf(bins, w, 40, u=u)) and relmax(got, g["rand40"]) < 5e-6
    assert torch.equal(rendering.sample_pdf(bins, w, 40, det=False, pytest=True), got)     # np.random.seed(0) draws formed on the host
    np.random.seed(0)
    u33 = dev(np.random.rand(n, 33).astype(np.float32))
    assert torch.equal(rendering.sample_pdf(bins, w, 33, pytest=True), rendering.sample_pdf(bins, w, 33, u=u33))
    lin = dev(np.broadcast_to(np.linspace(0., 1., 17), (n, 17)).copy())
    assert torch.equal(rendering.sample_pdf(bins, w, 17, det=True, pytest=True), rendering.sample_pdf(bins, w, 17, u=lin))
    torch.manual_seed(3)
    a = rendering.sample_pdf(bins, w, 21)
    torch.manual_seed(3)
    assert torch.equal(a, rendering.sample_pdf(bins, w, 21, u=torch.rand(n, 21, device=bins.device)))
    wg = w.clone().requires_grad_(True)
    for out in (rendering.sample_pdf(bins, wg, 17, det=True), rendering.sample_pdf(bins.clone().requires_grad_(True), wg, 17, u=lin)):
        assert not out.requires_grad and out.grad_fn is None      # detached, as the reference's only caller leaves it (:302)


# ---------------------------------------------------------------------------------------------- gradients: the stage
def backward(tag, raw, z, G, noise=None, std=0., want=("raw", "z")):
    ch = rc.MODES[tag][0]
    arg = raw[..., 0] if ch == 1 else raw
    graw, gz = eng.raw2outputs_backward(dev(arg), dev(z), {k: dev(v) for k, v in G.items()}, dev(noise), std, 0.1, want=want,
                                        **rc.engine_opts(tag))
    if graw is not None and ch == 1:
        graw = graw[..., None]
    return graw, gz


def upstream_cases(ch, n, N, gen):
    return [(k, {k: rc.one_upstream(k, n, N, gen)}) for k in rc.OUTPUTS[ch]] + [("all", rc.random_upstreams(ch, n, N, gen))]


@pytest.mark.parametrize("n,N", SHAPES)
def test_gradients_vs_float64_oracle(n, N):
    """d L/d raw and d L/d z for each upstream gradient alone and all together, in every arithmetic (rc.GRAD_MODES), M1 / M2 with explicit
    noise at std 0.5.  `acc` alone in the M3 modes is held to finiteness only: its true gradient is delta_i x the transmittance behind the
    ray, below fp32 on rays that end opaque (yardstick 1e8 and more), exactly as tests/test_gpu_maps_grad.py documents for the existing
    stage; test_acc_gradient_on_rays_that_let_light_through holds it to the bound."""
    fails = []
    for tag in rc.GRAD_MODES:
        ch = rc.MODES[tag][0]
        raw, z, noise, gen = rc.inputs(ch, n, N)
        std = 0.5 if ch != 9 else 0.
        for name, G in upstream_cases(ch, n, N, gen):
            graw, gz = backward(tag, raw, z, G, noise if std else None, std)
            assert graw.shape == raw.shape and gz.shape == z.shape and torch.isfinite(graw).all() and torch.isfinite(gz).all(), (tag, name)
            if ch == 9 and name == "acc":
                continue
            truth, yard = rc.yardstick(tag, raw, z, G, noise * std if std else None)
            e = rel_l2(graw, truth[0]), rel_l2(gz, truth[1])
            print(f"n={n} N={N} {tag} {name}: d raw {e[0]:.2e} (torch fp32: {yard[0]:.2e})  d z {e[1]:.2e} (torch fp32: {yard[1]:.2e})")
            assert np.isfinite(yard).all(), (tag, name, yard)
            for what, ee, yy in zip(("raw", "z"), e, yard):
                if not ee <= rc.bound(yy):
                    fails.append((tag, name, what, ee, yy))
            if ch != 9:      # exactly 0 on sigma behind a closed relu gate
                closed = (raw[..., -1] + std * noise) <= 0
                assert not bool(graw[..., -1].cpu()[closed].any()), (tag, name)
    assert not fails, fails


@pytest.mark.parametrize("n,N", [(5, 24), (7, 200)])
def test_acc_gradient_on_rays_that_let_light_through(n, N):
    """Rays with a nearly transparent last sample: d acc / d sigma is of order one, the yardstick is small (required: < 1e-5) and `acc`
    alone, `disp` alone and all together are held to the bound in every arithmetic."""
    for tag in rc.GRAD_MODES:
        ch = rc.MODES[tag][0]
        raw, z, _, gen = rc.inputs(ch, n, N, seed=3, light_through=True)
        cases = [("acc", dict(acc=torch.ones(n)))] + ([("disp", dict(disp=torch.ones(n)))] if ch != 1 else []) + \
                [("all", rc.random_upstreams(ch, n, N, gen))]
        for name, G in cases:
            graw, gz = backward(tag, raw, z, G)
            truth, yard = rc.yardstick(tag, raw, z, G)
            e = rel_l2(graw, truth[0]), rel_l2(gz, truth[1])
            print(f"transparent last sample n={n} N={N} {tag} {name}: d raw {e[0]:.2e} ({yard[0]:.2e})  d z {e[1]:.2e} ({yard[1]:.2e})")
            assert max(yard) < 1e-5 and e[0] <= rc.bound(yard[0]) and e[1] <= rc.bound(yard[1]), (tag, name, e, yard)
            assert float(truth[0][..., 3 if ch == 9 else -1].abs().max()) > 1e-3      # the sigma gradient is not below fp32 here


@pytest.mark.parametrize("N", [1, 24, 130])
def test_gradients_of_degenerate_rays(N):
    """Ray 0: duplicate depths (delta = 0, as the merged fine depths contain them); ray 1: an opaque first sample (sigma = 400 over an
    interval of 0.5 or more: exp(-200) is 0 in fp32); every ray when N = 1.  Finite, and inside the bound ray by ray."""
    n = 3
    for tag in rc.GRAD_MODES:
        ch = rc.MODES[tag][0]
        raw, z, _, gen = rc.inputs(ch, n, N, seed=4)
        if N > 1:
            z[0, N // 3: N // 3 + max(2, N // 6)] = z[0, N // 3]
            z[1, 0], z[1, 1:] = 0., z[1, 1:].clamp_min(0.5)
            raw[1, 0, 3 if ch == 9 else -1] = 400.
        G = rc.random_upstreams(ch, n, N, gen)
        graw, gz = backward(tag, raw, z, G)
        assert torch.isfinite(graw).all() and torch.isfinite(gz).all(), tag
        truth = rc.oracle_grads(tag, raw, z, G, f64=True)
        ref = rc.oracle_grads(tag, raw, z, G)
        for i in range(n):
            for what, got, t, r in (("raw", graw, truth[0], ref[0]), ("z", gz, truth[1], ref[1])):
                yard, e = rel_l2(r[i], t[i]), rel_l2(got[i], t[i])
                print(f"N={N} {tag} ray {i} d {what}: {e:.2e} (torch fp32: {yard:.2e})")
                if np.isfinite(yard):      # torch's fp32 autograd divides by 1 - alpha and may itself return NaN on the opaque ray
                    assert e <= rc.bound(yard), (tag, i, what, e, yard)
                else:
                    assert e <= rc.bound(0.), (tag, i, what, e)


def test_want_halves_null_upstreams_and_errors():
    n, N = 7, 200
    for tag in rc.GRAD_MODES:
        ch = rc.MODES[tag][0]
        raw, z, noise, gen = rc.inputs(ch, n, N, seed=5)
        std = 0.5 if ch != 9 else 0.
        nz = noise if std else None
        G = rc.random_upstreams(ch, n, N, gen)
        graw, gz = backward(tag, raw, z, G, nz, std)
        only_raw, none_z = backward(tag, raw, z, G, nz, std, want=("raw",))
        none_raw, only_z = backward(tag, raw, z, G, nz, std, want=("z",))
        assert none_z is None and none_raw is None and torch.equal(only_raw, graw) and torch.equal(only_z, gz), tag
        # a NULL upstream is a tensor of zeros, bit for bit
        some = {k: v for i, (k, v) in enumerate(G.items()) if i % 2 == 0}
        full = {k: (v if k in some else torch.zeros_like(v)) for k, v in G.items()}
        a, b = backward(tag, raw, z, some, nz, std), backward(tag, raw, z, full, nz, std)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), tag
        with pytest.raises(_lib.DfnError, match=r"status -1"):
            backward(tag, raw, z, {})
        with pytest.raises(_lib.DfnError, match=r"status -1"):
            backward(tag, raw, z, {k: None for k in G})
        with pytest.raises(_lib.DfnError, match=r"status -1"):
            backward(tag, raw, z, G, want=())
        with pytest.raises(ValueError, match="unknown upstream"):
            backward(tag, raw, z, dict(depth_static=torch.ones(n)))
    raw, z, _, _ = rc.inputs(1, n, N, seed=5)
    with pytest.raises(_lib.DfnError, match=r"status -1"):      # M1 returns no rgb: nothing to differentiate
        backward("m1", raw, z, dict(rgb=torch.ones(n, 3)))


@pytest.mark.parametrize("n,N", [(5, 24), (7, 200), (5, 452), (5, 456), (5, 512)])
def test_m3_grad_raw_agrees_with_composite_fine_backward_maps(n, N):
    """(N = 452 is the largest ray whose rows the backward stages through LDS - four of them in 64 KB -, 456 the first it does not.)
    Without d L/d z and without a gradient on weights, M3's d L/d raw is what dfn_composite_fine_backward_maps computes: its `depth` is
    that stage's depth_static under test_time and static_only, and its depth otherwise (where disp, which that stage forms from
    depth_static, is left out)."""
    raw, z, _, gen = rc.inputs(9, n, N, seed=6)
    G = rc.random_upstreams(9, n, N, gen)
    del G["weights"]
    for tag in ("m3", "m3t"):
        Gm = dict(G) if tag == "m3" else {k: v for k, v in G.items() if k != "disp"}
        graw, _ = backward(tag, raw, z, Gm, want=("raw",))
        names = dict(Gm)
        if tag == "m3":
            names["depth_static"] = names.pop("depth")
        old = eng.composite_fine_backward_maps(dev(raw), dev(z), {k: dev(v) for k, v in names.items()})
        truth, yard = rc.yardstick(tag, raw, z, Gm)
        e = rel_l2(graw, old)
        print(f"n={n} N={N} {tag}: d raw vs composite_fine_backward_maps {e:.2e} (torch fp32 vs float64: {yard[0]:.2e})")
        assert e <= rc.bound(yard[0])


# ---------------------------------------------------------------------------------------------- gradients: autograd through the public function
@pytest.mark.parametrize("tag", rc.GRAD_MODES)
def test_autograd_through_the_public_function(tag):
    n, N = 7, 65
    ch = rc.MODES[tag][0]
    raw, z, noise, gen = rc.inputs(ch, n, N, seed=7)
    if ch == 1:      # M1 reads channel 0 of a wider raw
        raw = torch.cat([raw, torch.rand(n, N, 2, generator=gen)], -1).contiguous()
    std = 0.5 if ch != 9 else 0.
    G = {k: dev(v) for k, v in rc.random_upstreams(ch, n, N, gen).items()}
    r, zz = dev(raw).requires_grad_(True), dev(z).requires_grad_(True)
    nz = dev(noise) if std else None
    res = public_forward(tag, r, zz, nz, std)
    out = check_tuple(tag, tuple(None if t is None else t.detach() for t in res), n, N, r.detach())
    names = ("rgb", "disp", "acc", "weights", "depth", "tsig", "beta")
    attached = {k: t for k, t in zip(names, res) if t is not None and not (ch == 4 and k == "beta")}
    assert all(t.requires_grad for t in attached.values()), tag
    plain = engine_forward(tag, raw[..., 0] if ch == 1 else raw, z, noise if std else None, std)
    for k in out:
        assert torch.equal(out[k], plain[k]), k      # the tracked forward is the plain forward
    sum((attached[k] * G[k]).sum() for k in G).backward()
    graw, gz = eng.raw2outputs_backward(r.detach()[..., 0].contiguous() if ch == 1 else r.detach(), zz.detach(), G, nz, std, 0.1,
                                        **rc.engine_opts(tag))
    if ch == 1:
        assert torch.equal(r.grad[..., 0], graw) and not bool(r.grad[..., 1:].any())
    else:
        assert torch.equal(r.grad, graw)
    assert torch.equal(zz.grad, gz)
    # one input alone: needs_input_grad picks the half, the other input gets nothing
    r2, z2 = dev(raw).requires_grad_(True), dev(z)
    res2 = public_forward(tag, r2, z2, nz, std)
    sum((t * G[k]).sum() for k, t in zip(names, res2) if k in G).backward()
    assert torch.equal(r2.grad, r.grad) and z2.grad is None
    r3, z3 = dev(raw), dev(z).requires_grad_(True)
    res3 = public_forward(tag, r3, z3, nz, std)
    sum((t * G[k]).sum() for k, t in zip(names, res3) if k in G).backward()
    assert torch.equal(z3.grad, gz) and r3.grad is None
    # a subset of the outputs: the unused ones arrive as NULL upstreams
    k0 = "weights" if ch == 1 else "rgb"
    r4, z4 = dev(raw).requires_grad_(True), dev(z).requires_grad_(True)
    res4 = dict(zip(names, public_forward(tag, r4, z4, nz, std)))
    (res4[k0] * G[k0]).sum().backward()
    g1 = eng.raw2outputs_backward(r.detach()[..., 0].contiguous() if ch == 1 else r.detach(), zz.detach(), {k0: G[k0]}, nz, std, 0.1,
                                  **rc.engine_opts(tag))
    assert torch.equal(r4.grad[..., 0] if ch == 1 else r4.grad, g1[0]) and torch.equal(z4.grad, g1[1])
    with torch.no_grad():
        res5 = public_forward(tag, r, zz, nz, std)
    assert all(t is None or not t.requires_grad for t in res5)


def test_autograd_transient_sigmas_alone():
    """transient_sigmas is raw[..., 7]: a loss on it alone reaches that channel and nothing else, and no compositing kernel runs."""
    n, N = 5, 24
    raw, z, _, gen = rc.inputs(9, n, N, seed=8)
    G = dev(torch.randn(n, N, generator=gen))
    r, zz = dev(raw).requires_grad_(True), dev(z).requires_grad_(True)
    res = public_forward("m3t", r, zz)
    (res[5] * G).sum().backward()
    assert torch.equal(r.grad[..., 7], G) and not bool(r.grad[..., :7].any()) and not bool(r.grad[..., 8].any())
    assert zz.grad is None or not bool(zz.grad.any())
