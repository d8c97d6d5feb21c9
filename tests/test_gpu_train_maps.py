"""Training-mode render with every output attached: the compositing backward of both passes for all their outputs
(dfn_composite_coarse_train_backward_maps / dfn_composite_fine_train_backward_maps, models/rendering.py:161-243 with test_time=False),
the two depths of rendering.py:241 (dfn_nerfh_train_depths), the step entries that use them (dfn_nerfh_train_backward_maps /
_backward_rays_maps, all three train modes) and render(test_time=False, diff_maps=True).

Truth: torch.autograd through the CPU oracle in float64 (tests/yardstick.py).  Yardstick: torch's own fp32 autograd of the same oracle.
Bounds are those of the tests whose inputs these copy (named at each test).  Measured figures: the docstrings and LABBOOK R10.1."""
import ctypes

import numpy as np
import pytest
import torch

from dfnet_amd import _lib, engine as eng, nerf_train, synthetic as syn
from oracle import nerfh_oracle as orc
from tests import test_gpu_maps_grad as mg
from tests import test_gpu_train as tt
from tests.yardstick import float64_default, rays_off_a_gate, rel_l2, to64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.from_numpy
COARSE = ("rgb0", "disp0", "acc0", "depth0")
FINE = ("rgb", "disp", "acc", "depth", "beta")
bound = mg.bound   # 1.5 x yardstick + 2e-4: the form the project applies to compositing gradients


def dev(x):
    return None if x is None else torch.as_tensor(x).float().to(DEV).contiguous()


def act_prime(raw):
    """d raw / d pre-activation from the outputs: c (1 - c) on the Sigmoid heads, 1 - exp(-sigma) on the Softplus heads (3, 7, 8)."""
    d = raw * (1 - raw)
    for c in (3, 7, 8):
        if c < raw.shape[-1]:
            d[..., c] = -torch.expm1(-raw[..., c])
    return d


def weighted(out, G, strip):
    return sum((out[k[:-1] if strip else k] * G[k]).sum() for k in G)


def coarse_gpre(raw4, z, noise, G, f64=False):
    """Expected gpre [n,Nc,4]: autograd d sum_k (output_k G_k) / d raw4 through orc.composite_coarse_train, times the activation derivative."""
    if f64:
        with float64_default():
            return coarse_gpre(*to64((raw4, z, noise, G)))
    r = raw4.detach().clone().requires_grad_(True)
    g = torch.autograd.grad(weighted(orc.composite_coarse_train(r, z, noise), G, True), r)[0]
    return g * act_prime(raw4)


def fine_gpre(raw, z, G, f64=False):
    if f64:
        with float64_default():
            return fine_gpre(*to64((raw, z, G)))
    r = raw.detach().clone().requires_grad_(True)
    g = torch.autograd.grad(weighted(orc.composite_fine(r, z, test_time=False), G, False), r)[0]
    return g * act_prime(raw)


def one_hot(name, n):
    return mg.one_hot("rgb" if name.startswith("rgb") else "x", n)


def random_weights(names, n, gen):
    return {k: torch.randn((n, 3) if k.startswith("rgb") else (n,), generator=gen) for k in names}


def coarse_inputs(n, Nc, seed=0, with_noise=False):
    raw, z, gen = mg.stage_inputs(n, Nc, seed)
    noise = torch.randn(n, Nc, generator=gen) if with_noise else None
    return raw[..., :4].contiguous(), z, noise, gen


def hip_coarse(raw4, z, noise, G):
    return eng.composite_coarse_train_backward_maps(dev(raw4), dev(z), {k: dev(v) for k, v in G.items()}, noise=dev(noise), noise_std=1.).cpu()


def hip_fine(raw, z, G, **kw):
    return eng.composite_fine_train_backward_maps(dev(raw), dev(z), {k: dev(v) for k, v in G.items()}, **kw).cpu()


# ---------------------------------------------------------------------------------------------- 1. the stages against float64
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("n,Nc", [(n, Nc) for n in (5, 7) for Nc in (3, 24, 63, 64, 65, 130)])
def test_coarse_stage_vs_float64_oracle(n, Nc, with_noise):
    """Each upstream gradient alone (one-hot per ray) and all four with random weights; noise = N(0,1) x 1 closes a fair share of the ReLU
    gates (those entries are exactly 0), and noise = NULL.
    Measured on an MI355X (LABBOOK R10.1; relative L2 from float64, torch fp32's own in brackets), worst over the 24 cases: rgb0 alone
    5.9e-7 (4.8e-7), depth0 alone 5.8e-7 (1.5e-7), disp0 alone 6.0e-7 (1.5e-7), all four 7.0e-7 (1.9e-7); acc0 alone: the true gradient is
    below fp32 on most of these rays (see the transparent-last-sample test): 1.0 (1.0) where both return 0."""
    raw4, z, noise, gen = coarse_inputs(n, Nc, with_noise=with_noise)
    cases = [(k, {k: one_hot(k, n)}) for k in COARSE] + [("all", random_weights(COARSE, n, gen))]
    fails = []
    for tag, G in cases:
        truth, ref = coarse_gpre(raw4, z, noise, G, f64=True), coarse_gpre(raw4, z, noise, G)
        got = hip_coarse(raw4, z, noise, G)
        assert got.shape == (n, Nc, 4) and torch.isfinite(got).all()
        yard, e = rel_l2(ref, truth), rel_l2(got, truth)
        print(f"coarse n={n} Nc={Nc} noise={with_noise} {tag}: HIP {e:.2e} vs float64 (torch fp32: {yard:.2e})")
        assert np.isfinite(yard)
        if not e <= bound(yard):
            fails.append((tag, e, yard))
        if with_noise:
            closed = (raw4[..., 3] + noise) <= 0
            assert closed.any() and bool((got[..., 3][closed] == 0).all()), tag
    assert not fails, fails


@pytest.mark.parametrize("n,Nf", [(n, Nf) for n in (5, 7) for Nf in (4, 24, 63, 64, 65, 128, 200, 512)])
def test_fine_stage_vs_float64_oracle(n, Nf):
    """Each upstream gradient alone and all five with random weights, over the 64-sample block boundaries and the largest ray.
    Measured on an MI355X (LABBOOK R10.1), worst over the 16 shapes, all at Nf = 512: rgb alone 2.3e-6 (torch fp32: 2.0e-6), beta alone
    2.6e-6 (2.5e-6), depth alone 1.1e-6 (1.7e-7), disp alone 3.9e-7 (1.3e-7), all five 1.3e-6 (1.1e-6); acc alone 1.0 (2.9e10): below fp32."""
    raw, z, gen = mg.stage_inputs(n, Nf)
    cases = [(k, {k: one_hot(k, n)}) for k in FINE] + [("all", random_weights(FINE, n, gen))]
    fails = []
    for tag, G in cases:
        truth, ref = fine_gpre(raw, z, G, f64=True), fine_gpre(raw, z, G)
        got = hip_fine(raw, z, G)
        assert got.shape == (n, Nf, 9) and torch.isfinite(got).all()
        yard, e = rel_l2(ref, truth), rel_l2(got, truth)
        print(f"fine n={n} Nf={Nf} {tag}: HIP {e:.2e} vs float64 (torch fp32: {yard:.2e})")
        assert np.isfinite(yard)
        if not e <= bound(yard):
            fails.append((tag, e, yard))
    assert not fails, fails


def test_stages_stay_finite_with_an_opaque_sample():
    """sigma = 50 on one sample, next to a wide interval so that 1 - alpha underflows to 0 in fp32 (torch's cumprod backward divides by it):
    finite gradients from both kernels; held to the bound wherever torch's own fp32 gradient is finite.
    Measured on an MI355X (LABBOOK R10.1), the ray with the opaque sample: fine 1.3e-7 (torch fp32: 9.8e-8), coarse 1.7e-7 (1.1e-7)."""
    n, gen = 5, torch.Generator().manual_seed(77)
    raw, z, _ = mg.stage_inputs(n, 24, seed=2)
    raw[0, 3, 3] = 50.
    z[0, 4:] += 3.   # delta_3 > 3: exp(-150) = 0
    G = random_weights(FINE, n, gen)
    got = hip_fine(raw, z, G)
    assert torch.isfinite(got).all()
    truth, ref = fine_gpre(raw, z, G, f64=True), fine_gpre(raw, z, G)
    for i in range(n):
        yard, e = rel_l2(ref[i], truth[i]), rel_l2(got[i], truth[i])
        print(f"fine, ray {i}{' (opaque sample)' if i == 0 else ''}: HIP {e:.2e} vs float64 (torch fp32: {yard:.2e})")
        assert not np.isfinite(yard) or e <= bound(yard), (i, e, yard)
    raw4, zc, noise, _ = coarse_inputs(n, 24, seed=2, with_noise=True)
    raw4[0, 3, 3], noise[0, 3] = 50., 0.
    zc[0, 4:] += 3.
    G = random_weights(COARSE, n, gen)
    got = hip_coarse(raw4, zc, noise, G)
    assert torch.isfinite(got).all()
    truth, ref = coarse_gpre(raw4, zc, noise, G, f64=True), coarse_gpre(raw4, zc, noise, G)
    for i in range(n):
        yard, e = rel_l2(ref[i], truth[i]), rel_l2(got[i], truth[i])
        print(f"coarse, ray {i}{' (opaque sample)' if i == 0 else ''}: HIP {e:.2e} vs float64 (torch fp32: {yard:.2e})")
        assert not np.isfinite(yard) or e <= bound(yard), (i, e, yard)


@pytest.mark.parametrize("kernel,n,N", [("coarse", 5, 24), ("coarse", 7, 130), ("fine", 5, 24), ("fine", 7, 200)])
def test_stage_acc_gradient_on_rays_that_let_light_through(kernel, n, N):
    """tests/test_gpu_maps_grad.py's transparent-last-sample case: with a last interval of 1e2 the true acc gradient (delta_i x the
    transmittance behind the last sample) is below fp32 on the rays above; here the last sample is nearly transparent (coarse sigma 1e-3;
    fine 1e-3 / 2e-3) and it is of order one.  acc alone, disp alone, all together; the yardstick must be < 1e-5.
    Measured on an MI355X (LABBOOK R10.1): coarse acc0 1.5e-7 (torch fp32: 1.4e-7) / 4.8e-7 (1.8e-7), disp0 1.1e-7 / 2.2e-7, all 2.0e-7 /
    3.2e-7 at 5 x 24 / 7 x 130; fine acc 2.1e-7 (4.9e-7) / 5.6e-7 (5.9e-7), disp 1.7e-7 / 1.9e-7, all 2.0e-7 / 4.7e-7 at 5 x 24 / 7 x 200."""
    if kernel == "coarse":
        raw, z, noise, gen = coarse_inputs(n, N, seed=3)
        raw[:, -1, 3] = 1e-3
        names, sfx = COARSE, "0"
        run = lambda G, f64=False: coarse_gpre(raw, z, None, G, f64=f64)
        hip = lambda G: hip_coarse(raw, z, None, G)
    else:
        raw, z, gen = mg.stage_inputs(n, N, seed=3)
        raw[:, -1, 3], raw[:, -1, 7] = 1e-3, 2e-3
        names, sfx = FINE, ""
        run = lambda G, f64=False: fine_gpre(raw, z, G, f64=f64)
        hip = lambda G: hip_fine(raw, z, G)
    for tag, G in (("acc", {"acc" + sfx: torch.ones(n)}), ("disp", {"disp" + sfx: torch.ones(n)}), ("all", random_weights(names, n, gen))):
        truth, ref, got = run(G, f64=True), run(G), hip(G)
        yard, e = rel_l2(ref, truth), rel_l2(got, truth)
        print(f"transparent last sample, {kernel} n={n} N={N} {tag}: HIP {e:.2e} vs float64 (torch fp32: {yard:.2e})")
        assert np.isfinite(yard) and yard < 1e-5 and e <= bound(yard), (tag, e, yard)


# ---------------------------------------------------------------------------------------------- 2. NULL and linearity
def test_null_is_zero_subsets_and_raw_ext():
    """A NULL member is a zero tensor, bit for bit; any subset equals the full struct with zeros elsewhere; grad_raw_ext alone reproduces
    itself times the activation derivative; with upstream gradients it is the sum of the two results (1e-6 of the largest entry: the sum
    is formed before the activation derivative in one case and after it in the other); nothing given is DFN_ERR_ARG."""
    n, Nf, Nc = 7, 200, 65
    raw, z, gen = mg.stage_inputs(n, Nf, seed=1)
    rawd, zd = dev(raw), dev(z)
    G = {k: dev(v) for k, v in random_weights(FINE, n, gen).items()}
    zeros = {k: torch.zeros_like(v) for k, v in G.items()}
    fine = lambda g, **kw: eng.composite_fine_train_backward_maps(rawd, zd, g, **kw)
    for given in (("rgb",), ("disp",), ("acc",), ("depth", "beta"), ("rgb", "acc", "disp"), FINE[:-1]):
        some = fine({k: G[k] for k in given})
        assert torch.equal(some, fine({k: (G[k] if k in given else zeros[k]) for k in FINE})), given
        assert torch.equal(some, fine({k: (G[k] if k in given else None) for k in FINE})), given
    for bad in ({}, {k: None for k in FINE}, {k: G["acc"] for k in ("acc0", "disp0")}):   # coarse members do not count for the fine kernel
        with pytest.raises(_lib.DfnError, match=r"status -1"):
            fine(bad)
    ext = dev(torch.randn(n, Nf, 9, generator=gen))
    prime = rawd * (1 - rawd)
    for c in (3, 7, 8):
        prime[..., c] = -torch.expm1(-rawd[..., c])
    alone = fine({}, grad_raw=ext)
    print(f"grad_raw_ext alone vs ext x activation derivative (torch): max difference {float((alone - ext * prime).abs().max()):.2e}")
    assert torch.equal(alone[..., (0, 1, 2, 4, 5, 6)], (ext * rawd * (1 - rawd))[..., (0, 1, 2, 4, 5, 6)])
    assert torch.equal(alone[..., (3, 7, 8)], (ext * prime)[..., (3, 7, 8)])
    both, apart = fine(G, grad_raw=ext), fine(G) + alone
    assert float((both - apart).abs().max()) <= 1e-6 * float(apart.abs().max())
    const = fine({}, g_tsigma=0.25)   # the constant d L / d transient_sigma alone: channel 7 only
    assert torch.equal(const[..., 7], 0.25 * prime[..., 7])
    assert float(const[..., :7].abs().max()) == 0 and float(const[..., 8].abs().max()) == 0
    # coarse
    raw4, zc, noise, gen = coarse_inputs(n, Nc, seed=1, with_noise=True)
    r4, zcd, nd = dev(raw4), dev(zc), dev(noise)
    Gc = {k: dev(v) for k, v in random_weights(COARSE, n, gen).items()}
    zc0 = {k: torch.zeros_like(v) for k, v in Gc.items()}
    coarse = lambda g: eng.composite_coarse_train_backward_maps(r4, zcd, g, noise=nd, noise_std=1.)
    for given in (("rgb0",), ("disp0",), ("acc0",), ("depth0",), ("rgb0", "disp0"), COARSE[1:]):
        some = coarse({k: Gc[k] for k in given})
        assert torch.equal(some, coarse({k: (Gc[k] if k in given else zc0[k]) for k in COARSE})), given
    for bad in ({}, {k: None for k in COARSE}, {"acc": Gc["acc0"]}):
        with pytest.raises(_lib.DfnError, match=r"status -1"):
            coarse(bad)
    assert torch.equal(coarse(Gc), coarse(Gc))   # deterministic
    assert torch.equal(fine(G, grad_raw=ext), both)


# ---------------------------------------------------------------------------------------------- step setups (copied from tests/test_gpu_train.py)
def lossA(out, depth, depth0, td, R):
    """Mean squares of depth - td, depth0 - td, disp - 1/td, disp0 - 1/td, acc - 0.9, acc0 - 0.9 (sums divided by R)."""
    sq = lambda x, t: ((x - t) ** 2).sum() / R
    return (sq(depth, td) + sq(depth0, td) + sq(out["disp_map"], 1. / td) + sq(out["disp0"], 1. / td) + sq(out["acc_map"], 0.9) +
            sq(out["acc0"], 0.9))


def nerfw(out, target):
    return sum(orc.nerfw_loss({'rgb_fine': out['rgb_map'], 'rgb_coarse': out['rgb0'], 'beta': out['beta'],
                               'transient_sigmas': out['raw'][..., 7]}, target).values())


SEED_KEYS = dict(rgb="rgb_map", disp="disp_map", acc="acc_map", depth="depth", beta="beta", rgb0="rgb0", disp0="disp0", acc0="acc0", depth0="depth0")


def seeds(out, td, target=None, extra=None):
    """(g_maps, g_raw) of loss A (+ NerfWLoss when target is given, + extra(leaves)) at the outputs of a forward(maps=True), by torch."""
    leaves = {k: out[k].detach().clone().requires_grad_(True) for k in list(SEED_KEYS.values()) + ["raw"]}
    loss = lossA(leaves, leaves["depth"], leaves["depth0"], td, td.shape[0])
    if target is not None:
        loss = loss + nerfw(leaves, target)
    if extra is not None:
        loss = loss + extra(leaves)
    loss.backward()
    return {k: leaves[v].grad for k, v in SEED_KEYS.items() if leaves[v].grad is not None}, leaves["raw"].grad


def oracle_step(rows, target, cw, fw, ea, et, Nc, Ni, draws, std, td, with_nerfw, f64=False):
    """{name: gradient or None} of loss A (+ NerfWLoss) through orc.render_rays_train, and the oracle's outputs with the two depths."""
    if f64:
        with float64_default():
            return oracle_step(*to64((rows, target, cw, fw, ea, et)), Nc, Ni, to64(draws), std, to64(td), with_nerfw)
    P = {"coarse." + k: v.detach().clone().requires_grad_(True) for k, v in cw.items()}
    P.update({"fine." + k: v.detach().clone().requires_grad_(True) for k, v in fw.items()})
    P["embedding_a.weight"], P["embedding_t.weight"] = ea.detach().clone().requires_grad_(True), et.detach().clone().requires_grad_(True)
    c = {k[7:]: v for k, v in P.items() if k.startswith("coarse.")}
    f = {k[5:]: v for k, v in P.items() if k.startswith("fine.")}
    st = {}
    out = orc.render_rays_train(rows, c, f, P["embedding_a.weight"], P["embedding_t.weight"], Nc, Ni, *draws, 1., std, stages=st)
    out["depth"] = st["depth_fine"]
    out["depth0"] = orc.composite_coarse_train(st["raw_coarse"], st["z_coarse"], draws[1] * std)["depth"]
    loss = lossA(out, out["depth"], out["depth0"], td, td.shape[0])
    if with_nerfw:
        loss = loss + nerfw(out, target)
    g = torch.autograd.grad(loss, list(P.values()), allow_unused=True)
    return dict(zip(P, g)), {k: v.detach() for k, v in out.items()}


def draw_td(R, gen):
    return 1. + 0.3 * torch.sigmoid(torch.randn(R, generator=gen))


def rows_of(o, d, hist, far=2.5):
    R = o.shape[0]
    return torch.cat([o, d, torch.zeros(R, 1), torch.full((R, 1), far), d / d.norm(dim=-1, keepdim=True), hist.expand(R, -1)], 1)


@pytest.fixture(scope="module")
def setup96():
    """The rays and draws of tests/test_gpu_train.py::test_render_training_autograd_surface_and_optimizer_step (96 rays, 16 + 32)."""
    E, mods, w = tt.modules()
    tr = nerf_train.NerfHTrainer(E, *mods)
    R, Nc, Ni = 96, 16, 32
    rng = np.random.default_rng(6)
    ro, rd = orc.get_rays(480, 640, 585.0, T(syn.orbit_pose(6, 8))[:3, :4])
    sel = rng.choice(480 * 640, R, replace=False)
    o, d = ro.reshape(-1, 3)[sel].contiguous().to(DEV), rd.reshape(-1, 3)[sel].contiguous().to(DEV)
    hist, target = T(syn.HIST_IDX)[None].to(DEV), T(rng.uniform(0, 1, (R, 3)).astype(np.float32)).to(DEV)
    draws = nerf_train.NerfHTrainer.draw(R, Nc, Ni, 1., DEV, torch.Generator(device=DEV).manual_seed(3))
    td = draw_td(R, torch.Generator().manual_seed(3)).to(DEV)
    return dict(E=E, mods=mods, w=w, tr=tr, R=R, Nc=Nc, Ni=Ni, o=o, d=d, hist=hist, target=target, draws=draws, td=td)


# ---------------------------------------------------------------------------------------------- 3. old and new agree where they overlap
@pytest.mark.parametrize("exact", [True, False])
def test_new_entry_equals_the_old_one_on_the_nerfw_operands(setup96, exact):
    """backward(g_maps = rgb, rgb0, beta; g_raw with channel 7 alone) against backward(g_rgb, g_rgb0, g_beta, g_tsigma_dense): two
    differently rounded compositing kernels in front of the same step, every gradient tensor within 5e-5 relative L2
    (tests/test_gpu_train.py:222).
    The coarse stage keeps the default step's own kernel for its rgb0 term (csrc/nerfh_train_maps.hip), so the coarse gradients are the
    old entry's bit for bit; the fine kernels differ by round-off.  Measured on an MI355X (LABBOOK R10.1): exact 9.8e-8
    (embedding_t.weight), fused 1.9e-6 (fine.xyz_encoding_1.0.weight) worst.  (With the rgb0 term inside the new coarse kernel — same
    source expressions, contracted differently by the compiler — coarse.static_sigma.0.weight / .bias sat 6.7e-5 / 6.9e-5 (exact) and
    9.6e-5 (fused) away: that head's gradient cancels to ~1e-3 of its terms.)"""
    s = setup96
    tr, R, Nc, Ni = s["tr"], s["R"], s["Nc"], s["Ni"]
    out = tr.forward(s["o"], s["d"], s["hist"], Nc, Ni, 0., 2.5, s["draws"][0], s["draws"][1], 0., s["draws"][2], exact=exact)
    _, (g_rgb, g_rgb0, g_beta), g_ts = tr.loss(out, s["target"])
    dense = torch.rand(R, Nc + Ni, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8)) * (2 * g_ts)
    old = [g.clone() for g in tr.backward(g_rgb, g_rgb0, g_beta, 0., dense, grads=[torch.empty_like(p) for p in tr.params])]
    g_raw = torch.zeros(R, Nc + Ni, 9, device=DEV)
    g_raw[..., 7] = dense
    new = tr.backward(g_maps=dict(rgb=g_rgb, rgb0=g_rgb0, beta=g_beta), g_raw=g_raw, grads=[torch.empty_like(p) for p in tr.params])
    worst = max((rel_l2(a, b), k) for k, a, b in zip(tr.names, new, old))
    print(f"new entry vs old entry on the NerfWLoss operands ({'exact' if exact else 'fused'}): worst {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < 5e-5, worst
    with pytest.raises(ValueError, match="given twice"):
        tr.backward(g_rgb, g_rgb0, g_beta, g_maps=dict(rgb=g_rgb))
    assert s["E"].range_flags() == 0


# ---------------------------------------------------------------------------------------------- 4. whole step against float64, parameters
UNREACHED_A = [f"{net}.{k}.{p}" for net, keys in (("coarse", ("xyz_encoding_final", "dir_encoding.0", "static_rgb.0")),
                                                   ("fine", ("dir_encoding.0", "static_rgb.0", "transient_rgb.0", "transient_beta.0")))
               for k in keys for p in ("weight", "bias")] + ["embedding_a.weight"]


def test_map_losses_on_trained_like_weights_against_the_float64_oracle():
    """The inputs of tests/test_gpu_train.py::test_fused_step_on_trained_like_weights_against_the_float64_oracle (trained-like weights, 256
    rays, 64 + 128, raw_noise_std 1, generator seed 9), td drawn next from the same generator.  Loss A (the six map terms) and loss B
    (A + NerfWLoss): every gradient tensor of the three implementations against float64 autograd, that test's bounds — exact <= 3 x
    yardstick + 2e-4, fused and fused-split <= 3 x max(yardstick, exact) + 5e-4.  Under loss A the 15 tensors the reference does not
    reach are exactly zero.  Measured on an MI355X (LABBOOK R10.1), worst tensor per implementation: loss A yardstick 3.0e-4, exact 7.4e-5,
    fused 3.1e-4, fused-split 3.0e-4; loss B yardstick 7.1e-4, exact 6.6e-4, fused 8.2e-4, fused-split 7.1e-4 (all fine.xyz_encoding_1 / _3)."""
    assert len(UNREACHED_A) == 15
    E, mods, _ = tt.modules()
    cw, fw, ea, et = syn.trained_nerfh_weights()
    mods[0].load_state_dict({k: T(v) for k, v in cw.items()})
    mods[1].load_state_dict({k: T(v) for k, v in fw.items()})
    mods[2].weight.data.copy_(T(ea)); mods[3].weight.data.copy_(T(et))
    E.load_numpy(cw, fw, ea, et)
    R, Nc, Ni, FAR = 256, 64, 128, 2.5
    H, W, focal = 60, 80, 585.0 / 8
    pose = syn.orbit_pose(7, 16)[:3, :4]
    rng = np.random.default_rng(0)
    ro, rd = orc.get_rays(H, W, focal, T(pose))
    sel = rng.choice(H * W, R, replace=False)
    o, d = ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous()
    target = T(syn.analytic_scene_image(pose, H, W, focal, FAR)).reshape(-1, 3)[sel].contiguous()
    hist = T(syn.HIST_IDX)[None].repeat(R, 1).contiguous()
    gen = torch.Generator().manual_seed(9)
    draws = (torch.rand(R, Nc, generator=gen), torch.randn(R, Nc, generator=gen), torch.rand(R, Ni, generator=gen))
    td = draw_td(R, gen)
    rows = rows_of(o, d, hist, FAR)
    c, f = {k: T(v) for k, v in cw.items()}, {k: T(v) for k, v in fw.items()}
    tr = nerf_train.NerfHTrainer(E, *mods)
    fails = []
    for loss_tag, with_nerfw in (("A", False), ("B", True)):
        g32, _ = oracle_step(rows, target, c, f, T(ea), T(et), Nc, Ni, draws, 1., td, with_nerfw)
        g64, _ = oracle_step(rows, target, c, f, T(ea), T(et), Nc, Ni, draws, 1., td, with_nerfw, f64=True)
        got = {}
        for tag, exact, split in (("exact", True, False), ("fused", False, False), ("fused_split", False, True)):
            tr.fused_split = split
            out = tr.forward(o.to(DEV), d.to(DEV), hist.to(DEV), Nc, Ni, 0., FAR, draws[0].to(DEV), draws[1].to(DEV), 1., draws[2].to(DEV),
                             exact=exact, maps=True)
            g_maps, g_raw = seeds(out, td.to(DEV), target.to(DEV) if with_nerfw else None)
            assert (g_raw is not None) == with_nerfw
            grads = tr.backward(g_maps=g_maps, g_raw=g_raw, grads=[torch.empty_like(p) for p in tr.params])
            got[tag] = {k: g.detach().cpu().clone() for k, g in zip(tr.names, grads)}
        tr.fused_split = False
        worst = {"yard": (0., ""), "exact": (0., ""), "fused": (0., ""), "fused_split": (0., "")}
        for k in tr.names:
            unreached = g64[k] is None or float(g64[k].abs().max()) == 0.
            assert unreached == (loss_tag == "A" and k in UNREACHED_A), (loss_tag, k)
            if unreached:
                for t in got:
                    assert float(got[t][k].abs().max()) == 0., (loss_tag, k, t)
                continue
            yard = rel_l2(g32[k], g64[k])
            e = {t: rel_l2(got[t][k], g64[k]) for t in got}
            worst["yard"] = max(worst["yard"], (yard, k))
            for t in e:
                worst[t] = max(worst[t], (e[t], k))
            if not e["exact"] <= 3. * yard + 2e-4:
                fails.append((loss_tag, k, "exact", e, yard))
            for t in ("fused", "fused_split"):
                if not e[t] <= 3. * max(yard, e["exact"]) + 5e-4:
                    fails.append((loss_tag, k, t, e, yard))
        print(f"loss {loss_tag}, trained-like weights, worst distance from float64 over the gradient tensors:",
              {k: f"{v[0]:.2e} ({v[1]})" for k, v in worst.items()})
    assert E.range_flags() == 0
    assert not fails, fails


# ---------------------------------------------------------------------------------------------- 5. fused equals exact with map gradients
@pytest.mark.parametrize("perturb,per_ray_hist,lindisp", [(0., False, False), (1., True, True)])
def test_fused_step_equals_exact_step_with_map_gradients(perturb, per_ray_hist, lindisp):
    """The setup of tests/test_gpu_train.py::test_fused_step_equals_exact_step (77 rays, 24 + 40, ragged last tile; its first and second
    parameter rows) with loss B: worst gradient relative L2 between the fused and the exact step < 5e-4, that test's bound.
    Measured on an MI355X (LABBOOK R10.1; the one-plane fused mode): 3.3e-4 and 1.0e-4, both fine.xyz_encoding_1.0.weight."""
    E, mods, _ = tt.modules()
    tr = nerf_train.NerfHTrainer(E, *mods)
    R, Nc, Ni = 77, 24, 40
    rng = np.random.default_rng(21)
    ro, rd = orc.get_rays(480, 640, 585.0, T(syn.orbit_pose(5, 8))[:3, :4])
    sel = rng.choice(480 * 640, R, replace=False)
    o, d = ro.reshape(-1, 3)[sel].contiguous().to(DEV), rd.reshape(-1, 3)[sel].contiguous().to(DEV)
    hist = (T(rng.integers(0, 40, (R, 10)).astype(np.float32)) if per_ray_hist else T(syn.HIST_IDX)[None]).to(DEV)
    target = T(rng.uniform(0, 1, (R, 3)).astype(np.float32)).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(4)
    t_rand, noise, u = nerf_train.NerfHTrainer.draw(R, Nc, Ni, perturb, DEV, gen)
    td = 1. + 0.3 * torch.sigmoid(torch.randn(R, device=DEV, generator=gen))
    E.set_render_options(lindisp=lindisp)
    try:
        res = {}
        for tag, exact in (("exact", True), ("fused", False)):
            out = tr.forward(o, d, hist, Nc, Ni, 0.05 if lindisp else 0., 2.5, t_rand, noise, 0.5, u, exact=exact, maps=True)
            g_maps, g_raw = seeds(out, td, target)
            grads = tr.backward(g_maps=g_maps, g_raw=g_raw, grads=[torch.empty_like(p) for p in tr.params])
            res[tag] = ({k: v.clone() for k, v in out.items()}, [g.clone() for g in grads])
    finally:
        E.set_render_options(lindisp=False)
    assert E.range_flags() == 0
    worst = max((rel_l2(a, b), k) for k, a, b in zip(tr.names, res["fused"][1], res["exact"][1]))
    print(f"fused vs exact step with map gradients, loss B (perturb {perturb}, per-ray hist {per_ray_hist}, lindisp {lindisp}): "
          f"worst gradient rel L2 {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < 5e-4, worst


# ---------------------------------------------------------------------------------------------- 6. ray gradients
def test_training_render_ray_gradients_of_the_map_losses_vs_oracle_64_rays():
    """The inputs of tests/test_gpu_train.py::test_training_render_ray_gradients_vs_oracle_64_rays (64 rays, 64 + 128, seeds 15 / 19), td
    drawn after the three draws; loss A.  forward(exact=True, maps=True), backward_rays(g_maps=...): that test's procedure and bound —
    rays_off_a_gate at max_frac 0.04 (at most 2 of 64 rays left out), then <= 1.5 x yardstick + 2e-4 on both tensors; deterministic.
    Measured on an MI355X (LABBOOK R10.1): d rays_o 4.5e-4 (torch fp32: 9.8e-4), d rays_d 1.0e-3 (1.7e-3), 2 of 64 rays left out."""
    E, mods, (cw, fw, ea, et) = tt.modules()
    tr = nerf_train.NerfHTrainer(E, *mods)
    R, Nc, Ni = 64, 64, 128
    rng = np.random.default_rng(15)
    ro, rd = orc.get_rays(480, 640, 585.0, T(syn.orbit_pose(3, 8))[:3, :4])
    sel = rng.choice(480 * 640, R, replace=False)
    o, d = ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous()
    hist = T(rng.integers(0, 40, (R, 10)).astype(np.float32))
    gen = torch.Generator().manual_seed(19)
    t_rand, noise, u = torch.rand(R, Nc, generator=gen), torch.randn(R, Nc, generator=gen), torch.rand(R, Ni, generator=gen)
    td = draw_td(R, gen)
    c, f = {k: T(v) for k, v in cw.items()}, {k: T(v) for k, v in fw.items()}

    def ray_grads(o, d, hist, c, f, ea, et, draws, td):
        """d loss A (sums divided by the batch's R = 64) / d (rays_o, rays_d) of the given rays, in the dtype of the inputs."""
        o, d = o.detach().clone().requires_grad_(True), d.detach().clone().requires_grad_(True)
        st = {}
        out = orc.render_rays_train(orc.pack_ray_rows(o, d, 0., 2.5, hist), c, f, ea, et, Nc, Ni, *draws, 1., 1., stages=st)
        d0 = orc.composite_coarse_train(st["raw_coarse"], st["z_coarse"], draws[1] * 1.)["depth"]
        lossA(out, st["depth_fine"], d0, td, R).backward()
        return o.grad, d.grad

    go_ref, gd_ref = ray_grads(o, d, hist, c, f, T(ea), T(et), (t_rand, noise, u), td)
    with float64_default():
        a64 = to64((o, d, hist, c, f, T(ea), T(et), (t_rand, noise, u), td))
        go64, gd64 = ray_grads(*a64)
    out = tr.forward(o.to(DEV), d.to(DEV), hist.to(DEV), Nc, Ni, 0., 2.5, t_rand.to(DEV), noise.to(DEV), 1., u.to(DEV), exact=True, maps=True)
    g_maps, g_raw = seeds(out, td.to(DEV))
    assert g_raw is None
    go, gd = tr.backward_rays(g_maps=g_maps)
    tru = torch.cat([go64, gd64], -1)

    def single64(i, delta):
        with float64_default():
            o6, d6, h6, c6, f6, ea6, et6, dr6, td6 = a64
            a, b = ray_grads(o6[i:i + 1] + delta, d6[i:i + 1], h6[i:i + 1], c6, f6, ea6, et6, tuple(t[i:i + 1] for t in dr6), td6[i:i + 1])
        return torch.cat([a[0], b[0]])
    keep = rays_off_a_gate(torch.cat([go, gd], -1), tru, single64)
    left = int((~keep).sum())
    yo, yd = rel_l2(go_ref[keep], go64[keep]), rel_l2(gd_ref[keep], gd64[keep])
    eo, ed = rel_l2(go.cpu()[keep], go64[keep]), rel_l2(gd.cpu()[keep], gd64[keep])
    print(f"training-render ray gradients of loss A, 64 rays @ 64+128, vs float64: d rays_o {eo:.2e} (torch fp32: {yo:.2e}), d rays_d {ed:.2e} "
          f"(torch fp32: {yd:.2e}); rays on a gate (left out): {left} of {keep.numel()}")
    assert left <= 2
    assert eo <= 1.5 * yo + 2e-4 and ed <= 1.5 * yd + 2e-4
    go2, gd2 = tr.backward_rays(g_maps=g_maps)
    assert torch.equal(go, go2) and torch.equal(gd, gd2)   # deterministic
    tr.forward(o.to(DEV), d.to(DEV), hist.to(DEV), Nc, Ni, 0., 2.5, t_rand.to(DEV), noise.to(DEV), 1., u.to(DEV))   # fused: no activations
    with pytest.raises(RuntimeError):
        tr.backward_rays(g_maps=g_maps)


# ---------------------------------------------------------------------------------------------- 7. the surface
def test_render_training_diff_maps_surface_and_optimizer_step(setup96):
    """render(test_time=False, diff_maps=True, retraw=True, ret_maps=True) on the 96-ray setup: every output but z_std attached, the values
    the bits of the same call without diff_maps, the two depths within 3e-5 of the oracle's (the bound of
    tests/test_gpu_train.py::test_train_step_vs_oracle_autograd_c2_samples on this forward), loss.backward() over all of them = the gradients
    of trainer.backward(g_maps, g_raw) within 5e-5, an Adam step moves the render, rays that require grad receive the map gradients; without
    diff_maps flags, extras and refusals as before.  Measured on an MI355X (LABBOOK R10.1): depth 3.2e-7, depth0 2.1e-7 from the oracle;
    autograd vs the direct call 0 (the same kernels on the same seeds)."""
    from dfnet_amd import rendering
    from dfnet_amd.nerfw import HipQuery
    s = setup96
    E, mods, tr, R, Nc, Ni, o, d, hist, target, draws, td = (s[k] for k in ("E", "mods", "tr", "R", "Nc", "Ni", "o", "d", "hist", "target", "draws", "td"))
    cw, fw, ea, et = s["w"]
    state = [p.detach().clone() for p in tr.params]
    kw = dict(network_query_fn=HipQuery(E, trainer=tr), perturb=1., N_importance=Ni, network_fine=mods[1], N_samples=Nc, network_fn=mods[0],
              use_viewdirs=True, white_bkgd=False, raw_noise_std=0., embedding_a=mods[2], embedding_t=mods[3], test_time=False, ndc=False,
              lindisp=False, near=0., far=2.5)
    rays = torch.stack([o, d], 0)
    render = lambda **over: rendering.render(480, 640, 585.0, rays=over.pop("rays", rays), img_idx=hist, draws=draws, **dict(kw, **over))
    try:
        # without diff_maps: flags, extras and refusals exactly as today
        rgb, disp, acc, ex = render(retraw=True)
        assert sorted(ex) == sorted(["raw", "rgb0", "disp0", "acc0", "z_std", "transient_sigmas", "beta"])
        assert rgb.requires_grad and ex["rgb0"].requires_grad and ex["beta"].requires_grad and ex["transient_sigmas"].requires_grad
        assert not any(t.requires_grad for t in (disp, acc, ex["raw"], ex["disp0"], ex["acc0"], ex["z_std"]))
        plain = dict(rgb=rgb, disp=disp, acc=acc, **ex)
        with pytest.raises(NotImplementedError, match="ret_maps"):
            render(ret_maps=True)
        with pytest.raises(NotImplementedError, match="ndc / c2w_staticcam together with training-mode rendering"):
            render(diff_maps=True, ndc=True)
        for bad in ("depth_static", "rgb_static", "rgb_transient", "beta", ("depth", "depht")):
            with pytest.raises(ValueError, match=r"\['depth', 'depth0'\]"):
                render(diff_maps=True, ret_maps=bad)
        assert set(render(diff_maps=True, ret_maps="depth0")[3]) == set(plain) - {"rgb", "disp", "acc", "raw"} | {"depth0"}
        # with diff_maps: everything attached but z_std, the same bits
        opt = torch.optim.Adam(tr.params, lr=5e-4)
        opt.zero_grad()
        rgb, disp, acc, ex = render(retraw=True, diff_maps=True, ret_maps=True)
        got = dict(rgb=rgb, disp=disp, acc=acc, **ex)
        assert set(got) == set(plain) | {"depth", "depth0"}
        for k, v in got.items():
            assert v.requires_grad == (k != "z_std"), k
            if k in plain:
                assert torch.equal(v.detach(), plain[k].detach()), k
        c, f = {k: T(v) for k, v in cw.items()}, {k: T(v) for k, v in fw.items()}
        cpu_draws = tuple(t.cpu() for t in draws)
        _, ref = oracle_step(rows_of(o.cpu(), d.cpu(), hist.cpu()), target.cpu(), c, f, T(ea), T(et), Nc, Ni, cpu_draws, 0., td.cpu(), False)
        for k in ("depth", "depth0"):
            e = tt.relmax(got[k], ref[k])
            print(f"render(test_time=False, diff_maps=True) {k} vs the oracle: {e:.2e}")
            assert e < 3e-5, k
        Gr = torch.randn(R, Nc + Ni, 9, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) / (R * (Nc + Ni))
        as_out = lambda g: dict(disp_map=g["disp"], acc_map=g["acc"], disp0=g["disp0"], acc0=g["acc0"], rgb_map=g["rgb"], rgb0=g["rgb0"],
                                beta=g["beta"], raw=g["raw"])
        loss = lossA(as_out(got), got["depth"], got["depth0"], td, R) + nerfw(as_out(got), target) + (got["raw"] * Gr).sum()
        loss.backward()
        by_autograd = [p.grad.clone() for p in tr.params]
        out = tr.forward(o, d, hist, Nc, Ni, 0., 2.5, draws[0], draws[1], 0., draws[2], maps=True)
        g_maps, g_raw = seeds(out, td, target, extra=lambda lv: (lv["raw"] * Gr).sum())
        direct = tr.backward(g_maps=g_maps, g_raw=g_raw, grads=[torch.empty_like(p) for p in tr.params])
        worst = max((rel_l2(a, b), k) for k, a, b in zip(tr.names, by_autograd, direct))
        print(f"loss.backward() through render(diff_maps=True) vs trainer.backward(g_maps, g_raw): worst {worst[0]:.2e} ({worst[1]})")
        assert worst[0] < 5e-5, worst
        before = {k: got[k].detach().clone() for k in ("rgb", "depth")}
        opt.step()
        again = render(diff_maps=True, ret_maps=True)
        assert float((again[0].detach() - before["rgb"]).abs().max()) > 1e-5
        assert float((again[3]["depth"].detach() - before["depth"]).abs().max()) > 1e-6
        # rays that require grad: the node switches to the exact step and the map gradients reach d rays
        r2 = rays.clone().requires_grad_(True)
        rgb, disp, acc, ex = render(rays=r2, diff_maps=True, ret_maps=True)
        lossA(dict(disp_map=disp, acc_map=acc, disp0=ex["disp0"], acc0=ex["acc0"]), ex["depth"], ex["depth0"], td, R).backward()
        assert r2.grad is not None and bool(torch.isfinite(r2.grad).all()) and float(r2.grad.abs().max()) > 0
        assert E.range_flags() == 0
    finally:
        with torch.no_grad():
            for p, v in zip(tr.params, state):
                p.copy_(v)
                p.grad = None


# ---------------------------------------------------------------------------------------------- 8. ABI: state and workspace checks
def test_new_entries_check_workspace_and_state(setup96):
    s = setup96
    tr, Nc, Ni, R = s["tr"], s["Nc"], s["Ni"], s["R"]
    lib, h = tr.lib, tr.engine.handle
    out = tr.forward(s["o"], s["d"], s["hist"], Nc, Ni, 0., 2.5, s["draws"][0], s["draws"][1], 0., s["draws"][2], exact=True, maps=True)
    sv = tr._saved
    ws, P = sv["ws"], ctypes.c_void_p
    g = torch.ones(R, device=DEV)
    st = _lib.TrainMapGrads(acc=g.data_ptr())
    params, grads = tr._ptr_array(tr.params), tr._ptr_array([torch.empty_like(p) for p in tr.params])
    go = torch.empty(R, 3, device=DEV)
    scratch = torch.empty(lib.dfn_nerfh_train_backward_rays_scratch_bytes(R, Nc, Ni), dtype=torch.uint8, device=DEV)
    bw = lambda nbytes, stp=ctypes.byref(st): lib.dfn_nerfh_train_backward_maps(
        h, params, _lib.ptr(sv["hist"]), 1, R, Nc, Ni, None, 0., _lib.ptr(sv["raw"]), stp, 0., None, grads, P(ws.data_ptr()), nbytes, None)
    br = lambda nbytes, sbytes: lib.dfn_nerfh_train_backward_rays_maps(
        h, params, _lib.ptr(sv["rays_o"]), _lib.ptr(sv["rays_d"]), _lib.ptr(sv["hist"]), 1, R, Nc, Ni, None, 0., _lib.ptr(sv["raw"]), ctypes.byref(st),
        0., None, _lib.ptr(go), _lib.ptr(go), P(ws.data_ptr()), nbytes, P(scratch.data_ptr()), sbytes, None)
    dp = lambda nbytes: lib.dfn_nerfh_train_depths(h, R, Nc, Ni, _lib.ptr(sv["raw"]), P(ws.data_ptr()), nbytes, _lib.ptr(g), None, None)
    assert bw(1024) == -1 and b"dfn_nerfh_train_backward_maps: workspace too small" in lib.dfn_last_error()
    assert br(1024, scratch.numel()) == -1 and br(ws.numel(), 16) == -1 and b"dfn_nerfh_train_backward_rays_maps" in lib.dfn_last_error()
    assert dp(1024) == -1 and b"dfn_nerfh_train_depths: workspace too small" in lib.dfn_last_error()
    assert bw(ws.numel(), ctypes.byref(_lib.TrainMapGrads())) == -1 and bw(ws.numel(), None) == -1   # nothing given
    tr.set_mode(False)   # a mode switch after the forward: DFN_ERR_STATE from every entry that reads the workspace
    try:
        assert bw(ws.numel()) == -3 and b"dfn_nerfh_train_backward_maps" in lib.dfn_last_error()
        assert dp(ws.numel()) == -3 and b"dfn_nerfh_train_depths" in lib.dfn_last_error()
    finally:
        tr.set_mode(True)
    assert bw(ws.numel()) == 0 and dp(ws.numel()) == 0
    torch.cuda.synchronize()
    assert torch.equal(g, out["depth"])
