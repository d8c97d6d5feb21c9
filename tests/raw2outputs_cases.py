"""Shared by the raw2outputs_NeRFW tests (CPU and GPU): the modes of the function, the oracle's restatement of each, inputs, and the
float64 yardstick of its gradients.

Modes (models/rendering.py:132-243) and the oracle function that restates each (oracle/nerfh_oracle.py, pinned to the reference's own
outputs and autograd by tests/golden/g17_raw2outputs.npz, tests/test_raw2outputs_oracle_golden.py):
  M1  typ == "coarse" and test_time          orc.coarse_weights          acc, weights
  M2  output_transient=False otherwise       orc.composite_coarse_train  rgb, disp, acc, weights, depth
  M3  output_transient=True                  orc.composite_fine          the same and beta
"""
import torch

from oracle import nerfh_oracle as orc
from tests.yardstick import float64_default, rel_l2, to64

DEV = "cuda:0"

# tag -> (channel count of the arithmetic, the reference's keyword arguments)
MODES = {
    "m1": (1, dict(output_transient=False, white_bkgd=False, test_time=True, static_only=True, typ="coarse")),
    "m2": (4, dict(output_transient=False, white_bkgd=False, test_time=False, static_only=True, typ="coarse")),
    "m2w": (4, dict(output_transient=False, white_bkgd=True, test_time=False, static_only=True, typ="coarse")),
    "m2f": (4, dict(output_transient=False, white_bkgd=False, test_time=True, static_only=False, typ="fine")),
    "m2fw": (4, dict(output_transient=False, white_bkgd=True, test_time=False, static_only=False, typ="fine")),
    "m3": (9, dict(output_transient=True, white_bkgd=False, test_time=True, static_only=True, typ="fine")),
    "m3w": (9, dict(output_transient=True, white_bkgd=True, test_time=True, static_only=True, typ="fine")),
    "m3t": (9, dict(output_transient=True, white_bkgd=False, test_time=False, static_only=True, typ="fine")),
    "m3tw": (9, dict(output_transient=True, white_bkgd=True, test_time=False, static_only=True, typ="fine")),
    "m3j": (9, dict(output_transient=True, white_bkgd=False, test_time=True, static_only=False, typ="fine")),
    "m3jw": (9, dict(output_transient=True, white_bkgd=True, test_time=True, static_only=False, typ="fine")),
    "m3c": (9, dict(output_transient=True, white_bkgd=False, test_time=False, static_only=False, typ="coarse")),
}
# one of each arithmetic (static-only and joint depth, with and without the white background) for the gradient sweeps
GRAD_MODES = ("m1", "m2", "m2w", "m3", "m3w", "m3t", "m3tw")
OUTPUTS = {1: ("acc", "weights"), 4: ("rgb", "disp", "acc", "weights", "depth"), 9: ("rgb", "disp", "acc", "weights", "depth", "beta")}


def dev(x):
    return None if x is None else torch.as_tensor(x).float().to(DEV).contiguous()


def engine_opts(tag):
    """The keyword arguments of engine.raw2outputs / raw2outputs_backward for a mode."""
    kw = MODES[tag][1]
    return dict(test_time=kw["test_time"], static_only=kw["static_only"], white_bkgd=kw["white_bkgd"], coarse=kw["typ"] == "coarse")


def oracle(tag, raw, z, noise=None):
    """{name: tensor} of the outputs of mode `tag` by the oracle.  raw: [n,N,1] / [n,N,4] / [n,N,9]; noise already times its std."""
    ch, kw = MODES[tag]
    if ch == 1:
        acc, w = orc.coarse_weights(raw[..., 0], z, noise)
        return dict(acc=acc, weights=w)
    if ch == 4:
        return orc.composite_coarse_train(raw, z, noise, white_bkgd=kw["white_bkgd"])
    out = orc.composite_fine(raw, z, 0.1, white_bkgd=kw["white_bkgd"], test_time=kw["test_time"], static_only=kw["static_only"])
    return {k: out[k] for k in OUTPUTS[9]}


def inputs(ch, n, N, seed=0, light_through=False):
    """(raw [n,N,ch], z [n,N] sorted in [0, 2.5], noise [n,N], generator).
    ch = 9: colours and beta in (0,1), sigma_s, sigma_t = softplus(N(0,1)) (tests/test_gpu_maps_grad.py::stage_inputs).
    ch = 1, 4: sigma = N(0.5, 1.5), of BOTH signs, so that the relu matters; one sample per ray (index ray mod N) has sigma = 2 + |.|, an
    open gate whatever the noise (0.5 N(0,1), asserted): a ray all of whose gates are closed has acc = 0 and disp = 1 / max(1e-10, 0 / 0),
    which is NaN in torch and 1e10 in the kernel, and is not a case of the reference's use.
    light_through: the last sample is nearly transparent (sigma 1e-3, 2e-3; noise 0 there), so that the transmittance behind the ray,
    which is all of d acc / d sigma, is of order one (tests/test_gpu_maps_grad.py::test_stage_acc_gradient_on_rays_that_let_light_through)."""
    gen = torch.Generator().manual_seed(100000 * seed + 1000 * ch + 10 * N + n)
    z = torch.sort(torch.rand(n, N, generator=gen) * 2.5, -1)[0].contiguous()
    noise = torch.randn(n, N, generator=gen)
    if ch == 9:
        raw = torch.rand(n, N, 9, generator=gen) * 0.98 + 0.01
        raw[..., 3] = torch.nn.functional.softplus(torch.randn(n, N, generator=gen))
        raw[..., 7] = torch.nn.functional.softplus(torch.randn(n, N, generator=gen))
        if light_through:
            raw[:, -1, 3], raw[:, -1, 7] = 1e-3, 2e-3
        return raw.contiguous(), z, noise, gen
    raw = torch.rand(n, N, ch, generator=gen) * 0.98 + 0.01
    sig = torch.randn(n, N, generator=gen) * 1.5 + 0.5
    rows = torch.arange(n)
    sig[rows, rows % N] = 2. + sig[rows, rows % N].abs()
    if light_through:
        sig[:, -1], noise[:, -1] = 1e-3, 0.
        if N > 1:
            sig[:, 0] = 1. + sig[:, 0].abs()
    raw[..., ch - 1] = sig
    assert bool(((sig + 0.5 * noise) > 0).any(-1).all())
    return raw.contiguous(), z, noise, gen


def random_upstreams(ch, n, N, gen):
    return {k: torch.randn((n, 3) if k == "rgb" else (n, N) if k == "weights" else (n,), generator=gen) for k in OUTPUTS[ch]}


def one_upstream(name, n, N, gen):
    """A gradient on output `name` alone: one-hot per ray (1 for the [n] outputs, channel ray mod 3 for rgb), random dense for weights."""
    if name == "rgb":
        g = torch.zeros(n, 3)
        g[torch.arange(n), torch.arange(n) % 3] = 1.
        return g
    if name == "weights":
        return torch.randn(n, N, generator=gen)
    return torch.ones(n)


def oracle_grads(tag, raw, z, G, noise=None, f64=False):
    """(d L/d raw, d L/d z) of L = sum_k (output_k * G_k) by torch autograd through the oracle, in fp32 or float64."""
    if f64:
        with float64_default():
            return oracle_grads(tag, *to64((raw, z, G)), None if noise is None else to64(noise))
    r, zz = raw.detach().clone().requires_grad_(True), z.detach().clone().requires_grad_(True)
    out = oracle(tag, r, zz, noise)
    loss = sum((out[k] * G[k]).sum() for k in G)
    gr, gz = torch.autograd.grad(loss, (r, zz), allow_unused=True)
    return (torch.zeros_like(r) if gr is None else gr), (torch.zeros_like(zz) if gz is None else gz)


def bound(yard):
    """tests/test_gpu_maps_grad.py::bound: the project's bound of a gradient through the compositor."""
    return 1.5 * yard + 2e-4


def yardstick(tag, raw, z, G, noise=None):
    """((truth_raw, truth_z) in float64, (yard_raw, yard_z)): torch's own fp32 autograd of the oracle measured against its float64 one."""
    truth = oracle_grads(tag, raw, z, G, noise, f64=True)
    ref = oracle_grads(tag, raw, z, G, noise)
    return truth, (rel_l2(ref[0], truth[0]), rel_l2(ref[1], truth[1]))
