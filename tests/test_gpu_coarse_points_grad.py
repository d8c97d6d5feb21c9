"""The coarse point query under autograd: dfn_mlp_coarse_points_backward (nerfh_coarse_backward_pts_kernel),
NerfHEngine.mlp_coarse_points_backward, nerfw._CoarsePointsFn and HipQuery.__call__(..., typ='coarse', diff=True).

Truth is torch autograd through oracle.nerfh_oracle.query_coarse_sigma in FLOAT64 (the oracle is dtype-generic: the weights are loaded
as double).  Points, seeds and helpers are those of tests/test_gpu_points.py.  The bound on d L/d points is the suite's own for
d sigma_static / d inputs of the fine network, the same trunk and head (TOL_NET = 1e-5, relative maximum and relative L2); the fp32 CPU
oracle itself sits 2e-7 .. 5e-7 from float64 on these inputs.

Measured figures are in the docstrings of the tests that print them."""
import ctypes

import pytest
import torch

from dfnet_amd import _lib, engine as eng, rendering, synthetic as syn
from dfnet_amd._lib import current_stream, ptr
from oracle import nerfh_oracle as orc
from tests.test_gpu_points import DEV, big_shape, dev, rel_l2, relmax, scattered, tt, wrapped
from tests.test_gpu_sample_pdf_grad import CHAIN_FACTOR, ULP, cdf64, row_err

pytestmark = pytest.mark.gpu
T = torch.from_numpy
GRAD_PRECS = ("f32", "f16x3")
TOL = 1e-5


def d64(p):
    return {k: v.double() for k, v in p.items()}


def seed_grad(rows, N, seed=11):
    return torch.randn(rows, N, generator=torch.Generator().manual_seed(seed))


def oracle_grad(c, pts, G, dtype=torch.float64):
    """d sum(sigma * G) / d pts by autograd through the oracle in `dtype` on the CPU -> float64."""
    p = pts.to(dtype).clone().requires_grad_(True)
    w = {k: v.to(dtype) for k, v in c.items()}
    (orc.query_coarse_sigma(w, p)[..., 0] * G.to(dtype)).sum().backward()
    return p.grad.double()


@pytest.fixture(scope="module")
def scene():
    cw, fw, ea, et = syn.nerfh_weights(0)
    return eng.NerfHEngine().load_numpy(cw, fw, ea, et), tt(cw)


# ---------------------------------------------------------------------------------------------- 1. the kernel against autograd
@pytest.mark.parametrize("prec", GRAD_PRECS)
@pytest.mark.parametrize("rows,N", [(1, 1), (3, 5), (37, 7), (9, 192)])
def test_kernel_vs_float64_autograd(scene, prec, rows, N):
    """One live lane, a partial wave, 259 points (a second, partial tile at both tile sizes), 1 728 points.
    Measured on an MI355X (LABBOOK R22.2), relative maximum, f32 / f16x3: (1,1) 1.30e-7 / 2.87e-7, (3,5) 4.15e-7 / 6.65e-7, (37,7)
    3.64e-7 / 6.19e-7, (9,192) 3.53e-7 / 7.70e-7; relative L2 no larger."""
    E, c = scene
    pts = scattered(rows, N, False, rows * 1000 + N)[0]
    G = seed_grad(rows, N)
    ref = oracle_grad(c, pts, G)
    got = E.mlp_coarse_points_backward(dev(pts), dev(G), precision=prec)
    assert got.shape == (rows, N, 3)
    e, l2 = relmax(got, ref), rel_l2(got, ref)
    print(f"coarse points gradient {prec} ({rows},{N}): relmax {e:.2e} L2 {l2:.2e}")
    assert e < TOL and l2 < TOL
    assert E.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 2. the tile loop
@pytest.mark.parametrize("prec", GRAD_PRECS)
def test_tile_loop(scene, prec):
    """More points than 512 x the compute units, the last tile partial: every workgroup takes a second tile.  The first 37 and the
    last 3 rows have the bits they have when queried alone, everything is finite, and 2 000 random points agree with float64.
    Measured on an MI355X, (515, 257): f32 2.35e-7 (L2 2.83e-7), f16x3 7.62e-7 (L2 5.55e-7)."""
    E, c = scene
    rows, N = big_shape()
    g = torch.Generator().manual_seed(rows * 1000 + N)
    pts = torch.rand(rows, N, 3, generator=g) * 3 - 1.5
    G = seed_grad(rows, N)
    P, Gd = dev(pts), dev(G)
    got = E.mlp_coarse_points_backward(P, Gd, precision=prec)
    assert got.shape == (rows, N, 3) and bool(torch.isfinite(got).all())
    assert torch.equal(got[:37], E.mlp_coarse_points_backward(P[:37], Gd[:37], precision=prec))
    assert torch.equal(got[-3:], E.mlp_coarse_points_backward(P[-3:], Gd[-3:], precision=prec))
    pick = torch.randperm(rows * N, generator=g)[:2000]
    sub_p, sub_g = pts.reshape(-1, 1, 3)[pick], G.reshape(-1, 1)[pick]
    ref = oracle_grad(c, sub_p, sub_g)
    sub = got.reshape(-1, 1, 3)[pick.to(DEV)]
    e, l2 = relmax(sub, ref), rel_l2(sub, ref)
    print(f"coarse points gradient {prec} ({rows},{N}), 2 000 points: relmax {e:.2e} L2 {l2:.2e}")
    assert e < TOL and l2 < TOL
    assert E.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 3. scale and isolation
@pytest.mark.parametrize("prec", GRAD_PRECS)
def test_scale_and_isolation(scene, prec):
    """G 2^k gives 2^k x the gradient bit for bit (k = +-20): the per-point scale is a power of two taken from |g sigmoid(pre)|, the
    final division by it is exact, and every other operation is linear in g.  Rows with G = 0 give exact zeros; a row with G = 1e6
    beside a row with G = 1e-6 gives each the bits it has alone; the raw entry writes n_rows N 3 floats and nothing else."""
    E, c = scene
    rows, N = 37, 7
    P = dev(scattered(rows, N, False, rows * 1000 + N)[0])
    G = seed_grad(rows, N)
    base = E.mlp_coarse_points_backward(P, dev(G), precision=prec)
    assert float(base.abs().max()) > 0
    for k in (20, -20):
        scaled = E.mlp_coarse_points_backward(P, dev(G * 2. ** k), precision=prec)
        assert torch.equal(scaled, base * 2. ** k), f"k = {k}: {int((scaled != base * 2. ** k).sum())} values differ"
    Gz = G.clone()
    Gz[5] = 0.
    Gz[20] = 0.
    Gz[11, 3] = 0.
    gz = E.mlp_coarse_points_backward(P, dev(Gz), precision=prec)
    assert bool((gz[5] == 0).all() and (gz[20] == 0).all() and (gz[11, 3] == 0).all())
    keep = torch.ones(rows, dtype=torch.bool)
    keep[[5, 20, 11]] = False
    assert torch.equal(gz[keep.to(DEV)], base[keep.to(DEV)])
    Gm = G.clone()
    Gm[3] = 1e6
    Gm[4] = 1e-6
    gm = E.mlp_coarse_points_backward(P, dev(Gm), precision=prec)
    for r in (3, 4):
        assert torch.equal(gm[r:r + 1], E.mlp_coarse_points_backward(P[r:r + 1], dev(Gm[r:r + 1]), precision=prec))
    assert bool(torch.isfinite(gm).all())
    # the raw entry into the middle of a NaN-filled buffer
    pad, n = 1024, rows * N * 3
    buf = torch.full((n + 2 * pad,), float("nan"), device=DEV)
    Gd = dev(G)
    dst = ctypes.c_void_p(buf.data_ptr() + 4 * pad)
    rc = E.lib.dfn_mlp_coarse_points_backward(E.handle, _lib.PRECISIONS[prec], ptr(P), rows, N, ptr(Gd), dst, current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + n:]).all())
    assert torch.equal(buf[pad:pad + n].reshape(rows, N, 3), base)
    assert E.range_flags() == 0


def test_entry_status_codes(scene):
    """What needs a committed handle: plain f16 and another width are DFN_ERR_UNSUPPORTED (-4), null pointers DFN_ERR_ARG (-1),
    N < 1 DFN_ERR_ARG, n_rows == 0 DFN_OK."""
    E, _ = scene
    fn, one, s = E.lib.dfn_mlp_coarse_points_backward, ctypes.c_void_p(16), current_stream()
    f32 = _lib.PRECISIONS["f32"]
    assert fn(E.handle, _lib.PRECISIONS["f16"], one, 4, 8, one, one, s) == -4
    assert fn(E.handle, f32, one, 0, 8, one, one, s) == 0
    assert fn(E.handle, f32, None, 4, 8, one, one, s) == -1
    assert fn(E.handle, f32, one, 4, 8, None, one, s) == -1
    assert fn(E.handle, f32, one, 4, 8, one, None, s) == -1
    assert fn(E.handle, f32, one, 4, 0, one, one, s) == -1
    cw, fw, ea, et = syn.nerfh_weights(2, W=256)
    E256 = eng.NerfHEngine(width=256).load_numpy(cw, fw, ea, et)
    with pytest.raises(_lib.DfnError, match=r"status -4\).*netwidth 128 only"):
        E256.mlp_coarse_points_backward(torch.zeros(2, 3, 3, device=DEV), torch.zeros(2, 3, device=DEV), precision="f32")
    with pytest.raises(_lib.DfnError, match=r"status -4\)"):
        E.mlp_coarse_points_backward(torch.zeros(2, 3, 3, device=DEV), torch.zeros(2, 3, device=DEV), precision="f16")
    none = E.mlp_coarse_points_backward(torch.zeros(0, 3, 3, device=DEV), torch.zeros(0, 3, device=DEV), precision="f16x3")
    assert none.shape == (0, 3, 3)


# ---------------------------------------------------------------------------------------------- 4. trained-like weights
@pytest.mark.parametrize("prec", GRAD_PRECS)
def test_trained_like_weights_against_the_fine_kernel(prec):
    """No bound in the suite covers trained-like weights (sigma in the hundreds, input gradients of 1e4..1e5), so the yardstick is
    measured in the same run: the engine's COARSE slot holds the trained fixture's FINE trunk and static_sigma (the fixture's own coarse
    net supplies the tensors sigma does not use), its fine slot the trained fine net, and then the new kernel and
    mlp_fine_points_backward with grad_raw on channel 3 only differentiate the same function.  Both against float64:
    e_new <= 2 max(e_fine, y), y the fp32 CPU oracle's own distance; the chains differ in how d h8 is seeded and where they
    renormalise.
    Measured on an MI355X (LABBOOK R22.2; relative maximum; new / fine / y; sigma up to 310, |gradient| up to 4.01e4):
    f32 2.19e-7 / 2.19e-7 / 3.08e-7, f16x3 7.22e-7 / 7.22e-7 / 3.08e-7."""
    cw, fw, ea, et = syn.trained_nerfh_weights()
    mixed = dict(cw)
    for k in fw:
        if k.startswith("xyz_encoding_") and not k.startswith("xyz_encoding_final") or k.startswith("static_sigma."):
            assert mixed[k].shape == fw[k].shape
            mixed[k] = fw[k]
    E = eng.NerfHEngine().load_numpy(mixed, fw, ea, et)
    c = tt(mixed)
    rows, N = 9, 192
    g = torch.Generator().manual_seed(4)
    pts = (torch.rand(rows, N, 3, generator=g) * 2 - 1) * .8
    v = torch.randn(rows, 3, generator=g)
    v = v / v.norm(dim=-1, keepdim=True)
    hist = T(syn.HIST_IDX)[None].clone()
    G = seed_grad(rows, N)
    ref = oracle_grad(c, pts, G)
    y = relmax(oracle_grad(c, pts, G, torch.float32), ref)
    new = E.mlp_coarse_points_backward(dev(pts), dev(G), precision=prec)
    graw = torch.zeros(rows, N, 9)
    graw[..., 3] = G
    fine = E.mlp_fine_points_backward(dev(pts), dev(v), dev(hist), dev(graw), precision=prec)[..., :3]
    e_new, e_fine = relmax(new, ref), relmax(fine, ref)
    with torch.no_grad():
        smax = float(orc.query_coarse_sigma(d64(c), pts.double()).max())
    print(f"trained-like weights {prec}: new kernel {e_new:.2e}  fine kernel {e_fine:.2e}  fp32 CPU oracle {y:.2e}  "
          f"(sigma up to {smax:.3g}, |gradient| up to {float(ref.abs().max()):.3g})")
    assert bool(torch.isfinite(new).all())
    assert e_new <= 2 * max(e_fine, y)


# ---------------------------------------------------------------------------------------------- 5. chunking
@pytest.mark.parametrize("prec", GRAD_PRECS)
def test_chunked_call_has_the_bits_of_the_unsplit_one(scene, prec, monkeypatch):
    E, _ = scene
    P = dev(scattered(37, 7, False, 5)[0])
    G = dev(seed_grad(37, 7, 3))
    whole = E.mlp_coarse_points_backward(P, G, precision=prec)
    monkeypatch.setattr(E, "POINTS_CHUNK", 70)         # 10 rows of 7 points per call: 10, 10, 10, 7
    assert len(E._point_chunks(37, 7, False)) == 4
    assert torch.equal(E.mlp_coarse_points_backward(P, G, precision=prec), whole)


# ---------------------------------------------------------------------------------------------- 6. the callable
@pytest.mark.parametrize("precision", ["f16x3", "f16", "f32"])
def test_query_diff(precision):
    """q(..., 'coarse', ..., diff=True): sigma attached to the points; an engine in plain f16 differentiates in split-f16.
    Measured on an MI355X, d inputs from float64 (relative maximum): engine f16x3 6.91e-7, f16 6.91e-7, f32 4.43e-7."""
    q, (coarse, fine, emb_a, emb_t), (c, f, ea, et) = wrapped(precision=precision)
    rows, N = 4, 33
    pts, v, hist = scattered(rows, N, True, 23)
    G = seed_grad(rows, N, 5)
    ref = oracle_grad(c, pts, G)
    x, w, h = dev(pts).requires_grad_(True), dev(v).requires_grad_(True), dev(hist)
    sigma = q(x, w, h, coarse, 'coarse', emb_a, emb_t, False, True, diff=True)
    assert sigma.shape == (rows, N, 1) and sigma.requires_grad
    (sigma[..., 0] * dev(G)).sum().backward()
    e, l2 = relmax(x.grad, ref), rel_l2(x.grad, ref)
    print(f"engine {precision}: d inputs of the coarse query {e:.2e} (L2 {l2:.2e})")
    assert e < TOL and l2 < TOL
    assert w.grad is None
    plain = q(x.detach(), w.detach(), h, coarse, 'coarse', emb_a, emb_t, False, True)
    if precision != "f16":
        assert torch.equal(sigma.detach(), plain)
    # nothing to track, or no graph wanted: the plain query
    quiet = q(x.detach(), w.detach(), h, coarse, 'coarse', emb_a, emb_t, False, True, diff=True)
    assert not quiet.requires_grad and torch.equal(quiet, plain)
    with torch.no_grad():
        quiet = q(x, w, h, coarse, 'coarse', emb_a, emb_t, False, True, diff=True)
    assert not quiet.requires_grad and quiet.grad_fn is None and torch.equal(quiet, plain)
    only_v = q(x.detach(), w, h, coarse, 'coarse', emb_a, emb_t, False, True, diff=True)     # sigma does not see the view direction
    assert not only_v.requires_grad
    # the default does not move
    with pytest.raises(NotImplementedError, match="autograd"):
        q(x, w, h, coarse, 'coarse', emb_a, emb_t, False, True)
    with pytest.raises(NotImplementedError, match="test_time=False"):
        q(x, w, h, coarse, 'coarse', emb_a, emb_t, False, False, diff=True)
    # typ='fine' accepts the keyword and ignores it
    raw = q(x, w, h, fine, 'fine', emb_a, emb_t, True, True, diff=True)
    assert raw.requires_grad and torch.equal(raw.detach(), q(x, w, h, fine, 'fine', emb_a, emb_t, True, True).detach())
    assert not q(x.detach(), w.detach(), h, fine, 'fine', emb_a, emb_t, True, True, diff=True).requires_grad
    # a flat list of points
    flat = dev(pts).reshape(-1, 1, 3).requires_grad_(True)
    sf = q(flat, None, None, coarse, 'coarse', diff=True)
    assert sf.shape == (rows * N, 1, 1) and sf.requires_grad
    (sf[..., 0] * dev(G).reshape(-1, 1)).sum().backward()
    assert torch.equal(flat.grad.reshape(rows, N, 3), x.grad)
    assert q.engine.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 7. the composed chain
def test_composed_chain_reaches_the_rays():
    """coarse query (diff=True) -> raw2outputs_NeRFW(typ="coarse", test_time=True) -> sample_pdf(diff=True, u=u) -> sort -> fine query ->
    raw2outputs_NeRFW(typ="fine"): d L/d rays_o and d L/d rays_d of a loss on rgb and depth against float64 autograd through the
    oracle's query_coarse_sigma, coarse_weights, sample_pdf, sort, query_fine and composite_fine.  The ratio rule of
    test_gpu_sample_pdf_grad.py: device error over the fp32 CPU oracle's error, both against float64, per row.  The margin is measured in
    the same test: the same chain with the samples DETACHED (kernels of the fine path alone) gives r_det, and the attached chain must
    hold r_att <= max(CHAIN_FACTOR, 2 r_det) for each of the two gradients.  u is built from the float64 cdf: every draw in the middle
    80 % of a bin wider than 1e-3, so at least 1e-4 from any knot (asserted).  The attached and detached device gradients must differ
    by more than 5 % (relative maximum): the path is connected.
    Measured on an MI355X (LABBOOK R22.2), device error / yardstick = ratio: attached d o 7.18e-5 / 6.68e-5 = 1.08, d d 1.72e-4 /
    1.51e-4 = 1.14; detached d o 8.77e-5 / 8.40e-5 = 1.04, d d 1.83e-4 / 1.63e-4 = 1.12.  Attached against detached: d o 0.223,
    d d 0.620, on the device and in float64 alike."""
    n, Nc, Ni = 6, 16, 24
    q, (coarse, fine, emb_a, emb_t), (c, f, ea, et) = wrapped()
    gen = torch.Generator().manual_seed(31)
    o = torch.rand(n, 3, generator=gen) - .5
    d = torch.randn(n, 3, generator=gen) * .7
    hist = torch.randint(0, 60, (n, 10), generator=gen).float()
    G_rgb, G_depth = torch.randn(n, 3, generator=gen), torch.randn(n, generator=gen)
    z = (.5 + 2.5 * torch.linspace(0., 1., Nc)).expand(n, Nc).contiguous()
    z_mid = .5 * (z[:, 1:] + z[:, :-1])
    with torch.no_grad():
        s64 = orc.query_coarse_sigma(d64(c), o.double()[:, None] + d.double()[:, None] * z.double()[..., None])[..., 0]
        knots = cdf64(orc.coarse_weights(s64, z.double())[1][:, 1:-1])
    width = knots[:, 1:] - knots[:, :-1]
    wide = width > 1e-3
    assert bool((wide.sum(-1) >= 1).all())
    pick = torch.multinomial(wide.float(), Ni, replacement=True, generator=gen)
    u = (knots[:, :-1].gather(1, pick) + (.1 + .8 * torch.rand(n, Ni, generator=gen).double()) * width.gather(1, pick)).float()
    assert bool((width.gather(1, pick) > 1e-3).all())
    assert float((u.double()[:, :, None] - knots[:, None, :]).abs().min()) >= 1e-4

    def oracle(dtype, attached):
        cc, ff = ({k: t.to(dtype) for k, t in p.items()} for p in (c, f))
        oo, dd = o.to(dtype).clone().requires_grad_(True), d.to(dtype).clone().requires_grad_(True)
        zz, zm = z.to(dtype), z_mid.to(dtype)
        v = dd / dd.norm(dim=-1, keepdim=True)
        sigma = orc.query_coarse_sigma(cc, oo[:, None] + dd[:, None] * zz[..., None])[..., 0]
        zs = orc.sample_pdf(zm, orc.coarse_weights(sigma, zz)[1][:, 1:-1], Ni, False, u.to(dtype))
        zf = torch.sort(torch.cat([zz, zs if attached else zs.detach()], -1), -1).values
        raw = orc.query_fine(ff, ea.to(dtype), et.to(dtype), oo[:, None] + dd[:, None] * zf[..., None], v, hist)
        out = orc.composite_fine(raw, zf, test_time=True, static_only=True)
        ((out["rgb"] * G_rgb.to(dtype)).sum() + (out["depth"] * G_depth.to(dtype)).sum()).backward()
        return oo.grad.double(), dd.grad.double()

    def device(attached):
        oo, dd = dev(o).requires_grad_(True), dev(d).requires_grad_(True)
        zd, h = dev(z), dev(hist)
        v = dd / dd.norm(dim=-1, keepdim=True)
        if attached:
            sigma = q(oo[:, None] + dd[:, None] * zd[..., None], v, h, coarse, 'coarse', emb_a, emb_t, False, True, diff=True)
            assert sigma.requires_grad
        else:
            with torch.no_grad():
                sigma = q(oo[:, None] + dd[:, None] * zd[..., None], v, h, coarse, 'coarse', emb_a, emb_t, False, True)
        weights = rendering.raw2outputs_NeRFW(sigma, zd, None, 0., False, test_time=True, typ="coarse")[3]
        zs = rendering.sample_pdf(dev(z_mid), weights[..., 1:-1], Ni, u=dev(u), diff=attached)
        assert zs.requires_grad == attached
        zf = torch.sort(torch.cat([zd, zs], -1), -1).values
        raw = q(oo[:, None] + dd[:, None] * zf[..., None], v, h, fine, 'fine', emb_a, emb_t, True, True)
        rgb, _, _, _, depth, _, _ = rendering.raw2outputs_NeRFW(raw, zf, None, 0., True, test_time=True, typ="fine")
        ((rgb * dev(G_rgb)).sum() + (depth * dev(G_depth)).sum()).backward()
        assert bool(torch.isfinite(oo.grad).all() and torch.isfinite(dd.grad).all())
        return oo.grad, dd.grad

    ratios, grads = {}, {}
    for attached in (True, False):
        r64, r32, got = oracle(torch.float64, attached), oracle(torch.float32, attached), device(attached)
        grads[attached] = (got, r64)
        for name, g, a, b in zip(("d o", "d d"), got, r64, r32):
            e, y = row_err(g, a), row_err(b, a)
            ratios[attached, name] = e / max(y, ULP)
            print(f"composed chain, samples {'attached' if attached else 'detached'}: {name} device {e:.2e} yardstick {y:.2e} "
                  f"ratio {ratios[attached, name]:.2f}")
    for i, name in enumerate(("d o", "d d")):
        share64 = relmax(grads[True][1][i], grads[False][1][i])
        share = relmax(grads[True][0][i], grads[False][0][i].cpu())
        print(f"composed chain: {name} attached against detached, relative maximum: device {share:.3f} float64 {share64:.3f}")
        assert share > .05
        assert ratios[True, name] <= max(CHAIN_FACTOR, 2 * ratios[False, name]), (name, ratios)
    assert q.engine.range_flags() == 0
