"""The coarse network's TRAINING query on points and its input gradient: dfn_mlp_coarse_static_points /
dfn_mlp_coarse_static_points_backward (nerfh_coarse_static[_fold]_pts_kernel, nerfh_coarse_static_backward_pts_kernel),
NerfHEngine.mlp_coarse_static_points[_backward], nerfw._CoarseStaticPointsFn and HipQuery.__call__(..., typ='coarse', test_time=False,
static=True) -- run_network_NeRFW's `typ == 'coarse'` training branch (models/nerfw.py:47-60, 326-343): raw4 = (static_rgb, static_sigma).

Truth for the forward is the fp32 CPU oracle (orc.query_coarse_static) under the suite's bounds for the same layers of the same trunk
(TOL_FINE for the rgb channels, TOL_COARSE for sigma: tests/test_gpu_points.py); for the gradient, torch autograd through the oracle in
FLOAT64 under TOL_NET = 1e-5 (relative maximum and relative L2), the suite's bound for the fine network's input gradient.  Points, seeds
and helpers are those of tests/test_gpu_points.py.  Measured figures are in the docstrings of the tests that print them (LABBOOK R23)."""
import ctypes

import pytest
import torch

from dfnet_amd import _lib, engine as eng, rendering, synthetic as syn
from dfnet_amd._lib import current_stream, ptr
from oracle import nerfh_oracle as orc
from tests.test_gpu_points import DEV, TOL_COARSE, TOL_FINE, TOL_NET, big_shape, dev, rel_l2, relmax, scattered, tt, wrapped
from tests.test_gpu_sample_pdf_grad import CHAIN_FACTOR, ULP, row_err

pytestmark = pytest.mark.gpu
T = torch.from_numpy
PRECS = ("f32", "f16x3", "f16")
GRAD_PRECS = ("f32", "f16x3")
SHAPES = [(1, 1), (3, 5), (37, 7), (9, 192)]   # one live lane; a partial wave; 259 points: a second, partial tile; 1 728 points
TRAINED_FACTOR = 4.0                           # test_trained_like_weights: measured, see its docstring (the suite's stage FACTOR is 2)


def oracle_static(c, pts, v, dtype=torch.float32):
    with torch.no_grad():
        return orc.query_coarse_static({k: t.to(dtype) for k, t in c.items()}, pts.to(dtype), v.to(dtype))


def oracle_grad(c, pts, v, G, dtype=torch.float64):
    """d sum(raw4 * G) / d (pts, viewdirs) by autograd through the oracle in `dtype` on the CPU -> float64."""
    p, w = pts.to(dtype).clone().requires_grad_(True), v.to(dtype).clone().requires_grad_(True)
    (orc.query_coarse_static({k: t.to(dtype) for k, t in c.items()}, p, w) * G.to(dtype)).sum().backward()
    return p.grad.double(), w.grad.double()


def seed_grad(rows, N, seed=11):
    return torch.randn(rows, N, 4, generator=torch.Generator().manual_seed(seed))


def forward_errs(got, ref):
    return relmax(got[..., :3], ref[..., :3]), relmax(got[..., 3], ref[..., 3])


@pytest.fixture(scope="module")
def scene():
    cw, fw, ea, et = syn.nerfh_weights(0)
    return eng.NerfHEngine().load_numpy(cw, fw, ea, et), tt(cw)


@pytest.fixture(scope="module")
def scene256():
    cw, fw, ea, et = syn.nerfh_weights(2, W=256)
    return eng.NerfHEngine(width=256).load_numpy(cw, fw, ea, et), tt(cw)


# ---------------------------------------------------------------------------------------------- 1. forward against the fp32 oracle
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rows,N", SHAPES)
def test_forward_vs_oracle(scene, prec, rows, N):
    """Measured on an MI355X (LABBOOK R23.2), relative maximum rgb / sigma, worst of the four shapes: f32 1.15e-7 / 8.20e-8, f16x3
    1.18e-7 / 8.20e-8, f16 4.48e-5 / 2.52e-5."""
    E, c = scene
    pts, v, _ = scattered(rows, N, False, rows * 1000 + N)
    got = E.mlp_coarse_static_points(dev(pts), dev(v), precision=prec)
    assert got.shape == (rows, N, 4)
    e_rgb, e_sig = forward_errs(got, oracle_static(c, pts, v))
    print(f"coarse static query {prec} ({rows},{N}): rgb {e_rgb:.2e} sigma {e_sig:.2e}")
    assert e_rgb < TOL_FINE[prec] and e_sig < TOL_COARSE[prec]
    assert E.range_flags() == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rows,N", SHAPES[1:3])
def test_forward_vs_oracle_width_256(scene256, prec, rows, N):
    """The W = 256 instantiations of the plain unit, under the same bounds.  Measured on an MI355X, rgb / sigma, worst of the two
    shapes: f32 1.12e-7 / 8.57e-8, f16x3 the same, f16 2.95e-5 / 1.14e-5."""
    E, c = scene256
    pts, v, _ = scattered(rows, N, False, rows * 1000 + N)
    got = E.mlp_coarse_static_points(dev(pts), dev(v), precision=prec)
    e_rgb, e_sig = forward_errs(got, oracle_static(c, pts, v))
    print(f"coarse static query, netwidth 256, {prec} ({rows},{N}): rgb {e_rgb:.2e} sigma {e_sig:.2e}")
    assert e_rgb < TOL_FINE[prec] and e_sig < TOL_COARSE[prec]
    assert E.range_flags() == 0


def test_kernel_vs_golden_g18(scene, gold):
    """The kernels against the reference's own numbers (tests/golden/make_golden_coarse_static.py): the forward under test 1's
    bounds, the gradient (the reference's fp32 autograd) under TOL_NET.  Measured on an MI355X: forward rgb / sigma f32 1.22e-7 / 0,
    f16x3 1.22e-7 / 8.18e-8, f16 3.54e-5 / 1.55e-5; gradient d pts / d viewdirs f32 4.72e-7 / 2.05e-7, f16x3 5.76e-7 / 1.43e-7."""
    E, _ = scene
    g = gold("g18_coarse_static")
    for prec in PRECS:
        got = E.mlp_coarse_static_points(dev(T(g["pts"])), dev(T(g["viewdirs"])), precision=prec)
        e_rgb, e_sig = forward_errs(got, T(g["raw4"]))
        print(f"coarse static query {prec} vs G18: rgb {e_rgb:.2e} sigma {e_sig:.2e}")
        assert e_rgb < TOL_FINE[prec] and e_sig < TOL_COARSE[prec]
    for prec in GRAD_PRECS:
        gp = E.mlp_coarse_static_points_backward(dev(T(g["pts"])), dev(T(g["viewdirs"])), dev(T(g["G"])), precision=prec)
        e_p, e_v = relmax(gp[..., :3], T(g["g_pts"])), relmax(gp[..., 3:].sum(1), T(g["g_viewdirs"]))
        print(f"coarse static gradient {prec} vs G18: d pts {e_p:.2e} d viewdirs {e_v:.2e}")
        assert e_p < TOL_NET[prec] and e_v < TOL_NET[prec]
    assert E.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 2. the tile loop
@pytest.mark.parametrize("prec", PRECS)
def test_tile_loop(scene, prec):
    """More points than 512 x the compute units, the last tile partial: every workgroup takes a second tile, so the next tile's
    points come through the prefetch behind dir_encoding.0's mid_sync.  A different view direction per row: a wrong row index into
    the seed table would show.  The first 37 and the last 3 rows have the bits they have alone, everything is finite, and 2 000
    random points agree with the oracle under test 1's bounds.  Measured on an MI355X, (515, 257), 2 000 points, rgb / sigma: f32 1.08e-7 /
    8.14e-8, f16x3 the same, f16 4.25e-5 / 2.27e-5."""
    E, c = scene
    rows, N = big_shape()
    pts, v, _ = scattered(rows, N, False, rows * 1000 + N)
    P, V = dev(pts), dev(v)
    got = E.mlp_coarse_static_points(P, V, precision=prec)
    assert got.shape == (rows, N, 4) and bool(torch.isfinite(got).all())
    assert torch.equal(got[:37], E.mlp_coarse_static_points(P[:37], V[:37], precision=prec))
    assert torch.equal(got[-3:], E.mlp_coarse_static_points(P[-3:], V[-3:], precision=prec))
    pick = torch.randperm(rows * N, generator=torch.Generator().manual_seed(7))[:2000]
    ref = oracle_static(c, pts.reshape(-1, 1, 3)[pick], v[pick // N])
    e_rgb, e_sig = forward_errs(got.reshape(-1, 1, 4)[pick.to(DEV)], ref)
    print(f"coarse static query {prec} ({rows},{N}), 2 000 points: rgb {e_rgb:.2e} sigma {e_sig:.2e}")
    assert e_rgb < TOL_FINE[prec] and e_sig < TOL_COARSE[prec]
    assert E.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 3. row isolation, write bounds, chunking
@pytest.mark.parametrize("prec", PRECS)
def test_row_isolation_write_bounds_and_chunking(scene, prec, monkeypatch):
    E, _ = scene
    rows, N = 37, 7
    pts, v, _ = scattered(rows, N, False, 5)
    P, V = dev(pts), dev(v)
    whole = E.mlp_coarse_static_points(P, V, precision=prec)
    for r in (0, 5, 36):       # a row's output does not depend on its neighbours
        assert torch.equal(whole[r:r + 1], E.mlp_coarse_static_points(P[r:r + 1], V[r:r + 1], precision=prec)), r
    assert torch.equal(whole[10:13], E.mlp_coarse_static_points(P[10:13], V[10:13], precision=prec))
    # the raw entry into the middle of a NaN-filled buffer (an odd float offset: no alignment is asked of raw4)
    pad, n = 1023, rows * N * 4
    buf = torch.full((n + 2 * pad,), float("nan"), device=DEV)
    bias = torch.empty(E.lib.dfn_fine_bias_bytes(rows), dtype=torch.uint8, device=DEV)
    rc = E.lib.dfn_mlp_coarse_static_points(E.handle, _lib.PRECISIONS[prec], ptr(P), ptr(V), rows, N, ctypes.c_void_p(buf.data_ptr() + 4 * pad),
                                            ctypes.c_void_p(bias.data_ptr()), current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + n:]).all())
    assert torch.equal(buf[pad:pad + n].reshape(rows, N, 4), whole)
    # chunking: by points and by rows, the bits of the unsplit call
    monkeypatch.setattr(E, "POINTS_CHUNK", 70)         # 10 rows of 7 points per call: 10, 10, 10, 7
    assert len(E._point_chunks(rows, N, True)) == 4
    assert torch.equal(E.mlp_coarse_static_points(P, V, precision=prec), whole)
    monkeypatch.setattr(E, "POINT_ROWS_CHUNK", 3)      # the row limit of the fine queries: 13 calls
    assert len(E._point_chunks(rows, N, True)) == 13
    assert torch.equal(E.mlp_coarse_static_points(P, V, precision=prec), whole)
    assert E.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 4. sigma against the sigma-only query
@pytest.mark.parametrize("prec", PRECS)
def test_sigma_channel_vs_the_sigma_only_query(scene, prec):
    """Decided from the code.  Split-f16 (netwidth 128) runs the FOLDED sequence: static_sigma is the head block LY_SIG on h8, the
    layer mlp_coarse_points' kernel ends in, behind the same trunk() instantiation; that kernel packs the block half-height, which
    drops the fragments of the rows nothing reads and multiplies the rows ms = 0 by the same fragments in the same order -- the bits
    must agree.  Exact fp32 and f16 run the plain sequence: static_sigma is the FIFTH M-block of xyz_encoding_final's layer (LY_FIN),
    another layer instantiation (in f16 also another staging unit and conversion schedule) than the coarse kernel's LY_SIG; the same
    dot product in the same chunk order, but nothing in the code promises the same bits: the two are held to TOL_COARSE of each other.
    Measured on an MI355X: 0 of 259 values differ in all three modes (exact fp32 and f16 too, which the test does not ask for)."""
    E, _ = scene
    pts, v, _ = scattered(37, 7, False, 37007)
    P, V = dev(pts), dev(v)
    sig4 = E.mlp_coarse_static_points(P, V, precision=prec)[..., 3]
    sig1 = E.mlp_coarse_points(P, precision=prec)
    if prec == "f16x3":
        assert torch.equal(sig4, sig1), f"{int((sig4 != sig1).sum())} of {sig1.numel()} values differ"
    else:
        e = relmax(sig4, sig1.cpu())
        print(f"sigma channel against mlp_coarse_points, {prec}: {e:.2e} ({int((sig4 != sig1).sum())} of {sig1.numel()} values differ)")
        assert e < TOL_COARSE[prec]


# ---------------------------------------------------------------------------------------------- 5. the gradient against float64 autograd
@pytest.mark.parametrize("prec", GRAD_PRECS)
@pytest.mark.parametrize("rows,N", SHAPES)
def test_gradient_vs_float64_autograd(scene, prec, rows, N):
    """d sum(raw4 * G) / d (pts, viewdirs), all four channels weighted.  Measured on an MI355X (LABBOOK R23.2), relative maximum of
    d pts (relative L2) / d viewdirs summed per row, f32 then f16x3: (1,1) 2.26e-7 (2.42e-7) / 1.18e-7, 8.32e-7 (8.75e-7) / 2.58e-7; (3,5)
    2.97e-7 (3.60e-7) / 5.32e-7, 6.21e-7 (7.23e-7) / 4.66e-7; (37,7) 2.82e-7 (3.08e-7) / 1.35e-7, 6.63e-7 (5.62e-7) / 1.88e-7; (9,192)
    4.06e-7 (2.98e-7) / 3.15e-7, 6.90e-7 (5.70e-7) / 3.07e-7."""
    E, c = scene
    pts, v, _ = scattered(rows, N, False, rows * 1000 + N)
    G = seed_grad(rows, N)
    ref_p, ref_v = oracle_grad(c, pts, v, G)
    got = E.mlp_coarse_static_points_backward(dev(pts), dev(v), dev(G), precision=prec)
    assert got.shape == (rows, N, 6)
    gv = got[..., 3:].sum(1)
    e_p, l2, e_v, l2_v = relmax(got[..., :3], ref_p), rel_l2(got[..., :3], ref_p), relmax(gv, ref_v), rel_l2(gv, ref_v)
    print(f"coarse static gradient {prec} ({rows},{N}): d pts {e_p:.2e} (L2 {l2:.2e})  d viewdirs {e_v:.2e} (L2 {l2_v:.2e})")
    assert max(e_p, l2, e_v, l2_v) < TOL_NET[prec]
    assert E.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 6. the gradient's structure
@pytest.mark.parametrize("prec", GRAD_PRECS)
def test_gradient_structure(scene, prec):
    """G 2^k gives 2^k x the gradient bit for bit (k = +-20): the per-point scale is a power of two taken from the seeds, the final
    division by it is exact, and every other operation is linear in g.  Rows with G = 0 give exact zeros; a row with G = 1e6 beside
    one with 1e-6 gives each the bits it has alone.  G on the sigma channel alone reproduces mlp_coarse_points_backward's d points
    within TOL_NET with exactly zero d viewdir; G on the rgb channels alone gives a non-zero d viewdir.  The raw entry writes
    n_rows N 6 floats and nothing else.  Measured on an MI355X: G on sigma alone gives mlp_coarse_points_backward's d points BIT FOR BIT in
    both modes (relative maximum 0)."""
    E, _ = scene
    rows, N = 37, 7
    pts, v, _ = scattered(rows, N, False, rows * 1000 + N)
    P, V = dev(pts), dev(v)
    G = seed_grad(rows, N)
    back = lambda g, p=P, vv=V: E.mlp_coarse_static_points_backward(p, vv, dev(g), precision=prec)
    base = back(G)
    assert float(base[..., :3].abs().max()) > 0 and float(base[..., 3:].abs().max()) > 0
    for k in (20, -20):
        scaled = back(G * 2. ** k)
        assert torch.equal(scaled, base * 2. ** k), f"k = {k}: {int((scaled != base * 2. ** k).sum())} values differ"
    Gz = G.clone()
    Gz[5] = 0.
    Gz[20] = 0.
    Gz[11, 3] = 0.
    gz = back(Gz)
    assert bool((gz[5] == 0).all() and (gz[20] == 0).all() and (gz[11, 3] == 0).all())
    keep = torch.ones(rows, dtype=torch.bool)
    keep[[5, 20, 11]] = False
    assert torch.equal(gz[keep.to(DEV)], base[keep.to(DEV)])
    Gm = G.clone()
    Gm[3] = 1e6
    Gm[4] = 1e-6
    gm = back(Gm)
    for r in (3, 4):
        assert torch.equal(gm[r:r + 1], back(Gm[r:r + 1], P[r:r + 1], V[r:r + 1]))
    assert bool(torch.isfinite(gm).all())
    # one channel group at a time
    Gs = torch.zeros_like(G)
    Gs[..., 3] = G[..., 3]
    gs = back(Gs)
    assert bool((gs[..., 3:] == 0).all())                       # sigma does not see the view direction
    want = E.mlp_coarse_points_backward(P, dev(G[..., 3]), precision=prec)
    e = relmax(gs[..., :3], want.cpu())
    print(f"coarse static gradient {prec}, G on sigma alone, against mlp_coarse_points_backward: {e:.2e}")
    assert e < TOL_NET[prec]
    Gc = G.clone()
    Gc[..., 3] = 0.
    assert float(back(Gc)[..., 3:].abs().max()) > 0
    # the raw entry into the middle of a NaN-filled buffer
    pad, n = 1023, rows * N * 6
    buf = torch.full((n + 2 * pad,), float("nan"), device=DEV)
    Gd = dev(G)
    bias = torch.empty(E.lib.dfn_fine_bias_bytes(rows), dtype=torch.uint8, device=DEV)
    rc = E.lib.dfn_mlp_coarse_static_points_backward(E.handle, _lib.PRECISIONS[prec], ptr(P), ptr(V), rows, N, ptr(Gd),
                                                     ctypes.c_void_p(buf.data_ptr() + 4 * pad), ctypes.c_void_p(bias.data_ptr()),
                                                     current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + n:]).all())
    assert torch.equal(buf[pad:pad + n].reshape(rows, N, 6), base)
    assert E.range_flags() == 0


def test_entry_status_codes(scene, scene256):
    """What needs a committed handle: null pointers and N < 1 are DFN_ERR_ARG (-1), n_rows == 0 DFN_OK; the gradient refuses plain
    f16 and netwidth 256 with DFN_ERR_UNSUPPORTED (-4)."""
    E, _ = scene
    one, s = ctypes.c_void_p(16), current_stream()
    f32 = _lib.PRECISIONS["f32"]
    fwd, bwd = E.lib.dfn_mlp_coarse_static_points, E.lib.dfn_mlp_coarse_static_points_backward
    assert fwd(E.handle, f32, one, one, 0, 8, one, one, s) == 0 and bwd(E.handle, f32, one, one, 0, 8, one, one, one, s) == 0
    for i in (2, 3, 6, 7):
        args = [E.handle, f32, one, one, 4, 8, one, one, s]
        args[i] = None
        assert fwd(*args) == -1, i
    for i in (2, 3, 6, 7, 8):
        args = [E.handle, f32, one, one, 4, 8, one, one, one, s]
        args[i] = None
        assert bwd(*args) == -1, i
    assert fwd(E.handle, f32, one, one, 4, 0, one, one, s) == -1 and bwd(E.handle, f32, one, one, 4, 0, one, one, one, s) == -1
    assert bwd(E.handle, _lib.PRECISIONS["f16"], one, one, 4, 8, one, one, one, s) == -4
    z3, z1 = torch.zeros(2, 3, 3, device=DEV), torch.zeros(2, 3, device=DEV)
    with pytest.raises(_lib.DfnError, match=r"status -4\).*netwidth 128 only"):
        scene256[0].mlp_coarse_static_points_backward(z3, z1, torch.zeros(2, 3, 4, device=DEV), precision="f32")
    with pytest.raises(_lib.DfnError, match=r"status -4\)"):
        E.mlp_coarse_static_points_backward(z3, z1, torch.zeros(2, 3, 4, device=DEV), precision="f16")
    assert E.mlp_coarse_static_points(torch.zeros(0, 3, 3, device=DEV), torch.zeros(0, 3, device=DEV)).shape == (0, 3, 4)
    assert E.mlp_coarse_static_points_backward(torch.zeros(0, 3, 3, device=DEV), torch.zeros(0, 3, device=DEV),
                                               torch.zeros(0, 3, 4, device=DEV), precision="f32").shape == (0, 3, 6)


# ---------------------------------------------------------------------------------------------- 7. trained-like weights
@pytest.mark.parametrize("prec", GRAD_PRECS)
def test_trained_like_weights(prec):
    """The trained-like fixture's coarse network, 37 rays x 24 points along them (collinear-style: o + d z through the scene), forward
    and gradient against FLOAT64.  No bound in the suite covers trained-like weights, so the yardstick is the fp32 CPU oracle's own
    distance from float64 on the same inputs, floored at one fp32 ulp (tests/test_gpu_sample_pdf_grad.py), and the device must stay
    within TRAINED_FACTOR of it, in the fp32-grade modes (plain f16 has no fp32 yardstick).  
    Measured on an MI355X (LABBOOK R23.2; sigma up to 682, |d pts| up to 7.55e4), device / yardstick = ratio: f32 rgb 5.19e-6 / 4.19e-6 =
    1.24, sigma 1.86e-7 / 3.19e-7 = 0.58, d pts 3.85e-7 / 3.03e-7 = 1.27, d viewdirs 1.99e-5 / 8.73e-6 = 2.27; f16x3 rgb 1.61e-5 /
    4.19e-6 = 3.84, sigma 8.46e-7 / 3.19e-7 = 2.65, d pts 6.06e-7 / 3.03e-7 = 2.00, d viewdirs 2.25e-5 / 8.73e-6 = 2.57.  That is outside
    the suite's stage factor (FACTOR = 2), so TRAINED_FACTOR is 4: the measured worst, 3.84, with the margin
    tests/test_gpu_sample_pdf_grad.py left when it kept CHAIN_FACTOR = 4 over a measured 3.86.  Why the ratio is above 2: the yardstick is ONE
    fp32 evaluation whose own roundings partly cancel, while the split-f16 operands carry 22 bits and static_rgb's pre-activations are
    sums of terms in the hundreds at these weights (the random-init cases of test 1 sit at 1e-7 in both modes)."""
    cw, fw, ea, et = syn.trained_nerfh_weights()
    E, c = eng.NerfHEngine().load_numpy(cw, fw, ea, et), tt(cw)
    rows, N = 37, 24
    g = torch.Generator().manual_seed(rows * 1000 + N)
    o = torch.rand(rows, 3, generator=g) - .5
    d = torch.randn(rows, 3, generator=g) * .7
    v = d / d.norm(dim=-1, keepdim=True)
    z = torch.sort(torch.rand(rows, N, generator=g) * 2.5, -1)[0]
    pts = o[:, None] + d[:, None] * z[..., None]
    G = seed_grad(rows, N)
    ref, ref32 = oracle_static(c, pts, v, torch.float64), oracle_static(c, pts, v)
    got = E.mlp_coarse_static_points(dev(pts), dev(v), precision=prec)
    assert bool(torch.isfinite(got).all())
    ratios = {}
    for name, sl in (("rgb", slice(0, 3)), ("sigma", slice(3, 4))):
        e, y = relmax(got[..., sl], ref[..., sl]), relmax(ref32[..., sl], ref[..., sl])
        ratios[name] = e / max(y, ULP)
        print(f"trained-like weights {prec}: {name} device {e:.2e} yardstick {y:.2e} ratio {ratios[name]:.2f}")
    r64, r32 = oracle_grad(c, pts, v, G), oracle_grad(c, pts, v, G, torch.float32)
    gp = E.mlp_coarse_static_points_backward(dev(pts), dev(v), dev(G), precision=prec)
    assert bool(torch.isfinite(gp).all())
    for name, a, b, b32 in (("d pts", gp[..., :3], r64[0], r32[0]), ("d viewdirs", gp[..., 3:].sum(1), r64[1], r32[1])):
        e, y = relmax(a, b), relmax(b32, b)
        ratios[name] = e / max(y, ULP)
        print(f"trained-like weights {prec}: {name} device {e:.2e} yardstick {y:.2e} ratio {ratios[name]:.2f}  "
              f"(sigma up to {float(ref[..., 3].max()):.3g}, |gradient| up to {float(b.abs().max()):.3g})")
    assert all(r <= TRAINED_FACTOR for r in ratios.values()), ratios
    assert E.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 8. the public surface
@pytest.mark.parametrize("precision", ["f16x3", "f16", "f32"])
def test_query_static(precision):
    """q(pts, v, None, coarse, 'coarse', None, None, False, False, static=True): raw [..., N, 4] with the engine call's bits, attached to
    inputs and viewdirs under autograd (an engine in plain f16 differentiates in split-f16), no graph otherwise.  Measured on an MI355X, d inputs (L2) / d viewdirs from float64: engine f16x3 5.40e-7 (6.13e-7) / 3.82e-7, f16 the same, f32
    2.46e-7 (3.02e-7) / 2.54e-7."""
    q, (coarse, fine, emb_a, emb_t), (c, f, ea, et) = wrapped(precision=precision)
    rows, N = 4, 33
    pts, v, hist = scattered(rows, N, True, 23)
    G = seed_grad(rows, N, 5)
    ref_p, ref_v = oracle_grad(c, pts, v, G)
    x, w = dev(pts).requires_grad_(True), dev(v).requires_grad_(True)
    raw = q(x, w, None, coarse, 'coarse', None, None, False, False, static=True)
    assert raw.shape == (rows, N, 4) and raw.requires_grad
    (raw * dev(G)).sum().backward()
    e_p, l2, e_v = relmax(x.grad, ref_p), rel_l2(x.grad, ref_p), relmax(w.grad, ref_v)
    print(f"engine {precision}: static query, d inputs {e_p:.2e} (L2 {l2:.2e})  d viewdirs {e_v:.2e}")
    assert e_p < 1e-5 and l2 < 1e-5 and e_v < 1e-5      # TOL_NET
    plain = q(x.detach(), w.detach(), None, coarse, 'coarse', None, None, False, False, static=True)
    assert not plain.requires_grad and torch.equal(plain, q.engine.mlp_coarse_static_points(x.detach(), w.detach()))
    if precision != "f16":
        assert torch.equal(raw.detach(), plain)
    with torch.no_grad():
        quiet = q(x, w, None, coarse, 'coarse', None, None, False, False, static=True)
    assert not quiet.requires_grad and quiet.grad_fn is None and torch.equal(quiet, plain)
    only_v = q(x.detach(), w, dev(hist), coarse, 'coarse', emb_a, emb_t, False, False, static=True)     # ts is ignored
    assert only_v.requires_grad
    if precision != "f16":
        assert torch.equal(only_v.detach(), plain)
    # a leading shape of its own, and a flat list of points with a view direction each
    assert q(x.detach().reshape(2, 2, N, 3), w.detach().reshape(2, 2, 3), None, None, 'coarse', test_time=False,
             static=True, output_transient=False).shape == (2, 2, N, 4)
    flat = q(x.detach().reshape(-1, 1, 3), w.detach().repeat_interleave(N, 0), None, coarse, 'coarse', None, None, False, False, static=True)
    assert flat.shape == (rows * N, 1, 4) and torch.equal(flat.reshape(rows, N, 4), plain)
    assert q.engine.range_flags() == 0


def test_query_static_refusals_and_refresh():
    q, (coarse, fine, emb_a, emb_t), (c, f, ea, et) = wrapped()
    pts, v, hist = (dev(t) for t in scattered(2, 3, False, 22))
    with pytest.raises(NotImplementedError, match="test_time=False"):      # without the keyword nothing changes
        q(pts, v, hist, coarse, 'coarse', emb_a, emb_t, False, False)
    with pytest.raises(NotImplementedError, match="static=True"):          # ... and the message says how to opt in
        q(pts, v, hist, coarse, 'coarse', emb_a, emb_t, False, False)
    with pytest.raises(ValueError, match="output_transient"):
        q(pts, v, None, coarse, 'coarse', None, None, True, False, static=True)
    with pytest.raises(ValueError, match="network_fn"):
        q(pts, v, None, fine, 'coarse', None, None, False, False, static=True)
    with pytest.raises(ValueError, match="network_fn"):
        q(pts, v, None, torch.nn.Linear(3, 3), 'coarse', None, None, False, False, static=True)
    with pytest.raises(ValueError, match="viewdirs"):
        q(pts, None, None, coarse, 'coarse', None, None, False, False, static=True)
    with pytest.raises(ValueError, match="viewdirs"):
        q(pts, v[:1], None, coarse, 'coarse', None, None, False, False, static=True)
    # typ='fine', and typ='coarse' with test_time=True, accept the keyword and ignore it
    assert torch.equal(q(pts, v, hist, fine, 'fine', emb_a, emb_t, True, True, static=True), q(pts, v, hist, fine, 'fine', emb_a, emb_t, True, True))
    assert torch.equal(q(pts, v, hist, coarse, 'coarse', emb_a, emb_t, False, True, static=True), q(pts, v, hist, coarse, 'coarse'))
    # netwidth 64: no register-resident kernels
    q64, mods64, _ = wrapped(width=64, seed=3)
    with pytest.raises(NotImplementedError, match="netwidth 64"):
        q64(pts, v, None, mods64[0], 'coarse', None, None, False, False, static=True)
    for call in (lambda: q64.engine.mlp_coarse_static_points(pts, v),
                 lambda: q64.engine.mlp_coarse_static_points_backward(pts, v, torch.zeros(2, 3, 4, device=DEV), precision="f32")):
        with pytest.raises(_lib.DfnError, match=r"status -4\)"):
            call()
    # netwidth 256: the forward exists, a tracked query is refused at the call (the gradient kernels are netwidth 128's)
    q256, mods256, _ = wrapped(width=256, seed=2)
    assert q256(pts, v, None, mods256[0], 'coarse', None, None, False, False, static=True).shape == (2, 3, 4)
    with pytest.raises(NotImplementedError, match="netwidth 128 only"):
        q256(pts.clone().requires_grad_(True), v, None, mods256[0], 'coarse', None, None, False, False, static=True)
    with torch.no_grad():
        assert not q256(pts.clone().requires_grad_(True), v, None, None, 'coarse', output_transient=False, test_time=False, static=True).requires_grad
    # an in-place change of a coarse weight bumps its version counter: the next query sees the new weights
    before = q(pts, v, None, coarse, 'coarse', None, None, False, False, static=True)
    with torch.no_grad():
        coarse.static_rgb[0].bias.add_(0.5)
    after = q(pts, v, None, coarse, 'coarse', None, None, False, False, static=True)
    c2 = dict(c)
    c2["static_rgb.0.bias"] = c["static_rgb.0.bias"] + 0.5
    e_rgb, e_sig = forward_errs(after, oracle_static(c2, pts.cpu(), v.cpu()))
    assert not torch.equal(after[..., :3], before[..., :3]) and torch.equal(after[..., 3], before[..., 3])
    assert e_rgb < TOL_FINE["f16x3"] and e_sig < TOL_COARSE["f16x3"]


# ---------------------------------------------------------------------------------------------- 9. the composed training coarse pass
def test_composed_training_coarse_pass():
    """query(static=True) -> rendering.raw2outputs_NeRFW(raw, z, rays_d, 0, False, test_time=False, typ="coarse") on 12 rays x 16
    stratified depths (models/rendering.py:269-295): rgb0, disp0, acc0 and weights against orc.composite_coarse_train(
    orc.query_coarse_static(...), z) under the bound tests/test_gpu_raw2outputs_compose.py holds its composed stages to (4e-5), and
    d sum(rgb0 G) / d rays_o through both public stages against float64 autograd through the two oracle functions: the yardstick is
    the fp32 CPU oracle's own error, the factor CHAIN_FACTOR, per row (tests/test_gpu_sample_pdf_grad.py::row_err).  Measured on an MI355X (LABBOOK R23.2): rgb0 / disp0 / acc0 / weights 1.12e-7 / 1.28e-7 / 5.96e-8 / 2.92e-7; d rays_o device 9.48e-5,
    yardstick 9.50e-5, ratio 1.00."""
    n, Nc = 12, 16
    q, (coarse, fine, emb_a, emb_t), (c, f, ea, et) = wrapped()
    gen = torch.Generator().manual_seed(41)
    o = torch.rand(n, 3, generator=gen) - .5
    d = torch.randn(n, 3, generator=gen) * .7
    t_rand = torch.rand(n, Nc, generator=gen)
    G = torch.randn(n, 3, generator=gen)
    z = orc.stratified_z(orc.coarse_z(0., 2.5, Nc, n), t_rand).contiguous()
    v = d / d.norm(dim=-1, keepdim=True)

    def oracle(dtype):
        cc = {k: t.to(dtype) for k, t in c.items()}
        oo = o.to(dtype).clone().requires_grad_(True)
        pts = oo[:, None] + d.to(dtype)[:, None] * z.to(dtype)[..., None]
        out = orc.composite_coarse_train(orc.query_coarse_static(cc, pts, v.to(dtype)), z.to(dtype))
        (out["rgb"] * G.to(dtype)).sum().backward()
        return {k: t.detach() for k, t in out.items()}, oo.grad.double()

    (ref, g32), (_, g64) = oracle(torch.float32), oracle(torch.float64)
    oo, dd, zd = dev(o).requires_grad_(True), dev(d), dev(z)
    raw = q(oo[:, None] + dd[:, None] * zd[..., None], dev(v), None, coarse, 'coarse', None, None, False, False, static=True)
    assert raw.shape == (n, Nc, 4) and raw.requires_grad
    rgb0, disp0, acc0, weights, depth0, tsig, beta = rendering.raw2outputs_NeRFW(raw, zd, dd, 0., False, test_time=False, typ="coarse")
    assert tsig is None and weights.shape == (n, Nc)
    for name, a in (("rgb", rgb0), ("disp", disp0), ("acc", acc0), ("weights", weights)):
        e = relmax(a, ref[name])
        print(f"composed training coarse pass: {name}0 {e:.2e}")
        assert e < 4e-5, name
    (rgb0 * dev(G)).sum().backward()
    assert bool(torch.isfinite(oo.grad).all()) and float(oo.grad.abs().max()) > 0
    e, y = row_err(oo.grad, g64), row_err(g32, g64)
    print(f"composed training coarse pass: d rays_o device {e:.2e} yardstick {y:.2e} ratio {e / max(y, ULP):.2f}")
    assert e / max(y, ULP) <= CHAIN_FACTOR
    assert q.engine.range_flags() == 0
