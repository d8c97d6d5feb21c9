"""GPU tests of the point queries: NerfHEngine.mlp_coarse_points / mlp_fine_points / mlp_fine_points_backward (dfn_mlp_*_points) and
the callable network_query_fn (nerfw.HipQuery.__call__, the reference's run_network_NeRFW: models/nerfw.py:15-95).

Two checkers.
  * The ray entries.  The points kernels are the ray kernels behind the three inputs of a point, so for pts = fl(o + fl(d z)), formed
    on the CPU in fp32 with two separately rounded operations as the ray kernels form them, every output must have the SAME BITS.
  * The CPU oracle (orc.query_fine / orc.query_coarse_sigma and torch autograd through them) on scattered points, which the ray
    entries cannot express, under the bounds of test_gpu_nerfh.py::test_mlp_fine / test_mlp_coarse and of
    test_gpu_grad.py::test_mlp_fine_backward_vs_autograd."""
import numpy as np
import pytest
import torch

from dfnet_amd import _lib, engine as eng, nerfw, synthetic as syn
from oracle import nerfh_oracle as orc

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda:0"
PRECS = ("f32", "f16x3", "f16")
TOL_FINE = {"f32": 3e-6, "f16x3": 3e-6, "f16": 3e-4}      # test_mlp_fine
TOL_COARSE = {"f32": 2e-6, "f16x3": 2e-6, "f16": 2e-4}    # test_mlp_coarse
TOL_NET = {"f32": 1e-5, "f16x3": 1e-5}                    # test_mlp_fine_backward_vs_autograd (relative maximum; relative L2 of d pts)
GROUPS = (slice(0, 3), slice(3, 4), slice(4, 7), slice(7, 8), slice(8, 9))


def relmax(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert not torch.isnan(a).any()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().double()
    return float((a - b).norm() / b.norm())


def tt(d):
    return {k: T(v) for k, v in d.items()}


def dev(x):
    return torch.as_tensor(x).float().to(DEV).contiguous()


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for width, seed in ((128, 0), (256, 2)):
        cw, fw, ea, et = syn.nerfh_weights(seed, W=width)
        out[width] = (eng.NerfHEngine(width=width).load_numpy(cw, fw, ea, et), tt(cw), tt(fw), T(ea), T(et))
    return out


def big_shape():
    """More points than 512 x the compute units (one 512-point tile of the f16 kernel per persistent workgroup; the other kernels'
    tiles are smaller), not a multiple of 512: a workgroup takes a second tile in every kernel, the last tile is partial."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows, N = 515, 512 * cus // 515 + 3    # 256 compute units: (515, 257)
    while rows * N % 512 == 0:
        N += 1
    assert rows * N > 512 * cus
    return rows, N


FORWARD_SHAPES = [(1, 1, False), (3, 5, False), (37, 7, False), (129, 24, True), "big"]
_collinear_cache = {}


def collinear(shape):
    """Rays, depths, view directions, histograms and the points fl(o + fl(d z)) (fp32, on the CPU) of a case; made once."""
    if shape not in _collinear_cache:
        rows, N, per_row_hist = big_shape() + (False,) if shape == "big" else shape
        g = torch.Generator().manual_seed(rows * 1000 + N)
        o = torch.rand(rows, 3, generator=g) - .5
        d = torch.randn(rows, 3, generator=g) * .7
        v = d / d.norm(dim=-1, keepdim=True)
        z = torch.sort(torch.rand(rows, N, generator=g) * 2.5, -1)[0]
        hist = torch.randint(0, 60, (rows, 10), generator=g).float() if per_row_hist else T(syn.HIST_IDX)[None].clone()
        pts = o[:, None] + d[:, None] * z[..., None]      # two separately rounded fp32 operations: add_rn(o, mul_rn(d, z))
        _collinear_cache[shape] = tuple(t.to(DEV).contiguous() for t in (o, d, v, z, hist, pts))
    return _collinear_cache[shape]


def scattered(rows, N, per_row_hist, seed):
    """Points uniform in [-1.5, 1.5]^3 with one random unit view direction per row: on no common ray."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(rows, N, 3, generator=g) * 3 - 1.5
    v = torch.randn(rows, 3, generator=g)
    v = v / v.norm(dim=-1, keepdim=True)
    hist = torch.randint(0, 60, (rows, 10), generator=g).float() if per_row_hist else T(syn.HIST_IDX)[None].clone()
    return pts, v, hist


# ---------------------------------------------------------------------------------------------- 1. the bits of the ray entries
@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", FORWARD_SHAPES, ids=str)
def test_fine_points_have_the_bits_of_the_ray_entry(scenes, width, prec, shape):
    E = scenes[width][0]
    o, d, v, z, hist, pts = collinear(shape)
    want = E.mlp_fine(o, d, v, hist, z, precision=prec)
    got = E.mlp_fine_points(pts, v, hist, precision=prec)
    assert got.shape == want.shape == pts.shape[:2] + (9,)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} values differ"
    assert E.range_flags() == 0


@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", FORWARD_SHAPES, ids=str)
def test_coarse_points_have_the_bits_of_the_ray_entry(scenes, width, prec, shape):
    """Each point as a ray of its own with rays_o = point, rays_d = 0 and two coarse samples: o + 0 z = o exactly, so column 0 of
    mlp_coarse is the network at the point."""
    E = scenes[width][0]
    pts = collinear(shape)[5]
    flat = pts.reshape(-1, 3)
    want = E.mlp_coarse(flat, torch.zeros_like(flat), 2, 0., 1., precision=prec)[:, 0].reshape(pts.shape[:2])
    got = E.mlp_coarse_points(pts, precision=prec)
    assert got.shape == pts.shape[:2]
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} values differ"
    assert E.range_flags() == 0


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("shape", FORWARD_SHAPES[:4], ids=str)
def test_points_backward_has_the_bits_of_the_ray_entry(scenes, prec, shape):
    E = scenes[128][0]
    o, d, v, z, hist, pts = collinear(shape)
    G = torch.randn(pts.shape[:2] + (9,), generator=torch.Generator().manual_seed(7)).to(DEV)
    want = E.mlp_fine_backward(o, d, v, hist, z, G, precision=prec)
    got = E.mlp_fine_points_backward(pts, v, hist, G, precision=prec)
    assert got.shape == want.shape == pts.shape[:2] + (6,)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} values differ"
    assert E.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 2. the oracle on scattered points
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rows,N,per_row_hist", [(1, 5, False), (40, 192, False), (77, 50, True)])
def test_fine_points_vs_oracle_on_scattered_points(scenes, prec, rows, N, per_row_hist):
    E, c, f, ea, et = scenes[128]
    pts, v, hist = scattered(rows, N, per_row_hist, rows * 1000 + N)
    with torch.no_grad():
        ref = orc.query_fine(f, ea, et, pts, v, hist.expand(rows, 10))
    got = E.mlp_fine_points(dev(pts), dev(v), dev(hist), precision=prec)
    errs = [relmax(got[..., ch], ref[..., ch]) for ch in GROUPS]
    print(f"{prec} ({rows},{N}): rgb {errs[0]:.2e} sigma {errs[1]:.2e} t_rgb {errs[2]:.2e} t_sigma {errs[3]:.2e} beta {errs[4]:.2e}")
    assert max(errs) < TOL_FINE[prec], errs
    assert E.range_flags() == 0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rows,N", [(1, 5), (40, 192), (77, 50)])
def test_coarse_points_vs_oracle_on_scattered_points(scenes, prec, rows, N):
    E, c, f, ea, et = scenes[128]
    pts = scattered(rows, N, False, rows * 1000 + N)[0]
    with torch.no_grad():
        ref = orc.query_coarse_sigma(c, pts)[..., 0]
    err = relmax(E.mlp_coarse_points(dev(pts), precision=prec), ref)
    print(f"{prec} ({rows},{N}): sigma {err:.2e}")
    assert err < TOL_COARSE[prec]
    assert E.range_flags() == 0


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("rows,N", [(5, 24), (3, 70), (9, 192)])
def test_points_backward_vs_autograd_on_scattered_points(scenes, prec, rows, N):
    """d sum(raw * G) / d (points, viewdirs) of the fine network, all nine output channels weighted."""
    E, c, f, ea, et = scenes[128]
    pts, v, hist = scattered(rows, N, False, rows * 1000 + N)
    G = torch.randn(rows, N, 9, generator=torch.Generator().manual_seed(11))
    p, vv = pts.clone().requires_grad_(True), v.clone().requires_grad_(True)
    (orc.query_fine(f, ea, et, p, vv, hist.expand(rows, 10)) * G).sum().backward()
    got = E.mlp_fine_points_backward(dev(pts), dev(v), dev(hist), dev(G), precision=prec)
    e_pts, e_v, l2 = relmax(got[..., :3], p.grad), relmax(got[..., 3:].sum(1), vv.grad), rel_l2(got[..., :3], p.grad)
    print(f"{prec} ({rows},{N}): d pts {e_pts:.2e} (L2 {l2:.2e})  d viewdirs {e_v:.2e}")
    assert e_pts < TOL_NET[prec] and e_v < TOL_NET[prec] and l2 < TOL_NET[prec]
    assert E.range_flags() == 0


@pytest.mark.parametrize("prec", PRECS)
def test_fine_points_width_256_vs_oracle(scenes, prec):
    """Netwidth 256 has no oracle bound of its own in the suite, so the yardstick is measured: the distance of the ray entry mlp_fine
    from the oracle on collinear points of the same count and seed (the largest relative maximum over the five channel groups).  The
    points entry on scattered points must stay within TWICE that: the kernels differ in the input path alone, which adds no arithmetic;
    the factor covers that the two point sets differ (scattered points reach |x| = 1.5 against ~1 along the rays).
    Measured on an MI355X, (40, 192) points, mlp_fine_points on scattered points / mlp_fine on collinear points (LABBOOK R13.1):
    f32 2.05e-7 / 2.06e-7, f16x3 2.05e-7 / 2.06e-7, f16 5.07e-5 / 5.66e-5."""
    E, c, f, ea, et = scenes[256]
    rows, N, seed = 40, 192, 256
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(rows, 3, generator=g) - .5
    d = torch.randn(rows, 3, generator=g) * .7
    vr = d / d.norm(dim=-1, keepdim=True)
    z = torch.sort(torch.rand(rows, N, generator=g) * 2.5, -1)[0]
    pts, v, hist = scattered(rows, N, False, seed)
    with torch.no_grad():
        ref_ray = orc.query_fine(f, ea, et, o[:, None] + d[:, None] * z[..., None], vr, hist.expand(rows, 10))
        ref_pts = orc.query_fine(f, ea, et, pts, v, hist.expand(rows, 10))
    ray = E.mlp_fine(dev(o), dev(d), dev(vr), dev(hist), dev(z), precision=prec)
    got = E.mlp_fine_points(dev(pts), dev(v), dev(hist), precision=prec)
    yard = max(relmax(ray[..., ch], ref_ray[..., ch]) for ch in GROUPS)
    err = max(relmax(got[..., ch], ref_pts[..., ch]) for ch in GROUPS)
    print(f"width 256 {prec}: mlp_fine_points on scattered points {err:.2e} from the oracle; mlp_fine on collinear points {yard:.2e}")
    assert err <= 2 * yard
    assert E.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 3. chunking
@pytest.mark.parametrize("width,prec", [(128, "f16x3"), (128, "f16"), (256, "f32")])
def test_chunked_query_has_the_bits_of_the_unsplit_one(scenes, width, prec, monkeypatch):
    E = scenes[width][0]
    pts, v, hist = (dev(t) for t in scattered(37, 7, True, 5))
    G = torch.randn(37, 7, 9, generator=torch.Generator().manual_seed(3)).to(DEV)
    whole = (E.mlp_coarse_points(pts, precision=prec), E.mlp_fine_points(pts, v, hist, precision=prec))
    if width == 128 and prec != "f16":
        whole += (E.mlp_fine_points_backward(pts, v, hist, G, precision=prec),)
    monkeypatch.setattr(E, "POINTS_CHUNK", 70)         # 10 rows of 7 points per call: 10, 10, 10, 7
    assert len(E._point_chunks(37, 7, True)) == 4
    split = (E.mlp_coarse_points(pts, precision=prec), E.mlp_fine_points(pts, v, hist, precision=prec))
    if len(whole) == 3:
        split += (E.mlp_fine_points_backward(pts, v, hist, G, precision=prec),)
    monkeypatch.setattr(E, "POINT_ROWS_CHUNK", 3)      # the row limit of the fine queries: 13 calls
    assert len(E._point_chunks(37, 7, True)) == 13 and len(E._point_chunks(37, 7, False)) == 4
    rows3 = E.mlp_fine_points(pts, v, hist, precision=prec)
    for a, b in zip(whole, split):
        assert torch.equal(a, b)
    assert torch.equal(whole[1], rows3)
    assert E.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 4. the callable
def wrapped(width=128, seed=0, precision="f16x3"):
    """An engine wrapped as create_nerf wraps it: the modules behind it and a HipQuery that carries both."""
    cw, fw, ea, et = syn.nerfh_weights(seed, W=width)
    coarse = nerfw.NeRFW('coarse', D=8, W=width, skips=[4], in_channels_xyz=63, in_channels_dir=27)
    fine = nerfw.NeRFW('fine', D=8, W=width, skips=[4], in_channels_xyz=63, in_channels_dir=27, encode_appearance=True,
                       encode_transient=True, in_channels_a=50, in_channels_t=20)
    coarse.load_state_dict(tt(cw))
    fine.load_state_dict(tt(fw))
    emb_a, emb_t = torch.nn.Embedding(1000, 5), torch.nn.Embedding(1000, 2)
    emb_a.weight.data.copy_(T(ea))
    emb_t.weight.data.copy_(T(et))
    mods = tuple(m.to(DEV) for m in (coarse, fine, emb_a, emb_t))
    E = eng.NerfHEngine(width=width, precision=precision)
    E.load_modules(*mods)
    return nerfw.HipQuery(E, modules=mods), mods, (tt(cw), tt(fw), T(ea), T(et))


@pytest.fixture(scope="module")
def query():
    return wrapped()


def test_query_shapes_and_channels(query):
    q, (coarse, fine, emb_a, emb_t), _ = query
    pts, v, hist = (dev(t) for t in scattered(6, 11, True, 21))
    raw = q(pts, v, hist, fine, 'fine', emb_a, emb_t, True, True)         # the reference's positional order
    assert raw.shape == (6, 11, 9) and torch.equal(raw, q.engine.mlp_fine_points(pts, v, hist))
    four = q(pts, v, hist, fine, 'fine', emb_a, emb_t, False, True)
    assert four.shape == (6, 11, 4) and torch.equal(four, raw[..., :4])
    sigma = q(pts, v, hist, coarse, 'coarse', emb_a, emb_t, False, True)
    assert sigma.shape == (6, 11, 1) and torch.equal(sigma[..., 0], q.engine.mlp_coarse_points(pts))
    assert torch.equal(q(pts, v, hist), raw)                              # the defaults: typ='fine', every module None
    # a flat list of points, each with a view direction of its own
    flat, vf, hf = pts.reshape(-1, 1, 3), v.repeat_interleave(11, 0), hist.repeat_interleave(11, 0)
    raw_flat = q(flat, vf, hf, fine, 'fine', emb_a, emb_t, True, True)
    assert raw_flat.shape == (66, 1, 9) and torch.equal(raw_flat.reshape(6, 11, 9), raw)
    assert q(flat, vf, hf, coarse, 'coarse').shape == (66, 1, 1)
    assert q.engine.range_flags() == 0


def test_query_refuses_foreign_modules_and_unbuilt_cases(query):
    q, (coarse, fine, emb_a, emb_t), _ = query
    pts, v, hist = (dev(t) for t in scattered(2, 3, False, 22))
    with pytest.raises(ValueError, match="network_fn"):
        q(pts, v, hist, coarse, 'fine', emb_a, emb_t)       # the coarse module is not the fine network
    with pytest.raises(ValueError, match="network_fn"):
        q(pts, v, hist, torch.nn.Linear(3, 3), 'coarse')
    with pytest.raises(ValueError, match="embedding_a"):
        q(pts, v, hist, fine, 'fine', torch.nn.Embedding(1000, 5), emb_t)
    with pytest.raises(NotImplementedError, match="test_time=False"):
        q(pts, v, hist, coarse, 'coarse', emb_a, emb_t, False, False)
    with pytest.raises(NotImplementedError, match="autograd"):
        q(pts.clone().requires_grad_(True), v, hist, coarse, 'coarse', emb_a, emb_t, False, True)
    with torch.no_grad():                                   # no graph wanted: the plain query
        assert q(pts.clone().requires_grad_(True), v, hist, coarse, 'coarse').shape == (2, 3, 1)
    q64, mods64, _ = wrapped(width=64, seed=3)
    with pytest.raises(NotImplementedError, match="netwidth 64"):
        q64(pts, v, hist, mods64[1], 'fine')
    for call in (lambda: q64.engine.mlp_fine_points(pts, v, hist), lambda: q64.engine.mlp_coarse_points(pts),
                 lambda: q64.engine.mlp_fine_points_backward(pts, v, hist, torch.zeros(2, 3, 9, device=DEV), precision="f32")):
        with pytest.raises(_lib.DfnError, match=r"status -4\).*dfn_nerfh_generic_"):   # DFN_ERR_UNSUPPORTED, the existing message
            call()


@pytest.mark.parametrize("precision", ["f16x3", "f16", "f32"])
def test_query_autograd_vs_oracle(precision):
    """(raw * G).sum().backward() through the callable: d L/d inputs and d L/d viewdirs against torch autograd through the oracle.
    An engine in plain f16 differentiates in split-f16, as render does under autograd."""
    q, (coarse, fine, emb_a, emb_t), (c, f, ea, et) = wrapped(precision=precision)
    rows, N = 4, 33
    pts, v, hist = scattered(rows, N, True, 23)
    G = torch.randn(rows, N, 9, generator=torch.Generator().manual_seed(5))
    p, vv = pts.clone().requires_grad_(True), v.clone().requires_grad_(True)
    (orc.query_fine(f, ea, et, p, vv, hist) * G).sum().backward()
    x, w = dev(pts).requires_grad_(True), dev(v).requires_grad_(True)
    raw = q(x, w, dev(hist), fine, 'fine', emb_a, emb_t, True, True)
    assert raw.requires_grad and raw.shape == (rows, N, 9)
    (raw * dev(G)).sum().backward()
    e_pts, e_v, l2 = relmax(x.grad, p.grad), relmax(w.grad, vv.grad), rel_l2(x.grad, p.grad)
    print(f"engine {precision}: d inputs {e_pts:.2e} (L2 {l2:.2e})  d viewdirs {e_v:.2e}")
    assert e_pts < 1e-5 and e_v < 1e-5 and l2 < 1e-5      # TOL_NET
    # the normals case: a loss on the static density alone, gradient with respect to the points only
    x2 = dev(pts).requires_grad_(True)
    q(x2, dev(v), dev(hist), None, 'fine', output_transient=False)[..., 3].sum().backward()
    p2 = pts.clone().requires_grad_(True)
    orc.query_fine(f, ea, et, p2, v, hist)[..., 3].sum().backward()
    assert torch.isfinite(x2.grad).all() and float(x2.grad.abs().max()) > 0
    e_n, l2_n = relmax(x2.grad, p2.grad), rel_l2(x2.grad, p2.grad)
    print(f"engine {precision}: d sigma / d inputs {e_n:.2e} (L2 {l2_n:.2e})")
    assert e_n < 1e-5 and l2_n < 1e-5
    assert q.engine.range_flags() == 0
