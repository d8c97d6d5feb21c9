"""A TRAINING query on points: dfn_nerfh_points_train_forward / _backward (train_fwd_chain_pts_kernel, train_bwd_chain_pts_kernel and the
fused step's weight-gradient stream), NerfHTrainer.points_forward / points_backward, nerf_train._PointsTrainFn and
HipQuery.__call__(..., train=True) -- run_network_NeRFW with test_time=False as an autograd expression of the network's parameters
(models/nerfw.py:47-95, 297-354).

Netwidth 128, random-init weights from NeRFW's own seeding (the constructor reseeds to 0), fixed seeds.  Truth for the forward is the
fp32 CPU oracle under the suite's split-f16 bounds (tests/test_gpu_points.py); for the weight gradients, torch autograd through the
oracle in FLOAT64 on the CPU, the yardstick being the oracle's own float32 autograd against float64 on the same inputs
(tests/yardstick.py).  Shapes (n_rows, N): (1, 1); (3, 37) = 111 points, under one tile and no multiple of 32; (5, 64) = 320 points,
two tiles, the second partial; (2, 300), a row crossing a tile.  hist_rows 1 and n_rows."""
import ctypes

import pytest
import torch

from dfnet_amd import _lib, engine as eng, nerf_train, nerfw, optim, rendering, synthetic as syn
from dfnet_amd._lib import current_stream, ptr
from oracle import nerfh_oracle as orc
from tests.test_gpu_points import DEV, GROUPS, TOL_COARSE, TOL_FINE, dev, relmax, scattered
from tests.yardstick import float64_default, rel_l2, to64

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SHAPES = [(1, 1), (3, 37), (5, 64), (2, 300)]
CASES = [("coarse", r, n, False) for r, n in SHAPES] + [("fine", r, n, ph) for r, n in SHAPES for ph in (False, True)]
IDS = [f"{net}-{r}x{n}-{'rowhist' if ph else 'onehist'}" for net, r, n, ph in CASES]
# Two-plane storage (the coarse network; the fine one under fused_split): the project's bound for the fused step against float64
# (tests/test_gpu_train.py::test_fused_step_on_trained_like_weights_against_the_float64_oracle): 3 * yardstick + 5e-4 per tensor.
two_plane_bound = lambda yard: 3. * yard + 5e-4
# One-plane fine storage (the default): at these point counts f16 rounding of the stored operands does not average out as it does over
# the step's 3e5 points.  Twice the worst tensor measured against float64 on an MI355X over the cases of
# test_weight_gradients_vs_float64 (its docstring): 1.80e-3, fine.transient_sigma.0.weight at (5, 64).
ONE_PLANE_BOUND = 2 * 1.80e-3


def build(width=128, precision="f16x3", trainer=True):
    """Modules from NeRFW's own seeding, the engine packed from them, a HipQuery that carries both (and a trainer)."""
    coarse = nerfw.NeRFW('coarse', D=8, W=width, skips=[4], in_channels_xyz=63, in_channels_dir=27)
    fine = nerfw.NeRFW('fine', D=8, W=width, skips=[4], in_channels_xyz=63, in_channels_dir=27, encode_appearance=True,
                       encode_transient=True, in_channels_a=50, in_channels_t=20)
    emb_a, emb_t = torch.nn.Embedding(1000, 5), torch.nn.Embedding(1000, 2)
    mods = tuple(m.to(DEV) for m in (coarse, fine, emb_a, emb_t))
    E = eng.NerfHEngine(width=width, precision=precision)
    E.load_modules(*mods)
    q = nerfw.HipQuery(E, modules=mods)
    if trainer:
        q.trainer = nerf_train.NerfHTrainer(E, *mods)
    return q


def cpu_weights(q):
    """{canonical name: fp32 CPU tensor} of the modules behind q ('coarse.<key>', 'fine.<key>', 'embedding_a.weight', ...)."""
    out = {}
    for pre, m in zip(("coarse.", "fine.", "embedding_a.", "embedding_t."), q.modules):
        out.update({pre + k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    return out


@pytest.fixture(scope="module")
def world():
    q = build()
    return q, q.trainer, cpu_weights(q)


def inputs_of(net, rows, N, per_row_hist):
    pts, v, hist = scattered(rows, N, per_row_hist, rows * 1000 + N)
    G = torch.randn(rows, N, 9 if net == "fine" else 4, generator=torch.Generator().manual_seed(rows * 7 + N))
    return pts, v, (hist if net == "fine" else None), G


def oracle_raw(W, net, pts, v, hist):
    cut = lambda pre: {k[len(pre):]: t for k, t in W.items() if k.startswith(pre)}
    if net == "coarse":
        return orc.query_coarse_static(cut("coarse."), pts, v)
    return orc.query_fine(cut("fine."), W["embedding_a.weight"], W["embedding_t.weight"], pts, v, hist.expand(pts.shape[0], hist.shape[1]))


def oracle_weight_grads(W, net, pts, v, hist, G, dtype):
    """{name: d sum(raw * G) / d parameter} of the queried network (and both tables for 'fine') by autograd through the oracle in `dtype`."""
    pre = ("coarse.",) if net == "coarse" else ("fine.", "embedding_")
    def run():
        P = {k: t.to(dtype).clone().requires_grad_(True) for k, t in W.items() if k.startswith(pre)}
        raw = oracle_raw(P, net, pts.to(dtype), v.to(dtype), hist)
        (raw * G.to(dtype)).sum().backward()
        return {k: (torch.zeros_like(p) if p.grad is None else p.grad).double() for k, p in P.items()}
    if dtype == torch.float64:
        with float64_default():
            return run()
    return run()


_ref_cache = {}


def reference(W, case):
    """(inputs, float64 gradients, yardstick per tensor) of a case; computed once and shared."""
    if case not in _ref_cache:
        net, rows, N, ph = case
        pts, v, hist, G = inputs_of(net, rows, N, ph)
        g64 = oracle_weight_grads(W, net, pts, v, hist, G, torch.float64)
        g32 = oracle_weight_grads(W, net, pts, v, hist, G, torch.float32)
        _ref_cache[case] = ((pts, v, hist, G), g64, {k: rel_l2(g32[k], g64[k]) for k in g64})
    return _ref_cache[case]


def hip_grads(tr, net, pts, v, hist, G, split=False, grads=None):
    """{name: gradient} of one query through NerfHTrainer.points_forward / points_backward."""
    tr.fused_split = split
    try:
        raw, saved = tr.points_forward(net, dev(pts), dev(v), None if hist is None else dev(hist))
        got = tr.points_backward(saved, dev(G), grads=grads)
    finally:
        tr.fused_split = False
    return raw, dict(zip((tr.names[i] for i in tr.net_slots(net)), got))


def disjoint_hist(rows):
    return (torch.arange(rows * 10).reshape(rows, 10) + 3).float()


# ---------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_vs_oracle(world, case):
    """raw of train=True against the fp32 oracle under the bounds of the split-f16 point queries (the same arithmetic: TOL_FINE for the
    fine network's five channel groups and the coarse rgb, TOL_COARSE for the coarse sigma).  Under no_grad: the plain forward."""
    q, tr, W = world
    net, rows, N, ph = case
    pts, v, hist, _ = inputs_of(net, rows, N, ph)
    with torch.no_grad():
        ref = oracle_raw(W, net, pts, v, hist)
        if net == "fine":
            got = q(dev(pts), dev(v), dev(hist), q.modules[1], 'fine', q.modules[2], q.modules[3], True, False, train=True)
        else:
            got = q(dev(pts), dev(v), None, q.modules[0], 'coarse', None, None, False, False, train=True)
    assert got.shape == ref.shape and not got.requires_grad
    if net == "fine":
        errs = [relmax(got[..., ch], ref[..., ch]) for ch in GROUPS]
        print(f"train query fine {rows}x{N}: rgb {errs[0]:.2e} sigma {errs[1]:.2e} t_rgb {errs[2]:.2e} t_sigma {errs[3]:.2e} beta {errs[4]:.2e}")
        assert max(errs) < TOL_FINE["f16x3"], errs
    else:
        e_rgb, e_sig = relmax(got[..., :3], ref[..., :3]), relmax(got[..., 3], ref[..., 3])
        print(f"train query coarse {rows}x{N}: rgb {e_rgb:.2e} sigma {e_sig:.2e}")
        assert e_rgb < TOL_FINE["f16x3"] and e_sig < TOL_COARSE["f16x3"]
    assert q.engine.range_flags() == 0


@pytest.mark.parametrize("net,split", [("coarse", False), ("fine", False), ("fine", True)])
def test_forward_writes_raw_and_nothing_else(world, net, split):
    """The C entry writes exactly n_rows * N * (9 | 4) floats: a sentinel band on both sides of raw is bit-unchanged, and raw has the
    bits of NerfHTrainer.points_forward."""
    q, tr, _ = world
    rows, N, C, pad = 3, 37, 9 if net == "fine" else 4, 64
    pts, v, hist, _ = inputs_of(net, rows, N, True)
    P, V, Hs = dev(pts), dev(v), None if hist is None else dev(hist)
    tr.fused_split = split
    try:
        want, _ = tr.points_forward(net, P, V, Hs)
        nid = _lib.DFN_NET_FINE if net == "fine" else _lib.DFN_NET_COARSE
        buf = torch.full((rows * N * C + 2 * pad,), -7.25, device=DEV)
        ws = torch.empty(tr.lib.dfn_nerfh_points_train_workspace_bytes(tr.engine.handle, nid, rows, N), dtype=torch.uint8, device=DEV)
        rc = tr.lib.dfn_nerfh_points_train_forward(tr.engine.handle, nid, tr._ptr_array(tr.params), ptr(P), ptr(V), ptr(Hs),
                                                   0 if Hs is None else Hs.shape[0], rows, N, ctypes.c_void_p(buf.data_ptr() + 4 * pad),
                                                   ctypes.c_void_p(ws.data_ptr()), ws.numel(), current_stream())
    finally:
        tr.fused_split = False
    assert rc == 0, tr.lib.dfn_last_error()
    assert bool((buf[:pad] == -7.25).all()) and bool((buf[-pad:] == -7.25).all())
    assert torch.equal(buf[pad:-pad].reshape(rows, N, C), want)


# ---------------------------------------------------------------------------------------------- 2. weight gradients against float64
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_weight_gradients_vs_float64(world, case):
    """L = sum(raw * G): every parameter tensor of the queried network (and both embedding tables for the fine one) by relative L2 against
    float64 autograd through the oracle; yardstick = the oracle's float32 autograd against float64.  No tensor is excused.
    Two planes (coarse; fine with fused_split): 3 * yard + 5e-4.  One plane (fine, default): ONE_PLANE_BOUND, and one- against
    two-plane gradients of the same call within it; a one-plane error above ten times the two-plane error of the same tensor is printed
    as a finding.
    Measured on an MI355X (worst tensor per case, relative L2 from float64):
      coarse (two planes)       9.5e-7 ... 1.07e-6   yardstick 3.4e-7 ... 5.8e-7   bound 3 * yard + 5e-4
      fine, fused_split (two)   9.5e-7 ... 2.99e-6    yardstick 4.3e-7 ... 8.6e-7   bound 3 * yard + 5e-4
      fine, default (one)       3.7e-4 (1 point), 1.15e-3 / 1.34e-3 (111), 1.80e-3 / 1.05e-3 (320), 9.0e-4 / 7.7e-4 (600 points; hist_rows
                                1 / n_rows); one against two planes: the same figures -> ONE_PLANE_BOUND = 2 x 1.80e-3.
    FINDING (reported, not absorbed): in the one-plane mode EVERY fine tensor sits two to four orders of magnitude further from float64
    than in the two-plane mode on the same call (worst: the single-row heads transient_sigma.0, transient_beta.0, static_sigma.0 at
    0.9 ... 1.8e-3; hidden layers 1 ... 5e-4).  That is the rounding of the stored operands to one f16 (2^-11 = 4.9e-4 per element), which a sum over a
    few hundred points does not average away as the step's 3e5 points do: at these point counts the one-plane query is f16-grade, and
    a caller who needs fp32-grade gradients from small queries sets trainer.fused_split = True."""
    q, tr, W = world
    net, rows, N, ph = case
    (pts, v, hist, G), g64, yard = reference(W, case)
    _, two = hip_grads(tr, net, pts, v, hist, G, split=True)
    assert set(two) == set(g64)
    worst = {"yard": 0., "two": 0., "one": 0., "one_vs_two": 0.}
    fails = []
    for k in g64:
        e2 = rel_l2(two[k], g64[k])
        worst["yard"], worst["two"] = max(worst["yard"], yard[k]), max(worst["two"], e2)
        print(f"  {net} {rows}x{N} {k}: yard {yard[k]:.2e} two-plane {e2:.2e}")
        if not e2 <= two_plane_bound(yard[k]):
            fails.append((k, "two", e2, yard[k]))
    if net == "fine":
        _, one = hip_grads(tr, net, pts, v, hist, G, split=False)
        for k in g64:
            e1, e2, d = rel_l2(one[k], g64[k]), rel_l2(two[k], g64[k]), rel_l2(one[k], two[k])
            worst["one"], worst["one_vs_two"] = max(worst["one"], e1), max(worst["one_vs_two"], d)
            print(f"  fine {rows}x{N} {k}: one-plane {e1:.2e} (two-plane {e2:.2e}, one vs two {d:.2e})"
                  + ("   FINDING: one-plane error above 10 x two-plane" if e1 > 10 * max(e2, 1e-7) else ""))
            if not (e1 <= ONE_PLANE_BOUND and d <= ONE_PLANE_BOUND):
                fails.append((k, "one", e1, d))
    print(f"points training query {net} {rows}x{N} hist_rows {'n_rows' if ph else 1}: worst over tensors", {k: f"{x:.2e}" for k, x in worst.items()})
    assert not fails, fails
    assert q.engine.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 3. structure
@pytest.mark.parametrize("net", ["coarse", "fine"])
def test_other_network_untouched_and_runs_bit_identical(world, net):
    """Gradient tensors of the OTHER network, pre-filled with a sentinel, are bit-unchanged (the guard included); two runs give the same
    bits (fixed-order reductions; per-row histograms with disjoint indices: no two rows add into one table entry)."""
    q, tr, _ = world
    rows, N = 5, 64
    pts, v, _, G = inputs_of(net, rows, N, True)
    hist = disjoint_hist(rows) if net == "fine" else None
    mine = set(tr.net_slots(net))
    grads = [torch.full_like(p, 3.5) for p in tr.params]
    _, a = hip_grads(tr, net, pts, v, hist, G, grads=grads)
    a = {k: t.clone() for k, t in a.items()}
    for i, g in enumerate(grads):
        if i not in mine:
            assert bool((g == 3.5).all()), tr.names[i]
        else:
            assert not bool((g == 3.5).all()), tr.names[i]      # overwritten, not accumulated into
    _, b = hip_grads(tr, net, pts, v, hist, G)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_zero_gradient_row_leaves_its_embedding_rows_zero(world):
    """G = 0 on one row: with per-row histograms on disjoint indices, the table rows that row alone indexes receive exact zeros, the
    others do not."""
    q, tr, _ = world
    rows, N = 5, 64
    pts, v, _, G = inputs_of("fine", rows, N, True)
    hist = disjoint_hist(rows)
    G = G.clone()
    G[2] = 0.
    _, g = hip_grads(tr, "fine", pts, v, hist, G)
    for k in ("embedding_a.weight", "embedding_t.weight"):
        t = g[k].cpu()
        assert float(t[hist[2].long()].abs().max()) == 0., k
        for r in (0, 1, 3, 4):
            assert float(t[hist[r].long()].abs().min()) > 0., (k, r)
        rest = torch.ones(t.shape[0], dtype=torch.bool)
        rest[hist.long().reshape(-1)] = False
        assert float(t[rest].abs().max()) == 0., k


@pytest.mark.parametrize("net,split", [("coarse", False), ("fine", False), ("fine", True)])
def test_gradients_scale_exactly_with_a_power_of_two(world, net, split):
    """G x 2^k gives every gradient x 2^k exactly: the seed, the wave scales and the stored halves move by powers of two only."""
    q, tr, _ = world
    rows, N = 3, 37
    pts, v, _, G = inputs_of(net, rows, N, True)
    hist = disjoint_hist(rows) if net == "fine" else None
    _, base = hip_grads(tr, net, pts, v, hist, G, split=split)
    base = {k: t.clone() for k, t in base.items()}
    for k2 in (3, -2):
        _, scaled = hip_grads(tr, net, pts, v, hist, G * 2. ** k2, split=split)
        for k in base:
            assert torch.equal(scaled[k], base[k] * 2. ** k2), (k, k2)


@pytest.mark.parametrize("net", ["coarse", "fine"])
def test_input_gradients_are_those_of_the_tracked_query(world, net):
    """d L / d inputs and d L / d viewdirs under train=True have the bits of the existing tracked query on the same weights (the same
    kernels); the weights receive their gradients in the same backward."""
    q, tr, _ = world
    rows, N = 3, 37
    pts, v, hist, G = inputs_of(net, rows, N, True)
    Gd = dev(G)
    def run(train):
        x, w = dev(pts).requires_grad_(True), dev(v).requires_grad_(True)
        if net == "fine":
            raw = q(x, w, dev(hist), None, 'fine', None, None, True, False, **({"train": True} if train else {}))
        else:
            raw = q(x, w, None, None, 'coarse', None, None, False, False, **({"train": True} if train else {"static": True}))
        assert raw.requires_grad
        for p in tr.params:
            p.grad = None
        (raw * Gd).sum().backward()
        return raw.detach(), x.grad, w.grad
    raw_t, gx_t, gw_t = run(True)
    mine = set(tr.net_slots(net))
    for i, p in enumerate(tr.params):
        assert (p.grad is not None) == (i in mine), tr.names[i]
    raw_p, gx_p, gw_p = run(False)
    assert all(p.grad is None for p in tr.params)       # the plain tracked query: the weights receive nothing
    assert torch.equal(gx_t, gx_p) and torch.equal(gw_t, gw_p)
    for p in tr.params:
        p.grad = None


# ---------------------------------------------------------------------------------------------- 4. several live nodes
def test_coarse_and_fine_queries_in_one_graph(world):
    """A coarse and a fine query live in one graph, one backward(): each network's .grad is what its query gives alone."""
    q, tr, _ = world
    pc, vc, _, Gc = inputs_of("coarse", 3, 37, False)
    pf, vf, hf, Gf = inputs_of("fine", 5, 64, True)
    _, alone_c = hip_grads(tr, "coarse", pc, vc, None, Gc)
    _, alone_f = hip_grads(tr, "fine", pf, vf, hf, Gf)
    alone = {**{k: t.clone() for k, t in alone_c.items()}, **{k: t.clone() for k, t in alone_f.items()}}
    for p in tr.params:
        p.grad = None
    raw_c = q(dev(pc), dev(vc), None, None, 'coarse', None, None, False, False, train=True)
    raw_f = q(dev(pf), dev(vf), dev(hf), None, 'fine', None, None, True, False, train=True)
    ((raw_c * dev(Gc)).sum() + (raw_f * dev(Gf)).sum()).backward()
    for k, p in zip(tr.names, tr.params):
        assert p.grad is not None and rel_l2(p.grad, alone[k]) <= 1e-6, k
        p.grad = None


def test_two_fine_queries_add_and_a_second_backward_doubles(world):
    """Two fine queries on different points: .grad is the sum of the single-query gradients (1e-6 relative); retain_graph=True and a
    second backward doubles it (X and the masks of each node survive, G is rewritten)."""
    q, tr, _ = world
    p1, v1, h1, G1 = inputs_of("fine", 3, 37, True)
    p2, v2, h2, G2 = inputs_of("fine", 2, 300, False)
    _, a1 = hip_grads(tr, "fine", p1, v1, h1, G1)
    a1 = {k: t.clone() for k, t in a1.items()}
    _, a2 = hip_grads(tr, "fine", p2, v2, h2, G2)
    names = [tr.names[i] for i in tr.net_slots("fine")]
    for p in tr.params:
        p.grad = None
    r1 = q(dev(p1), dev(v1), dev(h1), typ='fine', test_time=False, train=True)
    r2 = q(dev(p2), dev(v2), dev(h2), typ='fine', test_time=False, train=True)
    loss = (r1 * dev(G1)).sum() + (r2 * dev(G2)).sum()
    loss.backward(retain_graph=True)
    params = dict(zip(tr.names, tr.params))
    once = {}
    for k in names:
        assert rel_l2(params[k].grad, a1[k] + a2[k]) <= 1e-6, k
        once[k] = params[k].grad.clone()
    loss.backward()
    for k in names:
        assert rel_l2(params[k].grad, 2 * once[k]) <= 1e-6, k
    for p in tr.params:
        p.grad = None


# ---------------------------------------------------------------------------------------------- 5. the composed training chain
def composed_loss(q, o, d, view, hist, target, Nc, Ni, near, far):
    """The reference's training chain on public stages: query -> raw2outputs_NeRFW -> sample_pdf -> query -> raw2outputs_NeRFW -> NerfWLoss."""
    coarse, fine, emb_a, emb_t = q.modules
    t = torch.linspace(0., 1., Nc, device=o.device)
    z = (near * (1 - t) + far * t).expand(o.shape[0], Nc).contiguous()
    raw_c = q(o[:, None] + d[:, None] * z[..., None], view, None, coarse, 'coarse', None, None, False, False, train=True)
    rgb0, _, _, weights, _, _, _ = rendering.raw2outputs_NeRFW(raw_c, z, d, 0., False, test_time=False, typ="coarse")
    z_samples = rendering.sample_pdf(.5 * (z[:, 1:] + z[:, :-1]), weights[..., 1:-1], Ni, det=True)
    z_fine, _ = torch.sort(torch.cat([z, z_samples], -1), -1)
    raw = q(o[:, None] + d[:, None] * z_fine[..., None], view, hist, fine, 'fine', emb_a, emb_t, True, False, train=True)
    rgb, _, _, _, _, ts, beta = rendering.raw2outputs_NeRFW(raw, z_fine, d, 0., True, test_time=False, typ="fine")
    return (0.5 * ((rgb0 - target) ** 2).mean() + ((rgb - target) ** 2 / (2 * beta.unsqueeze(1) ** 2)).mean() + 3 + torch.log(beta).mean()
            + 0.01 * ts.mean())


@pytest.mark.parametrize("split", [True, False], ids=["two-plane", "one-plane"])
def test_composed_training_chain_vs_oracle_train_step(split):
    """24 rays, Nc = Ni = 8, perturb 0, raw_noise_std 0: all 64 gradients of the composed chain against oracle.train_step in float64, at
    3 * yard + 5e-4 (yard: the oracle's float32 step against float64); for one-plane fine storage the fine network's tensors and the two
    tables at ONE_PLANE_BOUND.  One Adam step (dfnet_amd.optim.Adam) then lowers the loss on the same rays.
    Measured on an MI355X: the worst tensors are the two first layers, where float32 itself leaves float64 and the HIP gradient sits
    where torch's float32 autograd sits (coarse.xyz_encoding_1.0 weight / bias yard 1.04e-2 / 1.10e-2, HIP 1.04e-2 / 1.10e-2;
    fine.xyz_encoding_1.0 6.9e-4 / 3.2e-4, HIP the same two-plane, 7.1e-4 / 3.2e-4 one-plane); then coarse.static_sigma.0 1.4e-4 (yard
    5e-5); every other tensor two-plane <= 9e-6, the one-plane fine tensors 1.2e-5 ... 9.1e-5.  Loss 2.451171 -> 2.449029 after the
    Adam step (lr 1e-4)."""
    q = build()
    tr, W = q.trainer, cpu_weights(q)
    tr.fused_split = split
    R, Nc, Ni, near, far = 24, 8, 8, 0., 2.5
    g = torch.Generator().manual_seed(77)
    o = torch.rand(R, 3, generator=g) - .5
    d = torch.randn(R, 3, generator=g) * .7
    view = d / d.norm(dim=-1, keepdim=True)
    hist = T(syn.HIST_IDX)[None].float().repeat(R, 1).contiguous()
    target = torch.rand(R, 3, generator=g)
    rows = torch.cat([o, d, torch.full((R, 1), near), torch.full((R, 1), far), view, hist], 1)
    cut = lambda pre: {k[len(pre):]: t for k, t in W.items() if k.startswith(pre)}
    c, f, ea, et = cut("coarse."), cut("fine."), W["embedding_a.weight"], W["embedding_t.weight"]
    _, _, g32, _ = orc.train_step(rows, target, c, f, ea, et, Nc, Ni, None, None, None, perturb=0., raw_noise_std=0.)
    with float64_default():
        _, _, g64, _ = orc.train_step(to64(rows), to64(target), to64(c), to64(f), to64(ea), to64(et), Nc, Ni, None, None, None, perturb=0.,
                                      raw_noise_std=0.)
    args = (q, dev(o), dev(d), dev(view), dev(hist), dev(target), Nc, Ni, near, far)
    opt = optim.Adam(params=tr.params, lr=1e-4, betas=(0.9, 0.999))
    opt.zero_grad(set_to_none=True)
    loss0 = composed_loss(*args)
    loss0.backward()
    assert len(tr.params) == 64 and all(p.grad is not None for p in tr.params)
    fails, worst = [], {"yard": 0., "err": 0.}
    for k, p in zip(tr.names, tr.params):
        ref = g64.get(k, torch.zeros_like(p, dtype=torch.float64, device="cpu"))
        yard = rel_l2(g32[k], ref) if k in g32 else 0.
        e = rel_l2(p.grad, ref) if float(ref.norm()) > 0 else float(p.grad.abs().max())
        one = not split and not k.startswith("coarse.")
        bound = ONE_PLANE_BOUND if one else two_plane_bound(yard)
        worst["yard"], worst["err"] = max(worst["yard"], yard), max(worst["err"], e)
        print(f"  composed chain {k}: yard {yard:.2e} err {e:.2e} bound {bound:.2e}")
        if not e <= bound:
            fails.append((k, e, yard, bound))
    print(f"composed training chain ({'two' if split else 'one'}-plane fine storage): worst over the 64 tensors", {k: f"{x:.2e}" for k, x in worst.items()})
    assert not fails, fails
    opt.step()
    with torch.no_grad():
        loss1 = composed_loss(*args)
    loss0 = loss0.detach()
    print(f"composed training chain: loss {float(loss0):.6f} -> {float(loss1):.6f} after one Adam step")
    assert float(loss1) < float(loss0)
    assert q.engine.range_flags() == 0


# ---------------------------------------------------------------------------------------------- 6. range guard
def test_query_is_zeroed_when_weights_outgrow_the_committed_scale():
    """One fine weight tensor x 1000 in place AFTER the commit: the packed operands saturate, the query's range word is raised, every
    gradient of the fine network and of both tables is exactly zero, the handle's range flag is raised, and the coarse network's
    sentinel-filled tensors are untouched."""
    q = build()
    tr = q.trainer
    pts, v, hist, G = inputs_of("fine", 3, 37, True)
    with torch.no_grad():
        w = dict(zip(tr.names, tr.params))["fine.xyz_encoding_3.0.weight"]
        w[:4, :4] *= 1000.
    grads = [torch.full_like(p, 3.5) for p in tr.params]
    _, got = hip_grads(tr, "fine", pts, v, hist, G, grads=grads)
    torch.cuda.synchronize()
    mine = set(tr.net_slots("fine"))
    for i, gr in enumerate(grads):
        if i in mine:
            assert float(gr.abs().max()) == 0., tr.names[i]
        else:
            assert bool((gr == 3.5).all()), tr.names[i]
    assert tr.engine.range_flags() != 0
    assert tr.engine.range_flags() == 0      # read and cleared


# ---------------------------------------------------------------------------------------------- 7. refusals and status codes
def test_refusals(world):
    q, tr, _ = world
    pts, v, hist, _ = inputs_of("fine", 2, 3, False)
    P, V, Hs = dev(pts), dev(v), dev(hist)
    with pytest.raises(NotImplementedError, match="sigma-only"):
        q(P, V, Hs, None, 'coarse', None, None, False, True, train=True)
    with pytest.raises(ValueError, match="output_transient"):
        q(P, V, Hs, None, 'coarse', None, None, True, False, train=True)
    bare = nerfw.HipQuery(q.engine, modules=q.modules)
    with pytest.raises(NotImplementedError, match="trainer"):
        bare(P, V, Hs, None, 'fine', None, None, True, False, train=True)
    q256 = build(width=256)
    with pytest.raises(NotImplementedError, match="netwidth 256"):
        q256(P, V, Hs, None, 'fine', None, None, True, False, train=True)
    # the C entries
    lib, h = tr.lib, tr.engine.handle
    F = _lib.DFN_NET_FINE
    raw, G = torch.empty(2, 3, 9, device=DEV), torch.zeros(2, 3, 9, device=DEV)
    nb = lib.dfn_nerfh_points_train_workspace_bytes(h, F, 2, 3)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    wp = ctypes.c_void_p(ws.data_ptr())
    grads = [torch.empty_like(p) for p in tr.params]
    fwd = lambda hh, net, n_rows, nbytes, params=None: lib.dfn_nerfh_points_train_forward(
        hh, net, tr._ptr_array(tr.params) if params is None else params, ptr(P), ptr(V), ptr(Hs), 1, n_rows, 3, ptr(raw), wp, nbytes, current_stream())
    bwd = lambda hh, net, params=None: lib.dfn_nerfh_points_train_backward(
        hh, net, tr._ptr_array(tr.params) if params is None else params, ptr(Hs), 1, 2, 3, ptr(raw), ptr(G), tr._ptr_array(grads), wp, nb,
        current_stream())
    tr._points_mode(False)
    assert fwd(h, 7, 2, nb) == -1 and b"unknown net" in lib.dfn_last_error()
    assert fwd(h, F, 2, nb - 256) == -1 and b"workspace too small" in lib.dfn_last_error()
    assert fwd(h, F, 0, 0) == 0
    assert lib.dfn_nerfh_points_train_forward(h, F, tr._ptr_array(tr.params), ptr(P), ptr(V), ptr(Hs), 1, 2, 0, ptr(raw), wp, nb, current_stream()) == -1
    assert lib.dfn_nerfh_points_train_forward(h, F, tr._ptr_array(tr.params), ptr(P), ptr(V), ptr(Hs), 1, 1 << 30, 4, ptr(raw), wp, nb, current_stream()) == -1
    assert lib.dfn_nerfh_points_train_forward(h, F, tr._ptr_array(tr.params), None, ptr(V), ptr(Hs), 1, 2, 3, ptr(raw), wp, nb, current_stream()) == -1
    assert lib.dfn_nerfh_set_train_mode(h, 1) == 0                    # DFN_TRAIN_EXACT: no layer-by-layer points path
    assert fwd(h, F, 2, nb) == -4 and b"DFN_TRAIN_EXACT" in lib.dfn_last_error()
    assert bwd(h, F) == -4
    assert lib.dfn_nerfh_set_train_mode(h, 0) == 0
    h256, tr256 = q256.engine.handle, q256.trainer
    assert fwd(h256, F, 2, nb, tr256._ptr_array(tr256.params)) == -4 and b"netwidth 128" in lib.dfn_last_error()
    assert lib.dfn_nerfh_points_train_workspace_bytes(h256, F, 2, 3) == 0
    fresh = build()                                                   # committed, no forward of any training kind yet
    ft = fresh.trainer
    assert bwd(ft.engine.handle, F, ft._ptr_array(ft.params)) == -3 and b"no forward pass" in lib.dfn_last_error()
    assert fwd(h, F, 2, nb) == 0 and bwd(h, F) == 0                   # and the same arguments pass
    assert tr.engine.range_flags() == 0


def test_calls_without_the_keyword_are_what_they_were(world):
    """Without train= every path returns what it returned: a tracked fine query and a static=True query, with the keyword absent and
    with it at its default, bit for bit -- forward values, input gradients, and no gradient on any weight."""
    q, tr, _ = world
    pts, v, hist, G = inputs_of("fine", 3, 37, True)
    def run(typ, **kw):
        x, w = dev(pts).requires_grad_(True), dev(v).requires_grad_(True)
        for p in tr.params:
            p.grad = None
        if typ == "fine":
            raw = q(x, w, dev(hist), None, 'fine', None, None, True, True, **kw)
        else:
            raw = q(x, w, None, None, 'coarse', None, None, False, False, static=True, **kw)
        (raw * dev(G)[..., :raw.shape[-1]]).sum().backward()
        assert all(p.grad is None for p in tr.params)
        return raw.detach(), x.grad, w.grad
    for typ in ("fine", "coarse"):
        a, b = run(typ), run(typ, train=False)
        assert all(torch.equal(s, t) for s, t in zip(a, b)), typ
    E = q.engine
    assert torch.equal(run("fine")[0], E.mlp_fine_points(dev(pts), dev(v), dev(hist)))
    assert torch.equal(run("coarse")[0], E.mlp_coarse_static_points(dev(pts), dev(v)))
