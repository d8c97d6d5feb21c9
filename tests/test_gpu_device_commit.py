"""The device-side re-commit of a NeRF-H engine: dfn_nerfh_recommit_device (weight_max_kernel, fold_kernel, pack_kernel),
NerfHEngine.load_device / load_modules_device, and the two callers that take it (HipQuery.refresh, NerfHTrainer.recommit).

The contract is byte equality: after load_device(W1) every device buffer of the engine (dfn_nerfh_packed_buffer) holds the bytes, and
every packed network the in_scale, that load_numpy(W1) gives a fresh engine.  W0 is NeRFW's own seeding (the constructor reseeds to
0).  W1 comes in two flavours: (a) another seed; (b) W0 with fine.xyz_encoding_3.0.weight x 40 and every coarse weight x 1/64, so
that the fine scale exponent moves down and the coarse one up, lo halves fall into f16 subnormals and the folded matrices exceed the
largest weight.  Netwidth 128 (every kernel variant's blobs, the gradient and training-query blobs, the folds), 256 and the generic
width 64.  Everything downstream is compared bit for bit against the host-committed engine: there is no tolerance in this file.

DFN_DEVICE_RECOMMIT=0 in the environment runs the file with the switches of nerfw.py and nerf_train.py off (the host path)."""
import ctypes
import math
import os

import pytest
import torch

from dfnet_amd import _lib, engine as eng, nerf_train, nerfw, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
SWITCH = os.environ.get("DFN_DEVICE_RECOMMIT", "1") != "0"
PRECS = ("f16", "f32", "f16x3")
GRAD_PRECS = ("f32", "f16x3")   # plain f16 differentiates nothing (dfn_mlp_*_backward: DFN_ERR_UNSUPPORTED)


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    monkeypatch.setattr(nerfw, "DEVICE_RECOMMIT", SWITCH)
    monkeypatch.setattr(nerf_train, "DEVICE_RECOMMIT", SWITCH)


def make_modules(width=128):
    """(network_fn, network_fine, embedding_a, embedding_t) on the GPU from NeRFW's own seeding."""
    coarse = nerfw.NeRFW('coarse', D=8, W=width, skips=[4], in_channels_xyz=63, in_channels_dir=27)
    fine = nerfw.NeRFW('fine', D=8, W=width, skips=[4], in_channels_xyz=63, in_channels_dir=27, encode_appearance=True,
                       encode_transient=True, in_channels_a=50, in_channels_t=20)
    torch.manual_seed(0)
    emb_a, emb_t = torch.nn.Embedding(1000, 5), torch.nn.Embedding(1000, 2)
    return tuple(m.to(DEV) for m in (coarse, fine, emb_a, emb_t))


def names_of(E):
    return [E.lib.dfn_nerfh_train_param_name(i).decode() for i in range(E.lib.dfn_nerfh_train_param_count())]


def host_engine(width, named, precision="f16x3"):
    """A fresh engine committed on the host from {canonical name: tensor}."""
    cut = lambda pre: {k[len(pre):]: v.detach().cpu().numpy() for k, v in named.items() if k.startswith(pre)}
    return eng.NerfHEngine(width=width, precision=precision).load_numpy(
        cut("coarse."), cut("fine."), named["embedding_a.weight"].detach().cpu().numpy(), named["embedding_t.weight"].detach().cpu().numpy())


def w0_named(width):
    E = eng.NerfHEngine(width=width)
    return dict(zip(names_of(E), (t.clone() for t in E.module_tensors(*make_modules(width)))))


def w1_named(w0, flavour):
    """{canonical name: contiguous fp32 CUDA tensor} of W1."""
    if flavour == "a":
        g = torch.Generator().manual_seed(7)
        out = {}
        for k, t in w0.items():
            if k.startswith("embedding"):
                v = torch.randn(t.shape, generator=g)
            else:
                v = (torch.rand(t.shape, generator=g) * 2 - 1) / math.sqrt(t.shape[-1] if t.dim() > 1 else 64)
            out[k] = v.to(DEV).contiguous()
        return out
    out = {k: t.clone() for k, t in w0.items()}
    out["fine.xyz_encoding_3.0.weight"] *= 40.
    for k in out:
        if k.startswith("coarse.") and k.endswith(".weight"):
            out[k] *= 1. / 64.
    return out


class _DeviceBytes:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def buffers(E):
    """{name: (device pointer, bytes as a uint8 tensor, in_scale)} of every packed buffer of the engine."""
    torch.cuda.synchronize()
    out = {}
    for name, p, n, scale in E.packed_buffers():
        out[name] = (p, torch.as_tensor(_DeviceBytes(p, n), device=DEV).clone(), scale)
    return out


def assert_same_buffers(A, B):
    a, b = buffers(A), buffers(B)
    assert list(a) == list(b) and len(a) >= 1
    bad = []
    for k in a:
        assert a[k][1].numel() == b[k][1].numel(), k
        diff = int((a[k][1] != b[k][1]).sum())
        if diff or a[k][2] != b[k][2]:
            bad.append((k, diff, a[k][1].numel(), a[k][2], b[k][2]))
    assert not bad, f"(buffer, mismatching bytes, bytes, in_scale host, in_scale device): {bad}"
    return a, b


_pairs = {}


def pair(width, flavour):
    """(A, B, W1): A host-committed with W1; B host-committed with W0, then device-re-committed with W1.  Made once per case."""
    if (width, flavour) not in _pairs:
        w0 = w0_named(width)
        w1 = w1_named(w0, flavour)
        A = host_engine(width, w1)
        B = host_engine(width, w0)
        before = buffers(B)
        B.load_device([w1[k] for k in names_of(B)])
        assert B.device_commits == 1
        _pairs[(width, flavour)] = (A, B, w1, before)
    return _pairs[(width, flavour)]


# ---------------------------------------------------------------------------------------------- 3. byte equality
@pytest.mark.parametrize("flavour", ["a", "b"])
@pytest.mark.parametrize("width", [128, 256, 64])
def test_device_recommit_is_byte_equal_to_the_host_commit(width, flavour):
    A, B, _, before = pair(width, flavour)
    a, b = assert_same_buffers(A, B)
    assert [v[0] for v in b.values()] == [v[0] for v in before.values()], "a device re-commit must keep every pointer"
    print(f"netwidth {width} ({flavour}): {len(a)} buffers, {sum(v[1].numel() for v in a.values())} bytes equal")
    if width in (128, 256):
        assert any(int((before[k][1] != b[k][1]).sum()) for k in b), "the re-commit changed nothing: W1 == W0?"
        if flavour == "b":   # both scale exponents moved: fine down, coarse up
            for net, cmp in (("net.coarse.f16x3.v0.blob", float.__gt__), ("net.fine.f16x3.v0.blob", float.__lt__)):
                assert cmp(b[net][2], before[net][2]), (net, b[net][2], before[net][2])


# ---------------------------------------------------------------------------------------------- 4. function
def _frame():
    return T(syn.orbit_pose(1, 8)).to(DEV), T(syn.HIST_IDX).to(DEV)


def _points():
    g = torch.Generator().manual_seed(3037)
    pts = (torch.rand(3, 37, 3, generator=g) * 3 - 1.5).to(DEV)
    v = torch.randn(3, 3, generator=g)
    v = (v / v.norm(dim=-1, keepdim=True)).to(DEV)
    return pts, v, T(syn.HIST_IDX)[None].to(DEV), torch.randn(3, 37, 9, generator=g).to(DEV)


@pytest.mark.parametrize("prec", PRECS)
def test_everything_downstream_has_the_bits_of_the_host_commit(prec):
    A, B, _, _ = pair(128, "b")
    c2w, hist1 = _frame()
    pts, v, hist, G = _points()
    def outputs(E):
        out = list(E.render_image(c2w, 6, 8, 7.3, hist1, 8, 8, 0., 2.5, precision=prec))
        out.append(E.mlp_fine_points(pts, v, hist, precision=prec))
        out.append(E.mlp_coarse_points(pts, precision=prec))
        out.append(E.mlp_coarse_static_points(pts, v, precision=prec))
        if prec in GRAD_PRECS:
            out.append(E.mlp_fine_points_backward(pts, v, hist, G, precision=prec))
            out.append(E.mlp_coarse_points_backward(pts, G[..., 0].contiguous(), precision=prec))
            out.append(E.mlp_coarse_static_points_backward(pts, v, G[..., :4].contiguous(), precision=prec))
        torch.cuda.synchronize()
        return out
    want, got = outputs(A), outputs(B)
    assert len(want) == len(got) == (9 if prec in GRAD_PRECS else 6)
    for i, (a, b) in enumerate(zip(want, got)):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, i
        assert torch.equal(a, b), (prec, i, int((a != b).sum()), a.numel())


# ---------------------------------------------------------------------------------------------- 5. trainer
def _trainer():
    mods = make_modules()
    E = eng.NerfHEngine(precision="f32").load_modules(*mods)
    return E, nerf_train.NerfHTrainer(E, *mods)


def _step_inputs(R=24, Nc=8, Ni=8, seed=5):
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(R, 3, generator=g) - .5).to(DEV)
    d = torch.randn(R, 3, generator=g).to(DEV)
    target = torch.rand(R, 3, generator=g).to(DEV)
    draws = tuple(t.to(DEV) for t in (torch.rand(R, Nc, generator=g), torch.randn(R, Nc, generator=g), torch.rand(R, Ni, generator=g)))
    return o, d, T(syn.HIST_IDX)[None].to(DEV), target, Nc, Ni, draws


def test_trainer_recommit_on_the_device_gives_the_host_recommits_gradients(monkeypatch):
    o, d, hist, target, Nc, Ni, draws = _step_inputs()
    grads, commits = [], []
    for on in (True, False):
        monkeypatch.setattr(nerf_train, "DEVICE_RECOMMIT", on)
        E, tr = _trainer()
        tr.range_check = None   # the test drives the recovery itself
        step = lambda: tr.train_step(o, d, hist, target, Nc, Ni, 0., 2.5, perturb=1., raw_noise_std=0., draws=draws)
        step()
        assert E.range_flags() == 0
        with torch.no_grad():   # beyond the 64x headroom of the committed operand scale
            dict(zip(tr.names, tr.params))["fine.xyz_encoding_3.0.weight"][:4, :4] *= 1000.
        for p in tr.params:
            p.grad = None
        step()
        torch.cuda.synchronize()
        assert E.range_flags() != 0 and all(float(p.grad.abs().max()) == 0. for p in tr.params), "the range guard did not fire"
        tr.recommit()
        for p in tr.params:
            p.grad = None
        step()
        torch.cuda.synchronize()
        assert E.range_flags() == 0
        grads.append([p.grad.clone() for p in tr.params])
        commits.append(E.device_commits)
    assert commits == [1, 0]
    assert len(grads[0]) == 64 and any(float(g.abs().max()) > 0 for g in grads[0])
    bad = [k for k, a, b in zip(tr.names, *grads) if not torch.equal(a, b)]
    assert not bad, f"gradient tensors that differ after a device and a host re-commit: {bad}"


# ---------------------------------------------------------------------------------------------- 6. stream order
def test_load_device_is_ordered_behind_work_on_the_current_stream():
    mods = make_modules()
    E = eng.NerfHEngine(precision="f16x3").load_modules(*mods)
    tensors = E.module_tensors(*mods)
    c2w, hist1 = _frame()
    with torch.no_grad():
        mods[1].xyz_encoding_2[0].weight.mul_(1.5)     # enqueued, not waited for
    E.load_device(tensors)
    got = E.render_image(c2w, 6, 8, 7.3, hist1, 8, 8, 0., 2.5)
    A = host_engine(128, dict(zip(names_of(E), tensors)))
    want = A.render_image(c2w, 6, 8, 7.3, hist1, 8, 8, 0., 2.5)
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert_same_buffers(A, E)


# ---------------------------------------------------------------------------------------------- 7. HipQuery
def test_query_after_an_optimizer_step_repacks_once_on_the_device():
    mods = make_modules()
    E = eng.NerfHEngine(precision="f16x3").load_modules(*mods)
    q = nerfw.HipQuery(E, modules=mods)
    pts, v, hist, _ = _points()
    first = q(pts, v, hist)
    params = [p for m in mods for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=1e-2)
    g = torch.Generator().manual_seed(11)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    opt.step()
    c0 = E.device_commits
    got = q(pts, v, hist)
    assert E.device_commits == c0 + int(SWITCH)
    fresh = nerfw.HipQuery(eng.NerfHEngine(precision="f16x3").load_modules(*mods), modules=mods)
    want = fresh(pts, v, hist)
    assert torch.equal(got, want) and not torch.equal(got, first)
    again = q(pts, v, hist)
    assert E.device_commits == c0 + int(SWITCH) and torch.equal(again, got)


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    w0 = w0_named(128)
    E = eng.NerfHEngine()
    tensors = [w0[k] for k in names_of(E)]
    with pytest.raises(_lib.DfnError, match="never committed"):
        E.load_device(tensors)
    assert E.device_commits == 0
    E = host_engine(128, w0)
    holed = list(tensors)
    holed[3] = None
    with pytest.raises(_lib.DfnError, match="status -1"):
        E.load_device(holed)
    with pytest.raises(ValueError):
        E.load_device(tensors[:-1])
    with pytest.raises(ValueError):
        E.load_device([t.double() for t in tensors])
    E.load_device(tensors)
    assert E.lib.dfn_nerfh_commit(E.handle) == -3 and b"dfn_nerfh_recommit_device" in E.lib.dfn_last_error()
    A = host_engine(128, w0)
    cut = lambda pre: {k[len(pre):]: v.cpu().numpy() for k, v in w0.items() if k.startswith(pre)}
    E.load_numpy(cut("coarse."), cut("fine."), w0["embedding_a.weight"].cpu().numpy(), w0["embedding_t.weight"].cpu().numpy())
    assert_same_buffers(A, E)
