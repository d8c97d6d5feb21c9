"""The render maps through render_path: the device back-end (dfn_frame_post_maps) bit for bit against numpy in float32, render_path(ret_maps=...)
against render(c2w=..., ret_maps=True) per frame with its eight PNGs per frame, row bands against the full frame, and one rank under the
launcher with the collectives forced (RCCL)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR, FAR = 0.25, 2.5
MAPS = ("depth", "depth_static", "beta", "rgb_static", "rgb_transient")
PNG = {"depth": "_depth", "depth_static": "_depth_static", "beta": "_beta", "rgb_static": "_static", "rgb_transient": "_transient"}


def to8b(x):   # models/nerf.py:11
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def to16(d, near, far):   # the fixed-scale 16-bit depth, every operation in float32
    return (np.float32(65535) * np.clip((d - np.float32(near)) / (np.float32(far) - np.float32(near)), 0, 1)).astype(np.uint16)


def _plant(a, vals):
    flat = a.reshape(-1)
    k = min(flat.size, len(vals))
    flat[:k] = vals[:k]


def _inputs(n, H, W, single_gt):
    rng = np.random.default_rng(n * 1000 + H)
    near, far = np.float32(NEAR), np.float32(FAR)
    m = {}
    for k in ("depth", "depth_static"):
        m[k] = rng.uniform(NEAR - 0.3, FAR + 0.5, (n, H, W)).astype(np.float32)
        _plant(m[k], np.array([near, far, near + (far - near) / np.float32(65535), -0.0], np.float32))   # the ends of the scale, one step, -0
    m["beta"] = rng.uniform(0.1, 3, (n, H, W)).astype(np.float32)
    if n > 1:
        m["beta"][1].reshape(-1)[-1] = np.float32(3.5)       # frame 1's maximum at its last pixel
    for k in ("rgb_static", "rgb_transient"):
        m[k] = rng.uniform(-0.2, 1.2, (n, H, W, 3)).astype(np.float32)
        _plant(m[k], np.array([0.0, 1.0, 1.0 / 255, 254.999 / 255, -0.0, 0.5], np.float32))   # exact bin edges (tests/test_gpu_post.py)
    gt = rng.uniform(0, 1, (H, W, 3) if single_gt else (n, H, W, 3)).astype(np.float32)
    return m, gt


@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (5, 7, 9), (3, 12, 16), (2, 480, 640)])
@pytest.mark.parametrize("single_gt", [False, True])
def test_frame_post_maps_bit_exact_vs_numpy(n, H, W, single_gt):
    """Odd H W (frames 1.. start at addresses aligned to 4 / 2 / 1 bytes only), more than one block, more than one trip of the grid-stride
    loop (480 x 640: 150 blocks of 256 threads per frame, 8 pixels each).  Quantised planes and beta_max: np.array_equal.  mse_static: within
    1e-6 relative of the float64 mean (the bound tests/test_gpu_post.py holds mse to: the kernel sums fp32 differences in fp64)."""
    from dfnet_amd import engine as eng
    m, gt = _inputs(n, H, W, single_gt)
    dev = "cuda:0"
    dm = {k: torch.from_numpy(v).to(dev) for k, v in m.items()}
    dgt = torch.from_numpy(gt).to(dev)
    out = eng.frame_post_maps(dm, NEAR, FAR, gt=dgt)
    assert set(out) == {"depth16", "depth_static16", "beta8", "rgb_static8", "rgb_transient8", "beta_max", "mse_static"}
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("depth", "depth_static"):
        assert host[k + "16"].dtype == np.uint16 and np.array_equal(host[k + "16"], to16(m[k], NEAR, FAR)), k
    for k in ("rgb_static", "rgb_transient"):
        assert host[k + "8"].dtype == np.uint8 and np.array_equal(host[k + "8"], to8b(m[k])), k
    for i in range(n):
        assert np.array_equal(host["beta8"][i], to8b(m["beta"][i] / m["beta"][i].max())), i
        g = gt if single_gt else gt[i]
        ref = np.mean(np.square(m["rgb_static"][i].astype(np.float64) - g.astype(np.float64)))
        got = float(host["mse_static"][i])
        print(f"frame {i}: mse_static {got:.9e} float64 numpy {ref:.9e} rel {abs(got - ref) / ref:.2e}")
        assert abs(got - ref) <= 1e-6 * ref
    assert np.array_equal(host["beta_max"], m["beta"].reshape(n, -1).max(1))
    if n > 1:
        assert host["beta_max"][1] == np.float32(3.5)
    # subsets, as given maps and as `want` of the full set: only their keys, the bits of the full call
    keys = {("depth",): {"depth16"}, ("beta",): {"beta8", "beta_max"}, ("rgb_static", "depth_static"): {"rgb_static8", "depth_static16", "mse_static"}}
    for sub, want_keys in keys.items():
        for part in (eng.frame_post_maps({k: dm[k] for k in sub}, NEAR, FAR, gt=dgt), eng.frame_post_maps(dm, NEAR, FAR, gt=dgt, want=sub)):
            assert set(part) == want_keys, (sub, sorted(part))
            for k, v in part.items():
                assert np.array_equal(v.cpu().numpy(), host[k]), (sub, k)
    # no ground truth: no error
    plain = eng.frame_post_maps(dm, NEAR, FAR)
    assert "mse_static" not in plain and len(plain) == 6
    assert all(np.array_equal(v.cpu().numpy(), host[k]) for k, v in plain.items())


def _tiny_setup(N=19, H=12, W=16):
    """The setup of tests/test_gpu_post.py::test_render_path_writes_reference_pngs_per_frame."""
    from dfnet_amd import engine as eng, synthetic as syn
    from dfnet_amd.nerfw import HipQuery
    cw, fw, ea, et = syn.nerfh_weights(0)
    E = eng.NerfHEngine(precision="f16x3").load_numpy(cw, fw, ea, et)
    kw = dict(network_query_fn=HipQuery(E), perturb=False, N_importance=16, N_samples=8, use_viewdirs=True, white_bkgd=False,
              raw_noise_std=0., test_time=True, ndc=False, lindisp=False, near=0.0, far=2.5)
    poses = torch.stack([torch.from_numpy(syn.orbit_pose(k, N)) for k in range(N)])
    hist = torch.from_numpy(syn.HIST_IDX).repeat(N, 1)
    gt = np.random.default_rng(0).uniform(0, 1, (N, H, W, 3)).astype(np.float32)
    return kw, poses, hist, gt, [H, W, 21.9]


def test_render_path_with_maps(tmp_path, capsys):
    from PIL import Image
    from dfnet_amd import rendering
    N, H, W = 19, 12, 16   # more than one back-end batch
    kw, poses, hist, gt, hwf = _tiny_setup(N, H, W)
    with_maps, without, only_beta = tmp_path / "maps", tmp_path / "plain", tmp_path / "beta"
    for d in (with_maps, without, only_beta):
        d.mkdir()
    plain = rendering.render_path(None, poses, hwf, 32768, kw, gt_imgs=gt, savedir=str(without), img_ids=hist, ret_maps=False)
    assert isinstance(plain, tuple) and len(plain) == 2 and "maps" not in rendering.render_path.last_timing
    capsys.readouterr()
    rgbs, disps, maps = rendering.render_path(None, poses, hwf, 32768, kw, gt_imgs=gt, savedir=str(with_maps), img_ids=hist, ret_maps=True)
    printed = capsys.readouterr().out
    assert printed.index("Mean PSNR of this run is:") < printed.index("Mean static-only PSNR of this run is:")
    assert rendering.render_path.last_timing["maps"] == list(MAPS) and rendering.render_path.last_timing["gathered_bytes"] == 0
    # rgb, disp and the three PNGs of every frame are what they are without the keyword
    assert rgbs.dtype == np.float32 and np.array_equal(rgbs, plain[0]) and np.array_equal(disps, plain[1])
    assert sorted(os.listdir(without)) == sorted(f"{i:03d}{s}.png" for i in range(N) for s in ("", "_GT", "_disp"))
    for i in range(N):
        for s in ("", "_GT", "_disp"):
            assert (with_maps / f"{i:03d}{s}.png").read_bytes() == (without / f"{i:03d}{s}.png").read_bytes(), (i, s)
    assert sorted(os.listdir(with_maps)) == sorted(f"{i:03d}{s}.png" for i in range(N) for s in ("", "_GT", "_disp") + tuple(PNG.values()))
    assert tuple(maps) == MAPS
    for m in MAPS:
        assert maps[m].dtype == np.float32 and maps[m].shape == ((N, H, W, 3) if m.startswith("rgb_") else (N, H, W)), m
    for i in (0, 7, 16, 18):
        one = rendering.render(H, W, hwf[2], c2w=poses[i][:3, :4], img_idx=hist[i], ret_maps=True, **kw)
        assert np.array_equal(one[0].cpu().numpy(), rgbs[i]) and np.array_equal(one[1].cpu().numpy(), disps[i])
        for m in MAPS:
            assert np.array_equal(one[3][m].cpu().numpy(), maps[m][i]), (i, m)
        png = {m: np.asarray(Image.open(with_maps / f"{i:03d}{PNG[m]}.png")) for m in MAPS}
        for m in ("depth", "depth_static"):
            assert png[m].dtype == np.uint16 and np.array_equal(png[m], to16(maps[m][i], kw["near"], kw["far"])), (i, m)
        assert np.array_equal(png["beta"], to8b(maps["beta"][i] / np.max(maps["beta"][i]))), i
        for m in ("rgb_static", "rgb_transient"):
            assert png[m].dtype == np.uint8 and np.array_equal(png[m], to8b(maps[m][i])), (i, m)
    # a subset: one more PNG per frame, a one-key dict
    r2, d2, m2 = rendering.render_path(None, poses, hwf, 32768, kw, gt_imgs=gt, savedir=str(only_beta), img_ids=hist, ret_maps=("beta",))
    assert sorted(os.listdir(only_beta)) == sorted(f"{i:03d}{s}.png" for i in range(N) for s in ("", "_GT", "_disp", "_beta"))
    assert list(m2) == ["beta"] and np.array_equal(m2["beta"], maps["beta"]) and np.array_equal(r2, rgbs) and np.array_equal(d2, disps)
    assert (only_beta / "007_beta.png").read_bytes() == (with_maps / "007_beta.png").read_bytes()
    assert "static-only" not in capsys.readouterr().out
    with pytest.raises(ValueError, match="unknown render map"):
        rendering.render_path(None, poses, hwf, 32768, kw, img_ids=hist, ret_maps=("normals",))
    kw["network_query_fn"].engine.check_range()


def test_render_test_hands_render_maps_to_render_path(tmp_path):
    """--render_maps as render_test() sees it: the named maps' PNGs beside the three of both splits; "" writes the three alone."""
    from types import SimpleNamespace
    from dfnet_amd import rendering
    kw, poses, hist, gt, hwf = _tiny_setup(2)
    dl = [(torch.from_numpy(gt[i]).permute(2, 0, 1)[None], poses[i][:3, :4].reshape(1, 12), hist[i][None]) for i in range(2)]
    for value, more in (("beta,depth", ("_depth", "_beta")), ("", ())):
        args = SimpleNamespace(render_test=True, basedir=str(tmp_path), expname="maps" if value else "plain", chunk=32768, render_maps=value)
        rendering.render_test(args, dl, dl, hwf, 7, kw)
        for split in ("train", "val"):
            d = tmp_path / args.expname / f"evaluate_{split}_test_000007"
            assert sorted(os.listdir(d)) == sorted(f"{i:03d}{s}.png" for i in range(2) for s in ("", "_GT", "_disp") + more), (value, split)


def test_band_maps_equal_the_full_frame_bit_for_bit():
    """What each rank of a world-3 / world-8 group renders in row-band mode, simulated rank by rank as
    tests/test_gpu_dist.py::test_row_bands_equal_the_full_frame_bit_for_bit does: every band's maps are the same rows of the full frame's."""
    from dfnet_amd import dist as ddist, engine as eng, nerfw, rendering, synthetic as syn
    dev = torch.device("cuda:0")
    E = eng.NerfHEngine().load_numpy(*syn.nerfh_weights(0))
    kw = dict(network_query_fn=nerfw.HipQuery(E, 65536), perturb=False, N_importance=32, N_samples=16, use_viewdirs=True,
              white_bkgd=False, raw_noise_std=0., test_time=True, ndc=False, lindisp=False, near=0., far=2.5)
    H, W, focal = 22, 32, 29.0
    hist = torch.from_numpy(syn.HIST_IDX).float().to(dev)
    for world, n_frames in ((3, 1), (8, 3)):
        poses = torch.stack([torch.from_numpy(syn.orbit_pose(k, 8)) for k in range(n_frames)]).to(dev)
        full = [rendering.render(H, W, focal, c2w=poses[k][:3, :4], img_idx=hist, ret_maps=True, **kw) for k in range(n_frames)]
        for rank in range(world):
            f, r0, r1 = ddist.band_unit(n_frames, H, rank, world)
            out = rendering.render_band(H, W, focal, 32768, poses[f][:3, :4], hist, r0, r1, kw, ret_maps=True)
            assert len(out) == 3 and tuple(out[2]) == MAPS
            assert torch.equal(out[0], full[f][0][r0:r1]) and torch.equal(out[1], full[f][1][r0:r1]), (world, n_frames, rank)
            for m in MAPS:
                assert out[2][m].shape == (r1 - r0, W) + ((3,) if m.startswith("rgb_") else ())
                assert torch.equal(out[2][m], full[f][3][m][r0:r1]), (world, n_frames, rank, m)
        plain = rendering.render_band(H, W, focal, 32768, poses[0][:3, :4], hist, 0, 5, kw)
        assert len(plain) == 2 and torch.equal(plain[0], full[0][0][0:5])
        sub = rendering.render_band(H, W, focal, 32768, poses[0][:3, :4], hist, 0, 5, kw, ret_maps=("beta",))
        assert list(sub[2]) == ["beta"] and torch.equal(sub[2]["beta"], full[0][3]["beta"][0:5])
    E.check_range()


_CHILD = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from dfnet_amd import dist as ddist, rendering
from tests.test_gpu_post_maps import _tiny_setup
rank, world, local = ddist.init_from_env(backend="nccl")
assert torch.distributed.is_initialized() and torch.distributed.get_backend() == "nccl" and world == 1 and ddist.active()
kw, poses, hist, gt, hwf = _tiny_setup(3)
rgbs, disps, maps = rendering.render_path(None, poses, hwf, 32768, kw, gt_imgs=gt, savedir=sys.argv[3], img_ids=hist, ret_maps=True)
np.savez(sys.argv[2], rgbs=rgbs, disps=disps, **maps)
print("MAPS_RCCL_OK", sorted(rendering.render_path.last_timing["maps"]))
torch.distributed.destroy_process_group()
'''


def test_render_path_with_maps_under_the_launcher_with_rccl(tmp_path):
    """One rank under torch.distributed.run, nccl, collectives forced: the maps go through the path's gather (the padded RCCL gather of a
    one-rank group) and come back as the arrays this process computes without a process group."""
    from dfnet_amd import rendering
    from tests.test_gpu_dist import _launch
    kw, poses, hist, gt, hwf = _tiny_setup(3)
    (tmp_path / "here").mkdir()
    (tmp_path / "child").mkdir()
    rgbs, disps, maps = rendering.render_path(None, poses, hwf, 32768, kw, gt_imgs=gt, savedir=str(tmp_path / "here"), img_ids=hist, ret_maps=True)
    script = tmp_path / "c.py"
    script.write_text(_CHILD)
    r = _launch([str(script), ROOT, str(tmp_path / "child.npz"), str(tmp_path / "child")])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "MAPS_RCCL_OK" in r.stdout
    got = np.load(tmp_path / "child.npz")
    assert sorted(got.files) == sorted(("rgbs", "disps") + MAPS)
    assert np.array_equal(got["rgbs"], rgbs) and np.array_equal(got["disps"], disps)
    for m in MAPS:
        assert np.array_equal(got[m], maps[m]), m
    assert sorted(os.listdir(tmp_path / "child")) == sorted(os.listdir(tmp_path / "here"))
    for name in os.listdir(tmp_path / "here"):
        assert (tmp_path / "child" / name).read_bytes() == (tmp_path / "here" / name).read_bytes(), name
