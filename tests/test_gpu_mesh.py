"""GPU tests of the mesh export end to end: extract_mesh on the trained fixture against the restatement applied to the density grid,
vertex colours against the CPU oracle, the PLY round trip, and `run_nerf.py --mesh_only` as a subprocess."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dfnet_amd import engine as eng, mesh, nerfw, synthetic as syn
from oracle import nerfh_oracle as orc
from tests import isosurface_cases as ic
from tests.test_gpu_points import TOL_FINE, relmax
from tests.test_host_logic import make_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
DEV = "cuda:0"


@pytest.fixture(scope="module")
def trained():
    """The trained fixture on 24 x 20 x 22 over [-0.7, 0.7]^3: (query, weights, sigma, threshold, extract_mesh's result with
    colours).  The threshold is the 0.9 quantile of the grid: crossings are guaranteed without anyone having measured the fixture's
    densities."""
    cw, fw, ea, et = syn.trained_nerfh_weights()
    q = nerfw.HipQuery(eng.NerfHEngine(precision="f16x3").load_numpy(cw, fw, ea, et))
    bounds, size = (-.7, -.7, -.7, .7, .7, .7), (24, 20, 22)
    sigma = mesh.density_grid(q, mesh.grid_axes(bounds, size, device=torch.device(DEV)))
    threshold = float(np.quantile(sigma.cpu().numpy().astype(np.float64), 0.9))
    out = mesh.extract_mesh({'network_query_fn': q}, bounds, size, threshold=threshold, colors=True, img_idx=T(syn.HIST_IDX))
    return q, (fw, ea, et), sigma, threshold, out


def test_extract_mesh_equals_the_restatement_on_the_density_grid(trained):
    q, _, sigma, threshold, out = trained
    assert torch.equal(out["sigma"], sigma)
    axes = [a.cpu().numpy() for a in out["axes"]]
    rv, rf, _, _ = ic.marching_tets(sigma.cpu().numpy(), axes, np.float32(threshold))
    v, f = out["verts"].cpu().numpy(), out["faces"].cpu().numpy()
    print(f"trained fixture: threshold {threshold:.4g}, V {v.shape[0]} F {f.shape[0]}; sigma min {out['sigma_min']:.4g} max "
          f"{out['sigma_max']:.4g} deciles {out['sigma_deciles']}")
    assert v.shape[0] > 0 and v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(ic.canonical_faces(f), ic.canonical_faces(rf))
    assert float(np.abs(v - rv).max()) <= 16 * 2.0 ** -24 * 0.7          # the bound of tests/test_gpu_isosurface.py, M = 0.7
    s = np.sort(sigma.cpu().numpy().reshape(-1))
    assert out["sigma_min"] == s[0] and out["sigma_max"] == s[-1] and len(out["sigma_deciles"]) == 9
    assert out["sigma_deciles"] == [float(s[round(k / 10 * (s.size - 1))]) for k in range(1, 10)]
    assert q.engine.range_flags() == 0


def test_vertex_colours_vs_oracle(trained):
    """Static rgb at the vertices against orc.query_fine, inside TOL_FINE of tests/test_gpu_points.py (3e-6, the same for every
    fp32-grade mode).  vertex_colors queries in exact fp32 whatever the engine's precision (this engine's is split-f16); measured on
    an MI355X on this fixture: 1.7e-6 (split-f16 gave 4.1e-6: 3 of 4 715 vertices above the bound); the oracle's own fp32 evaluation
    sits 1.9e-6 from its float64 one."""
    q, (fw, ea, et), _, _, out = trained
    verts = out["verts"].cpu()
    with torch.no_grad():
        ref = orc.query_fine({k: T(v) for k, v in fw.items()}, T(ea), T(et), verts[None], torch.tensor([[0., 0., -1.]]),
                             T(syn.HIST_IDX)[None])[0, :, :3]
    assert out["colors"].shape == ref.shape
    err = relmax(out["colors"], ref)
    print(f"vertex colours: {err:.2e} from the oracle (bound {TOL_FINE['f32']:.0e})")
    assert q.engine.precision == "f16x3"                     # the colour query names its precision: the engine's own is not touched
    assert err < TOL_FINE["f32"]


def test_ply_round_trip(trained, tmp_path):
    out = trained[4]
    path = str(tmp_path / "m.ply")
    mesh.save_ply(path, out["verts"], out["faces"], out["colors"])
    v, f, c = mesh.load_ply(path)
    assert np.array_equal(v, out["verts"].cpu().numpy()) and np.array_equal(f, out["faces"].cpu().numpy())
    assert np.array_equal(c, nerfw.to8b(out["colors"].cpu().numpy()))


def test_run_nerf_mesh_only_cli(tmp_path):
    """`run_nerf.py --mesh_only` on the synthetic tree (random-init weights, no checkpoint): the threshold is the median of an
    in-process grid with the CLI's bounds and size, so crossings are guaranteed; the file parses, V and F equal the in-process
    result, its colours are those of training frame 0's histogram, and neither a checkpoint nor a render directory is written."""
    from dfnet_amd import options
    from PIL import Image
    from dfnet_amd import datasets
    datadir = make_scene(str(tmp_path), n_train=2, n_val=1, H=48, W=64)
    # a dark training frame 0 and a bright frame 1: their histograms, hence the exported colours, differ
    frames = os.path.join(str(tmp_path), "data", "deepslam_data", "7Scenes", "heads", "seq-02")
    rng = np.random.default_rng(5)
    for i, (lo, hi) in enumerate(((0, 70), (180, 256))):
        Image.fromarray(rng.integers(lo, hi, (48, 64, 3)).astype(np.uint8)).save(os.path.join(frames, f"frame-{i:06d}.color.png"))
    basedir = str(tmp_path / "logs")
    bounds = ["-1", "-0.9", "-1.1", "1", "0.8", "0.9"]
    base = ["--config", os.path.join(ROOT, "script", "config_nerfh.txt"), "--datadir", datadir, "--basedir", basedir,
            "--testskip", "1", "--trainskip", "1", "--mesh_only", "--mesh_grid_size", "12", "--mesh_colors", "--mesh_bounds"] + bounds
    args = options.nerf_parser().parse_args(base)
    torch.manual_seed(0)
    _, kwargs_test, start, _, _ = nerfw.create_nerf(args)
    assert start == 0
    sigma = mesh.density_grid(kwargs_test['network_query_fn'], mesh.grid_axes(args.mesh_bounds, 12))
    threshold = float(sigma.median())
    want = mesh.extract_mesh(kwargs_test, args.mesh_bounds, 12, threshold=threshold)
    V, F = want["verts"].shape[0], want["faces"].shape[0]
    assert V > 0 and F > 0
    r = subprocess.run([sys.executable, os.path.join(ROOT, "script", "run_nerf.py")] + base + ["--mesh_threshold", repr(threshold)],
                       cwd=os.path.join(ROOT, "script"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert f"MESH V {V} F {F}" in r.stdout and "deciles" in r.stdout, r.stdout[-2000:]
    out = os.path.join(basedir, "nerfh")
    v, f, c = mesh.load_ply(os.path.join(out, "mesh_000000.ply"))
    assert v.shape == (V, 3) and f.shape == (F, 3) and c.shape == (V, 3)
    assert np.array_equal(v, want["verts"].cpu().numpy()) and np.array_equal(f, want["faces"].cpu().numpy())
    # --mesh_colors: the histogram of training frame 0, whatever order the (shuffling) training loader would yield
    train_set = datasets.load_7Scenes_dataloader_NeRF(args)[0].dataset
    hist0, hist1 = train_set[0][2], train_set[1][2]
    assert not torch.equal(hist0, hist1)
    q = kwargs_test['network_query_fn']
    assert np.array_equal(c, nerfw.to8b(mesh.vertex_colors(q, want["verts"], hist0).cpu().numpy()))
    assert not np.array_equal(c, nerfw.to8b(mesh.vertex_colors(q, want["verts"], hist1).cpu().numpy()))
    assert "[TRAIN]" not in r.stdout
    assert not [n for n in os.listdir(out) if n.endswith(".tar") or n.startswith("evaluate_") or n.startswith(("trainset_", "testset_"))]
