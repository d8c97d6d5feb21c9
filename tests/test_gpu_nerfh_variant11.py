"""Kernel variant 11: one select per head value of the split-f16 16x16x32 coarse kernel and plain fused fine kernel.

Variant 11 is variant 10 (resident layers, claimed tiles, kept encoding, scaled seeds) whose two kernels are nerfh_mlp_sel.hip's: a
PrecX3M16 head block hands value c of the lane's sample over with one v_cndmask_b32 instead of a 16-way select chain (nerfh_layout.h:
kSelVariant; nerfh_mlp_core.h: layer()).  The same value reaches the same lane and goes through the same activation, so every output
must keep variant 10's bits.  The variant is latched per process (DFN_MLP_VARIANT), so each variant runs in a child with a time
limit, and no child is started after one fails:

  * variant 11 against variant 10 with torch.equal (zero elements may differ; finite, not all zero) on coarse sigma and the fused
    route's rgb / disp / acc, split-f16 at netwidth 128, dfn_nerfh_range_status 0 after each case:
      a  64 rays at 64 + 64: fewer tiles than workgroups;
      b  8 calls of 257 rays at 16 + 16: ragged last tiles whose points are clamped, several calls in one process;
      c  1 040 rays at 64 + 64: 260 coarse / 1 040 fine tiles on 256 workgroups, so workgroups take several tiles;
      d  case c a second time in the same process: the tile counters are re-armed;
      e  the rays of a 12 x 16 image from raygen at 64 + 128: origins and directions differ per ray, Nf = 192 as in the workload;
      h  case a with one histogram row per ray;
      t  case a's rays on weights whose fine static_sigma, transient_sigma, static_rgb and transient_rgb biases are moved so that the
         pre-activations of the samples lie on both sides of 20 (softplus_hw's pass-through) and of -80 (sigmoid_hw's clamp): the
         shifts are found on the CPU oracle (threshold minus the median pre-activation per head value), and the test asserts that
         both sides occur for each of the eight head values.  The weights are the synthetic ones at gain 2: at gain 1 the transient
         head values of all samples lie within 6e-5 of each other, which is the kernels' own error at 80 and separates nothing;
  * g  case a at precision f16 under DFN_MLP_VARIANT=11: the route falls back (nerfh_route.h: variant 11 outside split-f16 is variant
       4's plain kernels, as under variant 10) and gives variant 10's output there too;
  * under variant 11 a maps render (rgb / disp / acc and the five maps), a `raw` render (rgb / disp / acc / raw) and a fine point
    query (raw) on 64 rows give variant 10's bits: they resolve to the same kernels.

This file is also the child of its own tests: python tests/test_gpu_nerfh_variant11.py <out.pt>.
"""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dfnet_amd import synthetic as syn  # noqa: E402
from oracle import nerfh_oracle as orc  # noqa: E402

T = torch.from_numpy
TAGS = ("a", "b", "c", "d", "e", "g", "h", "t")
KEYS = ("sigma", "rgb", "disp", "acc")
# {tag: (calls, rays per call, Nc, Ni, precision, one histogram row per ray)}; e takes its rays from raygen, t runs on the moved heads
CASES = {"a": (1, 64, 64, 64, "f16x3", False), "b": (8, 257, 16, 16, "f16x3", False), "c": (1, 1040, 64, 64, "f16x3", False),
         "d": (1, 1040, 64, 64, "f16x3", False), "e": (1, 12 * 16, 64, 128, "f16x3", False), "g": (1, 64, 64, 64, "f16", False),
         "h": (1, 64, 64, 64, "f16x3", True), "t": (1, 64, 64, 64, "f16x3", False)}
OTHER = ("maps", "raw", "points")
MAPS = ("depth", "depth_static", "beta", "rgb_static", "rgb_transient")
# the eight activated head values of the fused fine kernel, each one the product of a select: (layer, row, the threshold at which its
# activation takes its other branch)
HEADS = tuple([("static_rgb.0", c, -80.) for c in range(3)] + [("static_sigma.0", 0, 20.)] +
              [("transient_rgb.0", c, -80.) for c in range(3)] + [("transient_sigma.0", 0, 20.)])
MARGIN = 1e-2   # a pre-activation counts as on one side when it is this far from the threshold: 600 x the 1.6e-5 that split-f16's 2e-7 is at 80


def rays(n, seed=3):
    """n rays of a 480 x 640 camera on the synthetic orbit, in a fixed random order"""
    ro, rd = orc.get_rays(480, 640, 585.0, T(syn.orbit_pose(2, 8))[:3, :4])
    sel = torch.randperm(480 * 640, generator=torch.Generator().manual_seed(seed))[:n]
    return ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous()


def ray_hists(n, seed=11):
    """one histogram row per ray: embedding indices drawn over the whole vocabulary, every ray its own"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1000, (n, len(syn.HIST_IDX)), generator=g).float()


def head_preactivations(fine, emb_a, emb_t, pts, viewdirs, hist_idx):
    """The oracle's fine network up to its heads (nerfh_oracle.nerfh_fine without the activations): [R, N, 8] in the order of HEADS"""
    R, N = pts.shape[:2]
    pe = orc.posenc(pts.reshape(-1, 3), 10)
    pd = orc.posenc(viewdirs[:, None].expand(pts.shape).reshape(-1, 3), 4)
    a = orc.hist_embed(emb_a, hist_idx).repeat_interleave(N, 0)
    t = orc.hist_embed(emb_t, hist_idx).repeat_interleave(N, 0)
    h = orc.nerfh_trunk(fine, pe)
    fin = orc._lin(fine, "xyz_encoding_final", h)
    dire = torch.relu(orc._lin(fine, "dir_encoding.0", torch.cat([fin, pd, a], -1)))
    tr = torch.cat([fin, t], -1)
    for j in (0, 2, 4, 6):
        tr = torch.relu(orc._lin(fine, f"transient_encoding.{j}", tr))
    pre = torch.cat([orc._lin(fine, "static_rgb.0", dire), orc._lin(fine, "static_sigma.0", h), orc._lin(fine, "transient_rgb.0", tr),
                     orc._lin(fine, "transient_sigma.0", tr)], -1)
    return pre.reshape(R, N, 8)


def moved_heads(o, d, Nc, Ni):
    """Seed-0 synthetic weights at gain 2 (the head values spread by 0.03 to 0.14) with the eight head biases moved onto their
    thresholds, on the CPU oracle: the fine samples of the rays come from the coarse network, which stays, so they are the samples
    of the unmoved weights; a head value's pre-activation is linear in its bias, so bias += threshold - median puts the samples'
    median on the threshold.  Returns the weights and, per head value, how many of the samples lie MARGIN below and above the
    threshold."""
    cw, fw, ea, et = syn.nerfh_weights(0, gain=2.0)
    fw = {k: v.copy() for k, v in fw.items()}
    tc, tf = {k: T(v) for k, v in cw.items()}, {k: T(v) for k, v in fw.items()}
    rows = orc.pack_ray_rows(o, d, 0., 2.5, syn.HIST_IDX)
    stages = {}
    with torch.no_grad():
        orc.render_rays(rows, tc, tf, T(ea), T(et), Nc, Ni, stages=stages)
        pts = o[:, None, :] + d[:, None, :] * stages["z_fine"][..., None]
        pre = head_preactivations(tf, T(ea), T(et), pts, rows[:, 8:11], rows[:, 11:])
    sides = []
    for i, (layer, row, thr) in enumerate(HEADS):
        shift = thr - float(pre[..., i].median())
        fw[layer + ".bias"][row] += np.float32(shift)
        moved = pre[..., i] + shift
        sides.append((int((moved < thr - MARGIN).sum()), int((moved > thr + MARGIN).sum())))
    return (cw, fw, ea, et), sides


def child(out_path):
    """Coarse sigma and the fused route's outputs of every case, then the maps / raw / point-query routes, in this process's variant;
    seed-0 synthetic weights, case t on the moved heads."""
    from dfnet_amd import engine as eng
    dev = "cuda:0"
    E0 = eng.NerfHEngine(precision="f16x3").load_numpy(*syn.nerfh_weights(0))
    shared = T(np.asarray(syn.HIST_IDX, dtype=np.float32)).to(dev)
    res = {}
    for tag, (calls, n, Nc, Ni, prec, per_ray) in CASES.items():
        E = E0
        if tag == "e":
            o, d, _ = eng.raygen(12, 16, 14.6, T(syn.orbit_pose(1, 8)).to(dev), want_viewdirs=False)
            o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        else:
            o, d = rays(calls * n)
            if tag == "t":
                weights, sides = moved_heads(o, d, Nc, Ni)
                E = eng.NerfHEngine(precision="f16x3").load_numpy(*weights)
            o, d = o.to(dev), d.to(dev)
        hists = ray_hists(calls * n).to(dev) if per_ray else None
        parts = {k: [] for k in KEYS}
        for c in range(calls):
            oc, dc = o[c * n:(c + 1) * n].contiguous(), d[c * n:(c + 1) * n].contiguous()
            hc = hists[c * n:(c + 1) * n].contiguous() if per_ray else shared
            parts["sigma"].append(E.mlp_coarse(oc, dc, Nc, 0., 2.5, precision=prec).cpu())
            f = E.render_rays(oc, dc, hc, Nc, Ni, 0., 2.5, precision=prec)
            assert f[3] is None
            for k, t in zip(("rgb", "disp", "acc"), f):
                parts[k].append(t.cpu())
        rec = {k: torch.cat(v) for k, v in parts.items()}
        rec["range_flags"] = E.range_flags()
        if tag == "t":
            rec["sides"] = sides
        res[tag] = rec
    # the routes that variant 11 leaves with variant 10's kernels: 64 rows at 64 + 64 in split-f16
    E = E0
    o, d = (t.to(dev) for t in rays(64))
    v = d / d.norm(dim=-1, keepdim=True)
    z = torch.linspace(0.1, 2.4, 64, device=dev)
    pts = (o[:, None, :] + d[:, None, :] * z[None, :, None]).contiguous()
    for kind in OTHER:
        if kind == "maps":
            rgb, disp, acc, raw, maps = E.render_rays_maps(o, d, shared, 64, 64, 0., 2.5, precision="f16x3")
            rec = dict(rgb=rgb, disp=disp, acc=acc, **{m: maps[m] for m in MAPS})
        elif kind == "raw":
            rgb, disp, acc, raw = E.render_rays(o, d, shared, 64, 64, 0., 2.5, retraw=True, precision="f16x3")
            rec = dict(rgb=rgb, disp=disp, acc=acc, raw=raw)
        else:
            rec = dict(raw=E.mlp_fine_points(pts, v, shared, precision="f16x3"))
        rec = {k: t.cpu() for k, t in rec.items()}
        rec["range_flags"] = E.range_flags()
        res[kind] = rec
    torch.save(res, out_path)


if __name__ == "__main__":
    child(sys.argv[1])
    sys.exit(0)

import pytest  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(variant, *argv):
    env = dict(os.environ, DFN_MLP_VARIANT=str(variant), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, *argv], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    if out.returncode < 0 or out.returncode in (134, 137, 139):   # the child died on the GPU: nothing more is started on it
        pytest.exit(f"variant {variant} child ended with status {out.returncode}: {out.stderr[-2000:]}", returncode=3)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """The child's outputs under variants 10 and 11 (an exception in the first child's run leaves the second unstarted)."""
    out = {}
    for variant in (10, 11):
        path = str(tmp_path_factory.mktemp("variant11") / f"v{variant}.pt")
        _run(variant, os.path.abspath(__file__), path)
        out[variant] = torch.load(path)
    return out


def _same_bits(a, b, keys):
    differ = {k: int((a[k] != b[k]).sum()) for k in keys}
    print(f"elements that differ between variants 10 and 11: {differ}")
    for k in keys:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, differ[k])
        assert float(a[k].abs().max()) > 0 and bool(torch.isfinite(a[k]).all()) and bool(torch.isfinite(b[k]).all()), k
    assert a["range_flags"] == 0 and b["range_flags"] == 0


@pytest.mark.parametrize("tag", TAGS)
def test_variant11_is_variant10_bit_for_bit(pair, tag):
    a, b = pair[10][tag], pair[11][tag]
    calls, n, Nc, _, prec, per_ray = CASES[tag]
    print(f"{tag} ({calls} x {n} rays, {prec}, {'one histogram per ray' if per_ray else 'shared histogram'})")
    assert tuple(a["sigma"].shape) == (calls * n, Nc) and tuple(a["rgb"].shape) == (calls * n, 3)
    _same_bits(a, b, KEYS)


def test_moved_heads_lie_on_both_sides_of_each_threshold(pair):
    """case t: for every activated head value, samples MARGIN below and MARGIN above the threshold of its activation's other branch"""
    sides = pair[11]["t"]["sides"]
    print({f"{layer}[{row}] around {thr:g}": s for (layer, row, thr), s in zip(HEADS, sides)})
    assert len(sides) == len(HEADS) and sides == pair[10]["t"]["sides"]
    for (layer, row, thr), (below, above) in zip(HEADS, sides):
        assert below >= 64 and above >= 64, (layer, row, thr, below, above)   # at least one sample per ray's worth on each side


def test_per_ray_histograms_reach_the_output(pair):
    """case h is case a's rays with other embeddings"""
    assert not torch.equal(pair[11]["a"]["rgb"], pair[11]["h"]["rgb"])


def test_second_run_repeats_the_first(pair):
    """case d is case c again in the same process: the counters are zeroed and the table rewritten in front of every pass"""
    for k in KEYS:
        assert torch.equal(pair[11]["c"][k], pair[11]["d"][k]), k


@pytest.mark.parametrize("kind", OTHER)
def test_other_routes_run_variant10s_kernels(pair, kind):
    a, b = pair[10][kind], pair[11][kind]
    keys = [k for k in a if k != "range_flags"]
    assert set(keys) == set(k for k in b if k != "range_flags") and keys
    _same_bits(a, b, keys)
