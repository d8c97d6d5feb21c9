"""Cases, helpers and the child process of the kernel-variant comparisons of the split-f16 render MLP (tests/test_gpu_nerfh_lean.py
describes the cases; tests/test_gpu_nerfh_variant10.py, _variant11.py and _variant12.py read the same children's outputs).

The kernel variant is latched per process (DFN_MLP_VARIANT), so each variant runs in a child with a time limit: outputs(variant) starts
python tests/test_gpu_nerfh_lean.py <out.pt> under that variant, once per test session, and no child is started after one dies.
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
KEYS = ("sigma", "rgb", "disp", "acc")
MAX_FUSED_CHUNK = 65536   # nerfh_api.hip: kMaxFusedChunkRays
# {tag: (calls, rays per call, Nc, Ni, precision, one histogram row per ray, near, lindisp)}; cu takes its ray count from the device
# (None here), e / e2 take their rays from raygen, t runs on the moved heads
CASES = {"a": (1, 64, 64, 64, "f16x3", False, 0., False), "b": (8, 257, 16, 16, "f16x3", False, 0., False),
         "c": (1, 1040, 64, 64, "f16x3", False, 0., False), "d": (1, 1040, 64, 64, "f16x3", False, 0., False),
         "cu": (1, None, 16, 16, "f16x3", False, 0., False),
         "n1": (1, 320, 3, 29, "f16x3", False, 0., False), "n2": (1, 320, 24, 40, "f16x3", False, 0., False),
         "n3": (1, 320, 100, 92, "f16x3", False, 0., False),
         "l0": (1, 64, 64, 64, "f16x3", False, 0.5, False), "l1": (1, 64, 64, 64, "f16x3", False, 0.5, True),
         "h": (1, 64, 64, 64, "f16x3", True, 0., False),
         "e": (1, 12 * 16, 64, 128, "f16x3", False, 0., False), "e2": (1, 24 * 32, 64, 128, "f16x3", False, 0., False),
         "m1": (1, MAX_FUSED_CHUNK + 64, 16, 16, "f16x3", False, 0., False), "m2": (1, 2 * 65600, 16, 16, "f16x3", False, 0., False),
         "m3": (1, MAX_FUSED_CHUNK + 64, 8, 24, "f16x3", False, 0., False),
         "g": (1, 64, 64, 64, "f16", False, 0., False), "t": (1, 64, 64, 64, "f16x3", False, 0., False)}
TAGS = tuple(CASES)
RAYGEN = {"e": (12, 16, 14.6), "e2": (24, 32, 29.25)}   # H, W, focal
# the routes that keep variant 7's kernels and the unscaled table: (kind, per-ray histogram)
OTHER = tuple((kind, per_ray) for kind in ("maps", "raw", "points") for per_ray in (False, True))
MAPS = ("depth", "depth_static", "beta", "rgb_static", "rgb_transient")
# the eight activated head values of the fused fine kernel, each one the product of a select: (layer, row, the threshold at which its
# activation takes its other branch)
HEADS = tuple([("static_rgb.0", c, -80.) for c in range(3)] + [("static_sigma.0", 0, 20.)] +
              [("transient_rgb.0", c, -80.) for c in range(3)] + [("transient_sigma.0", 0, 20.)])
MARGIN = 1e-2   # a pre-activation counts as on one side when it is this far from the threshold: 600 x the 1.6e-5 that split-f16's 2e-7 is at 80
# the guard's trips: (network, bias, unit, what the position covers)
POSITIONS = ("even piece, low half", "even piece, high half", "odd piece, low half", "odd piece, high half")
TRIPS = tuple([("coarse", "xyz_encoding_8.0.bias", r, "converted inside the layer: " + POSITIONS[r]) for r in range(4)] +
              [("coarse", "xyz_encoding_8.0.bias", 96 + r, "carried into static_sigma: " + POSITIONS[r]) for r in range(4)] +
              [("fine", "transient_encoding.6.bias", r, "converted inside the layer: " + POSITIONS[r]) for r in range(4)] +
              [("fine", "transient_encoding.6.bias", 48 + r, "carried into the transient head, half 1: " + POSITIONS[r]) for r in range(4)])
TRIP_BIAS = 1e9   # in_scale x 1e9 is far above 65504 for every scale a commit picks (in_scale >= 2^-13 for weights below 2^13)
# One child's time limit in seconds.  The ten children of the parent's five pair-wise files took 9.1, 7.8 (the guard's seventeen
# engines), 3.1, 3.7, 3.9, 3.2, 3.3, 3.1, 3.2 and 2.9 s on an MI355X, about 2 s of each being the start of the process; this child runs
# the union of their cases once and took 8.6 s there (case a alone: 2.5 s).  Seven times that, for a machine that is busy or starts cold.
CHILD_TIMEOUT = 60


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


def piece_and_half(unit):
    """(M-block, conversion pieces of the two point blocks, half of the packed word) of hidden unit `unit`: the lane map of a PrecX3M16
    accumulator (row 16 ms + 4 g + r -> register 8 ms + 4 nb + r) and X3Piece's register pairs (piece i = registers 2i, 2i + 1)"""
    row = unit % 32
    ms, r = row // 16, row % 4
    return unit // 32, tuple((8 * ms + 4 * nb + r) // 2 for nb in (0, 1)), r & 1


def child(out_path, tags):
    """In this process's variant, on seed-0 synthetic weights (case t on the moved heads): coarse sigma and the fused route's outputs of
    the cases in `tags`; with no tags every case, one frame, the maps / raw / point-query routes and the guard's trips."""
    from dfnet_amd import engine as eng
    dev = "cuda:0"
    everything = not tags
    base = syn.nerfh_weights(0)
    E0 = eng.NerfHEngine(precision="f16x3").load_numpy(*base)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shared = T(np.asarray(syn.HIST_IDX, dtype=np.float32)).to(dev)
    res = {"cus": cus}
    for tag in (TAGS if everything else tags):
        calls, n, Nc, Ni, prec, per_ray, near, lindisp = CASES[tag]
        n = 8 * (cus + 1) if n is None else n
        E = E0
        if tag in RAYGEN:
            H, W, focal = RAYGEN[tag]
            o, d, _ = eng.raygen(H, W, focal, T(syn.orbit_pose(1, 8)).to(dev), want_viewdirs=False)
            o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        else:
            o, d = rays(calls * n)
            if tag == "t":
                weights, sides = moved_heads(o, d, Nc, Ni)
                E = eng.NerfHEngine(precision="f16x3").load_numpy(*weights)
            o, d = o.to(dev), d.to(dev)
        hists = ray_hists(calls * n).to(dev) if per_ray else None
        parts = {k: [] for k in KEYS}
        E.set_render_options(lindisp=lindisp)   # the handle's option: coarse depths linear in disparity
        for c in range(calls):
            oc, dc = o[c * n:(c + 1) * n].contiguous(), d[c * n:(c + 1) * n].contiguous()
            hc = hists[c * n:(c + 1) * n].contiguous() if per_ray else shared
            parts["sigma"].append(E.mlp_coarse(oc, dc, Nc, near, 2.5, precision=prec).cpu())
            f = E.render_rays(oc, dc, hc, Nc, Ni, near, 2.5, precision=prec)
            assert f[3] is None
            for k, t in zip(("rgb", "disp", "acc"), f):
                parts[k].append(t.cpu())
        rec = {k: torch.cat(v) for k, v in parts.items()}
        rec["range_flags"] = E.range_flags()
        E.set_render_options(lindisp=False)
        if tag == "t":
            rec["sides"] = sides
        res[tag] = rec
    if not everything:
        torch.save(res, out_path)
        return
    E = E0
    rgb, disp, acc = E.render_image(T(syn.orbit_pose(0, 8)).to(dev), 480, 640, 585.0, shared, 64, 128, 0., 2.5)
    res["frame"] = dict(rgb=rgb.cpu(), disp=disp.cpu(), acc=acc.cpu(), range_flags=E.range_flags())
    # the routes that variant 12 leaves with variant 7's kernels and the unscaled table: 64 rows at 64 + 64 in split-f16
    o, d = (t.to(dev) for t in rays(64))
    v = d / d.norm(dim=-1, keepdim=True)
    z = torch.linspace(0.1, 2.4, 64, device=dev)
    pts = (o[:, None, :] + d[:, None, :] * z[None, :, None]).contiguous()
    for kind, per_ray in OTHER:
        hc = ray_hists(64).to(dev) if per_ray else shared
        if kind == "maps":
            rgb, disp, acc, raw, maps = E.render_rays_maps(o, d, hc, 64, 64, 0., 2.5, precision="f16x3")
            rec = dict(rgb=rgb, disp=disp, acc=acc, **{m: maps[m] for m in MAPS})
        elif kind == "raw":
            rgb, disp, acc, raw = E.render_rays(o, d, hc, 64, 64, 0., 2.5, retraw=True, precision="f16x3")
            rec = dict(rgb=rgb, disp=disp, acc=acc, raw=raw)
        else:
            rec = dict(raw=E.mlp_fine_points(pts, v, hc, precision="f16x3"))
        rec = {k: t.cpu() for k, t in rec.items()}
        rec["range_flags"] = E.range_flags()
        res[(kind, per_ray)] = rec
    # the guard: 64 rays at 64 + 64; the untripped engine first, then one engine per tripped unit
    flags = {"none": []}
    E0.mlp_coarse(o, d, 64, 0., 2.5, precision="f16x3")
    flags["none"].append(E0.range_flags())
    E0.render_rays(o, d, shared, 64, 64, 0., 2.5, precision="f16x3")
    flags["none"].append(E0.range_flags())
    for net, name, unit, _ in TRIPS:
        cw, fw, ea, et = base
        cw, fw = {k: a.copy() for k, a in cw.items()}, {k: a.copy() for k, a in fw.items()}
        (cw if net == "coarse" else fw)[name][unit] = np.float32(TRIP_BIAS)
        E = eng.NerfHEngine(precision="f16x3").load_numpy(cw, fw, ea, et)
        if net == "coarse":
            E.mlp_coarse(o, d, 64, 0., 2.5, precision="f16x3")
        else:
            E.render_rays(o, d, shared, 64, 64, 0., 2.5, precision="f16x3")
        flags[(net, name, unit)] = E.range_flags()
    res["guard"] = flags
    torch.save(res, out_path)


CHILD_SCRIPT = os.path.join(ROOT, "tests", "test_gpu_nerfh_lean.py")
_outputs = {}


def run_child(variant, *argv):
    import pytest
    env = dict(os.environ, DFN_MLP_VARIANT=str(variant), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, CHILD_SCRIPT, *argv], cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    if out.returncode < 0 or out.returncode in (134, 137, 139):   # the child died on the GPU: nothing more is started on it
        pytest.exit(f"variant {variant} child ended with status {out.returncode}: {out.stderr[-2000:]}", returncode=3)
    assert out.returncode == 0, out.stderr[-3000:]


def outputs(variant, tmp_path_factory):
    """Everything the child computes under `variant`; one child per variant and test session (an exception in one child's run leaves
    the next unstarted)."""
    if variant not in _outputs:
        path = str(tmp_path_factory.mktemp("lean") / f"v{variant}.pt")
        run_child(variant, path)
        _outputs[variant] = torch.load(path)
    return _outputs[variant]


def same_bits(a, b, keys, what):
    differ = {k: int((a[k] != b[k]).sum()) for k in keys}
    print(f"elements that differ between {what}: {differ}")
    for k in keys:
        assert a[k].shape == b[k].shape and differ[k] == 0 and torch.equal(a[k], b[k]), (k, differ[k])
        assert float(a[k].abs().max()) > 0 and bool(torch.isfinite(a[k]).all()) and bool(torch.isfinite(b[k]).all()), k
    assert a["range_flags"] == 0 and b["range_flags"] == 0


def same_case(ra, rb, tag, what):
    """case `tag` of two children's outputs: the shapes the case asks for, then same_bits"""
    a, b = ra[tag], rb[tag]
    calls, n, Nc, Ni, prec, per_ray, near, lindisp = CASES[tag]
    assert ra["cus"] == rb["cus"]
    n = 8 * (rb["cus"] + 1) if n is None else n
    print(f"{tag} ({calls} x {n} rays at {Nc} + {Ni}, {prec}, near {near}, lindisp {lindisp}, "
          f"{'one histogram per ray' if per_ray else 'shared histogram'}, CUs {rb['cus']})")
    assert tuple(a["sigma"].shape) == (calls * n, Nc) and tuple(a["rgb"].shape) == (calls * n, 3)
    same_bits(a, b, KEYS, what)


def same_route(ra, rb, kind, per_ray, what):
    a, b = ra[(kind, per_ray)], rb[(kind, per_ray)]
    keys = [k for k in a if k != "range_flags"]
    assert set(keys) == set(k for k in b if k != "range_flags") and keys
    same_bits(a, b, keys, what)


def heads_on_both_sides(ra, rb):
    """case t: for every activated head value, samples MARGIN below and MARGIN above the threshold of its activation's other branch"""
    sides = rb["t"]["sides"]
    print({f"{layer}[{row}] around {thr:g}": s for (layer, row, thr), s in zip(HEADS, sides)})
    assert len(sides) == len(HEADS) and sides == ra["t"]["sides"]
    for (layer, row, thr), (below, above) in zip(HEADS, sides):
        assert below >= 64 and above >= 64, (layer, row, thr, below, above)   # at least one sample per ray's worth on each side


def second_run_repeats(r):
    """case d is case c again in the same process: the counters are zeroed and the table rewritten in front of every pass"""
    for k in KEYS:
        assert torch.equal(r["c"][k], r["d"][k]), k


def same_trip_flag(ra, rb, trip, what):
    net, name, unit, covers = trip
    mb, pieces, half = piece_and_half(unit)
    a, b = ra["guard"][(net, name, unit)], rb["guard"][(net, name, unit)]
    print(f"{net} {name}[{unit}] = {TRIP_BIAS:g}: M-block {mb}, pieces {pieces} ({'odd' if pieces[0] % 2 else 'even'}), "
          f"{'high' if half else 'low'} half -- {covers}; flags under {what}: {a}, {b}")
    assert a == 2 and b == 2, (a, b)


TRIP_IDS = [f"{t[0]}-{t[2]}" for t in TRIPS]
