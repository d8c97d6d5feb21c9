"""Kernel variant 12: variant 11's coarse and plain fused fine kernel with a leaner tile seam and range guard (nerfh_mlp_lean.hip).

Variant 12 evaluates the fine kernel's eight head activations as four (the static pre-activations ride on lanes 32..63), takes
point -> ray by a multiply-high and a shift (nerfh_raydiv.h) and keeps the range guard of the ReLU conversions with one
v_pk_maximum3_f16 per two pieces (nerfh_layout.h: kLeanVariant).  The same values reach the same lanes through the same arithmetic, so
every output AND the range flag must be variant 11's.  The variant is latched per process (DFN_MLP_VARIANT), so each variant runs in a child with a time limit, and no child is
started after one fails:

  * variant 12 against variant 11, elements that differ (each count must be 0; finite, not all zero) on coarse sigma and the fused
    route's rgb / disp / acc, split-f16 at netwidth 128, dfn_nerfh_range_status 0 after each case:
      a  64 rays at 64 + 64: fewer tiles than workgroups;
      b  8 calls of 257 rays at 16 + 16: ragged last tiles whose points are clamped;
      c  1 040 rays at 64 + 64: workgroups claim second and third tiles;
      d  case c a second time in the same process;
      n1 n2 n3  320 rays at 3 + 29, 24 + 40 and 100 + 92: sample counts that are no powers of two (the magic number's general case);
      l0 l1  64 rays at 64 + 64 with near = 0.5, far = 2.5, lindisp off and on: both depth forms of the coarse kernel (l1's sigma must
         differ from l0's: the option reaches the kernel);
      h  case a with one histogram row per ray;
      e  the 192 rays of a 12 x 16 raygen image at 64 + 128;
      g  case a at precision f16: the route falls back to variant 4's plain kernels;
      t  variant 11's threshold case: weights at gain 2 whose eight fine head biases are moved so that the samples straddle
         softplus's pass-through at 20 and the sigmoid's clamp at -80 (tests/test_gpu_nerfh_variant11.py: moved_heads); these are the
         values that variant 12 moves across lanes;
  * under variant 12 a maps render, a `raw` render and a fine point query on 64 rows give variant 11's bits (the same kernels);
  * the guard.  A hidden unit's bias is no part of the commit's weight scan (nerfh_recommit.h), so a bias of 1e9 on ONE unit of the
    last ReLU layer in front of a head saturates the hi half of that unit alone and nothing downstream is converted again: the flag
    must read 2 (DFN_RANGE_F16X3) under variants 11 and 12 alike, and 0 without the trip.  Row 16 ms + 4 g + r of an M-block is
    accumulator register 8 ms + 4 nb + r of lane group g (nerfh_layout.h), i.e. conversion piece i = 4 ms + 2 nb + (r >> 1) and half
    r & 1 of its packed word (nerfh_mlp_core.h: X3Piece, x3_chunk / x3_pos), so units r = 0, 1, 2, 3 cover
        r = 0: even piece, low half     r = 1: even piece, high half     r = 2: odd piece, low half     r = 3: odd piece, high half
    -- an even piece's hi word is the one variant 12 holds for the odd piece's v_pk_maximum3_f16.  Tripped in the coarse kernel
    (xyz_encoding_8, unit r of M-block 0: converted inside layer 8; unit 96 + r of M-block 3: carried into static_sigma, where pieces
    2 and 3 lie in different chunks) and in the fine kernel (transient_encoding.6, unit r: converted inside the layer; unit 48 + r:
    pieces 4..7 of the carried-in M-block, the block form behind the transient head's first chunk).

This file is also the child of its own tests: python tests/test_gpu_nerfh_variant12.py <out.pt>.
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
from tests.test_gpu_nerfh_variant11 import HEADS, MAPS, OTHER, moved_heads, ray_hists, rays  # noqa: E402

T = torch.from_numpy
KEYS = ("sigma", "rgb", "disp", "acc")
# {tag: (calls, rays per call, Nc, Ni, precision, one histogram row per ray, near, lindisp)}; e takes its rays from raygen, t runs on the moved heads
CASES = {"a": (1, 64, 64, 64, "f16x3", False, 0., False), "b": (8, 257, 16, 16, "f16x3", False, 0., False),
         "c": (1, 1040, 64, 64, "f16x3", False, 0., False), "d": (1, 1040, 64, 64, "f16x3", False, 0., False),
         "n1": (1, 320, 3, 29, "f16x3", False, 0., False), "n2": (1, 320, 24, 40, "f16x3", False, 0., False),
         "n3": (1, 320, 100, 92, "f16x3", False, 0., False),
         "l0": (1, 64, 64, 64, "f16x3", False, 0.5, False), "l1": (1, 64, 64, 64, "f16x3", False, 0.5, True),
         "h": (1, 64, 64, 64, "f16x3", True, 0., False), "e": (1, 12 * 16, 64, 128, "f16x3", False, 0., False),
         "g": (1, 64, 64, 64, "f16", False, 0., False), "t": (1, 64, 64, 64, "f16x3", False, 0., False)}
TAGS = tuple(CASES)
# the guard's trips: (network, bias, unit, what the position covers)
POSITIONS = ("even piece, low half", "even piece, high half", "odd piece, low half", "odd piece, high half")
TRIPS = tuple([("coarse", "xyz_encoding_8.0.bias", r, "converted inside the layer: " + POSITIONS[r]) for r in range(4)] +
              [("coarse", "xyz_encoding_8.0.bias", 96 + r, "carried into static_sigma: " + POSITIONS[r]) for r in range(4)] +
              [("fine", "transient_encoding.6.bias", r, "converted inside the layer: " + POSITIONS[r]) for r in range(4)] +
              [("fine", "transient_encoding.6.bias", 48 + r, "carried into the transient head, half 1: " + POSITIONS[r]) for r in range(4)])
TRIP_BIAS = 1e9   # in_scale x 1e9 is far above 65504 for every scale a commit picks (in_scale >= 2^-13 for weights below 2^13)


def piece_and_half(unit):
    """(M-block, conversion pieces of the two point blocks, half of the packed word) of hidden unit `unit`: the lane map of a PrecX3M16
    accumulator (row 16 ms + 4 g + r -> register 8 ms + 4 nb + r) and X3Piece's register pairs (piece i = registers 2i, 2i + 1)"""
    row = unit % 32
    ms, r = row // 16, row % 4
    return unit // 32, tuple((8 * ms + 4 * nb + r) // 2 for nb in (0, 1)), r & 1


def child(out_path):
    """Coarse sigma and the fused route's outputs of every case, the maps / raw / point-query routes and the guard's trips, in this
    process's variant; seed-0 synthetic weights, case t on the moved heads."""
    from dfnet_amd import engine as eng
    dev = "cuda:0"
    base = syn.nerfh_weights(0)
    E0 = eng.NerfHEngine(precision="f16x3").load_numpy(*base)
    shared = T(np.asarray(syn.HIST_IDX, dtype=np.float32)).to(dev)
    res = {}
    for tag, (calls, n, Nc, Ni, prec, per_ray, near, lindisp) in CASES.items():
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
    # the routes that variant 12 leaves with variant 11's kernels: 64 rows at 64 + 64 in split-f16
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
    """The child's outputs under variants 11 and 12 (an exception in the first child's run leaves the second unstarted)."""
    out = {}
    for variant in (11, 12):
        path = str(tmp_path_factory.mktemp("variant12") / f"v{variant}.pt")
        _run(variant, os.path.abspath(__file__), path)
        out[variant] = torch.load(path)
    return out


def _same_bits(a, b, keys):
    differ = {k: int((a[k] != b[k]).sum()) for k in keys}
    print(f"elements that differ between variants 11 and 12: {differ}")
    for k in keys:
        assert a[k].shape == b[k].shape and differ[k] == 0 and torch.equal(a[k], b[k]), (k, differ[k])
        assert float(a[k].abs().max()) > 0 and bool(torch.isfinite(a[k]).all()) and bool(torch.isfinite(b[k]).all()), k
    assert a["range_flags"] == 0 and b["range_flags"] == 0


@pytest.mark.parametrize("tag", TAGS)
def test_variant12_is_variant11_bit_for_bit(pair, tag):
    a, b = pair[11][tag], pair[12][tag]
    calls, n, Nc, Ni, prec, per_ray, near, lindisp = CASES[tag]
    print(f"{tag} ({calls} x {n} rays at {Nc} + {Ni}, {prec}, near {near}, lindisp {lindisp}, "
          f"{'one histogram per ray' if per_ray else 'shared histogram'})")
    assert tuple(a["sigma"].shape) == (calls * n, Nc) and tuple(a["rgb"].shape) == (calls * n, 3)
    _same_bits(a, b, KEYS)


def test_moved_heads_lie_on_both_sides_of_each_threshold(pair):
    """case t: for every activated head value, samples MARGIN below and MARGIN above the threshold of its activation's other branch"""
    sides = pair[12]["t"]["sides"]
    print({f"{layer}[{row}] around {thr:g}": s for (layer, row, thr), s in zip(HEADS, sides)})
    assert len(sides) == len(HEADS) and sides == pair[11]["t"]["sides"]
    for (layer, row, thr), (below, above) in zip(HEADS, sides):
        assert below >= 64 and above >= 64, (layer, row, thr, below, above)   # at least one sample per ray's worth on each side


def test_lindisp_reaches_the_coarse_kernel(pair):
    """cases l0 / l1 differ in the depth form alone"""
    assert not torch.equal(pair[12]["l0"]["sigma"], pair[12]["l1"]["sigma"])


def test_second_run_repeats_the_first(pair):
    """case d is case c again in the same process: the counters are zeroed and the table rewritten in front of every pass"""
    for k in KEYS:
        assert torch.equal(pair[12]["c"][k], pair[12]["d"][k]), k


@pytest.mark.parametrize("kind", OTHER)
def test_other_routes_run_variant11s_kernels(pair, kind):
    a, b = pair[11][kind], pair[12][kind]
    keys = [k for k in a if k != "range_flags"]
    assert set(keys) == set(k for k in b if k != "range_flags") and keys
    _same_bits(a, b, keys)


def test_trip_positions_cover_both_pieces_and_both_halves():
    """no GPU work: the four positions per (network, path), from the lane map"""
    for base, mb in ((0, 0), (96, 3), (48, 1)):
        seen = set()
        for r in range(4):
            m, pieces, half = piece_and_half(base + r)
            assert m == mb and pieces[0] % 2 == pieces[1] % 2
            seen.add((pieces[0] % 2, half))
        assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert piece_and_half(98)[1] == (1, 3) and piece_and_half(50)[1] == (5, 7) and piece_and_half(2)[1] == (1, 3) and piece_and_half(0)[1] == (0, 2)


def test_guard_reads_0_without_a_trip(pair):
    assert pair[11]["guard"]["none"] == [0, 0] and pair[12]["guard"]["none"] == [0, 0]


@pytest.mark.parametrize("trip", TRIPS, ids=[f"{t[0]}-{t[2]}" for t in TRIPS])
def test_guard_raises_the_same_flag(pair, trip):
    net, name, unit, covers = trip
    mb, pieces, half = piece_and_half(unit)
    a, b = pair[11]["guard"][(net, name, unit)], pair[12]["guard"][(net, name, unit)]
    print(f"{net} {name}[{unit}] = {TRIP_BIAS:g}: M-block {mb}, pieces {pieces} ({'odd' if pieces[0] % 2 else 'even'}), "
          f"{'high' if half else 'low'} half -- {covers}; flag under variant 11: {a}, under variant 12: {b}")
    assert a == 2 and b == 2, (a, b)
