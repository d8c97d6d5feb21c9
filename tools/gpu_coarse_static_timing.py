#!/usr/bin/env python3
"""Times the coarse network's training query on points (NerfHEngine.mlp_coarse_static_points) and its input gradient
(mlp_coarse_static_points_backward) beside the fine points query / fine points gradient on the same 61 440 x 64 points, per
arithmetic mode.  Device events after a warm-up, the candidates alternating inside one process; per candidate the median over the
repetitions and the run-to-run spread (min .. max).

The new kernels execute a strict subset of the fine kernels' layers on the same geometry, so neither may be slower than its fine
counterpart beyond the fine kernel's own spread in the same run.  The EXPECTED ratio is the ratio of MFMA chunks ((M-block, 8-slot
K-chunk) pairs per 32-point block) of the two sequences, computed below from the layer shapes of dfnet_amd/csrc/nerfh_layout.h
(layer_shape / bwd_layer_shape at netwidth 128; seq_chunks and its static_assert there give the same forward counts).  A measured
ratio worse than the count predicts is a finding about the moved prefetch or the barriers.  Nothing is gated on these numbers.

Usage:  python tools/gpu_coarse_static_timing.py [--rows 61440] [--N 64] [--reps 7] [--inner 3] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dfnet_amd import engine as eng, synthetic as syn  # noqa: E402

DEV = "cuda:0"
W = 128
# nerfh_layout.h: layer_shape(id, W) = (slots per half, M-blocks)
FWD = {"L1": (32, W // 32), "L5": (32 + W // 2, W // 32), "L": (W // 2, W // 32), "FIN": (W // 2, W // 32 + 1), "DIR": (W // 2, W // 64),
       "RGB": (W // 4, 1), "TE0": (W // 2, W // 64), "TE": (W // 4, W // 64), "THEAD": (W // 4, 1), "SIG": (W // 2, 1)}
TRUNK = ["L1", "L", "L", "L", "L5", "L", "L", "L"]
SEQ = {"fine": TRUNK + ["FIN", "DIR", "RGB", "TE0", "TE", "TE", "TE", "THEAD"],              # kFineSeq
       "fine fold": TRUNK + ["SIG", "DIR", "RGB", "TE0", "TE", "TE", "TE", "THEAD"],         # kFineFoldSeq (LY_DIRF / LY_TE0F have LY_DIR's shape)
       "static": TRUNK + ["FIN", "DIR", "RGB"],                                              # kCoarseStaticSeq
       "static fold": TRUNK + ["SIG", "DIR", "RGB"]}                                         # kCoarseStaticFoldSeq
# nerfh_layout.h: bwd_layer_shape(id)
BWD = {"THEAD": (16, 2), "RGB": (16, 2), "TE": (32, 2), "FINCAT": (64, 5), "DIRCAT": (32, 5), "FIN": (80, 4), "L5": (64, 6), "L1": (64, 2),
       "L": (64, 4)}
BTRUNK = ["FIN", "L", "L", "L", "L5", "L", "L", "L", "L1"]
BSEQ = {"fine": ["THEAD", "TE", "TE", "TE", "RGB", "FINCAT"] + BTRUNK,                         # BW_THEAD .. BW_L1
        "static": ["RGB", "DIRCAT"] + BTRUNK}                                                 # kBwdCoarseStaticSeq


def chunks(seq, shapes):
    return sum(shapes[k][0] // 8 * shapes[k][1] for k in seq)


def expected():
    """(forward plain, forward folded, gradient = plain forward recompute + backward chain): static / fine MFMA chunks."""
    fs, ff = chunks(SEQ["static"], FWD), chunks(SEQ["fine"], FWD)
    gs, gf = fs + chunks(BSEQ["static"], BWD), ff + chunks(BSEQ["fine"], BWD)
    return fs / ff, chunks(SEQ["static fold"], FWD) / chunks(SEQ["fine fold"], FWD), gs / gf


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=61440)
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    e_plain, e_fold, e_grad = expected()
    print(f"expected static / fine from MFMA chunks: forward plain {e_plain:.3f} (f32, f16), forward folded {e_fold:.3f} (f16x3), "
          f"gradient {e_grad:.3f}")
    if not torch.cuda.is_available():
        sys.exit("gpu_coarse_static_timing: needs a GPU (a CPU run says nothing about these kernels)")
    cw, fw, ea, et = syn.nerfh_weights(0)
    E = eng.NerfHEngine().load_numpy(cw, fw, ea, et)
    rows, N = args.rows, args.N
    gen = torch.Generator().manual_seed(rows * 1000 + N)
    pts = (torch.rand(rows, N, 3, generator=gen) * 3 - 1.5).to(DEV)
    v = torch.randn(rows, 3, generator=gen)
    v = (v / v.norm(dim=-1, keepdim=True)).to(DEV)
    hist = torch.from_numpy(syn.HIST_IDX)[None].float().to(DEV)
    g9 = torch.randn(rows, N, 9, generator=gen).to(DEV)
    g4 = g9[..., :4].contiguous()
    cands = {}
    for prec in ("f32", "f16x3", "f16"):
        cands[f"static query {prec}"] = lambda p=prec: E.mlp_coarse_static_points(pts, v, precision=p)
        cands[f"fine query {prec}"] = lambda p=prec: E.mlp_fine_points(pts, v, hist, precision=p)
    for prec in ("f32", "f16x3"):
        cands[f"static gradient {prec}"] = lambda p=prec: E.mlp_coarse_static_points_backward(pts, v, g4, precision=p)
        cands[f"fine gradient {prec}"] = lambda p=prec: E.mlp_fine_points_backward(pts, v, hist, g9, precision=p)
    for fn in cands.values():      # warm-up: code objects, allocator
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(args.reps):
        for k, fn in cands.items():      # alternating
            times[k].append(timed(fn, args.inner))
    out = []
    for k, t in times.items():
        med = statistics.median(t)
        out.append(dict(what=k, rows=rows, N=N, us=med * 1e6, us_min=min(t) * 1e6, us_max=max(t) * 1e6,
                        ns_per_point=med * 1e9 / (rows * N)))
        print(f"{rows} x {N}  {k:24s} {med * 1e6:10.1f} us  ({min(t) * 1e6:.1f} .. {max(t) * 1e6:.1f})  "
              f"{med * 1e9 / (rows * N):6.3f} ns per point")
    for what, precs in (("query", ("f32", "f16x3", "f16")), ("gradient", ("f32", "f16x3"))):
        for prec in precs:
            s, f = times[f"static {what} {prec}"], times[f"fine {what} {prec}"]
            want = e_grad if what == "gradient" else (e_fold if prec == "f16x3" else e_plain)
            ratio, spread = statistics.median(s) / statistics.median(f), (max(f) - min(f)) / statistics.median(f)
            out.append(dict(what=f"{what} {prec} static / fine", ratio=ratio, expected=want, fine_spread=spread))
            print(f"{what} {prec}: static / fine = {ratio:.3f} (expected from MFMA chunks {want:.3f}; spread of the fine kernel "
                  f"(max - min) / median = {spread:.3f})")
    if args.json:
        with open(args.json, "w") as fjson:
            json.dump(out, fjson, indent=1)


if __name__ == "__main__":
    main()
