#!/usr/bin/env python3
"""Times the training query on points (NerfHTrainer.points_forward / points_backward: dfn_nerfh_points_train_*) at the shapes of the
judged step — the fine network at 1 536 x 192 points, the coarse one at 1 536 x 64 — beside NerfHTrainer.train_step's own forward and
backward on 1 536 rays of 64 + 128 samples, in one call on one machine.  The step runs both networks' chains, streams and tails on
the same byte counts (plus two compositors and the sampler), so the two queries together are expected to cost about the step's
forward + backward; what a query adds per call is the weight pack (the step has it too), its own workspace allocation and
HipQuery.refresh() (a re-pack of the test-time engine whenever the master weights moved), which is timed on its own.

Device events after a warm-up; per candidate the median over the repetitions and the spread (min .. max).  Every measurement is a
child process of its own under a time limit; the first one that fails or runs out of time ends the run.  Nothing is gated on these
numbers.

Usage:  python tools/gpu_points_train_timing.py [--reps 9] [--limit 120] [--json out.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R, NC, NI = 1536, 64, 128
WHATS = ("fine", "fine-split", "coarse", "step", "refresh")


def world():
    import torch
    from dfnet_amd import engine as eng, nerf_train, nerfw
    dev = "cuda:0"
    coarse = nerfw.NeRFW('coarse', D=8, W=128, skips=[4], in_channels_xyz=63, in_channels_dir=27)
    fine = nerfw.NeRFW('fine', D=8, W=128, skips=[4], in_channels_xyz=63, in_channels_dir=27, encode_appearance=True,
                       encode_transient=True, in_channels_a=50, in_channels_t=20)
    mods = tuple(m.to(dev) for m in (coarse, fine, torch.nn.Embedding(1000, 5), torch.nn.Embedding(1000, 2)))
    E = eng.NerfHEngine(width=128, precision="f16x3")
    E.load_modules(*mods)
    q = nerfw.HipQuery(E, modules=mods)
    q.trainer = nerf_train.NerfHTrainer(E, *mods)
    return q


def events(fns, reps):
    """[[seconds per phase] per repetition] of the phases `fns` run back to back."""
    import torch
    out = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
        ev[0].record()
        for i, fn in enumerate(fns):
            fn()
            ev[i + 1].record()
        ev[-1].synchronize()
        out.append([ev[i].elapsed_time(ev[i + 1]) * 1e-3 for i in range(len(fns))])
    return out


def measure(what, reps):
    import torch
    from dfnet_amd import synthetic as syn
    dev = "cuda:0"
    q = world()
    tr = q.trainer
    gen = torch.Generator().manual_seed(1)
    hist = torch.from_numpy(syn.HIST_IDX)[None].float().to(dev)
    rows = []
    if what in ("fine", "fine-split", "coarse"):
        net, N = ("coarse", NC) if what == "coarse" else ("fine", NC + NI)
        tr.fused_split = what == "fine-split"
        pts = (torch.rand(R, N, 3, generator=gen) * 3 - 1.5).to(dev)
        v = torch.randn(R, 3, generator=gen)
        v = (v / v.norm(dim=-1, keepdim=True)).to(dev)
        G = torch.randn(R, N, 9 if net == "fine" else 4, generator=gen).to(dev)
        state = {}
        def fwd():
            state["raw"], state["saved"] = tr.points_forward(net, pts, v, hist if net == "fine" else None)
        def bwd():
            tr.points_backward(state["saved"], G)
        for _ in range(3):
            fwd(); bwd()
        torch.cuda.synchronize()
        t = events([fwd, bwd], reps)
        names = (f"{what} query forward {R} x {N}", f"{what} query backward {R} x {N}")
    elif what == "step":
        import numpy as np
        from oracle import nerfh_oracle as orc
        rng = np.random.default_rng(0)
        ro, rd = orc.get_rays(480, 640, 585.0, torch.from_numpy(syn.orbit_pose(0, 8))[:3, :4])
        sel = rng.choice(480 * 640, R, replace=False)
        o, d = ro.reshape(-1, 3)[sel].contiguous().to(dev), rd.reshape(-1, 3)[sel].contiguous().to(dev)
        target = torch.rand(R, 3, device=dev)
        draws = tr.draw(R, NC, NI, 1., dev)
        state = {}
        def fwd():
            state["out"] = tr.forward(o, d, hist, NC, NI, 0., 2.5, *draws[:2], 0., draws[2])
        def loss():
            state["loss"] = tr.loss(state["out"], target)
        def bwd():
            _, (g_rgb, g_rgb0, g_beta), g_ts = state["loss"]
            tr.backward(g_rgb, g_rgb0, g_beta, g_ts)
        for _ in range(3):
            fwd(); loss(); bwd()
        torch.cuda.synchronize()
        t = events([fwd, loss, bwd], reps)
        names = (f"train_step forward {R} rays {NC}+{NI}", "train_step loss", f"train_step backward {R} rays {NC}+{NI}")
    else:   # refresh(): host + device, wall clock around a drained stream
        t = []
        q.refresh()
        for _ in range(reps):
            q.stale = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q.refresh()
            torch.cuda.synchronize()
            t.append([time.perf_counter() - t0])
        names = ("HipQuery.refresh() after the weights moved (wall clock)",)
    for i, name in enumerate(names):
        col = [r[i] for r in t]
        rows.append(dict(what=name, ms=statistics.median(col) * 1e3, ms_min=min(col) * 1e3, ms_max=max(col) * 1e3))
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=WHATS, default=None, help="one measurement, in this process (what the driver starts)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--limit", type=int, default=120, help="seconds per measurement")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.what:
        return measure(args.what, args.reps)
    rows = []
    for what in WHATS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--what", what, "--reps", str(args.reps)], capture_output=True,
                               text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"gpu_points_train_timing: '{what}' ran past {args.limit} s; nothing further is started")
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(f"gpu_points_train_timing: '{what}' ended with status {p.returncode}; nothing further is started")
        got = json.loads(p.stdout.strip().splitlines()[-1])
        rows += got
        for r in got:
            print(f"{r['what']:58s} {r['ms']:8.3f} ms  ({r['ms_min']:.3f} .. {r['ms_max']:.3f})", flush=True)
    ms = {r["what"].split(" 1536")[0]: r["ms"] for r in rows}
    both = ms["fine query forward"] + ms["fine query backward"] + ms["coarse query forward"] + ms["coarse query backward"]
    step = ms["train_step forward"] + ms["train_step backward"]
    print(f"fine + coarse query, forward + backward: {both:.3f} ms; train_step forward + backward (both networks, compositors, sampler): "
          f"{step:.3f} ms; ratio {both / step:.3f}")
    rows.append(dict(what="queries / step", ratio=both / step))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
