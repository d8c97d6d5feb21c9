#!/usr/bin/env python3
"""Times the re-pack of a NeRF-H engine after the master weights moved, netwidth 128, in one call on one machine:

  refresh-host     HipQuery.refresh() with nerfw.DEVICE_RECOMMIT off: load_modules -> dfn_nerfh_set_param x 64 + dfn_nerfh_commit
  refresh-device   the same call with the switch on: NerfHEngine.load_device -> dfn_nerfh_recommit_device
  recommit-events  load_device alone between two device events (the 8-byte read of the weight maxima in the middle included)
  first-call       the first load_device of an engine: the plan is built by the host packer and uploaded

refresh-* are wall clock around a drained stream, recommit-events device time; per candidate the median over the repetitions and the
spread (min .. max).  Every measurement is a child process of its own under a time limit; the first one that fails or runs out of
time ends the run.  The byte counts come from dfn_nerfh_recommit_selfcheck (host only).  Nothing is gated on these numbers.

Usage:  python tools/gpu_recommit_timing.py [--reps 31] [--limit 120] [--json out.json]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WHATS = ("refresh-host", "refresh-device", "recommit-events", "first-call")


def world():
    import torch
    from dfnet_amd import engine as eng, nerfw
    dev = "cuda:0"
    coarse = nerfw.NeRFW('coarse', D=8, W=128, skips=[4], in_channels_xyz=63, in_channels_dir=27)
    fine = nerfw.NeRFW('fine', D=8, W=128, skips=[4], in_channels_xyz=63, in_channels_dir=27, encode_appearance=True,
                       encode_transient=True, in_channels_a=50, in_channels_t=20)
    mods = tuple(m.to(dev) for m in (coarse, fine, torch.nn.Embedding(1000, 5), torch.nn.Embedding(1000, 2)))
    E = eng.NerfHEngine(width=128, precision="f16x3")
    E.load_modules(*mods)
    return E, mods, nerfw.HipQuery(E, modules=mods)


def measure(what, reps):
    import torch
    from dfnet_amd import nerfw
    E, mods, q = world()
    tensors = E.module_tensors(*mods)
    t = []
    if what.startswith("refresh"):
        nerfw.DEVICE_RECOMMIT = what == "refresh-device"
        q.stale = True
        q.refresh()
        for _ in range(reps):
            q.stale = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q.refresh()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        assert E.device_commits == (reps + 1 if what == "refresh-device" else 0)
        name = f"HipQuery.refresh(), DEVICE_RECOMMIT {'on' if what == 'refresh-device' else 'off'} (wall clock)"
    elif what == "recommit-events":
        E.load_device(tensors)
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            E.load_device(tensors)
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) * 1e-3)
        name = "load_device alone (device events)"
    else:   # one sample per process: the plan exists after the first call
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E.load_device(tensors)
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
        name = "first load_device of an engine: plan build + upload + re-commit (wall clock)"
    print(json.dumps([dict(what=name, ms=statistics.median(t) * 1e3, ms_min=min(t) * 1e3, ms_max=max(t) * 1e3)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=WHATS, default=None, help="one measurement, in this process (what the driver starts)")
    ap.add_argument("--reps", type=int, default=31)
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
            sys.exit(f"gpu_recommit_timing: '{what}' ran past {args.limit} s; nothing further is started")
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(f"gpu_recommit_timing: '{what}' ended with status {p.returncode}; nothing further is started")
        got = json.loads(p.stdout.strip().splitlines()[-1])
        rows += got
        for r in got:
            print(f"{r['what']:80s} {r['ms']:9.3f} ms  ({r['ms_min']:.3f} .. {r['ms_max']:.3f})", flush=True)
    from dfnet_amd import _lib
    lib = _lib.load()
    if lib.dfn_nerfh_recommit_selfcheck(128) == 0:
        text = lib.dfn_last_error().decode()
        print(text)
        m = re.search(r"\((\d+) bytes\) and \d+ segments; (\d+) bytes written", text)
        ev = rows[2]["ms"] * 1e-3
        plan, written = int(m.group(1)), int(m.group(2))
        print(f"re-commit alone: {written / ev / 1e9:.1f} GB/s of packed bytes stored, {(written + plan) / ev / 1e9:.1f} GB/s with the plan's reads")
        rows.append(dict(what="bytes", plan_bytes=plan, written_bytes=written, stored_GBps=written / ev / 1e9))
    print(f"refresh(): host path / device path = {rows[0]['ms'] / rows[1]['ms']:.1f}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
