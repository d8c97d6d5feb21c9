"""Cost of the render maps on one 640 x 480 frame at 64 + 128 samples in split-f16 (the default arithmetic), and the register counts of
the two flavours of the fine kernel.

  python tools/gpu_render_maps_ab.py            three timings on cuda:0, one JSON line each (median / min / max of REPS device-event
                                                timings after three warm-up calls):
      plain        E.render_image                               rgb, disp, acc
      maps         E.render_image_maps, all five maps           the fused epilogue's maps flavour + composite_combine_maps
      raw+stage    E.render_rays(retraw=True) + composite_fine(want_aux=True): the only route to a depth / beta map before the maps
                   entries (raw [n, 192, 9] goes through HBM: 2.1 GB for this frame).  The render does not return z_fine, so this
                   route recomputes it (coarse MLP + sample_fine); that recompute is timed on its own too ("z_recompute_ms") and
                   the line carries the figure without it ("median_without_z_recompute_ms")
    and the per-launch averages of the fine kernel and the segment combine in both flavours (dfn_profile_read).
  python tools/gpu_render_maps_ab.py --registers   no GPU: VGPR / SGPR / scratch / code bytes of every nerfh_fine_kernel instantiation in
                                                dfnet_amd/csrc/build/nerfh_mlp.o, nerfh_mlp_maps.o, nerfh_mlp_fold.o (kernel variant 5's
                                                nerfh_fine_fold_kernel) and nerfh_mlp_half.o (kernel variant 6's nerfh_fine_half_kernel and
                                                nerfh_coarse_half_kernel) and nerfh_mlp_res.o (kernel variant 7's nerfh_fine_res_kernel and
                                                nerfh_coarse_res_kernel); the fine kernels' last template argument is the maps flavour.
                                                Also every kernel of the points flavour (nerfh_*_pts_kernel: nerfh_mlp_pts.o,
                                                nerfh_mlp_pts_fold.o, nerfh_mlp_pts_half.o, nerfh_bwd_pts.o).
  python tools/gpu_render_maps_ab.py --text-sha [nerfh_mlp.o ...]   no GPU: sha256 and size of the .text of each object's gfx950 code
                                                object (default: this build's nerfh_mlp.o): equal digests of two builds = the same
                                                instructions at the same offsets for every kernel that runs without maps.
The headline itself is bench.py's (bench.py --gpus 1 --steps 20 --warmup 5, alternated between two library builds with
tools/gpu_ab_libs.sh)."""
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def registers():
    for name in ("nerfh_mlp.o", "nerfh_mlp_maps.o", "nerfh_mlp_fold.o", "nerfh_mlp_half.o", "nerfh_mlp_res.o", "nerfh_mlp_pts.o", "nerfh_mlp_pts_fold.o",
                 "nerfh_mlp_pts_half.o", "nerfh_bwd_pts.o"):
        registers_of(os.path.join(ROOT, "dfnet_amd", "csrc", "build", name))


def unbundle(obj, tmp):
    """The gfx950 code object inside a host object's .hip_fatbin."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    fb, co = os.path.join(tmp, "fb"), os.path.join(tmp, "co")
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fb}", obj], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fb}", f"--output={co}", "--unbundle"], check=True)
    return co


def text_sha(objs):
    import hashlib
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    for obj in objs or [os.path.join(ROOT, "dfnet_amd", "csrc", "build", "nerfh_mlp.o")]:
        with tempfile.TemporaryDirectory() as tmp:
            text = os.path.join(tmp, "text")
            subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.text", unbundle(obj, tmp), text], check=True)
            data = open(text, "rb").read()
        print(json.dumps(dict(object=os.path.basename(obj), text_bytes=len(data), text_sha256=hashlib.sha256(data).hexdigest())))


def registers_of(obj):
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    with tempfile.TemporaryDirectory() as tmp:
        co = unbundle(obj, tmp)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
        syms = subprocess.run([os.path.join(llvm, "llvm-readelf"), "-sW", co], capture_output=True, text=True, check=True).stdout
    size = {f[7]: int(f[2]) for f in (l.split() for l in syms.splitlines()) if len(f) >= 8 and f[3] == "FUNC"}
    for blk in notes.split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)
        name = g("name")
        if not any(k in name for k in ("nerfh_fine_kernel", "nerfh_fine_fold_kernel", "nerfh_fine_half_kernel", "nerfh_coarse_half_kernel", "nerfh_fine_res_kernel",
                                       "nerfh_coarse_res_kernel", "_pts_kernel")):
            continue
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("dfn::", "")
        print(json.dumps(dict(kernel=dem, vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")), scratch_bytes=int(g("private_segment_fixed_size")),
                              vgpr_spills=int(g("vgpr_spill_count")), code_bytes=size.get(name, -1))))


def timings():
    import numpy as np
    import torch
    from dfnet_amd import _lib, engine as eng, synthetic as syn
    DEV, T = "cuda:0", torch.from_numpy
    REPS = int(os.environ.get("AB_REPS", "10"))
    H, W, focal, Nc, Ni, near, far = 480, 640, 585.0, 64, 128, 0., 2.5
    E = eng.NerfHEngine(precision="f16x3").load_numpy(*syn.nerfh_weights(0))
    c2w = T(syn.orbit_pose(1, 8)).to(DEV)
    hist = torch.as_tensor(syn.HIST_IDX).float().to(DEV)
    o, d, _ = eng.raygen(H, W, focal, c2w)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)

    def raw_route():
        rgb, disp, acc, raw = E.render_rays(o, d, hist, Nc, Ni, near, far, retraw=True)
        z = eng.sample_fine(E.mlp_coarse(o, d, Nc, near, far), Ni, near, far)   # the depths the stage needs: not returned by the render
        return eng.composite_fine(raw, z, want_aux=True)

    z_again = lambda: eng.sample_fine(E.mlp_coarse(o, d, Nc, near, far), Ni, near, far)

    cases = (("plain", lambda: E.render_image(c2w, H, W, focal, hist, Nc, Ni, near, far)),
             ("maps", lambda: E.render_image_maps(c2w, H, W, focal, hist, Nc, Ni, near, far)),
             ("raw+stage", raw_route), ("z_recompute", z_again))
    for name, fn in cases:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        line = dict(case=name, median_ms=float(np.median(ms)), min_ms=min(ms), max_ms=max(ms), reps=REPS)
        if name in ("plain", "maps"):   # per-launch averages of the fine kernel (slot 1) and the segment combine (slot 4)
            E.lib.dfn_profile_enable(1)
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            for slot, key in ((1, "fine_kernel_ms"), (4, "combine_ms")):
                avg, n = ctypes.c_double(), ctypes.c_int()
                _lib.check(E.lib.dfn_profile_read(slot, ctypes.byref(avg), ctypes.byref(n)), "dfn_profile_read")
                line[key], line[key.replace("_ms", "_launches")] = avg.value, n.value
            E.lib.dfn_profile_enable(0)
        if name == "raw+stage":
            held = line
            continue
        if name == "z_recompute":
            held.update(z_recompute_ms=line["median_ms"], median_without_z_recompute_ms=held["median_ms"] - line["median_ms"])
            line = held
        print(json.dumps(line), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if "--registers" in sys.argv:
        registers()
    elif "--text-sha" in sys.argv:
        text_sha(sys.argv[sys.argv.index("--text-sha") + 1:])
    else:
        timings()
