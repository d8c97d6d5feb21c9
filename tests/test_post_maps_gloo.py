"""render_path(ret_maps=True)'s end gather over gloo on CPU tensors: the eight-tensor list (rgb, disp, mse, the five render maps) through
the path's one grouped exchange — gather_frames_direct at world 3 with 4 frames (uneven blocks) and with 2 (a rank that owns nothing),
gather_bands_direct at world 3 with 2 frames (2 + 1 ranks on the two frames) — equals on rank 0 what a single rank holds, bit for bit,
every tensor received in place."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_COMMON = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
from dfnet_amd import dist as ddist
from dfnet_amd._lib import MAP_NAMES
rank, world, _ = ddist.init_from_env(backend="gloo")
n_frames, H, W = int(sys.argv[2]), 5, 4
assert ddist.active() and world == 3 and len(MAP_NAMES) == 5
TAILS = [(H, W, 3), (H, W)] + [(H, W, 3) if m.startswith("rgb_") else (H, W) for m in MAP_NAMES]
def frame(t, k, f):      # tensor t of the list, frame f: every element a function of (tensor, frame, row, column, channel)
    n = 1
    for s in k:
        n *= s
    return (torch.arange(n, dtype=torch.float32).reshape(k) * 0.5 + 1000. * f + 100000. * t)
'''

_FRAMES_WORKER = _COMMON + r'''
lo, hi = ddist.frame_block(n_frames, rank, world)
tails = TAILS[:2] + [()] + TAILS[2:]        # rgb, disp, mse, then the maps: render_path's order
outs, bufs = ddist.root_buffers(tails, n_frames, torch.device("cpu"))
assert len(bufs) == 8 and all(b.shape[0] == hi - lo for b in bufs)
for t, (b, k) in enumerate(zip(bufs, tails)):
    for j in range(hi - lo):
        b[j].copy_(frame(t, k, lo + j))
full, extra = ddist.gather_frames_direct(bufs, n_frames, outs=outs)
flags = ddist.all_gather_flags(rank, torch.device("cpu"))      # the flag all-gather behind it is unchanged
assert flags == list(range(world)) and extra is None
if rank == 0:
    assert len(full) == 8
    for t, (o, k) in enumerate(zip(full, tails)):
        want = torch.stack([frame(t, k, f) for f in range(n_frames)])
        assert o.shape == (n_frames,) + tuple(k) and torch.equal(o, want), t
        assert o.data_ptr() == outs[t].data_ptr()                                          # received in place
    per_frame = sum(int(torch.Size(k).numel()) for k in tails) * 4
    assert ddist.gathered_bytes(bufs, n_frames) == (n_frames - (hi - lo)) * per_frame
    print("MAPS_FRAMES_OK", n_frames)
else:
    assert full == [None] * 8 and outs is None
ddist.barrier()
torch.distributed.destroy_process_group()
'''

_BANDS_WORKER = _COMMON + r'''
assert ddist.band_mode(n_frames, world)
f, r0, r1 = ddist.band_unit(n_frames, H, rank, world)
bands = [frame(t, k, f)[r0:r1].contiguous() for t, k in enumerate(TAILS)]      # rgb, disp, then the maps: _render_path_bands' order
full = ddist.gather_bands_direct(bands, n_frames, H)
flags = ddist.all_gather_flags(rank, torch.device("cpu"))
assert flags == list(range(world))
if rank == 0:
    assert len(full) == 7
    for t, (o, k) in enumerate(zip(full, TAILS)):
        want = torch.stack([frame(t, k, g) for g in range(n_frames)])
        assert o.shape == (n_frames,) + tuple(k) and torch.equal(o, want), t
    print("MAPS_BANDS_OK", n_frames)
else:
    assert full == [None] * 7
ddist.barrier()
torch.distributed.destroy_process_group()
'''


def _run(tmp_path, worker, n_frames, port):
    script = tmp_path / "w.py"
    script.write_text(worker)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(script), ROOT, str(n_frames)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("n_frames", [4, 2])
def test_eight_tensor_list_through_the_frame_gather(tmp_path, n_frames):
    assert f"MAPS_FRAMES_OK {n_frames}" in _run(tmp_path, _FRAMES_WORKER, n_frames, 29700 + n_frames)


def test_map_bands_through_the_band_gather(tmp_path):
    assert "MAPS_BANDS_OK 2" in _run(tmp_path, _BANDS_WORKER, 2, 29707)
