"""CPU-side checks of the render maps' frame back-end (dfn_frame_post_maps) and what render_path(ret_maps=...) adds on the host: the two
entries are exported, declared and bound, every refusal of the header's rules comes back as DFN_ERR_ARG without a GPU, the 16-bit gray
PNG writer round-trips through both of its paths, and --render_maps parses."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
ONE = 16                      # a non-null token: never dereferenced, every refused call returns before any device work
OUT_OF = {"depth16": "depth", "depth_static16": "depth_static", "beta8": "beta", "rgb_static8": "rgb_static", "rgb_transient8": "rgb_transient"}


def test_entries_are_exported_declared_and_bound():
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfnet_hip.h")).read(), flags=re.S)
    protos = {m.group(2): (m.group(1), m.group(3))
              for m in re.finditer(r"\b(int|size_t)\s+(dfn_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}
    want = {"dfn_frame_post_maps_scratch_bytes": (ctypes.c_size_t, [I]),
            "dfn_frame_post_maps": (I, [ctypes.POINTER(_lib.RenderMaps), P, I, I, I, I, F, F, ctypes.POINTER(_lib.FrameMapsOut), P, P, P, P])}
    for name, (res, args) in want.items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in protos, f"{name} is not declared in include/dfnet_hip.h"
        assert len([a for a in protos[name][1].split(",") if a.strip()]) == len(args), name
        assert _lib.SIGNATURES[name] == (res, args), name
        assert list(getattr(lib, name).argtypes) == args and getattr(lib, name).restype is res, name
    # dfn_frame_maps_out: five pointers in the header's order, the outputs of dfn_render_maps' members in that struct's order
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*dfn_frame_maps_out\s*;", src).group(1)
    assert re.findall(r"\*\s*([a-z0-9_]+)", body) == [n for n, _ in _lib.FrameMapsOut._fields_] == list(OUT_OF)
    assert [OUT_OF[n] for n, _ in _lib.FrameMapsOut._fields_] == list(_lib.MAP_NAMES)
    assert ctypes.sizeof(_lib.FrameMapsOut) == 5 * ctypes.sizeof(P)


def _call(lib, maps=(), outs=(), gt=None, n=2, H=4, W=4, near=0.25, far=2.5, beta_max=None, mse_static=None, scratch=ONE):
    m = _lib.RenderMaps(**{k: ONE for k in maps})
    o = _lib.FrameMapsOut(**{k: ONE for k in outs})
    return lib.dfn_frame_post_maps(ctypes.byref(m), gt, 1, n, H, W, near, far, ctypes.byref(o), beta_max, mse_static, scratch, None)


def test_bad_arguments_are_refused_without_a_gpu():
    lib = _lib.load()
    every = tuple(_lib.MAP_NAMES)
    bad = {f"{o} without maps->{m}": _call(lib, maps=tuple(k for k in every if k != m), outs=(o,)) for o, m in OUT_OF.items()}
    bad.update({
        "beta_max without maps->beta": _call(lib, maps=("depth",), beta_max=ONE),
        "mse_static without gt": _call(lib, maps=every, mse_static=ONE),
        "mse_static without maps->rgb_static": _call(lib, maps=("depth", "rgb_transient"), gt=ONE, mse_static=ONE),
        "far == near": _call(lib, maps=every, outs=("depth16",), near=1.0, far=1.0),
        "far < near": _call(lib, maps=every, outs=("depth16",), near=2.0, far=1.0),
        "n_frames < 0": _call(lib, maps=every, outs=("depth16",), n=-1),
        "n_frames > 65535": _call(lib, maps=every, outs=("depth16",), n=65536),
        "H < 1": _call(lib, maps=every, outs=("depth16",), H=0),
        "W < 1": _call(lib, maps=every, outs=("depth16",), W=0),
        "scratch NULL": _call(lib, maps=every, outs=("depth16",), scratch=None),
    })
    assert all(rc == -1 for rc in bad.values()), bad
    assert b"dfn_frame_post_maps" in lib.dfn_last_error()
    # no frame: DFN_OK whatever else is given; nothing asked for: DFN_OK with no launch (this box has no device to launch on)
    assert _call(lib, maps=every, outs=tuple(OUT_OF), gt=ONE, n=0, beta_max=ONE, mse_static=ONE) == 0
    assert _call(lib, n=0, scratch=None) == 0
    assert _call(lib) == 0 and _call(lib, maps=every) == 0
    assert lib.dfn_frame_post_maps(None, None, 0, 3, 4, 4, 0.0, 1.0, None, None, None, ONE, None) == 0
    sizes = [lib.dfn_frame_post_maps_scratch_bytes(n) for n in (0, 1, 2, 16, 17, 1000, 65535)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[1]


def _u16_pattern():
    a = (np.arange(7 * 9, dtype=np.uint32).reshape(7, 9) * 1031 % 65536).astype(np.uint16)
    a.reshape(-1)[:5] = [0, 1, 255, 256, 65535]
    return a


def test_png_16_bit_gray_round_trips_through_both_writers(tmp_path):
    from PIL import Image
    from dfnet_amd import rendering
    a = _u16_pattern()
    # the zlib writer (what _write_png falls back to without PIL): bit depth 16, gray, big-endian samples
    blob = rendering._png_bytes(a)
    assert blob[:8] == b"\x89PNG\r\n\x1a\n" and blob[12:16] == b"IHDR" and blob[24] == 16 and blob[25] == 0
    back = np.asarray(Image.open(io.BytesIO(blob)))
    assert back.dtype == np.uint16 and np.array_equal(back, a)
    # the PIL path (mode I;16)
    rendering._write_png(str(tmp_path / "d.png"), a)
    img = Image.open(tmp_path / "d.png")
    assert img.mode == "I;16"
    back = np.asarray(img)
    assert back.dtype == np.uint16 and np.array_equal(back, a)
    # 8-bit gray and RGB stay what they were, in both writers
    g = (np.arange(6 * 5).reshape(6, 5) * 9 % 256).astype(np.uint8)
    c = (np.arange(6 * 5 * 3).reshape(6, 5, 3) * 7 % 256).astype(np.uint8)
    for arr in (g, c):
        blob = rendering._png_bytes(arr)
        assert blob[24] == 8 and blob[25] == (2 if arr.ndim == 3 else 0)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(blob))), arr)
        rendering._write_png(str(tmp_path / "e.png"), arr)
        assert np.array_equal(np.asarray(Image.open(tmp_path / "e.png")), arr)
    with pytest.raises(ValueError):
        rendering._png_bytes(np.zeros((2, 2, 3), np.uint16))


def test_render_maps_flag_parses_in_all_three_parsers():
    from dfnet_amd import options
    for parser in (options.nerf_parser, options.feature_parser, options.dm_parser):
        assert parser().parse_args([]).render_maps == ""
        assert parser().parse_args(["--render_maps", "beta,depth"]).render_maps == "beta,depth"
    assert options.render_map_names("") == ()
    assert options.render_map_names("all") == tuple(_lib.MAP_NAMES) and len(_lib.MAP_NAMES) == 5
    assert options.render_map_names("rgb_static, depth") == ("depth", "rgb_static")      # the library's order
    with pytest.raises(ValueError, match="unknown render map"):
        options.render_map_names("depth,normals")
