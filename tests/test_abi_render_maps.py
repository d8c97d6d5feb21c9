"""CPU-side check of the render-maps entry points: the library exports them, the header declares them with the same argument counts,
the ctypes table carries their argument types, dfn_render_maps has the header's layout, and bad arguments are refused without a GPU."""
import ctypes
import os
import re

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, S, I, F = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float
M = ctypes.POINTER(_lib.RenderMaps)
NEW = {
    # h, prec, rays_o, rays_d, viewdirs, hist | hist_rows, n_rays | Nc, Ni | near, far | rgb, disp, acc, raw, workspace | bytes | maps, stream
    "dfn_render_rays_maps": (I, [P, I, P, P, P, P, S, S, I, I, F, F, P, P, P, P, P, S, M, P]),
    # h, prec, c2w | H, W | focal, near, far | Nc, Ni | hist, rgb, disp, acc, workspace | bytes | maps, stream
    "dfn_render_image_maps": (I, [P, I, P, I, I, F, F, F, I, I, P, P, P, P, P, S, M, P]),
    # h, rays_o, rays_d, viewdirs, hist | hist_rows, n_rays | Nc, Ni | near, far | rgb, disp, acc, raw, workspace | bytes | maps, stream
    "dfn_nerfh_generic_render_rays_maps": (I, [P, P, P, P, P, S, S, I, I, F, F, P, P, P, P, P, S, M, P]),
    # raw, z | n_rays | Nf | beta_min | maps, stream
    "dfn_composite_fine_maps": (I, [P, P, S, I, F, M, P]),
    "dfn_render_maps_workspace_bytes": (S, [S, I, I]),
}
MAPS = ("depth", "depth_static", "beta", "rgb_static", "rgb_transient")


def header():
    src = open(os.path.join(ROOT, "include", "dfnet_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_new_entries_are_exported_declared_and_bound():
    lib = _lib.load()
    _, code = header()
    protos = {m.group(2): (m.group(1), m.group(3))
              for m in re.finditer(r"\b(int|size_t)\s+(dfn_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S)}
    for name, (restype, argtypes) in NEW.items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in protos, f"{name} is not declared in include/dfnet_hip.h"
        assert protos[name][0] == ("int" if restype is I else "size_t"), name
        assert len([a for a in protos[name][1].split(",") if a.strip()]) == len(argtypes), name
        res, table = _lib.SIGNATURES[name]
        assert res is restype and list(table) == argtypes, name
        assert list(getattr(lib, name).argtypes) == argtypes and getattr(lib, name).restype is restype, name
        if restype is I:
            assert re.search(r"const dfn_render_maps\*\s*maps\s*,\s*void\*\s*stream\s*$", protos[name][1].strip()), name
    # each maps entry is the plain entry plus `maps`; the plain entries keep their signatures
    for new, old in (("dfn_render_rays_maps", "dfn_render_rays"), ("dfn_render_image_maps", "dfn_render_image"),
                     ("dfn_nerfh_generic_render_rays_maps", "dfn_nerfh_generic_render_rays_v")):
        a, b = list(_lib.SIGNATURES[new][1]), list(_lib.SIGNATURES[old][1])
        assert a[:-2] == b[:-1] and a[-1] is b[-1] and a[-2] is M, (new, old)
    assert len(_lib.SIGNATURES["dfn_render_rays"][1]) == 19 and len(_lib.SIGNATURES["dfn_render_image"][1]) == 17
    assert len(_lib.SIGNATURES["dfn_composite_fine"][1]) == 13


def test_every_new_entry_cites_the_reference():
    src, _ = header()
    for name in NEW:
        at = src.index(name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        assert "rendering.py:" in comment, f"{name}: the comment in front of it cites no reference line"


def test_struct_layout_matches_the_header():
    _, code = header()
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*dfn_render_maps\s*;", code)
    assert m, "dfn_render_maps is not declared"
    members = [n.strip() for n in re.sub(r"\bfloat\b", "", m.group(1)).replace(";", ",").replace("*", "").split(",") if n.strip()]
    assert tuple(members) == MAPS == _lib.MAP_NAMES
    assert [n for n, _ in _lib.RenderMaps._fields_] == list(MAPS)
    assert all(t is ctypes.c_void_p for _, t in _lib.RenderMaps._fields_)
    assert ctypes.sizeof(_lib.RenderMaps) == 5 * ctypes.sizeof(ctypes.c_void_p)
    for i, n in enumerate(MAPS):
        assert getattr(_lib.RenderMaps, n).offset == i * ctypes.sizeof(ctypes.c_void_p)
    st = _lib.RenderMaps()
    assert all(getattr(st, n) is None for n in MAPS)   # a fresh struct is five NULLs


def test_workspace_and_bad_arguments_without_a_gpu():
    lib = _lib.load()
    for n, Nc, Ni in ((1, 8, 16), (5000, 64, 128), (70000, 64, 100)):
        plain, maps = lib.dfn_render_workspace_bytes(n, Nc, Ni), lib.dfn_render_maps_workspace_bytes(n, Nc, Ni)
        assert maps >= plain > 0   # the 16-float segment records of the maps flavour
    one = ctypes.c_void_p(16)   # a non-null token: never dereferenced, every call below is refused before any device work
    st = _lib.RenderMaps(depth=16)
    assert lib.dfn_render_rays_maps(None, 2, one, one, None, one, 1, 4, 8, 8, 0., 1., one, one, one, None, one, 0, ctypes.byref(st), None) == -1
    assert b"dfn_render_rays_maps" in lib.dfn_last_error()
    assert lib.dfn_render_image_maps(None, 2, one, 4, 4, 1., 0., 1., 8, 8, one, one, one, one, one, 0, ctypes.byref(st), None) == -1
    assert b"dfn_render_image_maps" in lib.dfn_last_error()
    assert lib.dfn_nerfh_generic_render_rays_maps(None, one, one, None, one, 1, 4, 8, 8, 0., 1., one, one, one, one, one, 0, ctypes.byref(st), None) == -1
    assert b"dfn_nerfh_generic_render_rays_maps" in lib.dfn_last_error()
    assert lib.dfn_composite_fine_maps(None, one, 4, 8, 0.1, ctypes.byref(st), None) == -1
    assert lib.dfn_composite_fine_maps(one, one, 4, 513, 0.1, ctypes.byref(st), None) == -1
    assert b"dfn_composite_fine_maps" in lib.dfn_last_error()
    h = ctypes.c_void_p()
    d = _lib.NerfhDesc(8, 128, 10, 4, 10, 5, 2, 1000)
    assert lib.dfn_nerfh_create(ctypes.byref(d), ctypes.byref(h)) == 0
    try:   # an uncommitted handle refuses to run, under the name of the entry that was called
        assert lib.dfn_render_rays_maps(h, 2, one, one, None, one, 1, 4, 8, 8, 0., 1., one, one, one, None, one, 0, ctypes.byref(st), None) == -3
        assert b"dfn_render_rays_maps:" in lib.dfn_last_error()
        assert lib.dfn_render_image_maps(h, 2, one, 4, 4, 1., 0., 1., 8, 8, one, one, one, one, one, 0, None, None) == -3
        assert b"dfn_render_image_maps:" in lib.dfn_last_error()
        assert lib.dfn_render_rays(h, 2, one, one, None, one, 1, 4, 8, 8, 0., 1., one, one, one, None, one, 0, None) == -3
        assert b"dfn_render_rays:" in lib.dfn_last_error()
        assert lib.dfn_nerfh_generic_render_rays_maps(h, one, one, None, one, 1, 4, 8, 8, 0., 1., one, one, one, one, one, 0, ctypes.byref(st), None) == -3
        assert b"dfn_nerfh_generic_render_rays_maps:" in lib.dfn_last_error()
    finally:
        lib.dfn_nerfh_destroy(h)


def test_map_name_selection():
    from dfnet_amd.engine import map_names
    import pytest
    assert map_names(True) == MAPS and map_names(False) == () and map_names(None) == ()
    assert map_names(["rgb_static", "depth"]) == ("depth", "rgb_static") and map_names("beta") == ("beta",)
    with pytest.raises(ValueError, match="unknown render map"):
        map_names(("depth", "weights"))
