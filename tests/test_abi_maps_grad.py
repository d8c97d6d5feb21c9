"""CPU-side check of the entry points of the differentiable render maps: the library exports them, the header declares them with the same
argument counts, the ctypes table carries their argument types, dfn_map_grads has the header's layout (eight pointers, header order),
and bad arguments are refused without a GPU."""
import ctypes
import inspect
import os
import re

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, S, I, F = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float
GRADS = ("rgb", "acc", "depth", "depth_static", "disp", "beta", "rgb_static", "rgb_transient")


def header():
    src = open(os.path.join(ROOT, "include", "dfnet_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def new_entries():
    M = ctypes.POINTER(_lib.MapGrads)
    return {
        # raw, z | n_rays | Nf | beta_min | grads, grad_raw_ext, grad_raw, stream
        "dfn_composite_fine_backward_maps": [P, P, S, I, F, M, P, P, P],
        # h, rays_o, rays_d, viewdirs, hist | hist_rows, n_rays | Nc, Ni | near, far | grad_rgb, grad_raw, grad_rays_o, grad_rays_d,
        # grad_viewdirs, workspace | bytes | grads, stream
        "dfn_nerfh_generic_render_rays_backward_maps": [P, P, P, P, P, S, S, I, I, F, F, P, P, P, P, P, P, S, M, P],
    }


def test_new_entries_are_exported_declared_and_bound():
    lib = _lib.load()
    _, code = header()
    protos = {m.group(2): (m.group(1), m.group(3))
              for m in re.finditer(r"\b(int|size_t)\s+(dfn_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S)}
    for name, argtypes in new_entries().items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in protos, f"{name} is not declared in include/dfnet_hip.h"
        assert protos[name][0] == "int", name
        assert len([a for a in protos[name][1].split(",") if a.strip()]) == len(argtypes), name
        res, table = _lib.SIGNATURES[name]
        assert res is I and list(table) == argtypes, name
        assert list(getattr(lib, name).argtypes) == argtypes and getattr(lib, name).restype is I, name
        assert "const dfn_map_grads*" in protos[name][1], name
    # the generic entry is dfn_nerfh_generic_render_rays_backward_raw plus `grads` in front of the stream; that entry keeps its signature
    a, b = list(_lib.SIGNATURES["dfn_nerfh_generic_render_rays_backward_maps"][1]), list(_lib.SIGNATURES["dfn_nerfh_generic_render_rays_backward_raw"][1])
    assert a[:-2] == b[:-1] and a[-1] is b[-1] and len(b) == 19
    assert len(_lib.SIGNATURES["dfn_composite_fine_backward"][1]) == 7


def test_every_new_entry_cites_the_reference():
    src, _ = header()
    for name in new_entries():
        at = src.index(name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        assert "rendering.py:" in comment, f"{name}: the comment in front of it cites no reference line"


def test_struct_layout_matches_the_header():
    _, code = header()
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*dfn_map_grads\s*;", code)
    assert m, "dfn_map_grads is not declared"
    members = [n.strip() for n in re.sub(r"\b(const|float)\b", "", m.group(1)).replace(";", ",").replace("*", "").split(",") if n.strip()]
    assert tuple(members) == GRADS
    assert [n for n, _ in _lib.MapGrads._fields_] == list(GRADS)
    assert all(t is ctypes.c_void_p for _, t in _lib.MapGrads._fields_)
    assert ctypes.sizeof(_lib.MapGrads) == 8 * ctypes.sizeof(ctypes.c_void_p)
    for i, n in enumerate(GRADS):
        assert getattr(_lib.MapGrads, n).offset == i * ctypes.sizeof(ctypes.c_void_p)
    st = _lib.MapGrads()
    assert all(getattr(st, n) is None for n in GRADS)   # a fresh struct is eight NULLs


def test_bad_arguments_without_a_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # a non-null token: never dereferenced, every call below is refused or returns before any device work
    none, some = _lib.MapGrads(), _lib.MapGrads(acc=16)
    call = lib.dfn_composite_fine_backward_maps
    assert call(one, one, 4, 8, 0.1, ctypes.byref(none), None, one, None) == -1      # eight NULLs and no grad_raw_ext
    assert b"dfn_composite_fine_backward_maps" in lib.dfn_last_error()
    assert call(one, one, 4, 8, 0.1, None, None, one, None) == -1                    # no struct at all, no grad_raw_ext
    for Nf in (0, 513, -1):
        assert call(one, one, 4, Nf, 0.1, ctypes.byref(some), None, one, None) == -1
    assert call(None, one, 4, 8, 0.1, ctypes.byref(some), None, one, None) == -1     # raw
    assert call(one, None, 4, 8, 0.1, ctypes.byref(some), None, one, None) == -1     # z
    assert call(one, one, 4, 8, 0.1, ctypes.byref(some), None, None, None) == -1     # grad_raw
    assert call(one, one, 0, 8, 0.1, ctypes.byref(some), None, one, None) == 0       # no rays: nothing to do
    assert call(one, one, 0, 512, 0.1, ctypes.byref(none), one, one, None) == 0      # grad_raw_ext alone is a valid request
    gen = lib.dfn_nerfh_generic_render_rays_backward_maps
    assert gen(None, one, one, None, one, 1, 4, 8, 8, 0., 1., None, None, one, one, None, one, 0, ctypes.byref(some), None) == -1
    assert b"dfn_nerfh_generic_render_rays_backward_maps" in lib.dfn_last_error()
    h = ctypes.c_void_p()
    d = _lib.NerfhDesc(8, 32, 10, 4, 10, 5, 2, 1000)
    assert lib.dfn_nerfh_create(ctypes.byref(d), ctypes.byref(h)) == 0
    try:   # an uncommitted handle refuses to run, under the name of the entry that was called
        assert gen(h, one, one, None, one, 1, 4, 8, 8, 0., 1., None, None, one, one, None, one, 0, ctypes.byref(some), None) == -3
        assert b"dfn_nerfh_generic_render_rays_backward_maps:" in lib.dfn_last_error()
    finally:
        lib.dfn_nerfh_destroy(h)


def test_python_surface():
    from dfnet_amd import engine, rendering
    assert engine.GRAD_NAMES == GRADS
    assert callable(engine.composite_fine_backward_maps) and callable(engine.NerfHEngine.composite_fine_backward_maps)
    assert inspect.signature(engine.NerfHEngine.render_rays_backward).parameters["grad_maps"].default is None
    assert inspect.signature(engine.NerfHEngine.backward_from_saved).parameters["graw"].default is None
    assert inspect.signature(rendering.render).parameters["diff_maps"].default is False
