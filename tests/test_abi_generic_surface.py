"""CPU-side check of the two generic-width entry points added for render(retraw=True) under autograd and explicit view directions:
the library exports them, the header declares them, the ctypes table carries their argument types, and they refuse bad arguments
without a GPU."""
import ctypes
import os
import re

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, S, I, F = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float
NEW = {
    # h, rays_o, rays_d, viewdirs, hist | hist_rows, n_rays | Nc, Ni | near, far | rgb, disp, acc, raw, workspace | bytes | stream
    "dfn_nerfh_generic_render_rays_v": [P, P, P, P, P, S, S, I, I, F, F, P, P, P, P, P, S, P],
    # ... | grad_rgb, grad_raw, grad_rays_o, grad_rays_d, grad_viewdirs, workspace | bytes | stream
    "dfn_nerfh_generic_render_rays_backward_raw": [P, P, P, P, P, S, S, I, I, F, F, P, P, P, P, P, P, S, P],
}


def header_prototypes():
    src = open(os.path.join(ROOT, "include", "dfnet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(dfn_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_new_generic_entries_are_exported_declared_and_bound():
    lib = _lib.load()
    protos = header_prototypes()
    for name, argtypes in NEW.items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in protos, f"{name} is not declared in include/dfnet_hip.h"
        assert len([a for a in protos[name].split(",") if a.strip()]) == len(argtypes), name
        restype, table = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and list(table) == argtypes, name
        assert list(getattr(lib, name).argtypes) == argtypes, name
    # the parameter names the callers rely on, in the header
    assert "viewdirs" in protos["dfn_nerfh_generic_render_rays_v"]
    assert re.search(r"grad_rgb\s*,\s*const float\*\s*grad_raw\s*,\s*float\*\s*grad_rays_o", protos["dfn_nerfh_generic_render_rays_backward_raw"])
    # the two earlier entries keep their signatures
    assert len(_lib.SIGNATURES["dfn_nerfh_generic_render_rays"][1]) == 17
    assert len(_lib.SIGNATURES["dfn_nerfh_generic_render_rays_backward"][1]) == 18


def test_new_generic_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # a non-null token: never dereferenced, every call below is refused before any device work
    assert lib.dfn_nerfh_generic_render_rays_v(None, one, one, None, one, 1, 4, 8, 8, 0., 1., one, one, one, one, one, 0, None) == -1
    assert b"dfn_nerfh_generic_render_rays_v" in lib.dfn_last_error()
    assert lib.dfn_nerfh_generic_render_rays_backward_raw(None, one, one, None, one, 1, 4, 8, 8, 0., 1., one, one, one, one, None, one, 0, None) == -1
    assert b"dfn_nerfh_generic_render_rays_backward_raw" in lib.dfn_last_error()
    h = ctypes.c_void_p()
    d = _lib.NerfhDesc(8, 32, 10, 4, 10, 5, 2, 1000)
    assert lib.dfn_nerfh_create(ctypes.byref(d), ctypes.byref(h)) == 0
    try:   # an uncommitted handle refuses to run, under the name of the entry that was called
        assert lib.dfn_nerfh_generic_render_rays_v(h, one, one, one, one, 1, 4, 8, 8, 0., 1., one, one, one, one, one, 0, None) == -3
        assert b"dfn_nerfh_generic_render_rays_v:" in lib.dfn_last_error()
        assert lib.dfn_nerfh_generic_render_rays_backward_raw(h, one, one, None, one, 1, 4, 8, 8, 0., 1., None, one, one, one, None, one, 0,
                                                              None) == -3
        assert b"dfn_nerfh_generic_render_rays_backward_raw:" in lib.dfn_last_error()
        assert lib.dfn_nerfh_generic_render_rays(h, one, one, one, 1, 4, 8, 8, 0., 1., one, one, one, one, one, 0, None) == -3
        assert b"dfn_nerfh_generic_render_rays:" in lib.dfn_last_error()
    finally:
        lib.dfn_nerfh_destroy(h)
