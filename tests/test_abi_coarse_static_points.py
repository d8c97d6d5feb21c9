"""CPU-side checks of dfn_mlp_coarse_static_points / dfn_mlp_coarse_static_points_backward (the coarse network's training query on
points and autograd through it): declared in the header with the documented argument lists, exported, bound in the ctypes table with
matching arity, and refusing without a device what they can refuse there (as tests/test_abi_coarse_points_grad.py)."""
import ctypes
import os
import re
import subprocess

import pytest

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
ENTRIES = {
    "dfn_mlp_coarse_static_points": (
        ("dfn_nerfh_t h", "int prec", "const float* pts", "const float* viewdirs", "size_t n_rows", "int N", "float* raw4",
         "void* bias_table", "void* stream"),
        [P, I, P, P, Z, I, P, P, P]),
    "dfn_mlp_coarse_static_points_backward": (
        ("dfn_nerfh_t h", "int prec", "const float* pts", "const float* viewdirs", "size_t n_rows", "int N", "const float* grad_raw4",
         "float* grad_pts6", "void* bias_table", "void* stream"),
        [P, I, P, P, Z, I, P, P, P, P]),
}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_declared_exported_and_bound(name):
    proto, argtypes = ENTRIES[name]
    raw = open(os.path.join(ROOT, "include", "dfnet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/dfnet_hip.h"
    assert tuple(" ".join(a.split()) for a in m.group(1).split(",")) == proto
    # the comment in front of the declaration cites the reference lines it replaces
    doc = raw[:raw.index("int " + name + "(")].rsplit("/*", 1)[1]
    assert "nerfw.py:47-60, 326-343" in doc
    so = os.path.join(ROOT, "dfnet_amd", "libdfnet_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.split()
    assert name in exported, f"{name} is not exported by libdfnet_hip.so"
    lib = _lib.load()
    assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not in the ctypes table"
    assert _lib.SIGNATURES[name] == (ctypes.c_int, argtypes) and len(argtypes) == len(proto)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_refuses_null_and_uncommitted_handles_without_a_gpu(name):
    """check_net comes first, as in the sibling point entries: a null handle is DFN_ERR_ARG (-1), a created but uncommitted one
    DFN_ERR_STATE (-3) -- also with no rows to evaluate and with null pointers -- each with a message that names the entry.  (What
    needs a committed handle is in test_gpu_coarse_static_points.py: dfn_nerfh_commit uploads to the device.)"""
    lib = _lib.load()
    fn = getattr(lib, name)
    one = ctypes.c_void_p(16)      # a non-null token: never dereferenced when the handle is refused first
    extra = (one,) if name.endswith("_backward") else ()
    call = lambda h, prec, n_rows, p: fn(h, prec, p, p, n_rows, 8, p, *((p,) * len(extra)), p, None)
    for prec in (_lib.DFN_PREC_F16, _lib.DFN_PREC_F32, _lib.DFN_PREC_F16X3):
        assert call(None, prec, 4, one) == -1
    assert name.encode() + b": null handle" in lib.dfn_last_error()
    h = ctypes.c_void_p()
    d = _lib.NerfhDesc(8, 128, 10, 4, 10, 5, 2, 1000)
    assert lib.dfn_nerfh_create(ctypes.byref(d), ctypes.byref(h)) == 0
    try:
        for prec in (_lib.DFN_PREC_F16, _lib.DFN_PREC_F32, _lib.DFN_PREC_F16X3, 7):
            assert call(h, prec, 4, one) == -3
            assert name.encode() in lib.dfn_last_error() and b"dfn_nerfh_commit" in lib.dfn_last_error()
        assert call(h, _lib.DFN_PREC_F32, 0, one) == -3
        assert call(h, _lib.DFN_PREC_F32, 4, None) == -3
    finally:
        lib.dfn_nerfh_destroy(h)
