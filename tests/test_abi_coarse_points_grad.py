"""CPU-side checks of dfn_mlp_coarse_points_backward (autograd through the test-time coarse query into its points): declared in the
header with the documented argument list, exported, bound in the ctypes table, and refusing without a device what it can refuse there."""
import ctypes
import os
import re
import subprocess

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dfn_mlp_coarse_points_backward"
PROTO = ("dfn_nerfh_t h", "int prec", "const float* pts", "size_t n_rows", "int N", "const float* grad_sigma", "float* grad_pts",
         "void* stream")


def test_entry_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "dfnet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{NAME} is not declared in include/dfnet_hip.h"
    assert tuple(" ".join(a.split()) for a in m.group(1).split(",")) == PROTO
    so = os.path.join(ROOT, "dfnet_amd", "libdfnet_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.split()
    assert NAME in exported, f"{NAME} is not exported by libdfnet_hip.so"
    lib = _lib.load()
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME), f"{NAME} is not in the ctypes table"
    P = ctypes.c_void_p
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, [P, ctypes.c_int, P, ctypes.c_size_t, ctypes.c_int, P, P, P])


def test_entry_refuses_null_and_uncommitted_handles_without_a_gpu():
    """check_net comes first, as in dfn_mlp_fine_points_backward: a null handle is DFN_ERR_ARG (-1), a created but uncommitted one
    DFN_ERR_STATE (-3) -- also with no rows to evaluate -- and an unknown precision on it is refused as well, each with a message that
    names the entry.  (What needs a committed handle -- plain f16, netwidth 256, null pointers, n_rows == 0 -- is in
    test_gpu_coarse_points_grad.py: dfn_nerfh_commit uploads to the device.)"""
    lib = _lib.load()
    fn = getattr(lib, NAME)
    one = ctypes.c_void_p(16)      # a non-null token: never dereferenced when the handle is refused first
    for prec in (_lib.DFN_PREC_F16, _lib.DFN_PREC_F32, _lib.DFN_PREC_F16X3):
        assert fn(None, prec, one, 4, 8, one, one, None) == -1
    assert NAME.encode() + b": null handle" in lib.dfn_last_error()
    h = ctypes.c_void_p()
    d = _lib.NerfhDesc(8, 128, 10, 4, 10, 5, 2, 1000)
    assert lib.dfn_nerfh_create(ctypes.byref(d), ctypes.byref(h)) == 0
    try:
        for prec in (_lib.DFN_PREC_F16, _lib.DFN_PREC_F32, _lib.DFN_PREC_F16X3, 7):
            assert fn(h, prec, one, 4, 8, one, one, None) == -3
            assert NAME.encode() in lib.dfn_last_error() and b"dfn_nerfh_commit" in lib.dfn_last_error()
        assert fn(h, _lib.DFN_PREC_F32, one, 0, 8, one, one, None) == -3
        assert fn(h, _lib.DFN_PREC_F32, None, 4, 8, None, None, None) == -3
    finally:
        lib.dfn_nerfh_destroy(h)
