"""CPU-side checks of dfn_nerfh_points_train_workspace_bytes / _forward / _backward (a training query on points: one network of NeRF-H
under autograd with respect to its parameters): declared in the header with the documented argument lists, exported, bound in the
ctypes table with matching arity, refusing without a device what they can refuse there, and a workspace size that needs no device
(as tests/test_abi_coarse_static_points.py)."""
import ctypes
import os
import re
import subprocess

import pytest

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, Z, PP = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)
ENTRIES = {
    "dfn_nerfh_points_train_workspace_bytes": (
        "size_t", ("dfn_nerfh_t h", "int net", "size_t n_rows", "int N"), [P, I, Z, I]),
    "dfn_nerfh_points_train_forward": (
        "int", ("dfn_nerfh_t h", "int net", "const float* const* params", "const float* pts", "const float* viewdirs", "const float* hist",
                "size_t hist_rows", "size_t n_rows", "int N", "float* raw", "void* workspace", "size_t workspace_bytes", "void* stream"),
        [P, I, PP, P, P, P, Z, Z, I, P, P, Z, P]),
    "dfn_nerfh_points_train_backward": (
        "int", ("dfn_nerfh_t h", "int net", "const float* const* params", "const float* hist", "size_t hist_rows", "size_t n_rows", "int N",
                "const float* raw", "const float* grad_raw", "float* const* grads", "void* workspace", "size_t workspace_bytes",
                "void* stream"),
        [P, I, PP, P, Z, Z, I, P, P, PP, P, Z, P]),
}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_declared_exported_and_bound(name):
    res, proto, argtypes = ENTRIES[name]
    raw = open(os.path.join(ROOT, "include", "dfnet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\b" + res + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/dfnet_hip.h"
    assert tuple(" ".join(a.split()) for a in m.group(1).split(",")) == proto
    # the comment in front of the declarations cites the reference lines they replace, and names the two networks
    doc = raw[:raw.index(res + " " + name + "(")].rsplit("/*", 1)[1]
    assert "nerfw.py:47-95, 297-354" in doc
    assert re.search(r"enum\s*\{\s*DFN_NET_COARSE\s*=\s*0\s*,\s*DFN_NET_FINE\s*=\s*1\s*\}\s*;", src)
    assert (_lib.DFN_NET_COARSE, _lib.DFN_NET_FINE) == (0, 1)
    so = os.path.join(ROOT, "dfnet_amd", "libdfnet_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.split()
    assert name in exported, f"{name} is not exported by libdfnet_hip.so"
    lib = _lib.load()
    assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not in the ctypes table"
    assert _lib.SIGNATURES[name] == (ctypes.c_size_t if res == "size_t" else ctypes.c_int, argtypes) and len(argtypes) == len(proto)


def _calls(lib):
    """(name, call(h, net, n_rows, p)) of the two entries that return a status; p stands for every pointer."""
    fwd = lambda h, net, n_rows, p: lib.dfn_nerfh_points_train_forward(h, net, ctypes.cast(p, PP), p, p, p, 1, n_rows, 8, p, p, 1 << 20, None)
    bwd = lambda h, net, n_rows, p: lib.dfn_nerfh_points_train_backward(h, net, ctypes.cast(p, PP), p, 1, n_rows, 8, p, p, ctypes.cast(p, PP), p,
                                                                         1 << 20, None)
    return (("dfn_nerfh_points_train_forward", fwd), ("dfn_nerfh_points_train_backward", bwd))


def test_entries_refuse_null_and_uncommitted_handles_without_a_gpu():
    """The handle comes first, as in the sibling point entries: a null handle is DFN_ERR_ARG (-1), a created but uncommitted one
    DFN_ERR_STATE (-3) -- also with no rows to evaluate, with null pointers and with an unknown net -- each with a message that names
    the entry.  (What needs a committed handle is in test_gpu_points_train.py: dfn_nerfh_commit uploads to the device.)"""
    lib = _lib.load()
    one = ctypes.c_void_p(16)      # a non-null token: never dereferenced when the handle is refused first
    h = ctypes.c_void_p()
    d = _lib.NerfhDesc(8, 128, 10, 4, 10, 5, 2, 1000)
    assert lib.dfn_nerfh_create(ctypes.byref(d), ctypes.byref(h)) == 0
    try:
        for name, call in _calls(lib):
            for net in (_lib.DFN_NET_COARSE, _lib.DFN_NET_FINE):
                assert call(None, net, 4, one) == -1
                assert name.encode() + b": null handle" in lib.dfn_last_error()
            for net in (_lib.DFN_NET_COARSE, _lib.DFN_NET_FINE, 7):
                assert call(h, net, 4, one) == -3
                assert name.encode() in lib.dfn_last_error() and b"dfn_nerfh_commit" in lib.dfn_last_error()
            assert call(h, _lib.DFN_NET_FINE, 0, one) == -3
            assert call(h, _lib.DFN_NET_FINE, 4, None) == -3
    finally:
        lib.dfn_nerfh_destroy(h)


def test_workspace_size_needs_no_device_and_follows_the_point_count_and_the_planes():
    """dfn_nerfh_points_train_workspace_bytes reads the handle's geometry and train mode only: positive, monotone in n_rows * N, and in
    the default mode larger per point for the coarse network (its stored operands are hi | lo planes, the fine network's one plane);
    under DFN_TRAIN_FUSED_SPLIT the fine network stores two planes of more arrays and is the larger one.  0 for what cannot be sized."""
    lib = _lib.load()
    size = lib.dfn_nerfh_points_train_workspace_bytes
    h = ctypes.c_void_p()
    d = _lib.NerfhDesc(8, 128, 10, 4, 10, 5, 2, 1000)
    assert lib.dfn_nerfh_create(ctypes.byref(d), ctypes.byref(h)) == 0
    try:
        C, F = _lib.DFN_NET_COARSE, _lib.DFN_NET_FINE
        shapes = [(1, 1), (3, 37), (5, 64), (2, 300), (64, 64), (1536, 64), (1536, 192)]
        for net in (C, F):
            sizes = [size(h, net, r, n) for r, n in sorted(shapes, key=lambda s: s[0] * s[1])]
            assert all(s > 0 for s in sizes)
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
            assert sizes[0] < sizes[-1]
        P0, P1 = 256 * 64, 256 * 640       # whole tiles: the difference is the per-point part (stored arrays, masks, scales)
        per_point = lambda net: (size(h, net, 256, 640) - size(h, net, 256, 64)) / (P1 - P0)
        assert per_point(C) > per_point(F) > 0
        assert lib.dfn_nerfh_set_train_mode(h, 2) == 0
        assert per_point(F) > per_point(C)
        assert lib.dfn_nerfh_set_train_mode(h, 0) == 0
        assert size(None, F, 4, 8) == 0 and size(h, 7, 4, 8) == 0 and size(h, F, 4, 0) == 0
        assert size(h, F, 1 << 30, 4) == 0    # n_rows * N >= 2^31
    finally:
        lib.dfn_nerfh_destroy(h)
