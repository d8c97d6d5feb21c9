"""CPU-side checks of the entries behind render(ndc / c2w_staticcam, diff_view=True): the adjoints of ndc_rays and of viewdirs = d / |d|
(dfn_ndc_rays_backward, dfn_viewdirs_backward), the training forward with explicit view directions (dfn_nerfh_train_forward_v) and the two
ray backwards that return d L / d viewdirs (dfn_nerfh_train_backward_rays_v, dfn_nerfh_train_backward_rays_maps_v): declared in the header,
exported, bound in the ctypes table with one argument per parameter, and refusing bad arguments before any device work."""
import ctypes
import os
import re
import subprocess

import pytest

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dfn_ndc_rays_backward", "dfn_viewdirs_backward", "dfn_nerfh_train_forward_v", "dfn_nerfh_train_backward_rays_v",
         "dfn_nerfh_train_backward_rays_maps_v")
ONE = ctypes.c_void_p(16)      # a non-null token: never dereferenced when the call is refused (or has nothing to do) first


def test_view_grad_entries_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "dfnet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dfn_[a-z0-9_]+)\s*\(", src))
    so = os.path.join(ROOT, "dfnet_amd", "libdfnet_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.split()
    lib = _lib.load()
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/dfnet_hip.h"
        assert n in exported, f"{n} is not exported by libdfnet_hip.so"
        assert n in _lib.SIGNATURES and hasattr(lib, n), f"{n} is not in the ctypes table"
        proto = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src).group(1)
        assert len(_lib.SIGNATURES[n][1]) == len(proto.split(",")), n
    # each *_v entry is its plain form plus ONE pointer: the view directions behind rays_d, their gradient behind grad_rays_d
    P = ctypes.c_void_p
    for new, old, at in (("dfn_nerfh_train_forward_v", "dfn_nerfh_train_forward", 4), ("dfn_nerfh_train_backward_rays_v", "dfn_nerfh_train_backward_rays", 19),
                         ("dfn_nerfh_train_backward_rays_maps_v", "dfn_nerfh_train_backward_rays_maps", 17)):
        a, b = list(_lib.SIGNATURES[new][1]), list(_lib.SIGNATURES[old][1])
        assert a[:at] + a[at + 1:] == b and a[at] is P, new


def test_stage_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    ndc = lambda o, d, n, go, gd, oo, od: lib.dfn_ndc_rays_backward(6, 8, 7.3, 1., o, d, n, go, gd, oo, od, None)
    # n == 0: nothing to do, whatever the pointers are
    assert ndc(None, None, 0, None, None, None, None) == 0
    assert ndc(ONE, ONE, 0, ONE, ONE, ONE, ONE) == 0
    assert lib.dfn_viewdirs_backward(None, None, 0, 0, None, None) == 0
    assert lib.dfn_viewdirs_backward(ONE, ONE, 0, 1, ONE, None) == 0
    # a null ray or output pointer
    for args in ((None, ONE, 4, ONE, ONE, ONE, ONE), (ONE, None, 4, ONE, ONE, ONE, ONE), (ONE, ONE, 4, ONE, ONE, None, ONE),
                 (ONE, ONE, 4, ONE, ONE, ONE, None)):
        assert ndc(*args) == -1
        assert b"dfn_ndc_rays_backward" in lib.dfn_last_error()
    # both upstream gradients null (either one alone is allowed: it stands for zeros)
    assert ndc(ONE, ONE, 4, None, None, ONE, ONE) == -1
    assert b"dfn_ndc_rays_backward" in lib.dfn_last_error() and b"neither" in lib.dfn_last_error()
    # a camera that is none
    assert lib.dfn_ndc_rays_backward(0, 8, 7.3, 1., ONE, ONE, 4, ONE, ONE, ONE, ONE, None) == -1
    assert lib.dfn_ndc_rays_backward(6, 8, 0., 1., ONE, ONE, 4, ONE, ONE, ONE, ONE, None) == -1
    for args in ((None, ONE, 4, 0, ONE), (ONE, None, 4, 0, ONE), (ONE, ONE, 4, 1, None)):
        assert lib.dfn_viewdirs_backward(*args, None) == -1
        assert b"dfn_viewdirs_backward" in lib.dfn_last_error()


@pytest.fixture()
def handle():
    lib = _lib.load()
    h = ctypes.c_void_p()
    d = _lib.NerfhDesc(8, 128, 10, 4, 10, 5, 2, 1000)
    assert lib.dfn_nerfh_create(ctypes.byref(d), ctypes.byref(h)) == 0
    yield h
    lib.dfn_nerfh_destroy(h)


def test_training_entries_refuse_bad_arguments_without_a_gpu(handle):
    lib = _lib.load()
    Nc, Ni = 8, 16

    def fwd(h, params, n, o=ONE):
        return lib.dfn_nerfh_train_forward_v(h, params, o, ONE, ONE, ONE, 1, n, Nc, Ni, 0., 1., None, None, 0., None, ONE, ONE, ONE, ONE, ONE, ONE,
                                             ONE, ONE, ONE, ONE, 1 << 20, None)

    def rays(h, n, g_rgb=ONE, go=ONE, gv=ONE):
        return lib.dfn_nerfh_train_backward_rays_v(h, ONE, ONE, ONE, ONE, 1, n, Nc, Ni, None, 0., ONE, g_rgb, ONE, ONE, 0., None, go, ONE, gv,
                                                   ONE, 1 << 20, ONE, 1 << 20, None)

    def rays_maps(h, n, grads, go=ONE):
        return lib.dfn_nerfh_train_backward_rays_maps_v(h, ONE, ONE, ONE, ONE, 1, n, Nc, Ni, None, 0., ONE, grads, 0., None, go, ONE, ONE,
                                                        ONE, 1 << 20, ONE, 1 << 20, None)

    some = _lib.TrainMapGrads(rgb=16)
    # a null handle, by name
    for name, rc in (("dfn_nerfh_train_forward_v", fwd(None, None, 4)), ("dfn_nerfh_train_backward_rays_v", rays(None, 4)),
                     ("dfn_nerfh_train_backward_rays_maps_v", rays_maps(None, 4, ctypes.byref(some)))):
        assert rc == -1, name
    assert b"dfn_nerfh_train_backward_rays_maps_v: null handle" in lib.dfn_last_error()
    # no rays: DFN_OK whatever the pointers are
    assert fwd(handle, None, 0) == 0 and rays(handle, 0, None, None, None) == 0 and rays_maps(handle, 0, None, None) == 0
    # null pointers
    assert fwd(handle, None, 4) == -1 and b"dfn_nerfh_train_forward_v" in lib.dfn_last_error()
    assert fwd(handle, (ctypes.c_void_p * 64)(), 4, o=None) == -1 and b"dfn_nerfh_train_forward_v" in lib.dfn_last_error()
    assert rays(handle, 4, g_rgb=None) == -1 and b"dfn_nerfh_train_backward_rays_v" in lib.dfn_last_error()
    assert rays(handle, 4, go=None) == -1 and b"dfn_nerfh_train_backward_rays_v" in lib.dfn_last_error()
    assert rays_maps(handle, 4, ctypes.byref(some), go=None) == -1 and b"dfn_nerfh_train_backward_rays_maps_v" in lib.dfn_last_error()
    # no upstream gradient at all
    assert rays_maps(handle, 4, ctypes.byref(_lib.TrainMapGrads())) == -1
    assert b"dfn_nerfh_train_backward_rays_maps_v" in lib.dfn_last_error() and b"no upstream gradient" in lib.dfn_last_error()
    # a ray backward without an exact-mode forward on the handle: refused before any pointer is read
    assert rays(handle, 4) == -3 and b"dfn_nerfh_train_backward_rays_v" in lib.dfn_last_error()
