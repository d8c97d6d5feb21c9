"""CPU-side checks of the point-query entries (dfn_mlp_coarse_points, dfn_mlp_fine_points, dfn_mlp_fine_points_backward): declared in
the header, exported, bound in the ctypes table, and refusing a null or an uncommitted handle before any device work."""
import ctypes
import os
import re
import subprocess

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dfn_mlp_coarse_points", "dfn_mlp_fine_points", "dfn_mlp_fine_points_backward")


def test_point_entries_declared_exported_and_bound():
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
    # one argument per parameter of the header's prototype
    for n in NAMES:
        proto = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src).group(1)
        assert len(_lib.SIGNATURES[n][1]) == len(proto.split(",")), n


def test_point_entries_refuse_null_and_uncommitted_handles_without_a_gpu():
    """check_net comes first, as in dfn_mlp_coarse / dfn_mlp_fine: a null handle is DFN_ERR_ARG (-1), a created but uncommitted one
    DFN_ERR_STATE (-3), each with a message that names the entry."""
    lib = _lib.load()
    one = ctypes.c_void_p(16)      # a non-null token: never dereferenced when the handle is refused first

    def calls(h, prec):
        return {
            "dfn_mlp_coarse_points": lib.dfn_mlp_coarse_points(h, prec, one, 4, 8, one, None),
            "dfn_mlp_fine_points": lib.dfn_mlp_fine_points(h, prec, one, one, one, 1, 4, 8, one, one, None),
            "dfn_mlp_fine_points_backward": lib.dfn_mlp_fine_points_backward(h, prec, one, one, one, 1, 4, 8, one, one, one, None),
        }

    for prec in (_lib.DFN_PREC_F16, _lib.DFN_PREC_F32, _lib.DFN_PREC_F16X3):
        assert calls(None, prec) == {n: -1 for n in NAMES}
    assert b"dfn_mlp_fine_points_backward: null handle" in lib.dfn_last_error()
    h = ctypes.c_void_p()
    d = _lib.NerfhDesc(8, 128, 10, 4, 10, 5, 2, 1000)
    assert lib.dfn_nerfh_create(ctypes.byref(d), ctypes.byref(h)) == 0
    try:
        for prec in (_lib.DFN_PREC_F16, _lib.DFN_PREC_F32, _lib.DFN_PREC_F16X3):
            assert calls(h, prec) == {n: -3 for n in NAMES}
        assert b"dfn_nerfh_commit" in lib.dfn_last_error()
        # ... with no rows to evaluate as well: the handle is checked before n_rows == 0 returns DFN_OK
        assert lib.dfn_mlp_coarse_points(h, _lib.DFN_PREC_F32, one, 0, 8, one, None) == -3
    finally:
        lib.dfn_nerfh_destroy(h)
