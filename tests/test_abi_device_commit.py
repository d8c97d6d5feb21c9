"""CPU-side checks of the device re-commit (dfn_nerfh_recommit_device): the three entries are declared, bound and exported, the
host-only selfcheck executes the packer's plan against the packer's values byte for byte, and arguments are refused before any
device work."""
import ctypes
import json
import os
import re

import pytest

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
NEW = {
    "dfn_nerfh_recommit_device": (ctypes.c_int, [P, P, P]),
    "dfn_nerfh_packed_buffer": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(P),
                                               ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_float)]),
    "dfn_nerfh_recommit_selfcheck": (ctypes.c_int, [ctypes.c_int]),
}


def test_new_entries_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "dfnet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name, sig in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/dfnet_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name), f"{name} is not in the ctypes table / not exported"
        assert _lib.SIGNATURES[name] == sig and len(sig[1]) == len(m.group(1).split(","))


@pytest.mark.parametrize("width", [128, 256, 64])
def test_selfcheck_plan_reproduces_the_packer(width):
    """Netwidth 128 (every variant, gradient and training-query blob, the folds), 256 and a generic width: the plan executed on the
    host over another parameter set's buffers gives the packer's bytes and scales."""
    lib = _lib.load()
    rc = lib.dfn_nerfh_recommit_selfcheck(width)
    assert rc == 0, lib.dfn_last_error().decode()
    text = lib.dfn_last_error().decode()
    assert f"netwidth {width}:" in text and "bytes written per re-commit" in text
    print(text)


@pytest.mark.parametrize("width", [128, 256, 64])
def test_packer_output_matches_the_recorded_digest(width):
    """Every packed buffer of the selfcheck's parameter set B -- name, size, bytes, unit table, unit counts, in_scale, in enumeration
    order -- hashes to the digest recorded in tests/golden/pack_digest.json: a change of the host packer's output shows here."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pack_digest.json")))["digest"]
    lib = _lib.load()
    assert lib.dfn_nerfh_recommit_selfcheck(width) == 0, lib.dfn_last_error().decode()
    m = re.search(r"packed digest ([0-9a-f]{16})$", lib.dfn_last_error().decode())
    assert m, "the selfcheck's text carries no digest"
    assert m.group(1) == golden[str(width)]


def test_selfcheck_refuses_an_odd_width():
    lib = _lib.load()
    assert lib.dfn_nerfh_recommit_selfcheck(127) == -1 and b"dfn_nerfh_recommit_selfcheck" in lib.dfn_last_error()


def test_refusals_without_a_gpu():
    lib = _lib.load()
    n = lib.dfn_nerfh_train_param_count()
    tokens = (P * n)(*[16] * n)   # non-null, never dereferenced: the handle below is refused first
    h = P()
    d = _lib.NerfhDesc(8, 128, 10, 4, 10, 5, 2, 1000)
    assert lib.dfn_nerfh_create(ctypes.byref(d), ctypes.byref(h)) == 0
    try:
        assert lib.dfn_nerfh_recommit_device(None, tokens, None) == -1
        assert lib.dfn_nerfh_recommit_device(h, None, None) == -1
        holed = (P * n)(*[16] * n)
        holed[5] = None
        assert lib.dfn_nerfh_recommit_device(h, holed, None) == -1
        assert lib.dfn_nerfh_train_param_name(5) in lib.dfn_last_error()
        assert lib.dfn_nerfh_recommit_device(h, tokens, None) == -3 and b"never committed" in lib.dfn_last_error()
        assert lib.dfn_nerfh_packed_buffer(h, 0, None, None, None, None) == -3
        assert lib.dfn_nerfh_packed_buffer(None, 0, None, None, None, None) == -1
    finally:
        lib.dfn_nerfh_destroy(h)
