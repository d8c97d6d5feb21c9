"""CPU-side checks of the sampler's backward entry (dfn_sample_pdf_backward): declared in the header, exported, bound in the ctypes
table with one argument per prototype parameter, and refusing every bad argument before any device work."""
import ctypes
import os
import re
import subprocess

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dfn_sample_pdf_backward"


def test_entry_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "dfnet_hip.h")).read()
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+" + NAME + r"\s*\(", src, flags=re.S).group(1)
    for said in ("models/rendering.py:24-65", "den branch", "clamped ends", "no gradient through the search"):
        assert said in comment, f"the header comment of {NAME} does not state: {said}"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(dfn_[a-z0-9_]+)\s*\(", src))
    so = os.path.join(ROOT, "dfnet_amd", "libdfnet_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.split()
    lib = _lib.load()
    assert NAME in declared, f"{NAME} is not declared in include/dfnet_hip.h"
    assert NAME in exported, f"{NAME} is not exported by libdfnet_hip.so"
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME), f"{NAME} is not in the ctypes table"
    proto = re.search(r"\b" + NAME + r"\s*\(([^)]*)\)", src).group(1)
    assert len(_lib.SIGNATURES[NAME][1]) == len(proto.split(",")) == 11


def test_entry_refuses_bad_arguments_without_a_gpu():
    """Every refusal is DFN_ERR_ARG (-1) with a message that names the entry, and comes before any device work: the pointers here are
    tokens that are never dereferenced.  A shape whose row does not fit the LDS is refused too (DFN_ERR_UNSUPPORTED, -4), and n == 0 is
    DFN_OK without a launch."""
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    f = lib.dfn_sample_pdf_backward
    #                 bins weights n  nb Ni u    g    gb   gw   gu
    good = dict(bins=one, weights=one, n=4, nb=8, Ni=5, u=one, g=one, gb=one, gw=one, gu=one)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["bins"], a["weights"], a["n"], a["nb"], a["Ni"], a["u"], a["g"], a["gb"], a["gw"], a["gu"], None)

    refused = {
        "bins NULL": dict(bins=None),
        "weights NULL": dict(weights=None),
        "grad_out NULL": dict(g=None),
        "nb < 2": dict(nb=1),
        "nb < 0": dict(nb=-3),
        "Ni < 1": dict(Ni=0),
        "all outputs NULL": dict(gb=None, gw=None, gu=None),
        "grad_u without u": dict(u=None),
        "grad_u alone without u": dict(u=None, gb=None, gw=None),
    }
    for what, kw in refused.items():
        assert call(**kw) == -1, what
        assert lib.dfn_last_error().startswith(b"dfn_sample_pdf_backward: "), what
    # the same refusals with no rows: the arguments are checked before n == 0 returns DFN_OK
    assert call(n=0, bins=None) == -1 and call(n=0, nb=1) == -1 and call(n=0, u=None) == -1
    # nothing to do, and every accepted combination of outputs
    assert call(n=0) == 0
    assert call(n=0, u=None, gu=None) == 0 and call(n=0, gb=None, gw=None) == 0 and call(n=0, gw=None, gu=None) == 0
    # a row that cannot be staged: 3 nb + 7 Ni floats for each of a block's four rows against 64 KiB
    for kw in (dict(nb=1400, Ni=1), dict(nb=2, Ni=600), dict(nb=2 ** 31 - 1, Ni=2 ** 31 - 1)):
        assert call(**kw) == -4, kw
        assert call(n=0, **kw) == -4, kw
        assert lib.dfn_last_error().startswith(b"dfn_sample_pdf_backward: "), kw
