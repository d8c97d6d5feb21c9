"""dfn_raw2outputs / dfn_raw2outputs_backward at the C-ABI boundary, without a GPU: exported, bound with the header's argument counts,
every DFN_ERR_ARG case reported before any device work, n_rays == 0 accepted."""
import ctypes
import os
import re

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ctypes.c_void_p(16)      # a non-null token: never dereferenced when an argument is refused
CT = _lib.COMP_COARSE | _lib.COMP_TEST_TIME


def grads(**kw):
    return ctypes.byref(_lib.Raw2OutputsGrads(**{k: 16 for k in kw}))


def test_symbols_and_argument_counts():
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfnet_hip.h")).read(), flags=re.S)
    for name in ("dfn_raw2outputs", "dfn_raw2outputs_backward"):
        assert hasattr(lib, name)
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    fields = re.search(r"typedef struct \{([^}]*)\} dfn_raw2outputs_grads;", src).group(1)
    assert re.findall(r"\*(\w+)", fields) == [n for n, _ in _lib.Raw2OutputsGrads._fields_]
    assert int(re.search(r"DFN_COMP_COARSE\s*=\s*(\d+)", src).group(1)) == _lib.COMP_COARSE
    assert _lib.COMP_COARSE & (1 | 2 | 4 | 8) == 0      # 8 is the compositor launcher's own bit


def test_forward_refuses_bad_arguments():
    lib = _lib.load()
    f = lambda raw, ch, z, noise, N, flags, rgb=ONE: lib.dfn_raw2outputs(raw, ch, z, noise, 0.5, 7, N, 0.1, flags, rgb, ONE, ONE, ONE, ONE,
                                                                       ONE, None)
    bad = {
        "raw NULL": f(None, 9, ONE, None, 24, 3), "z NULL": f(ONE, 9, None, None, 24, 3),
        "N = 0": f(ONE, 9, ONE, None, 0, 3), "N = 513": f(ONE, 4, ONE, None, 513, 0),
        "ch = 3": f(ONE, 3, ONE, None, 24, 0), "ch = 0": f(ONE, 0, ONE, None, 24, 0),
        "noise with ch = 9": f(ONE, 9, ONE, ONE, 24, 3),
        "ch = 1 without the coarse bit": f(ONE, 1, ONE, None, 24, _lib.COMP_TEST_TIME),
        "ch = 1 without the test-time bit": f(ONE, 1, ONE, None, 24, _lib.COMP_COARSE),
        "ch = 4 with both": f(ONE, 4, ONE, None, 24, CT),
        "ch = 9 with both": f(ONE, 9, ONE, None, 24, CT),
        "ch = 9 without rgb": f(ONE, 9, ONE, None, 24, 3, None),
    }
    assert all(rc == -1 for rc in bad.values()), bad
    assert b"dfn_raw2outputs" in lib.dfn_last_error()
    for ch, flags, noise in ((1, CT, ONE), (4, 0, ONE), (4, _lib.COMP_WHITE_BKGD, None), (9, 3, None), (9, _lib.COMP_COARSE, None)):
        assert lib.dfn_raw2outputs(ONE, ch, ONE, noise, 0.5, 0, 512, 0.1, flags, ONE, ONE, ONE, ONE, ONE, ONE, None) == 0, (ch, flags)


def test_backward_refuses_bad_arguments():
    lib = _lib.load()
    b = lambda ch, N, flags, g, graw=ONE, gz=ONE, noise=None, raw=ONE: lib.dfn_raw2outputs_backward(raw, ch, ONE, noise, 0.5, 7, N, 0.1, flags,
                                                                                                  g, graw, gz, None)
    bad = {
        "raw NULL": b(9, 24, 3, grads(rgb=1), raw=None),
        "N = 0": b(9, 0, 3, grads(rgb=1)), "N = 513": b(9, 513, 3, grads(rgb=1)),
        "ch = 2": b(2, 24, 0, grads(acc=1)),
        "noise with ch = 9": b(9, 24, 3, grads(rgb=1), noise=ONE),
        "ch = 1 without its bits": b(1, 24, 0, grads(acc=1)),
        "ch = 4 with the bits of ch = 1": b(4, 24, CT, grads(acc=1)),
        "grads NULL": b(9, 24, 3, None), "no gradient": b(9, 24, 3, grads()),
        "ch = 1: a gradient on an output it does not return": b(1, 24, CT, grads(rgb=1, disp=1, depth=1, beta=1)),
        "ch = 4: beta alone (a constant there)": b(4, 24, 0, grads(beta=1)),
        "both outputs NULL": b(9, 24, 3, grads(rgb=1), graw=None, gz=None),
    }
    assert all(rc == -1 for rc in bad.values()), bad
    assert b"dfn_raw2outputs_backward" in lib.dfn_last_error()
    for ch, flags, g in ((1, CT, grads(weights=1)), (4, 0, grads(depth=1)), (9, 3, grads(beta=1)), (9, 0, grads(disp=1))):
        for graw, gz in ((ONE, ONE), (None, ONE), (ONE, None)):
            assert lib.dfn_raw2outputs_backward(ONE, ch, ONE, None, 0., 0, 1, 0.1, flags, g, graw, gz, None) == 0, (ch, flags)
