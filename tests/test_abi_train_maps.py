"""CPU-side check of the entry points of the training render with every output attached: the library exports them, the header declares
them with the same argument counts and cites the reference, the ctypes table carries their argument types, dfn_train_map_grads has the
header's layout (nine pointers, header order), and bad arguments are refused without a GPU.  (Workspace sizes and the state rules need a
forward pass: tests/test_gpu_train_maps.py.)"""
import ctypes
import inspect
import os
import re

from dfnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, S, I, F = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float
GRADS = ("rgb", "disp", "acc", "depth", "beta", "rgb0", "disp0", "acc0", "depth0")


def header():
    src = open(os.path.join(ROOT, "include", "dfnet_hip.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def new_entries():
    M, PP = ctypes.POINTER(_lib.TrainMapGrads), ctypes.POINTER(ctypes.c_void_p)
    return {
        # raw_c, z_c, noise | noise_std | n_rays | Nc | grads, gpre, stream
        "dfn_composite_coarse_train_backward_maps": [P, P, P, F, S, I, M, P, P],
        # raw, z | n_rays | Nf | grads | g_tsigma | grad_raw_ext, gpre, stream
        "dfn_composite_fine_train_backward_maps": [P, P, S, I, M, F, P, P, P],
        # h | n_rays | Nc, Ni | raw, workspace | bytes | depth, depth0, stream
        "dfn_nerfh_train_depths": [P, S, I, I, P, P, S, P, P, P],
        # h, params, hist | hist_rows, n_rays | Nc, Ni | noise | raw_noise_std | raw, grads | g_tsigma | grad_raw_ext, grads_out, workspace | bytes | stream
        "dfn_nerfh_train_backward_maps": [P, PP, P, S, S, I, I, P, F, P, M, F, P, PP, P, S, P],
        # h, params, rays_o, rays_d, hist | hist_rows, n_rays | Nc, Ni | noise | raw_noise_std | raw, grads | g_tsigma | grad_raw_ext, grad_rays_o,
        # grad_rays_d, workspace | bytes | scratch | bytes | stream
        "dfn_nerfh_train_backward_rays_maps": [P, P, P, P, P, S, S, I, I, P, F, P, M, F, P, P, P, P, S, P, S, P],
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
        assert ("const dfn_train_map_grads*" in protos[name][1]) == (name != "dfn_nerfh_train_depths"), name
    # the step entries are the old ones with (grads, g_tsigma, grad_raw_ext) in the place of (g_rgb, g_rgb0, g_beta, g_tsigma, g_tsigma_dense);
    # the old entries keep their signatures
    for new, old, at in (("dfn_nerfh_train_backward_maps", "dfn_nerfh_train_backward", 10), ("dfn_nerfh_train_backward_rays_maps", "dfn_nerfh_train_backward_rays", 12)):
        a, b = list(_lib.SIGNATURES[new][1]), list(_lib.SIGNATURES[old][1])
        assert len(a) == len(b) - 2 and a[:at] == b[:at] and a[at + 3:] == b[at + 5:], new
    assert len(_lib.SIGNATURES["dfn_nerfh_train_backward"][1]) == 19 and len(_lib.SIGNATURES["dfn_nerfh_train_backward_rays"][1]) == 24
    assert len(_lib.SIGNATURES["dfn_nerfh_train_forward"][1]) == 27


def test_every_new_entry_cites_the_reference():
    src, _ = header()
    for name in new_entries():
        at = src.index(name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        assert "rendering.py:" in comment, f"{name}: the comment in front of it cites no reference line"


def test_struct_layout_matches_the_header():
    _, code = header()
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*dfn_train_map_grads\s*;", code)
    assert m, "dfn_train_map_grads is not declared"
    members = [n.strip() for n in re.sub(r"\b(const|float)\b", "", m.group(1)).replace(";", ",").replace("*", "").split(",") if n.strip()]
    assert tuple(members) == GRADS
    assert [n for n, _ in _lib.TrainMapGrads._fields_] == list(GRADS)
    assert all(t is ctypes.c_void_p for _, t in _lib.TrainMapGrads._fields_)
    assert ctypes.sizeof(_lib.TrainMapGrads) == 9 * ctypes.sizeof(ctypes.c_void_p)
    for i, n in enumerate(GRADS):
        assert getattr(_lib.TrainMapGrads, n).offset == i * ctypes.sizeof(ctypes.c_void_p)
    st = _lib.TrainMapGrads()
    assert all(getattr(st, n) is None for n in GRADS)   # a fresh struct is nine NULLs


def test_bad_arguments_without_a_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # a non-null token: never dereferenced, every call below is refused or returns before any device work
    none, fine, coarse = _lib.TrainMapGrads(), _lib.TrainMapGrads(acc=16), _lib.TrainMapGrads(acc0=16)
    cc = lib.dfn_composite_coarse_train_backward_maps
    assert cc(one, one, None, 0., 4, 8, ctypes.byref(none), one, None) == -1           # nine NULLs
    assert b"dfn_composite_coarse_train_backward_maps" in lib.dfn_last_error()
    assert cc(one, one, None, 0., 4, 8, None, one, None) == -1                         # no struct at all
    assert cc(one, one, None, 0., 4, 8, ctypes.byref(fine), one, None) == -1           # a fine member alone is nothing for the coarse pass
    for Nc in (2, 513, -1):
        assert cc(one, one, None, 0., 4, Nc, ctypes.byref(coarse), one, None) == -1
    assert cc(None, one, None, 0., 4, 8, ctypes.byref(coarse), one, None) == -1        # raw_c
    assert cc(one, None, None, 0., 4, 8, ctypes.byref(coarse), one, None) == -1        # z_c
    assert cc(one, one, None, 0., 4, 8, ctypes.byref(coarse), None, None) == -1        # gpre
    assert cc(one, one, None, 0., 0, 8, ctypes.byref(coarse), one, None) == 0          # no rays: nothing to do
    cf = lib.dfn_composite_fine_train_backward_maps
    assert cf(one, one, 4, 8, ctypes.byref(none), 0., None, one, None) == -1           # nothing at all
    assert b"dfn_composite_fine_train_backward_maps" in lib.dfn_last_error()
    assert cf(one, one, 4, 8, None, 0., None, one, None) == -1
    assert cf(one, one, 4, 8, ctypes.byref(coarse), 0., None, one, None) == -1
    for Nf in (0, 513, -1):
        assert cf(one, one, 4, Nf, ctypes.byref(fine), 0., None, one, None) == -1
    assert cf(None, one, 4, 8, ctypes.byref(fine), 0., None, one, None) == -1          # raw
    assert cf(one, None, 4, 8, ctypes.byref(fine), 0., None, one, None) == -1          # z
    assert cf(one, one, 4, 8, ctypes.byref(fine), 0., None, None, None) == -1          # gpre
    assert cf(one, one, 0, 8, ctypes.byref(fine), 0., None, one, None) == 0            # no rays
    # the workspace-based entries: handle, sample counts, required pointers, then the state of the handle
    params = (ctypes.c_void_p * 64)(*[16] * 64)
    bw, br, dp = lib.dfn_nerfh_train_backward_maps, lib.dfn_nerfh_train_backward_rays_maps, lib.dfn_nerfh_train_depths
    assert bw(None, params, one, 1, 4, 8, 8, None, 0., one, ctypes.byref(fine), 0., None, params, one, 1 << 30, None) == -1
    assert b"dfn_nerfh_train_backward_maps" in lib.dfn_last_error()
    assert br(None, params, one, one, one, 1, 4, 8, 8, None, 0., one, ctypes.byref(fine), 0., None, one, one, one, 1 << 30, one, 1 << 30, None) == -1
    assert b"dfn_nerfh_train_backward_rays_maps" in lib.dfn_last_error()
    assert dp(None, 4, 8, 8, one, one, 1 << 30, one, one, None) == -1 and b"dfn_nerfh_train_depths" in lib.dfn_last_error()
    h = ctypes.c_void_p()
    d = _lib.NerfhDesc(8, 32, 10, 4, 10, 5, 2, 1000)
    assert lib.dfn_nerfh_create(ctypes.byref(d), ctypes.byref(h)) == 0
    try:
        args = lambda **o: [o.get("h", h), o.get("params", params), o.get("hist", one), 1, o.get("n", 4), o.get("Nc", 8), o.get("Ni", 8), None, 0.,
                            o.get("raw", one), o.get("st", ctypes.byref(fine)), 0., None, o.get("out", params), o.get("ws", one), 1 << 30, None]
        assert bw(*args(Nc=2)) == -4 and bw(*args(Ni=0)) == -4 and bw(*args(Nc=300, Ni=300)) == -4   # the sample counts of the training step
        assert bw(*args(n=0)) == 0
        assert bw(*args(st=ctypes.byref(none))) == -1 and bw(*args(st=None)) == -1                  # nothing given
        for k in ("params", "hist", "raw", "out", "ws"):
            assert bw(*args(**{k: None})) == -1, k
        holes = (ctypes.c_void_p * 64)(*[16] * 63 + [None])
        assert bw(*args(params=holes)) == -1 and bw(*args(out=holes)) == -1
        rargs = lambda **o: [h, o.get("params", params), o.get("o", one), o.get("d", one), o.get("hist", one), 1, o.get("n", 4), 8, 8, None, 0.,
                             o.get("raw", one), o.get("st", ctypes.byref(coarse)), 0., None, o.get("go", one), o.get("gd", one), o.get("ws", one),
                             1 << 30, o.get("scratch", one), 1 << 30, None]
        assert br(*rargs(n=0)) == 0 and br(*rargs(st=ctypes.byref(none))) == -1
        for k in ("params", "o", "d", "hist", "raw", "go", "gd", "ws", "scratch"):
            assert br(*rargs(**{k: None})) == -1, k
        assert br(*rargs()) == -3 and b"dfn_nerfh_train_backward_rays_maps" in lib.dfn_last_error()   # no exact-mode forward on this handle
        assert dp(h, 0, 8, 8, one, one, 1 << 30, one, one, None) == 0
        assert dp(h, 4, 8, 8, None, one, 1 << 30, one, one, None) == -1 and dp(h, 4, 8, 8, one, None, 1 << 30, one, one, None) == -1
        assert dp(h, 4, 8, 8, one, one, 1 << 30, None, None, None) == -1                             # neither depth wanted
        assert dp(h, 4, 2, 8, one, one, 1 << 30, one, one, None) == -4
    finally:
        lib.dfn_nerfh_destroy(h)


def test_python_surface():
    from dfnet_amd import engine, nerf_train, rendering
    assert engine.TRAIN_GRAD_NAMES == GRADS and nerf_train.TRAIN_MAP_NAMES == ("depth", "depth0")
    assert callable(engine.composite_coarse_train_backward_maps) and callable(engine.composite_fine_train_backward_maps)
    T = nerf_train.NerfHTrainer
    assert inspect.signature(T.forward).parameters["maps"].default is False
    for fn in (T.backward, T.backward_rays):
        sig = inspect.signature(fn).parameters
        assert sig["g_maps"].default is None and sig["g_raw"].default is None
        assert list(sig)[1:4] == ["g_rgb", "g_rgb0", "g_beta"]   # the positional operands of the NerfWLoss step stay where they are
    assert nerf_train.train_map_names(True) == ("depth", "depth0") and nerf_train.train_map_names(None) == ()
    assert nerf_train.train_map_names(["depth0"]) == ("depth0",)
    for bad in ("depth_static", "rgb_static", "rgb_transient", "beta"):
        try:
            nerf_train.train_map_names((bad,))
        except ValueError as e:
            assert "['depth', 'depth0']" in str(e)
        else:
            raise AssertionError(bad)
    assert inspect.signature(rendering.render).parameters["diff_maps"].default is False
