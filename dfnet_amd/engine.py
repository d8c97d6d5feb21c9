"""NerfHEngine — host-side owner of a `dfn_nerfh_t` handle and thin tensor-level wrappers of the
stage and whole-path entry points of libdfnet_hip.so.

All tensors are fp32 CUDA tensors owned by torch (device memory + streams are torch's job; the
arithmetic is the HIP library's).  Work is enqueued on torch's current stream.

The test-time render has one implementation per shape of call, `_render_rays` (a ray batch, generic-width chunk loop included) and
`_render_image` (a pose), with the render maps as an option; `render_rays`, `generic_render_rays`, `render_image` and their `_maps`
forms are front ends of the two.  Without maps a call goes to the plain library entry with the plain entry's workspace.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, ptr


def _grow_workspace(old, nbytes, device):
    """A persistent byte workspace of >= nbytes on `device` (the old one if it fits).  Engines keep one workspace across calls that
    may come from different torch streams (direct_feature_matching runs the target features on a side stream), so a new block is
    always taken from the DEFAULT stream's pool — never tied to a side stream — the calling stream waits for whatever the default
    stream still has queued on a recycled block, and the block being replaced is marked in use by the calling stream: the allocator
    hands it out again only after the kernels queued there have finished."""
    if old is not None and old.device == device and old.numel() >= nbytes:
        return old
    if device.type != "cuda":
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    cur, default = torch.cuda.current_stream(device), torch.cuda.default_stream(device)
    if old is not None and old.is_cuda:
        old.record_stream(cur)
    with torch.cuda.stream(default):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    if cur != default:
        cur.wait_stream(default)
    return ws


# DFN_DEBUG_POISON_UNREAD=1: feature planes / gradient planes that a "read only these levels" promise leaves unwritten (zero_unread=False,
# lazy_grad) are filled with NaN instead of being left as uninitialised memory — the DFNet_dm gradient tests run once under it
# (tests/test_gpu_grad.py) to prove that no unhinted level is ever read.
POISON_UNREAD = os.environ.get("DFN_DEBUG_POISON_UNREAD", "0") == "1"


def _f32c(t):
    return t.contiguous().float()


MAP_NAMES = _lib.MAP_NAMES   # depth, depth_static, beta [n]; rgb_static, rgb_transient [n,3] (models/rendering.py:196-241)


def map_names(maps):
    """The render maps a caller asks for, in the library's order: True = all five, False / None = none, or an iterable of names."""
    if maps is True:
        return MAP_NAMES
    if maps is False or maps is None:
        return ()
    if isinstance(maps, str):
        maps = (maps,)
    maps = tuple(maps)
    unknown = [m for m in maps if m not in MAP_NAMES]
    if unknown:
        raise ValueError(f"unknown render map(s) {unknown}: the maps are {list(MAP_NAMES)}")
    return tuple(m for m in MAP_NAMES if m in maps)


def _alloc_maps(names, n, dev):
    """({name: tensor [n] / [n,3]}, the dfn_render_maps struct pointing at them)."""
    out = {m: torch.empty((n, 3) if m.startswith("rgb_") else (n,), device=dev) for m in names}
    return out, _lib.RenderMaps(**{m: t.data_ptr() for m, t in out.items()})


def _maps_at(out, r0, m):
    """The struct for rows [r0, r0 + m) of the maps in `out`."""
    return _lib.RenderMaps(**{k: t[r0:r0 + m].data_ptr() for k, t in out.items()})


GRAD_NAMES = tuple(n for n, _ in _lib.MapGrads._fields_)   # rgb, acc, depth, depth_static, disp, beta, rgb_static, rgb_transient


def _map_grads(grads, n):
    """({name: contiguous fp32 tensor [n] / [n,3]} of the non-None entries of `grads`, kept alive by the caller) for dfn_map_grads."""
    unknown = [k for k in grads if k not in GRAD_NAMES]
    if unknown:
        raise ValueError(f"unknown upstream gradient(s) {unknown}: the compositor's outputs are {list(GRAD_NAMES)}")
    return {k: _f32c(t).reshape((n, 3) if k.startswith("rgb") else (n,)) for k, t in grads.items() if t is not None}


def _map_grads_at(held, r0=0, m=None):
    """The dfn_map_grads struct for rows [r0, r0 + m) of the tensors of _map_grads."""
    return _lib.MapGrads(**{k: (t if m is None else t[r0:r0 + m]).data_ptr() for k, t in held.items()})


class NerfHEngine:
    """NeRF-H coarse+fine networks resident on one GPU in MFMA-fragment layout."""

    def __init__(self, depth=8, width=128, multires=10, multires_views=4, hist_bin=10, dim_a=5, dim_t=2,
                 n_vocab=1000, precision="f16"):
        self.lib = _lib.load()
        self.desc = _lib.NerfhDesc(depth, width, multires, multires_views, hist_bin, dim_a, dim_t, n_vocab)
        self.handle = ctypes.c_void_p()
        check(self.lib.dfn_nerfh_create(ctypes.byref(self.desc), ctypes.byref(self.handle)), "dfn_nerfh_create")
        self.precision = precision
        self.hist_bin = hist_bin
        self.width = width
        self.fast = width in (128, 256)   # register-resident MFMA kernels; other widths run the generic layer-by-layer fp32 path
        self._ws = None
        self.lindisp = False
        self.coarse_f16 = False
        self._param_numel = None     # {canonical name: numel} of the last load_numpy (None: never committed)
        self.device_commits = 0      # load_device() calls that re-packed the engine on the GPU

    def set_render_options(self, lindisp=False, coarse_f16=None):
        """render_rays options that every entry point of this handle applies (dfn_nerfh_set_render_options): lindisp = coarse
        depths linear in disparity (rendering.py:272-273); coarse_f16 (None = leave as is) = the coarse network of the test-time
        render runs with f16 inputs whatever precision the call names (it only places the fine samples)."""
        lindisp = bool(lindisp)
        coarse_f16 = self.coarse_f16 if coarse_f16 is None else bool(coarse_f16)
        if lindisp != self.lindisp or coarse_f16 != self.coarse_f16:
            flags = (_lib.RENDER_LINDISP if lindisp else 0) | (_lib.RENDER_COARSE_F16 if coarse_f16 else 0)
            check(self.lib.dfn_nerfh_set_render_options(self.handle, flags), "dfn_nerfh_set_render_options")
            self.lindisp, self.coarse_f16 = lindisp, coarse_f16
        return self

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.dfn_nerfh_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def load_numpy(self, coarse, fine, emb_a, emb_t):
        """coarse/fine: {state_dict key: ndarray}; emb_a/emb_t: ndarrays."""
        items = [("coarse." + k, v) for k, v in coarse.items()] + [("fine." + k, v) for k, v in fine.items()]
        items += [("embedding_a.weight", emb_a), ("embedding_t.weight", emb_t)]
        for name, arr in items:
            a = np.ascontiguousarray(arr, dtype=np.float32)
            check(self.lib.dfn_nerfh_set_param(self.handle, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size),
                  f"dfn_nerfh_set_param({name})")
        check(self.lib.dfn_nerfh_commit(self.handle), "dfn_nerfh_commit")
        self._param_numel = {name: int(np.asarray(arr).size) for name, arr in items}
        return self

    def _canonical_names(self):
        return [self.lib.dfn_nerfh_train_param_name(i).decode() for i in range(self.lib.dfn_nerfh_train_param_count())]

    def device_ready(self, tensors):
        """Can load_device() take these tensors: the engine has been committed once on the host (load_numpy) and every tensor is a
        contiguous fp32 CUDA tensor of its parameter's size, in canonical order."""
        if self._param_numel is None or tensors is None:
            return False
        names = self._canonical_names()
        return len(tensors) == len(names) and all(
            t is not None and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == self._param_numel[k]
            for k, t in zip(names, tensors))

    def load_device(self, tensors):
        """Re-commit from tensors that live on the GPU (dfn_nerfh_recommit_device): `tensors` in the canonical order of
        dfn_nerfh_train_param_name(), contiguous fp32 CUDA tensors.  Every packed buffer of the engine is rewritten in place on the
        current stream, byte for byte what load_numpy would have packed from the same values; nothing goes through the host except
        one 8-byte read of the two weight maxima (one wait for the current stream at netwidth 128 and 256).  Refused before a first
        load_numpy (the host commit lays the buffers out).  Work on other streams that reads this engine is the caller's to order."""
        names = self._canonical_names()
        if len(tensors) != len(names):
            raise ValueError(f"load_device: {len(tensors)} tensors, the NeRF-H layout has {len(names)} parameters")
        for k, t in zip(names, tensors):
            if t is None:
                continue   # the library refuses a null entry by name
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f"load_device: parameter {k} must be a contiguous fp32 CUDA tensor")
            if self._param_numel is not None and t.numel() != self._param_numel[k]:
                raise ValueError(f"load_device: parameter {k} has {t.numel()} elements, the engine was committed with {self._param_numel[k]}")
        ptrs = (ctypes.c_void_p * len(names))(*[None if t is None else t.data_ptr() for t in tensors])
        check(self.lib.dfn_nerfh_recommit_device(self.handle, ptrs, current_stream()), "dfn_nerfh_recommit_device")
        self.device_commits += 1
        return self

    def module_tensors(self, network_fn, network_fine, embedding_a, embedding_t):
        """The parameters of the four modules in canonical order (None when they do not make up the NeRF-H layout)."""
        lookup = {}
        for pre, mod in (("coarse.", network_fn), ("fine.", network_fine), ("embedding_a.", embedding_a), ("embedding_t.", embedding_t)):
            for k, p in mod.named_parameters():
                lookup[pre + k] = p.detach()
        names = self._canonical_names()
        return [lookup[k] for k in names] if len(lookup) == len(names) and all(k in lookup for k in names) else None

    def load_modules_device(self, network_fn, network_fine, embedding_a, embedding_t):
        """load_device() from torch modules with the reference's state_dict layout whose parameters live on the GPU."""
        tensors = self.module_tensors(network_fn, network_fine, embedding_a, embedding_t)
        if tensors is None:
            raise ValueError("load_modules_device: the modules' parameters do not match the NeRF-H layout")
        return self.load_device(tensors)

    def packed_buffers(self):
        """[(name, device pointer, bytes, in_scale)] of every device buffer of the last commit (dfn_nerfh_packed_buffer)."""
        out, i = [], 0
        name, ptr, nbytes, scale = ctypes.c_char_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_float()
        while self.lib.dfn_nerfh_packed_buffer(self.handle, i, ctypes.byref(name), ctypes.byref(ptr), ctypes.byref(nbytes), ctypes.byref(scale)) == 0:
            out.append((name.value.decode(), ptr.value, nbytes.value, scale.value))
            i += 1
        return out

    def load_modules(self, network_fn, network_fine, embedding_a, embedding_t):
        """Take the weights of torch modules with the reference's state_dict layout."""
        sd = lambda m: {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        return self.load_numpy(sd(network_fn), sd(network_fine), embedding_a.weight.detach().cpu().numpy(),
                               embedding_t.weight.detach().cpu().numpy())

    def range_flags(self):
        """DFN_RANGE_* bits raised by the MLP kernels since the last call (waits for the current stream, clears them)."""
        v = ctypes.c_int(0)
        check(self.lib.dfn_nerfh_range_status(self.handle, ctypes.byref(v), current_stream()), "dfn_nerfh_range_status")
        return v.value

    def check_range(self):
        """Raise DfnError if an f16 / split-f16 activation overflowed / saturated in a render since the last check: such frames
        are not the network's output (render with precision='f32')."""
        check(self.lib.dfn_nerfh_range_status(self.handle, None, current_stream()), "NeRF-H range guard")

    def raise_range(self, flags, where=""):
        """The range guard's error for flags already fetched with range_flags() (render_path carries them through its gather so that
        every rank leaves the collective before anyone raises)."""
        if flags:
            narrow = "f16" if flags & 1 else "split-f16"
            why = ("an f16 layer output overflowed to inf: |activation| > 65504" if flags & 1
                   else "a split-f16 hi half saturated: |activation| >= 4094 (hidden layers of the render kernels: 4094 x the largest |weight|)")
            raise _lib.DfnError(f"NeRF-H range guard ({where}): activations left the range of the {narrow} arithmetic ({why}); the frames "
                                "rendered since the last check are not the network's output: render them with precision='f32'")

    def _prec(self, precision):
        return _lib.PRECISIONS[precision or self.precision]

    def _workspace(self, nbytes, device):
        self._ws = _grow_workspace(self._ws, nbytes, device)
        return self._ws

    # ------------------------------------------------------------------ stages
    def mlp_coarse(self, rays_o, rays_d, Nc, near, far, precision=None):
        rays_o, rays_d = _f32c(rays_o), _f32c(rays_d)
        n = rays_o.shape[0]
        sigma = torch.empty(n, Nc, device=rays_o.device)
        check(self.lib.dfn_mlp_coarse(self.handle, self._prec(precision), ptr(rays_o), ptr(rays_d), n, Nc,
                                      float(near), float(far), ptr(sigma), current_stream()), "dfn_mlp_coarse")
        return sigma

    def mlp_fine(self, rays_o, rays_d, viewdirs, hist, z_fine, precision=None):
        rays_o, rays_d, viewdirs, z_fine = _f32c(rays_o), _f32c(rays_d), _f32c(viewdirs), _f32c(z_fine)
        hist = _f32c(hist).reshape(-1, self.hist_bin)
        n, Nf = z_fine.shape
        raw = torch.empty(n, Nf, 9, device=rays_o.device)
        bias = torch.empty(self.lib.dfn_fine_bias_bytes(n), dtype=torch.uint8, device=rays_o.device)
        check(self.lib.dfn_mlp_fine(self.handle, self._prec(precision), ptr(rays_o), ptr(rays_d), ptr(viewdirs),
                                    ptr(hist), hist.shape[0], n, ptr(z_fine), Nf, ptr(raw),
                                    ctypes.c_void_p(bias.data_ptr()), current_stream()), "dfn_mlp_fine")
        return raw

    def mlp_fine_backward(self, rays_o, rays_d, viewdirs, hist, z_fine, grad_raw, precision=None):
        """d L/d raw [n,Nf,9] -> [n,Nf,6]: d L/d sample point (3) and d L/d viewdir through that sample (3)."""
        rays_o, rays_d, viewdirs, z_fine, grad_raw = (_f32c(t) for t in (rays_o, rays_d, viewdirs, z_fine, grad_raw))
        hist = _f32c(hist).reshape(-1, self.hist_bin)
        n, Nf = z_fine.shape
        gpts = torch.empty(n, Nf, 6, device=rays_o.device)
        bias = torch.empty(self.lib.dfn_fine_bias_bytes(n), dtype=torch.uint8, device=rays_o.device)
        check(self.lib.dfn_mlp_fine_backward(self.handle, self._prec(precision), ptr(rays_o), ptr(rays_d), ptr(viewdirs),
                                             ptr(hist), hist.shape[0], n, ptr(z_fine), Nf, ptr(grad_raw), ptr(gpts),
                                             ctypes.c_void_p(bias.data_ptr()), current_stream()), "dfn_mlp_fine_backward")
        return gpts

    def mlp_fine_saving(self, rays_o, rays_d, viewdirs, hist, z_fine):
        """mlp_fine in split-f16 that also records the ReLU signs: (raw [n,Nf,9], masks) for mlp_fine_backward_saved()."""
        rays_o, rays_d, viewdirs, z_fine = _f32c(rays_o), _f32c(rays_d), _f32c(viewdirs), _f32c(z_fine)
        hist = _f32c(hist).reshape(-1, self.hist_bin)
        n, Nf = z_fine.shape
        dev = rays_o.device
        raw = torch.empty(n, Nf, 9, device=dev)
        masks = torch.empty(self.lib.dfn_mlp_fine_mask_bytes(n * Nf), dtype=torch.uint8, device=dev)
        bias = torch.empty(self.lib.dfn_fine_bias_bytes(n), dtype=torch.uint8, device=dev)
        check(self.lib.dfn_mlp_fine_saving(self.handle, _lib.PRECISIONS["f16x3"], ptr(rays_o), ptr(rays_d), ptr(viewdirs), ptr(hist),
                                           hist.shape[0], n, ptr(z_fine), Nf, ptr(raw), ctypes.c_void_p(masks.data_ptr()),
                                           ctypes.c_void_p(bias.data_ptr()), current_stream()), "dfn_mlp_fine_saving")
        return raw, masks

    def mlp_fine_backward_saved(self, rays_o, rays_d, viewdirs, z_fine, raw, masks, grad_raw):
        """The gradient of mlp_fine_backward from the saved forward (raw + ReLU masks): no forward recompute."""
        rays_o, rays_d, viewdirs, z_fine, raw, grad_raw = (_f32c(t) for t in (rays_o, rays_d, viewdirs, z_fine, raw, grad_raw))
        n, Nf = z_fine.shape
        gpts = torch.empty(n, Nf, 6, device=rays_o.device)
        check(self.lib.dfn_mlp_fine_backward_saved(self.handle, _lib.PRECISIONS["f16x3"], ptr(rays_o), ptr(rays_d), ptr(viewdirs), n,
                                                   ptr(z_fine), Nf, ptr(raw), ctypes.c_void_p(masks.data_ptr()), ptr(grad_raw),
                                                   ptr(gpts), current_stream()), "dfn_mlp_fine_backward_saved")
        return gpts

    # ------------------------------------------------------------------ point queries
    POINTS_CHUNK = 1 << 28       # points per library call (the kernels index points with 32 bits)
    POINT_ROWS_CHUNK = 1 << 18   # rows per library call of the fine queries (one 1 KB bias-table row each)

    def _point_rows(self, pts, viewdirs=None, hist=None):
        """Contiguous fp32 pts [n, N, 3] (read in place by the kernels), view directions [n, 3] and histograms [1 | n, hist_bin]."""
        pts = _f32c(pts)
        if pts.dim() != 3 or pts.shape[-1] != 3 or pts.shape[1] < 1:
            raise ValueError(f"pts must be [rows, N, 3] with N >= 1, got {tuple(pts.shape)}")
        n = pts.shape[0]
        if viewdirs is not None:
            viewdirs = _f32c(viewdirs).reshape(-1, 3)
            if viewdirs.shape[0] != n:   # the kernels read one row per row of points
                raise ValueError(f"viewdirs must have {n} rows, got {tuple(viewdirs.shape)}")
        if hist is not None:
            hist = _f32c(hist).reshape(-1, self.hist_bin)
            if hist.shape[0] not in (1, n):
                raise ValueError(f"hist must have 1 or {n} rows, got {tuple(hist.shape)}")
        return pts, viewdirs, hist

    def _point_chunks(self, n, N, fine):
        """Row ranges [r0, r1) of one library call each.  A single trailing row is not left a call of its own (it takes a row from the
        call before it): the bias-table kernel sums a lone row's histogram in its shared-histogram order, whose rounding differs from
        the per-row order the same row gets inside a larger call, and a split query must return the bits of the unsplit one."""
        step = max(1, self.POINTS_CHUNK // N)
        if fine:
            step = min(step, self.POINT_ROWS_CHUNK)
        chunks = [(r0, min(n, r0 + step)) for r0 in range(0, n, step)]
        if fine and len(chunks) > 1 and step >= 3 and chunks[-1][1] - chunks[-1][0] == 1:
            (a, b), (_, c) = chunks[-2], chunks[-1]
            chunks[-2:] = [(a, b - 1), (b - 1, c)]
        return chunks

    def mlp_coarse_points(self, pts, precision=None):
        """The coarse network's density at the caller's own points: pts [n, N, 3] -> sigma [n, N] (nerfw.py:37-46)."""
        pts, _, _ = self._point_rows(pts)
        n, N = pts.shape[:2]
        sigma = torch.empty(n, N, device=pts.device)
        for r0, r1 in self._point_chunks(n, N, False) or [(0, 0)]:
            check(self.lib.dfn_mlp_coarse_points(self.handle, self._prec(precision), ptr(pts[r0:r1]), r1 - r0, N, ptr(sigma[r0:r1]),
                                                 current_stream()), "dfn_mlp_coarse_points")
        return sigma

    def mlp_coarse_points_backward(self, pts, grad_sigma, precision=None):
        """d L/d sigma [n, N] of mlp_coarse_points -> d L/d point [n, N, 3] (autograd through nerfw.py:37-46, 315-334; the forward
        is recomputed inside the gradient kernel).  Netwidth 128, f16x3 or f32."""
        pts, _, _ = self._point_rows(pts)
        n, N = pts.shape[:2]
        grad_sigma = _f32c(grad_sigma).reshape(n, N)
        gpts = torch.empty(n, N, 3, device=pts.device)
        for r0, r1 in self._point_chunks(n, N, False) or [(0, 0)]:
            check(self.lib.dfn_mlp_coarse_points_backward(self.handle, self._prec(precision), ptr(pts[r0:r1]), r1 - r0, N,
                                                          ptr(grad_sigma[r0:r1]), ptr(gpts[r0:r1]), current_stream()),
                  "dfn_mlp_coarse_points_backward")
        return gpts

    def mlp_coarse_static_points(self, pts, viewdirs, precision=None):
        """The coarse network's training query at the caller's own points: pts [n, N, 3] and one view direction [n, 3] per row ->
        raw [n, N, 4] = (static_rgb, static_sigma) (nerfw.py:47-60, 326-343).  Rows are chunked as the fine query's."""
        pts, viewdirs, _ = self._point_rows(pts, viewdirs)
        if viewdirs is None:
            raise ValueError("mlp_coarse_static_points needs viewdirs [rows, 3]")
        n, N = pts.shape[:2]
        raw = torch.empty(n, N, 4, device=pts.device)
        for r0, r1 in self._point_chunks(n, N, True) or [(0, 0)]:
            bias = torch.empty(self.lib.dfn_fine_bias_bytes(r1 - r0), dtype=torch.uint8, device=pts.device)
            check(self.lib.dfn_mlp_coarse_static_points(self.handle, self._prec(precision), ptr(pts[r0:r1]), ptr(viewdirs[r0:r1]), r1 - r0,
                                                        N, ptr(raw[r0:r1]), ctypes.c_void_p(bias.data_ptr()), current_stream()),
                  "dfn_mlp_coarse_static_points")
        return raw

    def mlp_coarse_static_points_backward(self, pts, viewdirs, grad_raw, precision=None):
        """d L/d raw [n, N, 4] of mlp_coarse_static_points -> [n, N, 6]: d L/d point (3) and d L/d viewdir through that point (3).
        Netwidth 128, f16x3 or f32."""
        pts, viewdirs, _ = self._point_rows(pts, viewdirs)
        if viewdirs is None:
            raise ValueError("mlp_coarse_static_points_backward needs viewdirs [rows, 3]")
        n, N = pts.shape[:2]
        grad_raw = _f32c(grad_raw).reshape(n, N, 4)
        gpts = torch.empty(n, N, 6, device=pts.device)
        for r0, r1 in self._point_chunks(n, N, True) or [(0, 0)]:
            bias = torch.empty(self.lib.dfn_fine_bias_bytes(r1 - r0), dtype=torch.uint8, device=pts.device)
            check(self.lib.dfn_mlp_coarse_static_points_backward(self.handle, self._prec(precision), ptr(pts[r0:r1]), ptr(viewdirs[r0:r1]),
                                                                 r1 - r0, N, ptr(grad_raw[r0:r1]), ptr(gpts[r0:r1]),
                                                                 ctypes.c_void_p(bias.data_ptr()), current_stream()),
                  "dfn_mlp_coarse_static_points_backward")
        return gpts

    def mlp_fine_points(self, pts, viewdirs, hist, precision=None):
        """The fine network at the caller's own points: pts [n, N, 3], one view direction [n, 3] and one histogram (hist [1 | n,
        hist_bin]) per row -> raw [n, N, 9] (nerfw.py:62-95)."""
        pts, viewdirs, hist = self._point_rows(pts, viewdirs, hist)
        n, N = pts.shape[:2]
        raw = torch.empty(n, N, 9, device=pts.device)
        for r0, r1 in self._point_chunks(n, N, True) or [(0, 0)]:
            hs = hist if hist.shape[0] == 1 else hist[r0:r1]
            bias = torch.empty(self.lib.dfn_fine_bias_bytes(r1 - r0), dtype=torch.uint8, device=pts.device)
            check(self.lib.dfn_mlp_fine_points(self.handle, self._prec(precision), ptr(pts[r0:r1]), ptr(viewdirs[r0:r1]), ptr(hs),
                                               hs.shape[0], r1 - r0, N, ptr(raw[r0:r1]), ctypes.c_void_p(bias.data_ptr()),
                                               current_stream()), "dfn_mlp_fine_points")
        return raw

    def mlp_fine_points_backward(self, pts, viewdirs, hist, grad_raw, precision=None):
        """d L/d raw [n,N,9] of mlp_fine_points -> [n,N,6]: d L/d point (3) and d L/d viewdir through that point (3)."""
        pts, viewdirs, hist = self._point_rows(pts, viewdirs, hist)
        n, N = pts.shape[:2]
        grad_raw = _f32c(grad_raw).reshape(n, N, 9)
        gpts = torch.empty(n, N, 6, device=pts.device)
        for r0, r1 in self._point_chunks(n, N, True) or [(0, 0)]:
            hs = hist if hist.shape[0] == 1 else hist[r0:r1]
            bias = torch.empty(self.lib.dfn_fine_bias_bytes(r1 - r0), dtype=torch.uint8, device=pts.device)
            check(self.lib.dfn_mlp_fine_points_backward(self.handle, self._prec(precision), ptr(pts[r0:r1]), ptr(viewdirs[r0:r1]), ptr(hs),
                                                        hs.shape[0], r1 - r0, N, ptr(grad_raw[r0:r1]), ptr(gpts[r0:r1]),
                                                        ctypes.c_void_p(bias.data_ptr()), current_stream()),
                  "dfn_mlp_fine_points_backward")
        return gpts

    # ------------------------------------------------------------------ whole path
    GENERIC_GRAD_CHUNK = 8192   # rays per pass of the generic-width gradient (every fine activation is kept: ~1.3 MB per ray at 64+128, netwidth 256)
    GENERIC_CHUNK = 4096   # rays per pass of the generic path (its activations live in HBM: ~1.2 MB per ray at 64+128, W=128)

    def _ray_batch(self, rays_o, rays_d, hist, viewdirs):
        """What every ray-batch render starts from: contiguous fp32 rays [n,3], view directions [n,3] (None: d/|d|, formed by the
        library), histograms [rows, hist_bin] and the (rgb [n,3], disp [n], acc [n]) to render into."""
        rays_o, rays_d = _f32c(rays_o).reshape(-1, 3), _f32c(rays_d).reshape(-1, 3)
        n, dev = rays_o.shape[0], rays_o.device
        if viewdirs is not None:
            viewdirs = _f32c(viewdirs).reshape(-1, 3)
            if viewdirs.shape[0] != n:   # the kernels read one row per ray
                raise ValueError(f"viewdirs must have {n} rows, got {tuple(viewdirs.shape)}")
        hist = _f32c(hist).reshape(-1, self.hist_bin)
        return rays_o, rays_d, viewdirs, hist, (torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev))

    def _render_rays(self, rays_o, rays_d, hist, Nc, Ni, near, far, viewdirs=None, retraw=False, precision=None, names=()):
        """The test-time render of a ray batch behind render_rays, generic_render_rays and their _maps forms ->
        (rgb [n,3], disp [n], acc [n], raw|None, {name: map}).  names: the maps wanted, in the library's order (map_names()); with none
        of them the call is the plain entry's, with the plain entry's workspace.  precision "generic" (and every netwidth without
        register-resident kernels): exact fp32 layer by layer, GENERIC_CHUNK rays per pass."""
        rays_o, rays_d, viewdirs, hist, (rgb, disp, acc) = self._ray_batch(rays_o, rays_d, hist, viewdirs)
        n, dev = rays_o.shape[0], rays_o.device
        raw = torch.empty(n, Nc + Ni, 9, device=dev) if retraw else None
        mp, st = _alloc_maps(names, n, dev)
        if self.fast and precision != "generic":
            entry = "dfn_render_rays_maps" if names else "dfn_render_rays"
            size = self.lib.dfn_render_maps_workspace_bytes if names else self.lib.dfn_render_workspace_bytes
            ws = self._workspace(size(n, Nc, Ni), dev)
            args = [self.handle, self._prec(precision), ptr(rays_o), ptr(rays_d), ptr(viewdirs), ptr(hist), hist.shape[0], n, Nc, Ni,
                    float(near), float(far), ptr(rgb), ptr(disp), ptr(acc), ptr(raw), ctypes.c_void_p(ws.data_ptr()), ws.numel()]
            if names:
                args.append(ctypes.byref(st))
            check(getattr(self.lib, entry)(*args, current_stream()), entry)
            return rgb, disp, acc, raw, mp
        entry = "dfn_nerfh_generic_render_rays_maps" if names else "dfn_nerfh_generic_render_rays_v"
        C = self.GENERIC_CHUNK
        ws = self._workspace(self.lib.dfn_nerfh_generic_workspace_bytes(self.handle, min(n, C), Nc, Ni), dev)
        raw_tmp = None if retraw else torch.empty(min(n, C), Nc + Ni, 9, device=dev)
        for r0 in range(0, n, C):
            m = min(C, n - r0)
            cut = lambda t: None if t is None else t[r0:r0 + m]
            h = hist if hist.shape[0] == 1 else cut(hist)
            args = [self.handle, ptr(cut(rays_o)), ptr(cut(rays_d)), ptr(cut(viewdirs)), ptr(h), h.shape[0], m, Nc, Ni, float(near), float(far),
                    ptr(cut(rgb)), ptr(cut(disp)), ptr(cut(acc)), ptr(cut(raw) if retraw else raw_tmp[:m]),
                    ctypes.c_void_p(ws.data_ptr()), ws.numel()]
            if names:
                args.append(ctypes.byref(_maps_at(mp, r0, m)))
            check(getattr(self.lib, entry)(*args, current_stream()), entry)
        return rgb, disp, acc, raw, mp

    def _render_image(self, c2w, H, W, focal, hist, Nc, Ni, near, far, precision=None, out=None, names=()):
        """The test-time render of a full image behind render_image and render_image_maps -> (rgb [H,W,3], disp [H,W], acc [H,W],
        {name: [H,W] or [H,W,3]}), into the three tensors of `out` when given.  names as in _render_rays."""
        c2w = _f32c(c2w)[:3, :4].contiguous()
        dev = c2w.device
        hist = _f32c(hist).reshape(-1)[: self.hist_bin].contiguous()
        if self.fast and precision != "generic":
            res = rgb, disp, acc = tuple(out) if out is not None else (torch.empty(H, W, 3, device=dev), torch.empty(H, W, device=dev),
                                                                        torch.empty(H, W, device=dev))
            mp, st = _alloc_maps(names, H * W, dev)
            entry = "dfn_render_image_maps" if names else "dfn_render_image"
            size = self.lib.dfn_render_maps_workspace_bytes if names else self.lib.dfn_render_workspace_bytes
            ws = self._workspace(size(H * W, Nc, Ni), dev)
            args = [self.handle, self._prec(precision), ptr(c2w), H, W, float(focal), float(near), float(far), Nc, Ni, ptr(hist),
                    ptr(rgb), ptr(disp), ptr(acc), ctypes.c_void_p(ws.data_ptr()), ws.numel()]
            if names:
                args.append(ctypes.byref(st))
            check(getattr(self.lib, entry)(*args, current_stream()), entry)
        else:   # get_rays, then the generic-width ray batch
            o, d, _ = raygen(H, W, focal, c2w, want_viewdirs=False)
            rgb, disp, acc, _, mp = self._render_rays(o.reshape(-1, 3), d.reshape(-1, 3), hist, Nc, Ni, near, far, precision="generic",
                                                      names=names)
            res = (rgb.reshape(H, W, 3), disp.reshape(H, W), acc.reshape(H, W))
            if out is not None:
                for dst, src in zip(out, res):
                    dst.copy_(src)
                res = tuple(out)
        return res + ({k: v.reshape(H, W, *v.shape[1:]) for k, v in mp.items()},)

    def render_rays(self, rays_o, rays_d, hist, Nc, Ni, near, far, viewdirs=None, retraw=False, precision=None):
        """Test-time render of a ray batch -> (rgb [n,3], disp [n], acc [n], raw|None).  viewdirs [n,3]: the fine network's view
        directions, used as given (None: d/|d|)."""
        return self._render_rays(rays_o, rays_d, hist, Nc, Ni, near, far, viewdirs, retraw, precision)[:4]

    def generic_render_rays(self, rays_o, rays_d, hist, Nc, Ni, near, far, retraw=False, viewdirs=None):
        """render_rays on the generic-width path whatever the netwidth: exact fp32."""
        return self._render_rays(rays_o, rays_d, hist, Nc, Ni, near, far, viewdirs, retraw, "generic")[:4]

    def render_image(self, c2w, H, W, focal, hist, Nc, Ni, near, far, precision=None, out=None):
        """Test-time render of a full image from a [3,4] (or [4,4]) c2w -> (rgb [H,W,3], disp, acc [H,W])."""
        return self._render_image(c2w, H, W, focal, hist, Nc, Ni, near, far, precision, out)[:3]

    # ------------------------------------------------------------------ render maps
    def render_rays_maps(self, rays_o, rays_d, hist, Nc, Ni, near, far, viewdirs=None, retraw=False, precision=None, maps=MAP_NAMES):
        """render_rays that also returns the maps the compositor forms and the plain render drops (models/rendering.py:196-241):
        (rgb [n,3], disp [n], acc [n], raw|None, {name: map}) with depth, depth_static, beta [n] and rgb_static, rgb_transient [n,3].
        maps: an iterable of those names (default: all five; none: render_rays).  rgb / disp / acc are the bits render_rays returns."""
        return self._render_rays(rays_o, rays_d, hist, Nc, Ni, near, far, viewdirs, retraw, precision, map_names(maps))

    def generic_render_rays_maps(self, rays_o, rays_d, hist, Nc, Ni, near, far, retraw=False, viewdirs=None, maps=MAP_NAMES):
        """generic_render_rays with the requested maps, chunked the same way: (rgb, disp, acc, raw|None, {name: map})."""
        return self._render_rays(rays_o, rays_d, hist, Nc, Ni, near, far, viewdirs, retraw, "generic", map_names(maps))

    def render_image_maps(self, c2w, H, W, focal, hist, Nc, Ni, near, far, precision=None, out=None, maps=MAP_NAMES):
        """render_image with the maps of render_rays_maps, shaped like the image: (rgb [H,W,3], disp, acc [H,W], None,
        {name: [H,W] or [H,W,3]})."""
        res = self._render_image(c2w, H, W, focal, hist, Nc, Ni, near, far, precision, out, map_names(maps))
        return res[:3] + (None, res[3])

    def composite_fine_maps(self, raw, z, beta_min=0.1, maps=MAP_NAMES):
        """The maps from raw [n,Nf,9] and z [n,Nf] (the module-level composite_fine_maps)."""
        return composite_fine_maps(raw, z, beta_min, maps)

    def composite_fine_backward_maps(self, raw, z, grads, beta_min=0.1, grad_raw=None):
        """d L/d raw from the upstream gradients of every compositor output (the module-level composite_fine_backward_maps)."""
        return composite_fine_backward_maps(raw, z, grads, beta_min, grad_raw)

    # ------------------------------------------------------------------ staged render that keeps what backward needs
    def render_rays_saving(self, rays_o, rays_d, viewdirs, hist, Nc, Ni, near, far, precision=None, with_masks=False):
        """render_rays composed from the stage entry points, returning (rgb, disp, acc, z_fine, raw[, masks]): the state
        from which backward_from_saved() differentiates without recomputing the forward.  with_masks: the fine net runs
        in split-f16 and records its ReLU signs, so the backward needs no forward pass of its own at all."""
        rays_o, rays_d, viewdirs = _f32c(rays_o).reshape(-1, 3), _f32c(rays_d).reshape(-1, 3), _f32c(viewdirs).reshape(-1, 3)
        sigma = self.mlp_coarse(rays_o, rays_d, Nc, near, far, precision)
        z = sample_fine(sigma, Ni, near, far, lindisp=self.lindisp)
        if with_masks:
            raw, masks = self.mlp_fine_saving(rays_o, rays_d, viewdirs, hist, z)
            out = composite_fine(raw, z)
            return out["rgb"], out["disp"], out["acc"], z, raw, masks
        raw = self.mlp_fine(rays_o, rays_d, viewdirs, hist, z, precision)
        out = composite_fine(raw, z)
        return out["rgb"], out["disp"], out["acc"], z, raw

    def backward_from_saved(self, rays_o, rays_d, viewdirs, hist, z, raw, grad_rgb, derive_viewdirs=True, precision=None, masks=None,
                            grad_raw=None, graw=None):
        """d L/d (rays_o, rays_d[, viewdirs]) from the saved (z_fine, raw[, masks]) of render_rays_saving().  grad_raw [n,Nf,9]: a
        gradient that reaches `raw` directly (render(retraw=True) under autograd), added to the compositor's.  graw [n,Nf,9]: the
        FINISHED d L/d raw (composite_fine_backward_maps: every compositor output, grad_raw already inside) — the compositing backward
        is skipped and grad_rgb / grad_raw are not read."""
        rays_o, rays_d, viewdirs = _f32c(rays_o).reshape(-1, 3), _f32c(rays_d).reshape(-1, 3), _f32c(viewdirs).reshape(-1, 3)
        if graw is not None:
            if grad_raw is not None:
                raise ValueError("backward_from_saved: graw is the finished d L/d raw, grad_raw belongs inside it")
            graw = _f32c(graw).reshape(z.shape[0], z.shape[1], 9)
        else:
            graw = composite_fine_backward(raw, z, _f32c(grad_rgb).reshape(-1, 3))
            if grad_raw is not None:
                graw += _f32c(grad_raw).reshape(graw.shape)
        if masks is not None:
            gpts = self.mlp_fine_backward_saved(rays_o, rays_d, viewdirs, z, raw, masks, graw)
        else:
            gpts = self.mlp_fine_backward(rays_o, rays_d, viewdirs, hist, z, graw, precision)
        n, Nf = z.shape
        go, gd = torch.empty(n, 3, device=z.device), torch.empty(n, 3, device=z.device)
        gv = None if derive_viewdirs else torch.empty(n, 3, device=z.device)
        check(self.lib.dfn_ray_grad_reduce(ptr(gpts), ptr(z), ptr(rays_d), n, Nf, int(derive_viewdirs), ptr(go), ptr(gd), ptr(gv),
                                           current_stream()), "dfn_ray_grad_reduce")
        return go, gd, gv

    # ------------------------------------------------------------------ gradient of the whole path
    def render_rays_backward(self, rays_o, rays_d, hist, Nc, Ni, near, far, grad_rgb, viewdirs=None, precision=None, grad_raw=None,
                             grad_maps=None):
        """d L/d (rays_o, rays_d[, viewdirs]) of render_rays from d L/d rgb [n,3].  With viewdirs=None they are
        d/|d| and their gradient is folded into grad_rays_d (what autograd does for render(rays=...)).  grad_raw [n,Nc+Ni,9]
        (generic-width path): d L/d of the returned raw, added to the compositor's; grad_rgb may then be None.  grad_maps
        (generic-width path): {name: d L/d output} over acc, depth, depth_static, disp, beta, rgb_static, rgb_transient (and rgb, when
        grad_rgb is None) — the compositing backward for every output (dfn_nerfh_generic_render_rays_backward_maps)."""
        rays_o, rays_d = _f32c(rays_o).reshape(-1, 3), _f32c(rays_d).reshape(-1, 3)
        n, dev = rays_o.shape[0], rays_o.device
        generic = self.width != 128 or precision == "generic"
        held = None
        if grad_maps is not None:
            if not generic:
                raise NotImplementedError("render_rays_backward(grad_maps=...) on the register-resident netwidth-128 kernels: use "
                                          "precision='generic' or composite_fine_backward_maps() + backward_from_saved(graw=...)")
            held = _map_grads(grad_maps, n)
            if grad_rgb is not None and "rgb" in held:
                raise ValueError("render_rays_backward: d L/d rgb given twice (grad_rgb and grad_maps['rgb'])")
        if grad_raw is not None:
            if not generic:
                raise NotImplementedError("render_rays_backward(grad_raw=...) on the register-resident netwidth-128 kernels: use "
                                          "precision='generic' or backward_from_saved(grad_raw=...)")
            grad_raw = _f32c(grad_raw).reshape(n, Nc + Ni, 9)
        elif grad_rgb is None and not held:
            raise ValueError("render_rays_backward: grad_rgb and grad_raw are both None")
        if grad_rgb is not None:
            grad_rgb = _f32c(grad_rgb).reshape(n, 3)
        hist = _f32c(hist).reshape(-1, self.hist_bin)
        go, gd = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
        gv = None
        if viewdirs is not None:
            viewdirs = _f32c(viewdirs).reshape(-1, 3)
            gv = torch.empty(n, 3, device=dev)
        if generic:
            # the register-resident gradient kernels are netwidth 128; every other width takes the layer-by-layer exact-fp32 path
            entry = "dfn_nerfh_generic_render_rays_backward_raw" if held is None else "dfn_nerfh_generic_render_rays_backward_maps"
            C = self.GENERIC_GRAD_CHUNK
            ws = self._workspace(self.lib.dfn_nerfh_generic_backward_workspace_bytes(self.handle, min(n, C), Nc, Ni), dev)
            for r0 in range(0, n, C):
                m = min(C, n - r0)
                cut = lambda t: None if t is None else t[r0:r0 + m]
                hh = hist if hist.shape[0] == 1 else cut(hist)
                args = [self.handle, ptr(cut(rays_o)), ptr(cut(rays_d)), ptr(cut(viewdirs)), ptr(hh), hh.shape[0], m, Nc, Ni, float(near),
                        float(far), ptr(cut(grad_rgb)), ptr(cut(grad_raw)), ptr(cut(go)), ptr(cut(gd)), ptr(cut(gv)),
                        ctypes.c_void_p(ws.data_ptr()), ws.numel()]
                if held is not None:
                    args.append(ctypes.byref(_map_grads_at(held, r0, m)))
                check(getattr(self.lib, entry)(*args, current_stream()), entry)
            return go, gd, gv
        ws = self._workspace(self.lib.dfn_render_backward_workspace_bytes(n, Nc, Ni), dev)
        check(self.lib.dfn_render_rays_backward(self.handle, self._prec(precision), ptr(rays_o), ptr(rays_d), ptr(viewdirs),
                                                ptr(hist), hist.shape[0], n, Nc, Ni, float(near), float(far),
                                                ptr(grad_rgb), ptr(go), ptr(gd), ptr(gv),
                                                ctypes.c_void_p(ws.data_ptr()), ws.numel(), current_stream()),
              "dfn_render_rays_backward")
        return go, gd, gv

    def render_image_backward(self, c2w, H, W, focal, hist, Nc, Ni, near, far, grad_rgb, precision=None):
        """d L/d c2w [3,4] of render_image from d L/d rgb [H,W,3]."""
        c2w = _f32c(c2w)[:3, :4].contiguous()
        dev = c2w.device
        hist = _f32c(hist).reshape(-1)[: self.hist_bin].contiguous()
        grad_rgb = _f32c(grad_rgb).reshape(H, W, 3)
        gc = torch.empty(3, 4, device=dev)
        if self.width != 128 or precision == "generic":   # get_rays, the generic-width ray gradient, get_rays backward
            o, d, _ = raygen(H, W, focal, c2w, want_viewdirs=False)
            go, gd, _ = self.render_rays_backward(o.reshape(-1, 3), d.reshape(-1, 3), hist, Nc, Ni, near, far, grad_rgb.reshape(-1, 3),
                                                  precision="generic")
            return raygen_backward(H, W, focal, go, gd)
        ws = self._workspace(self.lib.dfn_render_backward_workspace_bytes(H * W, Nc, Ni), dev)
        check(self.lib.dfn_render_image_backward(self.handle, self._prec(precision), ptr(c2w), H, W, float(focal),
                                                 float(near), float(far), Nc, Ni, ptr(hist), ptr(grad_rgb), ptr(gc),
                                                 ctypes.c_void_p(ws.data_ptr()), ws.numel(), current_stream()),
              "dfn_render_image_backward")
        return gc


class DfnetEngine:
    """DFNet / DFNet_s feature extractor resident on one GPU (convs packed as MFMA fragments)."""

    def __init__(self, n_taps=3, feat_dim=12, precision="f16x3"):
        self.lib = _lib.load()
        self.n_taps, self.feat_dim, self.precision = n_taps, feat_dim, precision
        self.kept_tapes = []   # data_ptr()s of the workspaces the last kept forwards filled (the handle remembers 8)
        self.handle = ctypes.c_void_p()
        check(self.lib.dfn_dfnet_create(n_taps, feat_dim, ctypes.byref(self.handle)), "dfn_dfnet_create")
        self._ws = None

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.dfn_dfnet_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def load_numpy(self, state):
        """state: {state_dict key: ndarray} with the reference's DFNet names (num_batches_tracked ignored)."""
        for name, arr in state.items():
            if name.endswith("num_batches_tracked"):
                continue
            a = np.ascontiguousarray(arr, dtype=np.float32)
            check(self.lib.dfn_dfnet_set_param(self.handle, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size),
                  f"dfn_dfnet_set_param({name})")
        check(self.lib.dfn_dfnet_commit(self.handle), "dfn_dfnet_commit")
        return self

    def forward(self, x, return_feature=False, isSingleStream=False, return_pose=True, upsampleH=240, upsampleW=427,
                precision=None, levels=None, zero_unread=True):
        """(features, pose): features is None, [n_taps,B,128,uH,uW] (single stream) or a (target, render) pair of
        [n_taps,B/2,128,uH,uW]; pose is None or [B, feat_dim].
        levels (features without pose only): the pyramid levels the caller will read (the reference's
        index_select(features, 0, args.feature_matching_lvl)): only those are computed (dfn_dfnet_forward_levels), the planes of
        the others are zeros — or, with zero_unread=False (a caller that promises to read only `levels`: the DFNet_dm step's
        one-shot hint), left UNWRITTEN: zeroing two unread 39 MB planes costs 0.06 ms per forward at batch 4."""
        x = _f32c(x)
        B, C, H, W = x.shape
        assert C == 3
        prec = _lib.PRECISIONS[precision or self.precision]
        dev = x.device
        feats = pose = None
        if return_feature:
            shape = (self.n_taps, B, 128, upsampleH, upsampleW) if isSingleStream else \
                (2, self.n_taps, B // 2, 128, upsampleH, upsampleW)
            pruned = levels is not None and not return_pose and set(int(t) for t in levels) != set(range(self.n_taps))
            feats = torch.zeros(shape, device=dev) if (pruned and zero_unread) else torch.empty(shape, device=dev)
            if pruned and not zero_unread and POISON_UNREAD:
                feats.fill_(float("nan"))   # debug: a consumer that reads a level it did not ask for sees NaN, not stale memory
        if return_pose:
            pose = torch.empty(B, self.feat_dim, device=dev)
        nbytes = self.lib.dfn_dfnet_workspace_bytes(self.handle, prec, B, H, W)
        self._ws = _grow_workspace(self._ws, nbytes, dev)
        if return_feature and pruned:
            mask = sum(1 << int(t) for t in set(levels))
            check(self.lib.dfn_dfnet_forward_levels(self.handle, prec, ptr(x), B, H, W, int(not isSingleStream), mask, int(upsampleH),
                                                    int(upsampleW), ptr(feats), ctypes.c_void_p(self._ws.data_ptr()), self._ws.numel(),
                                                    current_stream()), "dfn_dfnet_forward_levels")
            return ((feats[0], feats[1]) if not isSingleStream else feats), None
        check(self.lib.dfn_dfnet_forward(self.handle, prec, ptr(x), B, H, W, int(return_feature),
                                         int(not isSingleStream), int(return_pose), int(upsampleH), int(upsampleW),
                                         ptr(feats), ptr(pose), ctypes.c_void_p(self._ws.data_ptr()), self._ws.numel(),
                                         current_stream()), "dfn_dfnet_forward")
        if return_feature and not isSingleStream:
            feats = (feats[0], feats[1])
        return feats, pose

    CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)  # encoder positions of the 13 convs (VGG16 cfg "D")

    def _remember(self, ws):
        self.kept_tapes = [p for p in self.kept_tapes if p != ws.data_ptr()][-7:] + [ws.data_ptr()]

    def holds(self, tape):
        """True if `tape` is (still) one of the kept forwards the handle can run a backward from."""
        return tape is not None and tape.data_ptr() in self.kept_tapes

    def forward_pose_keep(self, x, precision=None):
        """Pose regression keeping the encoder's activations: (pose [B, feat_dim], tape) for backward_params(tape=...)."""
        x = _f32c(x)
        B, C, H, W = x.shape
        prec = _lib.PRECISIONS[precision or self.precision]
        pose = torch.empty(B, self.feat_dim, device=x.device)
        ws = torch.empty(self.lib.dfn_dfnet_backward_params_workspace_bytes(self.handle, prec, B, H, W), dtype=torch.uint8, device=x.device)
        check(self.lib.dfn_dfnet_forward_train(self.handle, prec, ptr(x), B, H, W, 0, 1, 0, 1, 0, 0, None, ptr(pose), None,
                                               ctypes.c_void_p(ws.data_ptr()), ws.numel(), current_stream()),
              "dfn_dfnet_forward_train")
        self._remember(ws)
        return pose, ws

    def backward_params(self, x, grad_pose, precision=None, tape=None):
        """Gradients of the pose-regression path w.r.t. its parameters: dict {state_dict key: tensor} for
        encoder.<k>.weight|bias (13 convs) and fc_pose.weight|bias, from d L/d pose [B, feat_dim].  tape: the state
        forward_pose_keep / forward_train(keep=True) left (no forward recompute)."""
        x, gp = _f32c(x), _f32c(grad_pose).reshape(x.shape[0], self.feat_dim)
        B, C, H, W = x.shape
        prec = _lib.PRECISIONS[precision or self.precision]
        dev = x.device
        chans, cin, names, grads = [64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512], 3, [], []
        for idx, co in zip(self.CONV_INDEX, chans):
            names += [f"encoder.{idx}.weight", f"encoder.{idx}.bias"]
            grads += [torch.empty(co, cin, 3, 3, device=dev), torch.empty(co, device=dev)]
            cin = co
        names += ["fc_pose.weight", "fc_pose.bias"]
        grads += [torch.empty(self.feat_dim, 512, device=dev), torch.empty(self.feat_dim, device=dev)]
        ptrs = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
        if tape is not None:
            check(self.lib.dfn_dfnet_backward_all_params(self.handle, prec, ptr(x), B, H, W, ptr(gp), None, 0, 0, 0, 0, 1, ptrs, len(grads),
                                                         ctypes.c_void_p(tape.data_ptr()), tape.numel(), current_stream()),
                  "dfn_dfnet_backward_all_params")
            return dict(zip(names, grads))
        nbytes = self.lib.dfn_dfnet_backward_params_workspace_bytes(self.handle, prec, B, H, W)
        self._ws = _grow_workspace(self._ws, nbytes, dev)
        check(self.lib.dfn_dfnet_backward_params(self.handle, prec, ptr(x), B, H, W, ptr(gp), ptrs, len(grads),
                                                 ctypes.c_void_p(self._ws.data_ptr()), self._ws.numel(), current_stream()),
              "dfn_dfnet_backward_params")
        return dict(zip(names, grads))

    def forward_train(self, x, isSingleStream=False, return_pose=True, bn_batch=True, upsampleH=240, upsampleW=427,
                      precision=None, keep=False):
        """DFNet.forward while the module is being trained: (features, pose, bn_stats).  bn_batch: BatchNorm on the
        statistics of this batch (train() mode) — bn_stats [n_taps, 2, 128] = batch mean, biased variance — or on its
        running statistics (--freezeBN; bn_stats None).  keep=True: returns (features, pose, bn_stats, tape) — the tape
        holds every activation for backward_all_params(tape=...), which then recomputes nothing."""
        x = _f32c(x)
        B, C, H, W = x.shape
        assert C == 3
        prec = _lib.PRECISIONS[precision or self.precision]
        dev = x.device
        shape = (self.n_taps, B, 128, upsampleH, upsampleW) if isSingleStream else (2, self.n_taps, B // 2, 128, upsampleH, upsampleW)
        feats = torch.empty(shape, device=dev)
        pose = torch.empty(B, self.feat_dim, device=dev) if return_pose else None
        stats = torch.empty(self.n_taps, 2, 128, device=dev) if bn_batch else None
        if keep:
            ws = torch.empty(self.lib.dfn_dfnet_backward_params_workspace_bytes(self.handle, prec, B, H, W), dtype=torch.uint8, device=dev)
        else:
            nbytes = self.lib.dfn_dfnet_workspace_bytes(self.handle, prec, B, H, W)
            self._ws = _grow_workspace(self._ws, nbytes, dev)
            ws = self._ws
        check(self.lib.dfn_dfnet_forward_train(self.handle, prec, ptr(x), B, H, W, int(not isSingleStream), int(return_pose),
                                               int(bool(bn_batch)), int(bool(keep)), int(upsampleH), int(upsampleW), ptr(feats), ptr(pose),
                                               ptr(stats), ctypes.c_void_p(ws.data_ptr()), ws.numel(), current_stream()),
              "dfn_dfnet_forward_train")
        if not isSingleStream:
            feats = (feats[0], feats[1])
        if keep:
            self._remember(ws)
        return (feats, pose, stats, ws) if keep else (feats, pose, stats)

    # ------------------------------------------------------------------ training forward that keeps the pyramid, enlarges nothing
    def forward_train_pyramid(self, x, return_pose=True, bn_batch=True, precision=None, feature_images=None):
        """The siamese training forward (x = cat([stream A, stream B])) WITHOUT the enlarged feature stacks: every level's adapted
        map stays at its own resolution in the tape; triplet_pyramid_forward / backward_all_params_triplet work from there
        (dfn_dfnet_forward_train_pyramid).  feature_images: the leading frames that are the siamese pair (default: all); frames
        beyond them run the encoder and the pose head only.  Returns (pose | None, bn_stats | None, tape)."""
        x = _f32c(x)
        B, C, H, W = x.shape
        nf = B if feature_images is None else int(feature_images)
        assert C == 3 and nf % 2 == 0 and 2 <= nf <= B
        prec = _lib.PRECISIONS[precision or self.precision]
        dev = x.device
        pose = torch.empty(B, self.feat_dim, device=dev) if return_pose else None
        stats = torch.empty(self.n_taps, 2, 128, device=dev) if bn_batch else None
        ws = torch.empty(self.lib.dfn_dfnet_backward_params_workspace_bytes(self.handle, prec, B, H, W), dtype=torch.uint8, device=dev)
        check(self.lib.dfn_dfnet_forward_train_pyramid(self.handle, prec, ptr(x), B, nf, H, W, int(return_pose), int(bool(bn_batch)), ptr(pose),
                                                       ptr(stats), ctypes.c_void_p(ws.data_ptr()), ws.numel(), current_stream()),
              "dfn_dfnet_forward_train_pyramid")
        self._remember(ws)
        return pose, stats, ws

    def triplet_pyramid_forward(self, tape, B, H, W, upH, upW, f1_half, margin, mining, precision=None, feature_images=None):
        """Triplet loss (mining 0 / 1 / 2 = misc.py:355 / :371 / :399) between the two halves of the kept siamese batch as enlarged
        to [upH, upW], from the low-resolution levels: (loss 0-dim device tensor, state for backward_all_params_triplet)."""
        prec = _lib.PRECISIONS[precision or self.precision]
        dev = tape.device
        nf = B if feature_images is None else int(feature_images)
        nbytes = self.lib.dfn_dfnet_triplet_pyramid_state_bytes(self.handle, nf, int(upH))
        state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        loss = torch.empty(1, device=dev)
        check(self.lib.dfn_dfnet_triplet_pyramid_forward(self.handle, prec, B, nf, H, W, int(upH), int(upW), int(f1_half), float(margin), int(mining),
                                                         ptr(loss), ctypes.c_void_p(state.data_ptr()), nbytes,
                                                         ctypes.c_void_p(tape.data_ptr()), tape.numel(), current_stream()),
              "dfn_dfnet_triplet_pyramid_forward")
        return loss.reshape(()), state

    def backward_all_params_triplet(self, x, grad_pose, grad_loss, state, f1_half, upH, upW, bn_batch, tape, precision=None,
                                    feature_images=None):
        """backward_all_params whose feature gradient is grad_loss (0-dim / [1] device tensor) x the gradient of the pyramid triplet
        loss recorded in `state`; dict keyed as train_param_names(bn_affine=bn_batch)."""
        x = _f32c(x)
        B, C, H, W = x.shape
        gp = None if grad_pose is None else _f32c(grad_pose).reshape(B, self.feat_dim)
        gl = _f32c(grad_loss).reshape(1)
        prec = _lib.PRECISIONS[precision or self.precision]
        dev = x.device
        names = self.train_param_names(bn_affine=bn_batch)
        grads = [torch.empty(sh, device=dev) for sh in self._train_grad_shapes(bn_batch)]
        ptrs = (ctypes.c_void_p * len(grads))(*[t.data_ptr() for t in grads])
        nf = B if feature_images is None else int(feature_images)
        check(self.lib.dfn_dfnet_backward_all_params_triplet(self.handle, prec, ptr(x), B, nf, H, W, ptr(gp), ptr(gl),
                                                             ctypes.c_void_p(state.data_ptr()), state.numel(), int(f1_half), int(upH), int(upW),
                                                             int(bool(bn_batch)), ptrs, len(grads), ctypes.c_void_p(tape.data_ptr()),
                                                             tape.numel(), current_stream()),
              "dfn_dfnet_backward_all_params_triplet")
        return dict(zip(names, grads))

    def _train_grad_shapes(self, bn_batch):
        """Shapes of the gradient tensors in train_param_names(bn_affine=bn_batch) order."""
        chans, cin, shapes = [64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512], 3, []
        for co in chans:
            shapes += [(co, cin, 3, 3), (co,)]
            cin = co
        shapes += [(self.feat_dim, 512), (self.feat_dim,)]
        for t, c in zip(range(self.n_taps), (64, 256, 512)):
            shapes += [(64, c, 1, 1), (64,), (128, 64, 5, 5), (128,)] + ([(128,), (128,)] if bn_batch else [])
        return shapes

    def train_param_names(self, bn_affine=True):
        """state_dict keys in the order of backward_all_params' gradients."""
        names = []
        for idx in self.CONV_INDEX:
            names += [f"encoder.{idx}.weight", f"encoder.{idx}.bias"]
        names += ["fc_pose.weight", "fc_pose.bias"]
        for t in range(self.n_taps):
            pre = f"adaptation_layers.adapt_layer_{t}"
            names += [f"{pre}.0.weight", f"{pre}.0.bias", f"{pre}.2.weight", f"{pre}.2.bias"]
            if bn_affine:
                names += [f"{pre}.3.weight", f"{pre}.3.bias"]
        return names

    def backward_all_params(self, x, grad_pose, grad_features, levels=None, bn_batch=False, precision=None, tape=None):
        """Gradients of BOTH heads w.r.t. every trained parameter (run_feature.py:166-230): dict keyed as
        train_param_names(bn_affine=bn_batch).  bn_batch False: BatchNorm frozen on its running statistics
        (--freezeBN); True: batch statistics, with the gradients of BatchNorm's weight and bias.
        grad_pose [B, feat_dim] or None; grad_features single-stream [n_taps, B, 128, uH, uW]."""
        x, g = _f32c(x), _f32c(grad_features)
        B, C, H, W = x.shape
        assert C == 3 and g.shape[:3] == (self.n_taps, B, 128), (x.shape, g.shape)
        gp = None if grad_pose is None else _f32c(grad_pose).reshape(B, self.feat_dim)
        mask = sum(1 << int(t) for t in (range(self.n_taps) if levels is None else levels))
        prec = _lib.PRECISIONS[precision or self.precision]
        dev = x.device
        names = self.train_param_names(bn_affine=bn_batch)
        shapes = self._train_grad_shapes(bn_batch)
        n_pose = 2 * 13 + 2
        # zeros for the adaptation layers: levels outside the mask are not written
        grads = [torch.empty(sh, device=dev) if i < n_pose else torch.zeros(sh, device=dev) for i, sh in enumerate(shapes)]
        ptrs = (ctypes.c_void_p * len(grads))(*[t.data_ptr() for t in grads])
        if tape is None:
            nbytes = self.lib.dfn_dfnet_backward_params_workspace_bytes(self.handle, prec, B, H, W)
            self._ws = _grow_workspace(self._ws, nbytes, dev)
        ws = self._ws if tape is None else tape
        check(self.lib.dfn_dfnet_backward_all_params(self.handle, prec, ptr(x), B, H, W, ptr(gp), ptr(g), g.shape[3], g.shape[4], mask,
                                                     int(bool(bn_batch)), int(tape is not None), ptrs, len(grads),
                                                     ctypes.c_void_p(ws.data_ptr()), ws.numel(), current_stream()),
              "dfn_dfnet_backward_all_params")
        return dict(zip(names, grads))

    def refresh_train_params_device(self, tensors, precisions=None):
        """Re-pack every tensor the training path reads from device tensors: train_param_names(True) with, per level,
        .3.running_mean and .3.running_var after .3.bias.  The folded inference weights are NOT updated."""
        ts = [_f32c(t) for t in tensors]
        assert len(ts) == 28 + 8 * self.n_taps and all(t.is_cuda for t in ts)
        ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        check(self.lib.dfn_dfnet_refresh_train_params_device(self.handle, ptrs, len(ts), self._prec_mask(precisions), current_stream()),
              "dfn_dfnet_refresh_train_params_device")

    def _prec_mask(self, precisions):
        """Bit mask of the precisions a device re-pack renews: the engine's own by default, 'all', or a list of names."""
        if precisions == 'all':
            return 7
        names = [self.precision] if precisions is None else list(precisions)
        return sum(1 << _lib.PRECISIONS[p] for p in set(names))

    def refresh_pose_params_device(self, tensors, precisions=None):
        """Re-pack the pose path's parameters from device tensors (order: encoder.<k>.weight, .bias for the 13 convs,
        fc_pose.weight, fc_pose.bias) — the fast path after an optimizer step."""
        ts = [_f32c(t) for t in tensors]
        assert len(ts) == 28 and all(t.is_cuda for t in ts)
        ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        check(self.lib.dfn_dfnet_refresh_pose_params_device(self.handle, ptrs, len(ts), self._prec_mask(precisions), current_stream()),
              "dfn_dfnet_refresh_pose_params_device")

    def backward_input(self, x, grad_features, levels=None, precision=None):
        """d L/d x [B,3,H,W] from d L/d features in the single-stream layout [n_taps,B,128,uH,uW]; `levels` lists the
        pyramid levels that carry gradient (default: all).  Weights are frozen (DFNet_dm's feat_model)."""
        x, g = _f32c(x), _f32c(grad_features)
        B, C, H, W = x.shape
        assert C == 3 and g.shape[:3] == (self.n_taps, B, 128), (x.shape, g.shape)
        mask = sum(1 << int(t) for t in (range(self.n_taps) if levels is None else levels))
        prec = _lib.PRECISIONS[precision or self.precision]
        gx = torch.empty_like(x)
        nbytes = self.lib.dfn_dfnet_backward_workspace_bytes(self.handle, prec, B, H, W)
        self._ws = _grow_workspace(self._ws, nbytes, x.device)
        check(self.lib.dfn_dfnet_backward_input(self.handle, prec, ptr(x), B, H, W, g.shape[3], g.shape[4], ptr(g), mask,
                                                ptr(gx), ctypes.c_void_p(self._ws.data_ptr()), self._ws.numel(),
                                                current_stream()), "dfn_dfnet_backward_input")
        return gx


# ---------------------------------------------------------------------- weight-free stage wrappers
def raygen(H, W, focal, c2w, want_viewdirs=True):
    lib = _lib.load()
    c2w = _f32c(c2w)[:3, :4].contiguous()
    dev = c2w.device
    o = torch.empty(H, W, 3, device=dev)
    d = torch.empty(H, W, 3, device=dev)
    v = torch.empty(H, W, 3, device=dev) if want_viewdirs else None
    check(lib.dfn_raygen(H, W, float(focal), ptr(c2w), ptr(o), ptr(d), ptr(v), current_stream()), "dfn_raygen")
    return o, d, v


def raygen_frames(H, W, focal, c2ws, want_viewdirs=True):
    """get_rays for the B poses c2ws [B,3,4] in one launch: rays_o, rays_d (, viewdirs) [B,H,W,3]."""
    c2ws = _f32c(c2ws)[:, :3, :4].contiguous()
    B, dev = c2ws.shape[0], c2ws.device
    o = torch.empty(B, H, W, 3, device=dev)
    d = torch.empty(B, H, W, 3, device=dev)
    v = torch.empty(B, H, W, 3, device=dev) if want_viewdirs else None
    check(_lib.load().dfn_raygen_frames(B, H, W, float(focal), ptr(c2ws), ptr(o), ptr(d), ptr(v), current_stream()), "dfn_raygen_frames")
    return o, d, v


def raygen_frames_backward(H, W, focal, grad_o, grad_d):
    """d L/d c2w [B,3,4] from d L/d rays_o, rays_d [B,H*W,3]."""
    grad_o, grad_d = _f32c(grad_o), _f32c(grad_d)
    B = grad_o.shape[0]
    gc = torch.empty(B, 3, 4, device=grad_o.device)
    check(_lib.load().dfn_raygen_frames_backward(B, int(H), int(W), float(focal), ptr(grad_o), ptr(grad_d), ptr(gc), current_stream()),
          "dfn_raygen_frames_backward")
    return gc


def upsample_bicubic_frames(imgs, outH, outW, nchw=False):
    """[B,H,W,C] -> [B,outH,outW,C] (nchw: [B,C,outH,outW]) in one launch (upsample_bicubic per frame)."""
    imgs = _f32c(imgs)
    B, H, W, C = imgs.shape
    out = torch.empty((B, C, int(outH), int(outW)) if nchw else (B, int(outH), int(outW), C), device=imgs.device)
    check(_lib.load().dfn_upsample_bicubic_frames(ptr(imgs), B, H, W, C, int(outH), int(outW), 1 if nchw else 0, ptr(out), current_stream()),
          "dfn_upsample_bicubic_frames")
    return out


def upsample_bicubic_frames_backward(grad_out, H, W, nchw=False):
    """Adjoint of upsample_bicubic_frames: [B,outH,outW,C] (nchw: [B,C,outH,outW]) -> [B,H,W,C]."""
    g = _f32c(grad_out)
    if nchw:
        B, C, outH, outW = g.shape
    else:
        B, outH, outW, C = g.shape
    out = torch.empty(B, int(H), int(W), C, device=g.device)
    check(_lib.load().dfn_upsample_bicubic_frames_backward(ptr(g), B, int(H), int(W), C, outH, outW, 1 if nchw else 0, ptr(out),
                                                           current_stream()), "dfn_upsample_bicubic_frames_backward")
    return out


def posenc(x, L, fast=False):
    lib = _lib.load()
    x = _f32c(x).reshape(-1, 3)
    out = torch.empty(x.shape[0], 3 + 6 * L, device=x.device)
    check(lib.dfn_posenc(ptr(x), x.shape[0], L, 1 if fast else 0, ptr(out), current_stream()), "dfn_posenc")
    return out


def coarse_weights(sigma, z):
    lib = _lib.load()
    sigma, z = _f32c(sigma), _f32c(z)
    w = torch.empty_like(sigma)
    check(lib.dfn_coarse_weights(ptr(sigma), ptr(z), sigma.shape[0], sigma.shape[1], ptr(w), current_stream()),
          "dfn_coarse_weights")
    return w


def sample_pdf(bins, weights, Ni, u=None):
    lib = _lib.load()
    bins, weights = _f32c(bins), _f32c(weights)
    if u is not None:
        u = _f32c(u)
    out = torch.empty(bins.shape[0], Ni, device=bins.device)
    check(lib.dfn_sample_pdf(ptr(bins), ptr(weights), bins.shape[0], bins.shape[1], Ni, ptr(u), ptr(out),
                             current_stream()), "dfn_sample_pdf")
    return out


def sample_pdf_backward(bins, weights, Ni, grad_out, u=None, want=("bins", "weights", "u")):
    """(d L/d bins [n,nb], d L/d weights [n,nb-1], d L/d u [n,Ni]) through sample_pdf (dfn_sample_pdf_backward) from grad_out [n,Ni] =
    d L/d samples; bins, weights, Ni, u as in the forward call.  want: which of the three are computed, the others are returned as None;
    'u' needs an explicit u (the linspace draws of u=None are constants).  The chosen bins are the forward's: the kernel rebuilds its cdf
    with the forward's code."""
    unknown = [k for k in want if k not in ("bins", "weights", "u")]
    if unknown:
        raise ValueError(f"want holds {unknown}: the inputs are 'bins', 'weights' and 'u'")
    if "u" in want and u is None:
        raise ValueError("want holds 'u' without an explicit u: the linspace draws are constants")
    bins, weights, grad_out = _f32c(bins), _f32c(weights), _f32c(grad_out)
    n, nb = bins.shape
    Ni = int(Ni)
    if weights.shape != (n, nb - 1) or grad_out.shape != (n, Ni) or (u is not None and u.shape != (n, Ni)):
        raise ValueError(f"bins {tuple(bins.shape)}, weights {tuple(weights.shape)}, grad_out {tuple(grad_out.shape)}"
                         f"{'' if u is None else f', u {tuple(u.shape)}'} do not go together with Ni = {Ni}")
    if u is not None:
        u = _f32c(u)
    gb = torch.empty(n, nb, device=bins.device) if "bins" in want else None
    gw = torch.empty(n, nb - 1, device=bins.device) if "weights" in want else None
    gu = torch.empty(n, Ni, device=bins.device) if "u" in want else None
    if n == 0:   # (an empty tensor has no pointer to pass)
        return gb, gw, gu
    check(_lib.load().dfn_sample_pdf_backward(ptr(bins), ptr(weights), n, nb, Ni, ptr(u), ptr(grad_out), ptr(gb), ptr(gw), ptr(gu),
                                              current_stream()), "dfn_sample_pdf_backward")
    return gb, gw, gu


def ndc_rays(H, W, focal, near, rays_o, rays_d):
    """ray_utils.ndc_rays (models/ray_utils.py:27-46) on the device: (rays_o, rays_d) in normalised device coordinates."""
    lib = _lib.load()
    o, d = _f32c(rays_o), _f32c(rays_d)
    oo, od = torch.empty_like(o), torch.empty_like(d)
    check(lib.dfn_ndc_rays(int(H), int(W), float(focal), float(near), ptr(o), ptr(d), o.numel() // 3, ptr(oo), ptr(od), current_stream()),
          "dfn_ndc_rays")
    return oo, od


def ndc_rays_backward(H, W, focal, near, rays_o, rays_d, grad_ndc_o=None, grad_ndc_d=None):
    """ndc_rays under autograd (models/ray_utils.py:27-44): (d L/d rays_o, d L/d rays_d) [n,3] from the gradients of the NDC rays, either
    of which may be None = zeros (dfn_ndc_rays_backward)."""
    if grad_ndc_o is None and grad_ndc_d is None:
        raise ValueError("ndc_rays_backward: grad_ndc_o and grad_ndc_d are both None")
    o, d = _f32c(rays_o).reshape(-1, 3), _f32c(rays_d).reshape(-1, 3)
    g_o, g_d = (None if g is None else _f32c(g).reshape(-1, 3) for g in (grad_ndc_o, grad_ndc_d))
    n = o.shape[0]
    if d.shape[0] != n or any(g is not None and g.shape[0] != n for g in (g_o, g_d)):
        raise ValueError(f"ndc_rays_backward: rays and gradients must have {n} rows")
    go, gd = torch.empty_like(o), torch.empty_like(d)
    check(_lib.load().dfn_ndc_rays_backward(int(H), int(W), float(focal), float(near), ptr(o), ptr(d), n, ptr(g_o), ptr(g_d), ptr(go),
                                            ptr(gd), current_stream()), "dfn_ndc_rays_backward")
    return go, gd


def viewdirs_backward(rays_d, grad_viewdirs, out=None):
    """viewdirs = d / |d| under autograd (rendering.py:364-371): d L/d rays_d [n,3] = (g - v (v.g)) / |d| (dfn_viewdirs_backward).
    out [n,3]: a contiguous fp32 buffer the result is ADDED to (and which is returned)."""
    d, g = _f32c(rays_d).reshape(-1, 3), _f32c(grad_viewdirs).reshape(-1, 3)
    if g.shape[0] != d.shape[0] or (out is not None and out.shape != d.shape):
        raise ValueError(f"viewdirs_backward: gradients must have {d.shape[0]} rows of 3")
    if out is not None and (out.device != d.device or out.dtype != torch.float32 or not out.is_contiguous()):
        raise ValueError(f"viewdirs_backward: out must be a contiguous fp32 tensor on {d.device}, got {out.dtype} {out.device} "
                         f"contiguous={out.is_contiguous()}")
    gd = torch.empty_like(d) if out is None else out
    check(_lib.load().dfn_viewdirs_backward(ptr(d), ptr(g), d.shape[0], 0 if out is None else 1, ptr(gd), current_stream()),
          "dfn_viewdirs_backward")
    return gd


def sample_fine(sigma, Ni, near, far, want_aux=False, lindisp=False):
    lib = _lib.load()
    sigma = _f32c(sigma)
    n, Nc = sigma.shape
    z = torch.empty(n, Nc + Ni, device=sigma.device)
    w = torch.empty(n, Nc, device=sigma.device) if want_aux else None
    zs = torch.empty(n, Ni, device=sigma.device) if want_aux else None
    check(lib.dfn_sample_fine_opt(ptr(sigma), n, Nc, Ni, float(near), float(far), _lib.RENDER_LINDISP if lindisp else 0, ptr(z), ptr(w),
                                  ptr(zs), current_stream()), "dfn_sample_fine")
    return (z, w, zs) if want_aux else z


def composite_fine(raw, z, beta_min=0.1, test_time=True, static_only=True, white_bkgd=False, want_aux=False):
    lib = _lib.load()
    raw, z = _f32c(raw), _f32c(z)
    n, Nf = z.shape
    dev = raw.device
    rgb, disp, acc = torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
    depth = torch.empty(n, device=dev) if want_aux else None
    w = torch.empty(n, Nf, device=dev) if want_aux else None
    beta = torch.empty(n, device=dev) if want_aux else None
    flags = (_lib.COMP_TEST_TIME if test_time else 0) | (_lib.COMP_STATIC_ONLY if static_only else 0) | \
            (_lib.COMP_WHITE_BKGD if white_bkgd else 0)
    check(lib.dfn_composite_fine(ptr(raw), ptr(z), n, Nf, float(beta_min), flags, ptr(rgb), ptr(disp), ptr(acc),
                                 ptr(depth), ptr(w), ptr(beta), current_stream()), "dfn_composite_fine")
    out = dict(rgb=rgb, disp=disp, acc=acc)
    if want_aux:
        out.update(depth=depth, weights=w, beta=beta)
    return out


R2O_GRAD_NAMES = tuple(n for n, _ in _lib.Raw2OutputsGrads._fields_)   # rgb, disp, acc, weights, depth, beta


def _r2o_args(raw, z, noise, noise_std, test_time, static_only, white_bkgd, coarse):
    """(raw, ch, z, noise, noise_std, n, N, flags) of dfn_raw2outputs / _backward: raw [n,N] or [n,N,1] (the coarse test-time mode), [n,N,4]
    or [n,N,9]; the channel count selects the arithmetic mode."""
    raw, z = _f32c(raw), _f32c(z)
    n, N = z.shape
    ch = 1 if raw.dim() == 2 else raw.shape[-1]
    if raw.numel() != n * N * ch:
        raise ValueError(f"raw {tuple(raw.shape)} does not go with z {tuple(z.shape)}")
    if noise is not None:
        noise = _f32c(noise).reshape(n, N)
    flags = (_lib.COMP_TEST_TIME if test_time else 0) | (_lib.COMP_STATIC_ONLY if static_only else 0) | \
            (_lib.COMP_WHITE_BKGD if white_bkgd else 0) | (_lib.COMP_COARSE if coarse else 0)
    return raw, ch, z, noise, (0. if noise is None else float(noise_std)), n, N, flags


def raw2outputs(raw, z, noise=None, noise_std=0., beta_min=0.1, test_time=False, static_only=True, white_bkgd=False, coarse=False):
    """raw2outputs_NeRFW (models/rendering.py:132-243) on the device (dfn_raw2outputs); the channel count of raw selects the mode:
    [n,N] / [n,N,1] the coarse test-time mode (needs coarse and test_time) -> dict(acc, weights); [n,N,4] -> dict(rgb, disp, acc,
    weights, depth); [n,N,9] -> the same and beta (composite_fine's bits).  noise [n,N] x noise_std is added to sigma before the relu
    (not with 9 channels)."""
    lib = _lib.load()
    raw, ch, z, noise, noise_std, n, N, flags = _r2o_args(raw, z, noise, noise_std, test_time, static_only, white_bkgd, coarse)
    dev = raw.device
    out = dict(acc=torch.empty(n, device=dev), weights=torch.empty(n, N, device=dev))
    if ch != 1:
        out.update(rgb=torch.empty(n, 3, device=dev), disp=torch.empty(n, device=dev), depth=torch.empty(n, device=dev))
    if ch == 9:
        out.update(beta=torch.empty(n, device=dev))
    check(lib.dfn_raw2outputs(ptr(raw), ch, ptr(z), ptr(noise), noise_std, n, N, float(beta_min), flags, ptr(out.get("rgb")),
                              ptr(out.get("disp")), ptr(out["acc"]), ptr(out["weights"]), ptr(out.get("depth")), ptr(out.get("beta")),
                              current_stream()), "dfn_raw2outputs")
    return out


def raw2outputs_backward(raw, z, grads, noise=None, noise_std=0., beta_min=0.1, test_time=False, static_only=True, white_bkgd=False,
                         coarse=False, want=("raw", "z")):
    """(d L/d raw, d L/d z) through raw2outputs (dfn_raw2outputs_backward) from grads = {name: tensor} over rgb [n,3], disp, acc, depth,
    beta [n] and a dense weights [n,N]; a missing name or None is a zero gradient.  d L/d raw has the shape of raw and is the gradient of
    the post-activation raw given (exactly 0 on sigma behind a closed relu gate); d L/d z [n,N].  want: which of the two is computed, the
    other is returned as None."""
    unknown = [k for k in grads if k not in R2O_GRAD_NAMES]
    if unknown:
        raise ValueError(f"unknown upstream gradient(s) {unknown}: raw2outputs returns {list(R2O_GRAD_NAMES)}")
    unknown = [k for k in want if k not in ("raw", "z")]
    if unknown:
        raise ValueError(f"want holds {unknown}: the inputs are 'raw' and 'z'")
    shape = raw.shape
    raw, ch, z, noise, noise_std, n, N, flags = _r2o_args(raw, z, noise, noise_std, test_time, static_only, white_bkgd, coarse)
    held = {k: _f32c(t).reshape({"rgb": (n, 3), "weights": (n, N)}.get(k, (n,))) for k, t in grads.items() if t is not None}
    st = _lib.Raw2OutputsGrads(**{k: t.data_ptr() for k, t in held.items()})
    graw = torch.empty(shape, device=raw.device) if "raw" in want else None
    gz = torch.empty(n, N, device=raw.device) if "z" in want else None
    check(_lib.load().dfn_raw2outputs_backward(ptr(raw), ch, ptr(z), ptr(noise), noise_std, n, N, float(beta_min), flags, ctypes.byref(st),
                                               ptr(graw), ptr(gz), current_stream()), "dfn_raw2outputs_backward")
    return graw, gz


def composite_fine_maps(raw, z, beta_min=0.1, maps=MAP_NAMES):
    """{name: map} of the requested render maps (models/rendering.py:196-241) from raw [n,Nf,9] and z [n,Nf]: depth, depth_static,
    beta [n]; rgb_static, rgb_transient [n,3] (dfn_composite_fine_maps)."""
    raw, z = _f32c(raw), _f32c(z)
    n, Nf = z.shape
    out, st = _alloc_maps(map_names(maps), n, raw.device)
    check(_lib.load().dfn_composite_fine_maps(ptr(raw), ptr(z), n, Nf, float(beta_min), ctypes.byref(st), current_stream()),
          "dfn_composite_fine_maps")
    return out


def upsample_bicubic(img, outH, outW, out=None):
    """[H,W,C] -> [outH,outW,C], torch's nn.Upsample(mode='bicubic') semantics (align_corners=False)."""
    lib = _lib.load()
    img = _f32c(img)
    H, W, C = img.shape
    if out is None:
        out = torch.empty(outH, outW, C, device=img.device)
    check(lib.dfn_upsample_bicubic(ptr(img), H, W, C, int(outH), int(outW), ptr(out), current_stream()),
          "dfn_upsample_bicubic")
    return out


def raygen_backward(H, W, focal, grad_o, grad_d):
    """d L/d c2w [3,4] from d L/d rays_o, rays_d [H*W,3] (get_rays backward)."""
    grad_o, grad_d = _f32c(grad_o).reshape(-1, 3), _f32c(grad_d).reshape(-1, 3)
    gc = torch.empty(3, 4, device=grad_o.device)
    check(_lib.load().dfn_raygen_backward(int(H), int(W), float(focal), ptr(grad_o), ptr(grad_d), ptr(gc), current_stream()),
          "dfn_raygen_backward")
    return gc


def upsample_bicubic_backward(grad_out, H, W, out=None):
    """Adjoint of upsample_bicubic: [outH,outW,C] -> [H,W,C]."""
    g = _f32c(grad_out)
    outH, outW, C = g.shape
    if out is None:
        out = torch.empty(H, W, C, device=g.device)
    check(_lib.load().dfn_upsample_bicubic_backward(ptr(g), int(H), int(W), C, outH, outW, ptr(out), current_stream()),
          "dfn_upsample_bicubic_backward")
    return out


def composite_fine_backward(raw, z, grad_rgb):
    """d L/d raw [n,Nf,9] from d L/d rgb [n,3] through the test-time fine compositing (rgb only)."""
    raw, z, grad_rgb = _f32c(raw), _f32c(z), _f32c(grad_rgb)
    n, Nf = z.shape
    graw = torch.empty(n, Nf, 9, device=raw.device)
    check(_lib.load().dfn_composite_fine_backward(ptr(raw), ptr(z), ptr(grad_rgb), n, Nf, ptr(graw), current_stream()),
          "dfn_composite_fine_backward")
    return graw


def composite_fine_backward_maps(raw, z, grads, beta_min=0.1, grad_raw=None):
    """d L/d raw [n,Nf,9] through the fine compositing (models/rendering.py:161-243) from the upstream gradients of ALL its outputs:
    grads = {name: tensor} over rgb, rgb_static, rgb_transient [n,3] and acc, depth, depth_static, disp, beta [n]; a missing name or
    None is a zero gradient.  grad_raw [n,Nf,9]: a gradient that reaches raw directly, added in the same kernel
    (dfn_composite_fine_backward_maps)."""
    raw, z = _f32c(raw), _f32c(z)
    n, Nf = z.shape
    held = _map_grads(grads, n)
    if grad_raw is not None:
        grad_raw = _f32c(grad_raw).reshape(n, Nf, 9)
    graw = torch.empty(n, Nf, 9, device=raw.device)
    st = _map_grads_at(held)
    check(_lib.load().dfn_composite_fine_backward_maps(ptr(raw), ptr(z), n, Nf, float(beta_min), ctypes.byref(st), ptr(grad_raw), ptr(graw),
                                                       current_stream()), "dfn_composite_fine_backward_maps")
    return graw


TRAIN_GRAD_NAMES = tuple(n for n, _ in _lib.TrainMapGrads._fields_)   # rgb, disp, acc, depth, beta, rgb0, disp0, acc0, depth0


def train_map_grads(grads, n):
    """({name: contiguous fp32 tensor [n] / [n,3]} of the non-None entries of `grads`, kept alive by the caller; the dfn_train_map_grads
    struct pointing at them): the upstream gradients of the outputs of the training render, a missing name or None = zero."""
    grads = grads or {}
    unknown = [k for k in grads if k not in TRAIN_GRAD_NAMES]
    if unknown:
        raise ValueError(f"unknown upstream gradient(s) {unknown}: the outputs of the training render are {list(TRAIN_GRAD_NAMES)}")
    held = {k: _f32c(t).reshape((n, 3) if k.startswith("rgb") else (n,)) for k, t in grads.items() if t is not None}
    return held, _lib.TrainMapGrads(**{k: t.data_ptr() for k, t in held.items()})


def composite_coarse_train_backward_maps(raw_c, z_c, grads, noise=None, noise_std=0.):
    """d L/d (pre-activation coarse outputs) [n,Nc,4] through the coarse pass of the training render (models/rendering.py:161-193,231-243)
    from grads = {name: tensor} over rgb0 [n,3] and disp0, acc0, depth0 [n] (dfn_composite_coarse_train_backward_maps)."""
    raw_c, z_c = _f32c(raw_c), _f32c(z_c)
    n, Nc = z_c.shape
    held, st = train_map_grads(grads, n)
    noise = None if noise is None else _f32c(noise).reshape(n, Nc)
    gpre = torch.empty(n, Nc, 4, device=raw_c.device)
    check(_lib.load().dfn_composite_coarse_train_backward_maps(ptr(raw_c), ptr(z_c), ptr(noise), float(noise_std), n, Nc, ctypes.byref(st),
                                                               ptr(gpre), current_stream()), "dfn_composite_coarse_train_backward_maps")
    return gpre


def composite_fine_train_backward_maps(raw, z, grads, g_tsigma=0., grad_raw=None):
    """d L/d (pre-activation fine outputs) [n,Nf,9] through the training compositor (models/rendering.py:168-209,241-242 with
    test_time=False) from grads = {name: tensor} over rgb [n,3] and disp, acc, depth, beta [n], the constant d L/d transient_sigma and
    grad_raw [n,Nf,9], a gradient that reaches raw directly (dfn_composite_fine_train_backward_maps)."""
    raw, z = _f32c(raw), _f32c(z)
    n, Nf = z.shape
    held, st = train_map_grads(grads, n)
    grad_raw = None if grad_raw is None else _f32c(grad_raw).reshape(n, Nf, 9)
    gpre = torch.empty(n, Nf, 9, device=raw.device)
    check(_lib.load().dfn_composite_fine_train_backward_maps(ptr(raw), ptr(z), n, Nf, ctypes.byref(st), float(g_tsigma), ptr(grad_raw),
                                                             ptr(gpre), current_stream()), "dfn_composite_fine_train_backward_maps")
    return gpre


def frame_prep(rgb_u8, H, W, hist_bins=10):
    """Dataset front-end of one frame on the device (dfn_frame_prep; seven_scenes.py:324-352): rgb_u8 CUDA uint8
    [h, w, 3] -> (img fp32 [3, H, W] in [0, 1], INTER_AREA-downscaled; hist fp32 [hist_bins], NeRF-H's histogram index
    vector)."""
    assert rgb_u8.is_cuda and rgb_u8.dtype == torch.uint8 and rgb_u8.dim() == 3 and rgb_u8.shape[2] == 3
    rgb_u8 = rgb_u8.contiguous()
    lib = _lib.load()
    h, w = int(rgb_u8.shape[0]), int(rgb_u8.shape[1])
    img = torch.empty(3, int(H), int(W), device=rgb_u8.device)
    hist = torch.empty(int(hist_bins), device=rgb_u8.device)
    scratch = torch.empty(lib.dfn_frame_prep_scratch_bytes(), dtype=torch.uint8, device=rgb_u8.device)
    check(lib.dfn_frame_prep(ctypes.c_void_p(rgb_u8.data_ptr()), h, w, int(H), int(W), int(hist_bins), ptr(img), ptr(hist),
                             ctypes.c_void_p(scratch.data_ptr()), current_stream()), "dfn_frame_prep")
    return img, hist


def frame_post(rgb, disp, gt=None, want_gt8=True):
    """render_path's per-frame back-end on the device (dfn_frame_post; models/rendering.py:423-452): rgb [n,H,W,3], disp [n,H,W]
    fp32 CUDA, gt None | [n,H,W,3] | [H,W,3] (one ground-truth frame for every render) -> dict(rgb8, disp8 uint8 CUDA,
    gt8 | None, mse fp32 [n] | None, disp_max fp32 [n])."""
    lib = _lib.load()
    rgb, disp = _f32c(rgb), _f32c(disp)
    n, H, W = disp.shape
    dev = rgb.device
    per_frame = gt is not None and gt.dim() == 4
    if gt is not None:
        gt = _f32c(gt)
    rgb8 = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
    disp8 = torch.empty(n, H, W, dtype=torch.uint8, device=dev)
    gt8 = None
    if gt is not None and want_gt8:
        gt8 = torch.empty((n, H, W, 3) if per_frame else (H, W, 3), dtype=torch.uint8, device=dev)
    mse = torch.empty(n, device=dev) if gt is not None else None
    dmax = torch.empty(n, device=dev)
    scratch = torch.empty(lib.dfn_frame_post_scratch_bytes(n), dtype=torch.uint8, device=dev)
    raw = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    check(lib.dfn_frame_post(ptr(rgb), ptr(disp), ptr(gt), 1 if per_frame else 0, n, H, W, raw(rgb8), raw(disp8), raw(gt8), ptr(mse),
                             ptr(dmax), raw(scratch), current_stream()), "dfn_frame_post")
    return {"rgb8": rgb8, "disp8": disp8, "gt8": gt8, "mse": mse, "disp_max": dmax}


def frame_post_maps(maps, near, far, gt=None, want=None):
    """render_path's per-frame back-end for the render maps on the device (dfn_frame_post_maps).  maps: {name: fp32 CUDA tensor} with names out
    of MAP_NAMES, depth / depth_static / beta [n,H,W], rgb_static / rgb_transient [n,H,W,3]; gt None | [n,H,W,3] | [H,W,3] as in frame_post;
    want: the names to quantise (None = every given one).  Returns a dict with, for what the names and gt allow: depth16, depth_static16
    uint16 [n,H,W] on the fixed scale (d - near) / (far - near); beta8 uint8 [n,H,W] with beta_max fp32 [n]; rgb_static8, rgb_transient8
    uint8 [n,H,W,3]; mse_static fp32 [n] (rgb_static against gt)."""
    lib = _lib.load()
    names = map_names(tuple(maps))
    want = names if want is None else map_names(want)
    missing = [m for m in want if m not in names]
    if missing:
        raise ValueError(f"frame_post_maps: {missing} wanted but not among the given maps {list(names)}")
    if not names:
        return {}
    held = {m: _f32c(maps[m]) for m in names}
    n, H, W = held[names[0]].shape[:3]
    for m, t in held.items():
        if tuple(t.shape) != ((n, H, W, 3) if m.startswith("rgb_") else (n, H, W)):
            raise ValueError(f"frame_post_maps: {m} has shape {tuple(t.shape)}, expected [{n},{H},{W}" + (",3]" if m.startswith("rgb_") else "]"))
    dev = held[names[0]].device
    per_frame = gt is not None and gt.dim() == 4
    if gt is not None:
        gt = _f32c(gt)
    suffix = lambda m: "16" if m.startswith("depth") else "8"
    res = {m + suffix(m): torch.empty(held[m].shape, dtype=torch.uint16 if suffix(m) == "16" else torch.uint8, device=dev) for m in want}
    if "beta" in want:
        res["beta_max"] = torch.empty(n, device=dev)
    if gt is not None and "rgb_static" in want:
        res["mse_static"] = torch.empty(n, device=dev)
    if not res:
        return res
    scratch = torch.empty(lib.dfn_frame_post_maps_scratch_bytes(n), dtype=torch.uint8, device=dev)
    raw = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    m_in = _lib.RenderMaps(**{m: t.data_ptr() for m, t in held.items()})
    m_out = _lib.FrameMapsOut(**{m + suffix(m): res[m + suffix(m)].data_ptr() for m in want})
    check(lib.dfn_frame_post_maps(ctypes.byref(m_in), ptr(gt) if "mse_static" in res else None, 1 if per_frame else 0, n, H, W, float(near),
                                  float(far), ctypes.byref(m_out), raw(res.get("beta_max")), raw(res.get("mse_static")), raw(scratch),
                                  current_stream()), "dfn_frame_post_maps")
    return res


# ------------------------------------------------------------------ mesh export (isosurface.hip; dfnet_amd/mesh.py is the user's side)
def _axes3(axes):
    xs, ys, zs = (_f32c(a).reshape(-1) for a in axes)
    if not (xs.is_cuda and ys.device == xs.device and zs.device == xs.device):
        raise ValueError("grid axes must be three fp32 CUDA vectors on one device")
    return xs, ys, zs


def grid_points(axes, i0=0, i1=None):
    """The nodes of planes i0 <= i < i1 of the grid spanned by axes = (xs [nx], ys [ny], zs [nz]) as pts [(i1 - i0) * ny, nz, 3]: rows
    of nz points, the layout the point queries read (dfn_grid_points)."""
    xs, ys, zs = _axes3(axes)
    nx, ny, nz = xs.numel(), ys.numel(), zs.numel()
    i1 = nx if i1 is None else int(i1)
    pts = torch.empty(max(i1 - int(i0), 0) * ny, nz, 3, device=xs.device)
    check(_lib.load().dfn_grid_points(ptr(xs), ptr(ys), ptr(zs), nx, ny, nz, int(i0), i1, ptr(pts), current_stream()), "dfn_grid_points")
    return pts


def isosurface(sigma, axes, iso):
    """Marching tetrahedra on the Kuhn split (dfn_isosurface_count -> read the totals -> dfn_isosurface_emit): sigma [nx,ny,nz] and the
    three axis vectors -> (verts fp32 [V,3], faces int32 [F,3]) on the device; `iso` is an fp32 value.  The read of the two totals is
    the one synchronisation; an empty surface is two empty tensors."""
    lib = _lib.load()
    sigma = _f32c(sigma)
    xs, ys, zs = _axes3(axes)
    if sigma.dim() != 3 or tuple(sigma.shape) != (xs.numel(), ys.numel(), zs.numel()) or sigma.device != xs.device:
        raise ValueError(f"sigma {tuple(sigma.shape)} on {sigma.device} does not match axes of {xs.numel()}, {ys.numel()}, {zs.numel()} "
                         f"nodes on {xs.device}")
    nx, ny, nz = sigma.shape
    dev = sigma.device
    nbytes = lib.dfn_isosurface_workspace_bytes(nx, ny, nz)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)   # 0 bytes for refused dimensions: the count entry names the reason
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    raw = lambda t: ctypes.c_void_p(t.data_ptr())
    check(lib.dfn_isosurface_count(ptr(sigma), nx, ny, nz, float(iso), raw(ws), nbytes, raw(totals), current_stream()),
          "dfn_isosurface_count")
    V, F = (int(v) for v in totals.tolist())
    verts = torch.empty(V, 3, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    if V or F:
        check(lib.dfn_isosurface_emit(ptr(sigma), ptr(xs), ptr(ys), ptr(zs), nx, ny, nz, float(iso), raw(ws), nbytes, ptr(verts), V,
                                      raw(faces), F, current_stream()), "dfn_isosurface_emit")
    return verts, faces
