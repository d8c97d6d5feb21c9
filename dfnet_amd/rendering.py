"""Host-side mirror of /root/reference/script/models/rendering.py: same function names, arguments
and return shapes (`render`, `render_path`, `render_test`, and the two stages a caller composes a renderer of their own from:
`raw2outputs_NeRFW`, differentiable in raw and z_vals, and `sample_pdf`), evaluated by the HIP library.

What the reference does per ray chunk in Python (`batchify_rays` -> `render_rays` -> `netchunk`
loops, rendering.py:245-351) is one call into libdfnet_hip.so here; `chunk`/`netchunk` are accepted
and ignored (tiling is internal).  `render_path`'s serial frame loop (rendering.py:420) becomes a
frame-sharded loop with one gather when torch.distributed is initialised (dfnet_amd/dist.py).

Test-time kwargs (`render_kwargs_test`: perturb=0, raw_noise_std=0, test_time=True) run on the packed MFMA engine;
training kwargs (`render_kwargs_train`: test_time=False, perturb, raw_noise_std) run on the exact-fp32 training kernels and
return tensors attached to autograd with the reference's extras (dfnet_amd/nerf_train.py).  `lindisp` works everywhere; `ndc`
and `c2w_staticcam` at test time without autograd (their only use in the reference: LLFF-style visualisation), at every netwidth, and with
render(..., diff_view=True) under autograd and in training mode too (the view directions become a tensor of their own: `_ViewdirsFn`,
`_NdcRaysFn` and the explicit-viewdirs form of the render nodes).  `white_bkgd=True`
raises: it is not a working option of this path in the reference either (rendering.py:295 passes it to the coarse compositor as
`output_transient`, which fails with a TypeError at test time and mis-slices the 4-channel coarse output in training).

Autograd: when grad is enabled and `c2w` / `rays` require grad (the DFNet_dm step,
feature/direct_feature_matching.py:340-376), `rgb_map` is returned attached to the graph through
torch.autograd.Function wrappers: the forward is composed from the stage entry points and keeps (z_fine, raw);
the backward runs the HIP gradient kernels on that saved state (compositing backward, fused fine-MLP input
gradient, ray / pose reductions) — the stateless dfn_render_image_backward / dfn_render_rays_backward compute
the same thing with an internal re-render.  disp_map / acc_map are returned detached (the reference's losses use
rgb only) unless render(..., diff_maps=True) is asked for: then disp_map, acc_map and the maps named by ret_maps come back attached
too (as in the reference, where they are torch expressions of raw, rendering.py:161-243), through the compositing backward for every
output (dfn_composite_fine_backward_maps) and the same network gradient.  The MLP gradient kernel defaults to the exact-fp32 MFMA path (`GRAD_PRECISION`), see
tests/test_gpu_grad.py.

There is one tracked forward (`_tracked_forward`) and one tracked backward (`_tracked_backward`) under all three Functions (`_RenderImageFn`,
`_RenderFramesFn`, `_RenderRaysFn`; diff_maps is a mode of the last).  The forward notes its route on ctx — generic width, one-pass or two-pass —
with Nc, Ni, near, far and lindisp as plain Python values; only tensors go through save_for_backward.
"""
import os
import time

import numpy as np
import torch

from . import dist as ddist
from .nerfw import to8b
from .ray_utils import get_rays, ndc_rays  # noqa: F401  (re-exported like the reference's `from models.ray_utils import *`)

DEBUG = False


def _engine_of(kwargs):
    q = kwargs.get('network_query_fn')
    eng = getattr(q, 'engine', None)
    if eng is None:
        raise TypeError("render(): render kwargs must come from dfnet_amd.nerfw.create_nerf "
                        "(network_query_fn carries the HIP engine)")
    return eng


GRAD_PRECISION = "f16x3"  # MLP gradient kernel: forward recompute AND gradient chain in split-f16 (per-point power-of-two
                          # gradient scale, fp32-grade: parity 6e-7 vs autograd); "f32": all fp32 MFMA
# Arithmetic of the tracked forward, whose (z_fine, raw) the backward starts from.  None = the engine's own
# precision (what the user renders with, f16 by default): outputs identical to the untracked render, and in the
# DFNet_dm step a pose gradient within 7e-6 of the all-fp32 one (tools/gpu_dm_step.py) at 43 instead of 55 ms per
# step.  "f32" (or "f16x3", 2.7x faster) makes the whole tracked path fp32-grade — needed only where the loss makes d c2w a badly conditioned
# signed sum (tests/test_gpu_grad.py::test_render_autograd_drop_in: random per-pixel weights on a 12x16 image,
# where the f16 forward's 1e-4 error is amplified to 1e-2).
GRAD_FORWARD_PRECISION = None   # with GRAD_TWO_PASS (below) this governs the COARSE net only: the fine net is split-f16 then
# Two-pass gradient (default with the split-f16 gradient kernel): the tracked forward runs the fine net in split-f16 and
# records its ReLU signs (dfn_mlp_fine_saving); the backward then starts from (raw, masks) and recomputes NO forward
# (dfn_mlp_fine_backward_saved) — the gradient kernel was half forward recompute.  The tracked render is fp32-grade as
# a side effect.  False: the one-pass kernel (forward recompute inside the backward).
GRAD_TWO_PASS = True


def _two_pass():
    return GRAD_TWO_PASS and GRAD_PRECISION == "f16x3"


def _tracked_forward(ctx, eng, o, d, v, hist, Nc, Ni, near, far, retraw=False, names=(), view_given=False):
    """The forward of every tracked render -> (rgb, disp, acc, {name: map} for `names`, raw if retraw else None).  Leaves on ctx
    what _tracked_backward starts from: the engine, the route taken and the render options as plain Python state, the tensors
    through save_for_backward.  view_given: v is an input of its own (not d/|d|): every route renders with it as given, and the
    backward returns d L/d v beside a d L/d rays_d that holds the point path alone."""
    ctx.eng, ctx.opts, ctx.view_given = eng, (Nc, Ni, near, far, eng.lindisp), view_given
    if eng.width != 128:
        # the register-resident gradient kernels (and their saved state) are netwidth 128: other widths render as usual and the
        # backward is the stateless generic-width gradient, which recomputes the forward layer by layer in exact fp32.  At
        # netwidth 256 (fast render kernels) GRAD_FORWARD_PRECISION, when set, names the arithmetic of this tracked forward.
        ctx.route = "generic"
        prec = GRAD_FORWARD_PRECISION if eng.fast else None
        if view_given:
            rgb, disp, acc, raw, maps = eng.render_rays_maps(o, d, hist, Nc, Ni, near, far, viewdirs=v, retraw=retraw, precision=prec, maps=names)
            ctx.save_for_backward(o, d, hist, v)
        else:
            rgb, disp, acc, raw, maps = eng.render_rays_maps(o, d, hist, Nc, Ni, near, far, retraw=retraw, precision=prec, maps=names)
            ctx.save_for_backward(o, d, hist)
        return rgb, disp, acc, maps, raw   # no raw is kept (the gradient recomputes it): the rendered tensor is the caller's own
    ctx.route = "two_pass" if _two_pass() else "one_pass"
    rgb, disp, acc, z, raw, *masks = eng.render_rays_saving(o, d, v, hist, Nc, Ni, near, far, precision=GRAD_FORWARD_PRECISION,
                                                           with_masks=ctx.route == "two_pass")
    ctx.save_for_backward(o, d, v, hist, z, raw, *masks)
    maps = eng.composite_fine_maps(raw, z, maps=names) if names else {}
    # the caller's raw is a copy: an in-place edit of it must not reach the state the backward reads
    return rgb, disp, acc, maps, (raw.clone() if retraw else None)


def _tracked_backward(ctx, g_rgb, g_raw=None, g_maps=None):
    """(d L/d rays_o, d L/d rays_d, None) from the state _tracked_forward left on ctx - or, after a forward with view_given,
    (d L/d rays_o, d L/d rays_d through the points alone, d L/d viewdirs).  g_raw: d L/d of the raw that retraw returned.
    g_maps None: d L/d rgb alone (never None: autograd materialises an unused output's gradient as zeros), through the rgb-only
    compositing backward (composite_fine_backward; g_raw is added afterwards).
    g_maps = {name: d L/d output or None} (diff_maps): with g_rgb, the upstream gradients of every compositor output, through
    composite_fine_backward_maps (g_raw is added in that kernel); an output the loss does not use is None = a NULL pointer.
    The two compositing backwards are different kernels with different rounding."""
    eng, saved = ctx.eng, ctx.saved_tensors
    Nc, Ni, near, far, lindisp = ctx.opts
    if g_maps is not None:
        g_maps = {k: g for k, g in dict(g_maps, rgb=g_rgb).items() if g is not None}
        g_rgb = None
        if not g_maps and g_raw is None:
            g_maps = dict(rgb=torch.zeros(saved[0].shape[0], 3, device=saved[0].device))
    if ctx.route == "generic":
        o, d, hist = saved[:3]
        eng.set_render_options(lindisp=lindisp)
        return eng.render_rays_backward(o, d, hist, Nc, Ni, near, far, g_rgb, viewdirs=saved[3] if ctx.view_given else None,
                                        precision="generic", grad_raw=g_raw, grad_maps=g_maps)
    o, d, v, hist, z, raw = saved[:6]
    masks = saved[6] if ctx.route == "two_pass" else None
    derive = not ctx.view_given
    if g_maps is None:
        return eng.backward_from_saved(o, d, v, hist, z, raw, g_rgb, derive, precision=GRAD_PRECISION, masks=masks, grad_raw=g_raw)
    graw = eng.composite_fine_backward_maps(raw, z, g_maps, grad_raw=g_raw)
    return eng.backward_from_saved(o, d, v, hist, z, raw, None, derive, precision=GRAD_PRECISION, masks=masks, graw=graw)


class _RenderImageFn(torch.autograd.Function):
    """rgb/disp/acc = render(c2w); backward: d L/d c2w from d L/d rgb.  The forward is composed from the stage
    entry points and keeps (rays, z_fine, raw), so backward differentiates from the saved state instead of
    re-rendering (dfn_render_image_backward is the stateless equivalent)."""

    @staticmethod
    def forward(ctx, c2w, eng, H, W, focal, hist, Nc, Ni, near, far):
        from . import engine as _e
        o, d, v = _e.raygen(H, W, focal, c2w.detach())
        rgb, disp, acc, _, _ = _tracked_forward(ctx, eng, o, d, v, hist, Nc, Ni, near, far)
        ctx.cfg = (H, W, focal)
        disp, acc = disp.reshape(H, W), acc.reshape(H, W)
        ctx.mark_non_differentiable(disp, acc)
        return rgb.reshape(H, W, 3), disp, acc

    @staticmethod
    def backward(ctx, g_rgb, _g_disp, _g_acc):
        from . import engine as _e
        go, gd, _ = _tracked_backward(ctx, g_rgb)
        return (_e.raygen_backward(*ctx.cfg, go, gd),) + (None,) * 9


class _RaygenFn(torch.autograd.Function):
    """get_rays as an autograd node (ray_utils.py:5-15): (rays_o, rays_d) [H*W,3] of a pose; backward: d L / d c2w [3,4] from the
    ray gradients (dfn_raygen_backward).  What lets a pose that requires grad reach the training render's ray gradients."""

    @staticmethod
    def forward(ctx, c2w, H, W, focal):
        from . import engine as _e
        o, d, _ = _e.raygen(H, W, focal, c2w.detach(), want_viewdirs=False)
        ctx.cfg = (H, W, focal)
        return o.reshape(-1, 3), d.reshape(-1, 3)

    @staticmethod
    def backward(ctx, go, gd):
        from . import engine as _e
        H, W, focal = ctx.cfg
        z = lambda g: torch.zeros(H * W, 3, device=(go if go is not None else gd).device) if g is None else g.contiguous()
        return _e.raygen_backward(H, W, focal, z(go), z(gd)), None, None, None


class _NdcRaysFn(torch.autograd.Function):
    """ndc_rays as an autograd node (ray_utils.py:27-44): (rays_o, rays_d) in normalised device coordinates, shaped like the inputs;
    backward: d L/d (rays_o, rays_d) from the gradients of the NDC rays (dfn_ndc_rays_backward).  The forward is engine.ndc_rays: the
    same bits as the untracked call."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, H, W, focal, near):
        from . import engine as _e
        o, d = rays_o.detach().contiguous().float(), rays_d.detach().contiguous().float()
        no, nd = _e.ndc_rays(H, W, focal, near, o.reshape(-1, 3), d.reshape(-1, 3))
        ctx.save_for_backward(o, d)
        ctx.cfg = (H, W, focal, near)
        ctx.set_materialize_grads(False)
        return no.reshape(o.shape), nd.reshape(d.shape)

    @staticmethod
    def backward(ctx, g_no, g_nd):
        from . import engine as _e
        o, d = ctx.saved_tensors
        if g_no is None and g_nd is None:
            return (None,) * 6
        go, gd = _e.ndc_rays_backward(*ctx.cfg, o, d, g_no, g_nd)
        return go.reshape(o.shape), gd.reshape(d.shape), None, None, None, None


class _ViewdirsFn(torch.autograd.Function):
    """viewdirs = rays_d / |rays_d| (rendering.py:364-371) as an autograd node: the torch expression of the untracked path (the same
    bits) forward, dfn_viewdirs_backward backward."""

    @staticmethod
    def forward(ctx, rays_d):
        d = rays_d.detach().contiguous().float()
        ctx.save_for_backward(d)
        return d / torch.norm(d, dim=-1, keepdim=True)

    @staticmethod
    def backward(ctx, g_v):
        from . import engine as _e
        d, = ctx.saved_tensors
        return _e.viewdirs_backward(d, g_v).reshape(d.shape)


class _RenderFramesFn(torch.autograd.Function):
    """rgb [B,H,W,3] = render of B frames (each with its own pose and histogram vector) as ONE ray batch: the DFNet_dm step
    renders every frame of its mini-batch (direct_feature_matching.py:340-348 loops over them); batching them gives each
    kernel B times the work per launch.  backward: d L/d c2w [B,3,4] from d L/d rgb."""

    @staticmethod
    def forward(ctx, c2ws, eng, H, W, focal, hists, Nc, Ni, near, far):
        from . import engine as _e
        B = c2ws.shape[0]
        o, d, v = (t.reshape(-1, 3) for t in _e.raygen_frames(H, W, focal, c2ws.detach()))
        hist = hists.reshape(B, 1, -1).expand(B, H * W, hists.shape[-1]).reshape(B * H * W, -1).contiguous()   # one row per ray
        rgb = _tracked_forward(ctx, eng, o, d, v, hist, Nc, Ni, near, far)[0]
        ctx.cfg = (B, H, W, focal)
        return rgb.reshape(B, H, W, 3)

    @staticmethod
    def backward(ctx, g_rgb):
        from . import engine as _e
        B, H, W, focal = ctx.cfg
        go, gd, _ = _tracked_backward(ctx, g_rgb)
        gc = _e.raygen_frames_backward(H, W, focal, go.reshape(B, H * W, 3), gd.reshape(B, H * W, 3))
        return (gc,) + (None,) * 9


def render_frames(H, W, focal, c2ws, img_idx, **kwargs):
    """rgb [B,H,W,3] of B frames at poses c2ws [B,3,4] with histogram vectors img_idx [B,bins] — render(c2w=...) per frame,
    batched into one launch per stage, differentiable w.r.t. c2ws.  Same option checks as render()."""
    near, far = kwargs.pop('near', 0.), kwargs.pop('far', 1.)
    if kwargs.get('diff_maps', False):
        raise NotImplementedError("dfnet_amd render_frames(): not implemented natively yet: diff_maps (render_frames returns rgb alone; use "
                                  "render(c2w=..., diff_maps=True) per frame) — there is deliberately no CPU fallback")
    _check_test_time(kwargs, kwargs.get('ndc', False), None, kwargs.get('use_viewdirs', True), tracked=True)
    eng = _engine_of(kwargs)
    _set_options(eng, kwargs, near)
    c2ws = c2ws[:, :3, :4]
    hists = torch.as_tensor(img_idx, dtype=torch.float32, device=c2ws.device).reshape(c2ws.shape[0], -1)
    return _RenderFramesFn.apply(c2ws, eng, int(H), int(W), float(focal), hists, int(kwargs['N_samples']), int(kwargs['N_importance']),
                                 float(near), float(far))


class _RenderRaysFn(torch.autograd.Function):
    """(rgb, disp, acc, *maps[, raw]) = render(rays); backward: d L/d rays_o, d L/d rays_d (viewdirs = d/|d| differentiated).
    With retraw, `raw` [n,Nf,9] is attached too (rendering.py:353-400 with retraw=True under autograd: a function of the sample points and
    view directions, the depths are detached): the fine network's backward is a full vector-Jacobian product of all nine raw channels,
    so an external d L/d raw is ADDED to the compositor's d L/d raw before it.
    names None: rgb (and raw) alone are differentiable, disp and acc come back detached and there are no maps.
    names a tuple (render(diff_maps=True)): EVERY output is attached - disp_map, acc_map and the maps named by ret_maps are differentiable
    functions of raw in the reference (raw2outputs_NeRFW, rendering.py:161-243) - and their upstream gradients go through the compositing
    backward for every output (_tracked_backward).
    viewdirs (render(ndc / c2w_staticcam, diff_view=True), rendering.py:364-376): None, or the view directions [n,3] as a tensor input of
    its own - rendered with as given, d L/d viewdirs returned as that input's gradient, and rays_d then receives the point path alone."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, eng, hist, Nc, Ni, near, far, retraw=False, names=None, viewdirs=None):
        o, d = rays_o.detach().contiguous(), rays_d.detach().contiguous()
        v = d / torch.norm(d, dim=-1, keepdim=True) if viewdirs is None else viewdirs.detach().contiguous()
        ctx.names, ctx.retraw = names, retraw
        rgb, disp, acc, maps, raw = _tracked_forward(ctx, eng, o, d, v, hist, Nc, Ni, near, far, retraw, names or (),
                                                     view_given=viewdirs is not None)
        if names is None:
            ctx.mark_non_differentiable(disp, acc)
        else:
            ctx.set_materialize_grads(False)   # an output the loss does not use arrives as None = a NULL upstream pointer
        return (rgb, disp, acc) + tuple(maps[k] for k in names or ()) + ((raw,) if retraw else ())

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, *rest):
        g_raw = rest[-1] if ctx.retraw else None
        g_maps = None if ctx.names is None else dict(zip(("disp", "acc") + ctx.names, (g_disp, g_acc) + rest))
        go, gd, gv = _tracked_backward(ctx, g_rgb, g_raw, g_maps)
        return (go, gd) + (None,) * 8 + (gv if ctx.view_given else None,)


def _set_options(eng, kw, near):
    """The render_rays keyword options the handle carries (lindisp, rendering.py:272-273)."""
    lindisp = bool(kw.get('lindisp', False))
    if lindisp and not float(near) > 0.:
        raise ValueError("render(): lindisp=True needs near > 0 (the depths are 1 / ((1 - t) / near + t / far))")
    eng.set_render_options(lindisp=lindisp)


def _check_test_time(kw, ndc, c2w_staticcam, use_viewdirs, training=False, tracked=False, ret_maps=False, diff_maps=False, diff_view=False):
    bad = []
    if kw.get('white_bkgd', False):
        raise TypeError("render(): white_bkgd=True is not a working option of the NeRF-H path: the reference hands it to the coarse "
                        "compositor as output_transient (models/rendering.py:295) and fails the same way")
    if (ndc or c2w_staticcam is not None) and (training or tracked) and not diff_view:
        bad.append("ndc / c2w_staticcam together with " + ("training-mode rendering" if training else "autograd") +
                   " without diff_view=True (render(..., diff_view=True) opts in; render_frames has no such form)")
    if ret_maps and (training or tracked) and not diff_maps:
        bad.append("ret_maps together with " + ("training-mode rendering without diff_maps" if training else
                                                "autograd (the maps are not differentiable)"))
    if not training:
        if not kw.get('test_time', False):
            bad.append("test_time=False without a trainer (render kwargs must come from create_nerf with gradient updates enabled)")
        if float(kw.get('perturb', 0.) or 0.) > 0.:
            bad.append("perturb>0 at test time")
        if float(kw.get('raw_noise_std', 0.) or 0.) != 0.:
            bad.append("raw_noise_std!=0 at test time")
    if not use_viewdirs:
        bad.append("use_viewdirs=False")
    if int(kw.get('N_importance', 0)) <= 0:
        bad.append("N_importance=0")
    if bad:
        raise NotImplementedError("dfnet_amd render(): not implemented natively yet: " + "; ".join(bad) +
                                  " — there is deliberately no CPU fallback")


def _shaped(lead, rgb, disp, acc, extras):
    """render()'s return value from per-ray outputs: every tensor with its leading dimension reshaped to `lead`."""
    return [rgb.reshape(lead + [3]), disp.reshape(lead), acc.reshape(lead), {k: v.reshape(lead + list(v.shape[1:])) for k, v in extras.items()}]


def _diff_view_rays(H, W, focal, rays, c2w, c2w_staticcam, ndc, dev):
    """rendering.py:364-376 as the reference runs it under autograd -> (rays_o [n,3], rays_d [n,3], viewdirs [n,3], leading shape): the
    view directions come from the given rays / pose (`_ViewdirsFn`), the rays that are marched are then the static camera's and / or
    the NDC ones (`_NdcRaysFn` at near = 1); a pose that requires grad reaches its rays through `_RaygenFn`.  Whatever does not require
    grad (or everything, under no_grad) takes the untracked calls: the values are the same bits either way."""
    grad = torch.is_grad_enabled()

    def rays_of(pose):
        pose = torch.as_tensor(pose, dtype=torch.float32, device=dev)
        if grad and pose.requires_grad:
            return tuple(t.reshape(int(H), int(W), 3) for t in _RaygenFn.apply(pose[:3, :4].contiguous(), int(H), int(W), float(focal)))
        return get_rays(H, W, focal, pose)

    if c2w is not None:
        rays_o, rays_d = rays_of(c2w)
    else:
        rays_o, rays_d = (torch.as_tensor(t, dtype=torch.float32, device=dev) for t in rays)
    lead = list(rays_d.shape[:-1])
    view = rays_d.reshape(-1, 3)
    view = _ViewdirsFn.apply(view) if grad and view.requires_grad else view / torch.norm(view, dim=-1, keepdim=True)
    if c2w_staticcam is not None:
        rays_o, rays_d = rays_of(c2w_staticcam)
    if ndc:
        if grad and (rays_o.requires_grad or rays_d.requires_grad):
            rays_o, rays_d = _NdcRaysFn.apply(rays_o, rays_d, int(H), int(W), float(focal), 1.)
        else:
            rays_o, rays_d = ndc_rays(H, W, focal, 1., rays_o, rays_d)
    rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    if rays_d.shape[0] != view.shape[0]:
        raise ValueError(f"render(): c2w_staticcam gives {rays_d.shape[0]} rays of an H x W image, the view directions have {view.shape[0]} rows")
    return rays_o, rays_d, view, lead


def render(H, W, focal, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0., far=1., use_viewdirs=False,
           c2w_staticcam=None, img_idx=torch.Tensor(0), ret_maps=False, diff_maps=False, diff_view=False, **kwargs):
    """Drop-in for rendering.py:353-400.  Returns [rgb_map, disp_map, acc_map, extras].

    diff_view (opt-in): ndc=True and c2w_staticcam (rendering.py:364-376) under autograd at test time - rays, c2w or c2w_staticcam
    requiring grad - and in training mode, as in the reference, where both are plain tensor ops: the view directions of the given rays /
    pose become a tensor input of the render node, the marched rays are the static camera's and / or the NDC ones, and every gradient
    reaches what it came from (c2w through the view directions alone once c2w_staticcam replaces its rays).  Composes with retraw and
    diff_maps.  False: both options are refused there, as ever.  Without ndc / c2w_staticcam the keyword changes nothing.

    ret_maps (beyond the reference, test time; under autograd only together with diff_maps): True, or an iterable of names out of depth, depth_static, beta,
    rgb_static, rgb_transient — the maps raw2outputs_NeRFW forms and the reference drops (rendering.py:196-241) are added to
    `extras` under those names, shaped like the rays ([H,W] / [H,W,3] for c2w).

    Training mode (test_time=False) with diff_maps=True: disp_map, acc_map, disp0, acc0 (and raw with retraw) come back attached as well, as the
    reference's are (rendering.py:161-243, :295-331; z_std stays detached, rendering.py:302), and ret_maps names depth / depth0 (True:
    both), the sums w z of rendering.py:241 in the fine and the coarse pass, attached too.  Without diff_maps the training render is
    what it was: gradients through rgb, rgb0, beta and transient_sigmas, ret_maps refused.

    diff_maps (opt-in, test time): under autograd (rays or c2w requiring grad) disp_map, acc_map and the maps of ret_maps come back attached
    to the graph as well, as the reference's are (they are torch expressions of raw, rendering.py:161-243).  False: as ever, disp_map and
    acc_map detached and ret_maps refused under autograd.  Without autograd it changes nothing.

    c2w given: full image, outputs [H,W,3], [H,W], [H,W].  Otherwise `rays` = (rays_o, rays_d) (a tuple
    or a stacked [2,N,3] tensor), outputs shaped like rays_d[..., :1].  `img_idx`: the 10-bin histogram
    index vector, shape [10], [1,10] or [N,10]."""
    eng = _engine_of(kwargs)
    _set_options(eng, kwargs, near)
    from .engine import map_names
    trainer = getattr(kwargs.get('network_query_fn'), 'trainer', None)
    training = not kwargs.get('test_time', False) and trainer is not None
    if training and diff_maps:
        from .nerf_train import train_map_names as map_names   # depth, depth0: what the training render forms at rendering.py:241
    map_list = map_names(ret_maps)
    if training:
        # training mode (rendering.py:245-337 with test_time=False): stratified depths, coarse rgb + noise, importance sampling
        # with random u, the training extras — on the exact-fp32 training kernels, attached to autograd (nerf_train.py)
        _check_test_time(kwargs, ndc, c2w_staticcam, use_viewdirs, training=True, ret_maps=bool(map_list), diff_maps=bool(diff_maps),
                         diff_view=bool(diff_view))
        # The reference's training render is differentiable w.r.t. its rays / pose too: rays that require grad make the autograd node
        # run the exact-fp32 step and return d L / d rays (nerf_train._RenderTrainFn); c2w reaches them through get_rays' own node.
        from . import nerf_train
        dev = torch.device("cuda", torch.cuda.current_device())
        view = None
        if ndc or c2w_staticcam is not None:   # (diff_view: refused above without it)
            rays_o, rays_d, view, lead = _diff_view_rays(H, W, focal, rays, c2w, c2w_staticcam, ndc, dev)
        elif c2w is not None:
            c2w = torch.as_tensor(c2w, dtype=torch.float32, device=dev)
            if torch.is_grad_enabled() and c2w.requires_grad:
                rays_o, rays_d = _RaygenFn.apply(c2w[:3, :4].contiguous(), int(H), int(W), float(focal))
                rays_o, rays_d = rays_o.reshape(int(H), int(W), 3), rays_d.reshape(int(H), int(W), 3)
            else:
                rays_o, rays_d = get_rays(H, W, focal, c2w)
        else:
            rays_o, rays_d = rays
        rays_o = torch.as_tensor(rays_o, dtype=torch.float32, device=dev)
        rays_d = torch.as_tensor(rays_d, dtype=torch.float32, device=dev)
        if view is None:
            lead = list(rays_d.shape[:-1])
        hist = torch.as_tensor(img_idx, dtype=torch.float32, device=dev).reshape(-1, eng.hist_bin)
        rgb, disp, acc, extras = nerf_train.render_train(trainer, rays_o.reshape(-1, 3), rays_d.reshape(-1, 3), hist, int(kwargs['N_samples']),
                                                         int(kwargs['N_importance']), near, far, float(kwargs.get('perturb', 0.) or 0.),
                                                         float(kwargs.get('raw_noise_std', 0.) or 0.), bool(kwargs.get('retraw', False)),
                                                         draws=kwargs.get('draws'), diff_maps=bool(diff_maps), maps=map_list, viewdirs=view)
        # (no `stale` mark here: a render does not move the weights; HipQuery.refresh() sees optimizer steps through the tensors'
        #  version counters, and the training loop marks them itself)
        return _shaped(lead, rgb, disp, acc, extras)
    if hasattr(kwargs.get('network_query_fn'), 'refresh'):
        kwargs.get('network_query_fn').refresh()
    def _needs_grad(t):
        if torch.is_tensor(t):
            return t.requires_grad
        return isinstance(t, (tuple, list)) and any(_needs_grad(u) for u in t)
    view_opts = bool(ndc) or c2w_staticcam is not None
    track = torch.is_grad_enabled() and (_needs_grad(c2w) or _needs_grad(rays) or (bool(diff_view) and view_opts and _needs_grad(c2w_staticcam)))
    diff_maps = bool(diff_maps) and track   # nothing to attach to without autograd
    _check_test_time(kwargs, ndc, c2w_staticcam, use_viewdirs, tracked=track, ret_maps=bool(map_list), diff_maps=diff_maps,
                     diff_view=bool(diff_view))
    Nc, Ni = int(kwargs['N_samples']), int(kwargs['N_importance'])
    retraw = bool(kwargs.get('retraw', False))
    dev = torch.device("cuda", torch.cuda.current_device())
    hist = torch.as_tensor(img_idx, dtype=torch.float32, device=dev)

    def _rays(o, d, h, lead, view=None):
        """The untracked ray render; the maps of ret_maps come with the same rgb / disp / acc bits."""
        rgb, disp, acc, raw, extras = eng.render_rays_maps(o, d, h, Nc, Ni, near, far, viewdirs=view, retraw=retraw, maps=map_list)
        if retraw:
            extras['raw'] = raw
        return _shaped(lead, rgb, disp, acc, extras)

    def _tracked_rays(o, d, h, lead, view=None):
        """The tracked ray render.  diff_maps: every output attached, the maps of ret_maps among them; otherwise rgb (and raw) alone,
        and ret_maps was refused above.  view: explicit view directions, a differentiable input of their own."""
        out = _RenderRaysFn.apply(o, d, eng, h, Nc, Ni, float(near), float(far), retraw, tuple(map_list) if diff_maps else None, view)
        extras = dict(zip(map_list, out[3:]))
        if retraw:
            extras['raw'] = out[-1]
        return _shaped(lead, *out[:3], extras)

    if view_opts and track:   # (diff_view: refused above without it) rendering.py:364-376 under autograd
        o, d, view, lead = _diff_view_rays(H, W, focal, rays, c2w, c2w_staticcam, ndc, dev)
        hist = hist.reshape(-1, eng.hist_bin)
        if hist.shape[0] not in (1, o.shape[0]):
            raise ValueError(f"img_idx must have 1 or {o.shape[0]} rows of {eng.hist_bin} bins, got {tuple(hist.shape)}")
        return _tracked_rays(o, d, hist, lead, view)
    if view_opts:   # untracked: the same composition, every step the plain call
        with torch.no_grad():
            o, d, view, lead = _diff_view_rays(H, W, focal, rays, c2w, c2w_staticcam, ndc, dev)
        return _rays(o, d, hist.reshape(-1, eng.hist_bin), lead, view)
    if c2w is not None:
        c2w = torch.as_tensor(c2w, dtype=torch.float32, device=dev)
        if retraw or diff_maps or hist.numel() != eng.hist_bin:   # what the image entries do not do: through the image's rays
            if track and c2w.requires_grad:    # the pose reaches the ray gradients through get_rays' own node
                o, d = (t.reshape(int(H), int(W), 3) for t in _RaygenFn.apply(c2w[:3, :4].contiguous(), int(H), int(W), float(focal)))
            else:
                o, d = get_rays(H, W, focal, c2w)
            return render(H, W, focal, chunk, rays=(o, d), ndc=ndc, near=near, far=far, use_viewdirs=use_viewdirs,
                          img_idx=img_idx, ret_maps=map_list, diff_maps=diff_maps, **kwargs)
        if track:   # (ret_maps was refused above: the maps are differentiable only with diff_maps)
            rgb, disp, acc = _RenderImageFn.apply(c2w[:3, :4], eng, int(H), int(W), float(focal), hist.reshape(-1), Nc, Ni,
                                                  float(near), float(far))
            extras = {}
        else:
            rgb, disp, acc, _, extras = eng.render_image_maps(c2w, int(H), int(W), float(focal), hist, Nc, Ni, near, far, maps=map_list)
        return [rgb, disp, acc, extras]   # the image entries shape their outputs [H,W,...] themselves
    rays_o, rays_d = rays
    rays_o = torch.as_tensor(rays_o, dtype=torch.float32, device=dev)
    rays_d = torch.as_tensor(rays_d, dtype=torch.float32, device=dev)
    sh = rays_d.shape
    n = rays_d.numel() // 3
    hist = hist.reshape(-1, eng.hist_bin)
    if hist.shape[0] not in (1, n):
        raise ValueError(f"img_idx must have 1 or {n} rows of {eng.hist_bin} bins, got {tuple(hist.shape)}")
    lead = list(sh[:-1])
    o, d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    if not track:
        return _rays(o, d, hist, lead)
    return _tracked_rays(o, d, hist, lead)


# ------------------------------------------------------------------------------------------ the compositor and the sampler as public stages
_R2O_OUTPUTS = {1: ("acc", "weights"), 4: ("rgb", "disp", "acc", "weights", "depth"), 9: ("rgb", "disp", "acc", "weights", "depth", "beta")}


class _Raw2OutputsFn(torch.autograd.Function):
    """engine.raw2outputs attached to autograd with respect to raw and z_vals (dfn_raw2outputs_backward).  The outputs are those of the
    mode (_R2O_OUTPUTS by channel count); one the loss does not use arrives as None = a NULL upstream pointer, and needs_input_grad
    decides which of d L/d raw and d L/d z_vals the kernel computes."""

    @staticmethod
    def forward(ctx, raw, z, noise, noise_std, beta_min, opts):
        from . import engine as _e
        raw, z = raw.detach().contiguous(), z.detach().contiguous()
        out = _e.raw2outputs(raw, z, noise, noise_std, beta_min, **opts)
        ctx.save_for_backward(raw, z, noise)
        ctx.noise_std, ctx.beta_min, ctx.opts = noise_std, beta_min, opts
        ctx.names = _R2O_OUTPUTS[1 if raw.dim() == 2 else raw.shape[-1]]
        ctx.set_materialize_grads(False)
        return tuple(out[k] for k in ctx.names)

    @staticmethod
    def backward(ctx, *gs):
        from . import engine as _e
        raw, z, noise = ctx.saved_tensors
        want = tuple(k for k, need in zip(("raw", "z"), ctx.needs_input_grad[:2]) if need)
        grads = {k: g for k, g in zip(ctx.names, gs) if g is not None}
        if not grads or not want:
            return (None,) * 6
        graw, gz = _e.raw2outputs_backward(raw, z, grads, noise, ctx.noise_std, ctx.beta_min, want=want, **ctx.opts)
        return (graw, gz) + (None,) * 4


def raw2outputs_NeRFW(raw, z_vals, rays_d, raw_noise_std=0, output_transient=False, beta_min=0.1, white_bkgd=False, test_time=False,
                      static_only=True, typ="coarse", noise=None):
    """Drop-in for models/rendering.py:132-243 on the device: the reference's signature and argument order plus `noise`, and its 7-tuple
    (rgb_map, disp_map, acc_map, weights, depth_map, transient_sigmas, beta).

    Modes and what they return, as in the reference:
      typ == "coarse" and test_time: raw [n,N,C>=1], channel 0 = sigma -> (None, None, acc, weights, None, None, None); with
        output_transient=True a TypeError, as there (`deltas * None`);
      output_transient=False otherwise: raw [n,N,4] = (rgb, sigma) -> beta is zeros [n], transient_sigmas None;
      output_transient=True: raw [n,N,9] -> everything, transient_sigmas = raw[..., 7]; with test_time and static_only the depth (and
        with it disp) comes from the static field's own transmittance.
    Another channel count raises NotImplementedError: feature heads are not part of the NeRF-H path.  rays_d is accepted and unused, as
    in the reference.  Inputs are fp32 device tensors; there is no CPU fallback.

    noise [n,N]: the draws the reference takes from torch.randn_like at :173 (multiplied by raw_noise_std, added to sigma before the
    relu).  Without it, raw_noise_std != 0 draws torch.randn on the device; at raw_noise_std == 0 NOTHING is drawn - the reference draws
    even then (and multiplies by 0), so a caller who relies on the generator's state after the call sees a difference.  The transient
    mode has no noise in the reference; an explicit `noise` there is refused.

    Autograd: under grad mode with raw or z_vals requiring grad every returned tensor is attached, and backward runs ONE kernel for
    d L/d raw and d L/d z_vals from whichever outputs the loss used (dfn_raw2outputs_backward; transient_sigmas is a slice of raw and
    needs none).  Otherwise this is the plain forward."""
    from . import engine as _e
    coarse_test = typ == "coarse" and bool(test_time)
    if coarse_test and output_transient:
        raise TypeError("raw2outputs_NeRFW: typ='coarse' with test_time and output_transient=True: transient_sigmas is None there "
                        "(unsupported operand type(s) for *: 'Tensor' and 'NoneType', models/rendering.py:170)")
    if raw.dim() != 3 or z_vals.dim() != 2 or raw.shape[:2] != z_vals.shape:
        raise ValueError(f"raw2outputs_NeRFW: raw [n,N,C] and z_vals [n,N] expected, got {tuple(raw.shape)} and {tuple(z_vals.shape)}")
    ch = raw.shape[-1]
    if not coarse_test and ch != (9 if output_transient else 4):
        raise NotImplementedError(f"raw2outputs_NeRFW: {ch} channels with output_transient={bool(output_transient)}: the NeRF-H path has "
                                  "(rgb, sigma) = 4 or static + transient = 9 (feature heads are not part of it)")
    std = 0. if output_transient else float(raw_noise_std)
    if output_transient and noise is not None:
        raise ValueError("raw2outputs_NeRFW: noise together with output_transient=True (the transient mode draws none)")
    if std != 0. and noise is None:
        noise = torch.randn(z_vals.shape, device=raw.device)
    if std == 0.:
        noise = None
    elif noise is not None:
        noise = noise.detach().float().contiguous()
    opts = dict(test_time=bool(test_time), static_only=bool(static_only), white_bkgd=bool(white_bkgd), coarse=typ == "coarse")
    arg = raw[..., 0] if coarse_test else raw   # a torch slice: its gradient needs no kernel
    if torch.is_grad_enabled() and (raw.requires_grad or z_vals.requires_grad):
        out = dict(zip(_R2O_OUTPUTS[1 if coarse_test else ch], _Raw2OutputsFn.apply(arg, z_vals, noise, std, float(beta_min), opts)))
    else:
        out = _e.raw2outputs(arg, z_vals, noise, std, float(beta_min), **opts)
        raw = raw.detach()   # (a slice of a leaf taken under no_grad would still say requires_grad)
    if coarse_test:
        return None, None, out["acc"], out["weights"], None, None, None
    if not output_transient:
        return out["rgb"], out["disp"], out["acc"], out["weights"], out["depth"], None, torch.zeros_like(out["acc"])
    return out["rgb"], out["disp"], out["acc"], out["weights"], out["depth"], raw[..., 7], out["beta"]


class _SamplePdfFn(torch.autograd.Function):
    """engine.sample_pdf attached to autograd with respect to bins, weights and an explicit u (dfn_sample_pdf_backward).  u None = the
    linspace draws, a constant; needs_input_grad decides which of the three gradients the kernel computes."""

    @staticmethod
    def forward(ctx, bins, weights, u, Ni):
        from . import engine as _e
        bins, weights = bins.detach().contiguous(), weights.detach().contiguous()
        u = None if u is None else u.detach().contiguous()
        ctx.save_for_backward(bins, weights, u)
        ctx.Ni = Ni
        return _e.sample_pdf(bins, weights, Ni, u=u)

    @staticmethod
    def backward(ctx, g):
        from . import engine as _e
        bins, weights, u = ctx.saved_tensors
        want = tuple(k for k, need in zip(("bins", "weights", "u"), ctx.needs_input_grad[:3]) if need)
        if not want:
            return (None,) * 4
        return _e.sample_pdf_backward(bins, weights, ctx.Ni, g, u=u, want=want) + (None,)


def sample_pdf(bins, weights, N_samples, det=False, pytest=False, u=None, diff=False):
    """Drop-in for models/rendering.py:24-65 on the device (dfn_sample_pdf): bins [n,nb], weights [n,nb-1] -> samples [n,N_samples].
    det: u = linspace(0, 1, N_samples); otherwise torch.rand on the device; pytest=True: the reference's np.random.seed(0) draws
    formed on the host (:39-47); u [n,N_samples]: explicit draws (this port's addition; it overrides the other three).

    diff=False (the default): the result is returned DETACHED whatever the inputs require, as the reference's only caller takes it
    (:302).  diff=True: the reference's function itself, which is differentiable in bins, weights and u - under grad mode with bins,
    weights or an explicit u requiring grad the samples are attached, and backward runs ONE kernel (dfn_sample_pdf_backward) for
    whichever of the three need a gradient.  The draws of det, pytest and torch.rand are constants and receive none; the search has no
    gradient, and where the cdf step of a bin is below 1e-5 its replaced denominator has none (torch.where).  With nothing requiring
    grad, or under no_grad, diff=True is the plain forward; the values are the same bits either way."""
    from . import engine as _e
    n = bins.shape[0]
    own_u = u is not None
    if u is None and pytest:
        np.random.seed(0)
        host = np.broadcast_to(np.linspace(0., 1., N_samples), (n, N_samples)) if det else np.random.rand(n, N_samples)
        u = torch.Tensor(np.ascontiguousarray(host)).to(bins.device)
    elif u is None and not det:
        u = torch.rand(n, N_samples, device=bins.device)
    if diff and torch.is_grad_enabled() and (bins.requires_grad or weights.requires_grad or (own_u and u.requires_grad)):
        return _SamplePdfFn.apply(bins, weights, u, int(N_samples))
    return _e.sample_pdf(bins.detach(), weights.detach(), int(N_samples), u=None if u is None else u.detach())


def _png_bytes(arr):
    """A PNG file as bytes from the minimal zlib writer (level 6, filter 0): uint8 gray [H,W] or RGB [H,W,3], or uint16 gray [H,W]
    (bit depth 16, big-endian samples)."""
    import struct
    import zlib
    a = np.ascontiguousarray(arr)
    h, w = a.shape[:2]
    ctype, depth = (2 if a.ndim == 3 else 0), 8
    if a.dtype == np.uint16:
        if a.ndim != 2:
            raise ValueError(f"16-bit PNGs are gray [H,W], got shape {a.shape}")
        a, depth = a.astype(">u2"), 16
    raw = b"".join(b"\x00" + a[r].tobytes() for r in range(h))
    chunk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def _write_png(path, arr8):
    """uint8 gray / RGB, or uint16 gray (PIL mode I;16), to `path`; PIL's default zlib level is 6 as well."""
    try:
        from PIL import Image
        Image.fromarray(arr8).save(path)
    except ImportError:  # minimal zlib PNG writer
        with open(path, "wb") as fh:
            fh.write(_png_bytes(arr8))


POST_BATCH = 16     # frames per dfn_frame_post call / device -> host copy / PNG job
PNG_WORKERS = 8     # host threads encoding PNGs while the GPU renders on (zlib releases the GIL)

# render map -> (its quantised plane out of engine.frame_post_maps, the PNG's suffix): 16-bit gray depths on the fixed near..far scale,
# 8-bit gray beta / max(beta), 8-bit RGB colours
MAP_PNGS = {"depth": ("depth16", "_depth"), "depth_static": ("depth_static16", "_depth_static"), "beta": ("beta8", "_beta"),
            "rgb_static": ("rgb_static8", "_static"), "rgb_transient": ("rgb_transient8", "_transient")}


def _write_frames(ev, host, savedir, first, maps_host=None):
    """PNG job of one batch (runs on a pool thread): wait for the batch's device -> host copy, then `{:03d}.png`,
    `{:03d}_GT.png`, `{:03d}_disp.png` per frame, numbered by GLOBAL frame index (rendering.py:438-452).  maps_host: {map name: quantised
    host tensor [n, ...]} of render_path(ret_maps=...) -> `{:03d}_depth.png` ... per MAP_PNGS as well."""
    ev.synchronize()
    rgb8, disp8, gt8 = (None if t is None else t.numpy() for t in host)
    planes = {m: t.numpy() for m, t in (maps_host or {}).items()}
    for k in range(rgb8.shape[0]):
        i = first + k
        _write_png(os.path.join(savedir, '{:03d}.png'.format(i)), rgb8[k])
        if gt8 is not None:
            _write_png(os.path.join(savedir, '{:03d}_GT.png'.format(i)), gt8[k] if gt8.ndim == 4 else gt8)
        _write_png(os.path.join(savedir, '{:03d}_disp.png'.format(i)), disp8[k])
        for m, a in planes.items():
            _write_png(os.path.join(savedir, '{:03d}{}.png'.format(i, MAP_PNGS[m][1])), a[k])


def _map_tail(m, H, W):
    return (H, W, 3) if m.startswith("rgb_") else (H, W)


def render_path(args, render_poses, hwf, chunk, render_kwargs, gt_imgs=None, savedir=None, render_factor=0,
                single_gt_img=False, img_ids=torch.Tensor(0), ret_maps=False):
    """Drop-in for rendering.py:403-458: returns (rgbs [N,H,W,3], disps [N,H,W]) as float32 numpy.

    With torch.distributed initialised (world > 1) each rank renders its contiguous block of frames.  The per-frame back-end
    (to8b truncation, disp / max(disp), the PSNR's mean squared error: rendering.py:423-452) runs on the device in batches
    of POST_BATCH frames (dfn_frame_post); what comes back to the host is uint8, and EVERY RANK writes the PNGs of its own
    block (`{:03d}.png`, `{:03d}_GT.png`, `{:03d}_disp.png` by global frame index) on a thread pool while its GPU renders the
    next batch.  One gather at the end brings the fp32 frames (the returned arrays) and the per-frame errors to rank 0, which
    prints the mean PSNR; ranks != 0 return (None, None).

    ret_maps (beyond the reference): True, or an iterable of names out of depth, depth_static, beta, rgb_static, rgb_transient — every frame
    is rendered with render(ret_maps=names) (rgb and disp keep their bits), the maps ride beside rgbs / disps through the same gather,
    and the return value becomes (rgbs, disps, {name: float32 numpy [N,H,W] / [N,H,W,3]}) on rank 0, (None, None, None) elsewhere.  With
    savedir their PNGs (MAP_PNGS; dfn_frame_post_maps per batch: depths 16-bit gray on the fixed near..far scale of render_kwargs, beta /
    max(beta) 8-bit gray, the colours 8-bit RGB) are written by the same pool job; with gt_imgs and rgb_static the static-only PSNR is
    printed too."""
    from concurrent.futures import ThreadPoolExecutor
    from . import engine as eng
    names = eng.map_names(ret_maps)
    H, W, focal = hwf
    if render_factor != 0:
        H, W, focal = int(H // render_factor), int(W // render_factor), focal / render_factor
    H, W = int(H), int(W)
    dev = torch.device("cuda", torch.cuda.current_device())
    render_poses = torch.as_tensor(render_poses, dtype=torch.float32, device=dev)
    img_ids = torch.as_tensor(img_ids, dtype=torch.float32, device=dev)
    N = render_poses.shape[0]
    rank, world = ddist.rank_world()
    if ddist.active() and ddist.band_mode(N, world):
        return _render_path_bands(render_poses, img_ids, H, W, focal, chunk, render_kwargs, gt_imgs, savedir, single_gt_img, names)
    lo, hi = ddist.frame_block(N, rank, world)
    n_loc = hi - lo
    near, far = float(render_kwargs.get('near', 0.)), float(render_kwargs.get('far', 1.))   # render()'s own defaults
    static_psnr = "rgb_static" in names and gt_imgs is not None
    # rank 0 renders straight into its block of the final [N, ...] tensors: the end gather receives the other blocks in place
    outs, bufs = ddist.root_buffers([(H, W, 3), (H, W), ()] + [_map_tail(m, H, W) for m in names] + [()] * static_psnr, N, dev)
    rgbs, disps, mse = bufs[:3]
    mbufs = dict(zip(names, bufs[3:]))
    mse.zero_()
    if static_psnr:
        bufs[-1].zero_()
    frame_kwargs = dict(render_kwargs, ret_maps=names) if names else render_kwargs   # the same call per frame, with the maps named
    gt_one = None
    if gt_imgs is not None and single_gt_img:
        gt_one = torch.as_tensor(np.asarray(gt_imgs), dtype=torch.float32).to(dev)
    pool = ThreadPoolExecutor(max_workers=PNG_WORKERS) if savedir is not None else None
    jobs = []
    t0 = time.time()
    t_post = 0.0
    for j0 in range(0, n_loc, POST_BATCH):
        j1 = min(n_loc, j0 + POST_BATCH)
        for j in range(j0, j1):
            i = lo + j
            rgb, disp, _, extras = render(H, W, focal, chunk=chunk, c2w=render_poses[i][:3, :4], img_idx=img_ids[i], **frame_kwargs)
            rgbs[j].copy_(rgb)
            disps[j].copy_(disp)
            for m in names:
                mbufs[m][j].copy_(extras[m])
            if i == 0:
                print(rgb.shape, disp.shape)
        if savedir is None and gt_imgs is None:
            continue
        tp = time.time()
        gt = gt_one
        if gt_imgs is not None and not single_gt_img:
            gt = torch.as_tensor(np.asarray(gt_imgs[lo + j0:lo + j1]), dtype=torch.float32).to(dev, non_blocking=True)
        post = eng.frame_post(rgbs[j0:j1], disps[j0:j1], gt, want_gt8=savedir is not None)
        if gt is not None:
            mse[j0:j1].copy_(post["mse"])
        if names and (savedir is not None or static_psnr):   # without a save directory only the static-only error is needed
            mpost = eng.frame_post_maps({m: mbufs[m][j0:j1] for m in names}, near, far, gt, want=None if savedir is not None else ("rgb_static",))
            if static_psnr:
                bufs[-1][j0:j1].copy_(mpost["mse_static"])
        if savedir is not None:
            host = []
            for t in (post["rgb8"], post["disp8"], post["gt8"]):
                host.append(None if t is None else torch.empty(t.shape, dtype=torch.uint8, pin_memory=True).copy_(t, non_blocking=True))
            mhost = {m: torch.empty(mpost[MAP_PNGS[m][0]].shape, dtype=mpost[MAP_PNGS[m][0]].dtype, pin_memory=True)
                     .copy_(mpost[MAP_PNGS[m][0]], non_blocking=True) for m in names}
            ev = torch.cuda.Event()
            ev.record()
            jobs.append(pool.submit(_write_frames, ev, host, savedir, lo + j0, mhost))
        t_post += time.time() - tp
    torch.cuda.synchronize()
    t_render = time.time() - t0
    # The range guard of the narrow arithmetic modes: a rank that raised before the collective would leave the others waiting in
    # it, and a rank that did NOT raise after it would walk into the caller's next collective alone.  So every rank's flag word goes
    # to EVERY rank (a 4-byte int32 all-gather behind the frame gather: bits OR, nothing is lost to a float MAX) and all of them raise
    # the same error, after the collective and after the PNG pool has been drained.
    eng_h = _engine_of(render_kwargs)
    my_flags = eng_h.range_flags()
    all_flags = [my_flags]
    tg = time.time()
    try:
        (all_rgb, all_disp, all_mse, *all_more), _ = ddist.gather_frames_direct(bufs, N, outs=outs)   # the path's ONE data collective
        all_flags = ddist.all_gather_flags(my_flags, dev)
        torch.cuda.synchronize()
    finally:
        t_gather = time.time() - tg
        tw = time.time()
        errs = []
        for jb in jobs:
            try:
                jb.result()
            except Exception as e:   # noqa: BLE001 - re-raised below, after the pool is shut down
                errs.append(e)
        if pool is not None:
            pool.shutdown(wait=True)
        t_tail = time.time() - tw
    if errs:
        raise errs[0]
    bad = 0
    for f in all_flags:
        bad |= int(f)
    if bad:   # the same message on every rank
        eng_h.raise_range(bad, where=f"render_path: frames {lo}..{hi - 1}" if len(all_flags) == 1 else
                          "render_path: ranks " + ", ".join(f"{r} (flags {f:#x})" for r, f in enumerate(all_flags) if f))
    if gt_imgs is None:
        all_mse = None
    n_gathered = ddist.gathered_bytes(bufs, N)
    if rank != 0:
        return (None, None, None) if names else (None, None)
    rgbs = all_rgb.cpu().numpy()
    disps = all_disp.cpu().numpy()
    maps = {m: t.cpu().numpy() for m, t in zip(names, all_more)}
    print(f"rendered {N} frames of {W}x{H} on {world} GPU(s) in {t_render:.2f} s (post-processing launches {t_post:.2f} s inside it, "
          f"PNG tail after the last frame {t_tail:.2f} s)")
    if all_mse is not None:
        psnr = -10. * np.log10(all_mse.cpu().numpy())
        print("Mean PSNR of this run is:", np.mean(psnr, 0))
        if static_psnr:   # the transient-free render against the same ground truth
            print("Mean static-only PSNR of this run is:", np.mean(-10. * np.log10(all_more[-1].cpu().numpy()), 0))
    render_path.last_timing = {"render_s": t_render, "post_launch_s": t_post, "gather_s": t_gather, "png_tail_s": t_tail, "frames": N, "world": world,
                               "gathered_bytes": n_gathered}
    if names:
        render_path.last_timing["maps"] = list(names)
        return rgbs, disps, maps
    return rgbs, disps


def render_band(H, W, focal, chunk, c2w, img_idx, r0, r1, render_kwargs, ret_maps=()):
    """Rows [r0, r1) of the frame at pose c2w: the band's rays out of get_rays (models/ray_utils.py:5-15) through render(rays=...).
    Rays are independent, so a band is bit-identical to the same rows of the full-frame render (tests/test_gpu_dist.py).
    ret_maps naming render maps: (rgb, disp, {name: the band's map}) — the same rows of the full frame's maps, bit for bit."""
    from .engine import map_names
    names = map_names(ret_maps)
    rays_o, rays_d = get_rays(H, W, focal, c2w)
    rgb, disp, _, extras = render(H, W, focal, chunk=chunk, rays=(rays_o[r0:r1].contiguous(), rays_d[r0:r1].contiguous()), img_idx=img_idx,
                                  **(dict(render_kwargs, ret_maps=names) if names else render_kwargs))
    if names:
        return rgb, disp, {m: extras[m] for m in names}
    return rgb, disp


def _render_path_bands(render_poses, img_ids, H, W, focal, chunk, render_kwargs, gt_imgs, savedir, single_gt_img, names=()):
    """SURVEY 8(e)'s small-batch fallback of render_path — fewer frames than ranks (the single validation frames of run_nerf.py:200,228;
    configs[0]'s four frames on eight GPUs): every rank renders ONE row band of one frame (dist.band_unit), the bands are gathered in
    place into rank 0's final [N, H, ...] tensors (dist.gather_bands_direct: the same single grouped send / receive batch), and the
    per-FRAME back-end — disp / max(disp) over the whole frame, the PSNR's mean squared error, to8b, the PNGs: rendering.py:423-452 —
    runs on rank 0 on the assembled frames (N < world <= 8 of them), so every number is the one a single GPU produces."""
    from . import engine as eng
    dev = render_poses.device
    N = render_poses.shape[0]
    rank, world = ddist.rank_world()
    f, r0, r1 = ddist.band_unit(N, H, rank, world)
    t0 = time.time()
    if r1 > r0:
        rgb, disp, *band_maps = render_band(H, W, focal, chunk, render_poses[f][:3, :4], img_ids[f], r0, r1, render_kwargs, names)
        band_maps = [band_maps[0][m] for m in names]
    else:   # more ranks on this frame than rows
        rgb, disp = torch.empty(0, W, 3, device=dev), torch.empty(0, W, device=dev)
        band_maps = [torch.empty((0,) + _map_tail(m, H, W)[1:], device=dev) for m in names]
    if rank == 0:
        print(torch.Size([H, W, 3]), torch.Size([H, W]))
    torch.cuda.synchronize() if dev.type == "cuda" else None
    t_render = time.time() - t0
    eng_h = _engine_of(render_kwargs)
    my_flags = eng_h.range_flags()
    tg = time.time()
    all_rgb, all_disp, *all_maps = ddist.gather_bands_direct([rgb, disp] + band_maps, N, H)      # the path's ONE data collective
    all_flags = ddist.all_gather_flags(my_flags, dev)
    t_gather = time.time() - tg
    bad = 0
    for fl in all_flags:
        bad |= int(fl)
    if bad:   # the same message on every rank, after the collective
        eng_h.raise_range(bad, where="render_path (row bands): ranks " + ", ".join(f"{r} (flags {fl:#x})" for r, fl in enumerate(all_flags) if fl))
    if rank != 0:
        return (None, None, None) if names else (None, None)
    tp = time.time()
    mse = mse_static = None
    if savedir is not None or gt_imgs is not None:
        gt = None
        if gt_imgs is not None:
            g = np.asarray(gt_imgs)
            gt = torch.as_tensor(g if single_gt_img else g[:N], dtype=torch.float32).to(dev)
        post = eng.frame_post(all_rgb, all_disp, gt, want_gt8=savedir is not None)
        mse = post["mse"] if gt is not None else None
        mhost = {}
        if names:   # the maps' back-end on the assembled frames too: beta's maximum is the whole frame's
            mpost = eng.frame_post_maps(dict(zip(names, all_maps)), float(render_kwargs.get('near', 0.)), float(render_kwargs.get('far', 1.)), gt)
            mse_static = mpost.get("mse_static")
            mhost = {m: mpost[MAP_PNGS[m][0]].cpu() for m in names} if savedir is not None else {}
        if savedir is not None:
            host = [None if t is None else t.cpu() for t in (post["rgb8"], post["disp8"], post["gt8"])]

            class _Done:
                def synchronize(self):
                    pass
            _write_frames(_Done(), host, savedir, 0, mhost)
    t_post = time.time() - tp
    print(f"rendered {N} frames of {W}x{H} as row bands on {world} GPU(s) in {t_render:.2f} s (gather {t_gather:.2f} s, frame back-end on "
          f"rank 0 {t_post:.2f} s)")
    if mse is not None:
        print("Mean PSNR of this run is:", np.mean(-10. * np.log10(mse.cpu().numpy()), 0))
    if mse_static is not None:
        print("Mean static-only PSNR of this run is:", np.mean(-10. * np.log10(mse_static.cpu().numpy()), 0))
    per_pixel = 4 + sum(3 if m.startswith("rgb_") else 1 for m in names)   # floats: rgb + disp (+ the maps)
    per_frame = (H * W * per_pixel) * 4
    own = r1 - r0
    render_path.last_timing = {"render_s": t_render, "post_launch_s": t_post, "gather_s": t_gather, "png_tail_s": 0.0, "frames": N, "world": world,
                               "gathered_bytes": N * per_frame - own * W * per_pixel * 4, "row_bands": True}
    if names:
        render_path.last_timing["maps"] = list(names)
        return all_rgb.cpu().numpy(), all_disp.cpu().numpy(), {m: t.cpu().numpy() for m, t in zip(names, all_maps)}
    return all_rgb.cpu().numpy(), all_disp.cpu().numpy()


def _drain(dl):
    imgs, poses, idxs = [], [], []
    for img, pose, img_idx in dl:
        imgs.append(img.permute(0, 2, 3, 1))
        p = torch.zeros(1, 4, 4)
        p[0, :3, :4] = pose.reshape(3, 4)[:3, :4]
        p[0, 3, 3] = 1.
        poses.append(p)
        idxs.append(img_idx)
    return torch.cat(imgs, 0).cpu().numpy(), torch.cat(poses, 0), torch.cat(idxs, 0)   # gt frames may be device tensors


def render_test(args, train_dl, val_dl, hwf, start, render_kwargs_test, decoder_coarse=None, decoder_fine=None):
    """Drop-in for rendering.py:460-530: render the train split then the val split, write PNGs under
    basedir/expname/evaluate_{train,val}_{test|path}_{start:06d}."""
    from .options import render_map_names
    tag = 'test' if args.render_test else 'path'
    maps = render_map_names(getattr(args, 'render_maps', ''))   # --render_maps: () = off, exactly the call without the keyword
    for name, dl in (("train", train_dl), ("val", val_dl)):
        savedir = os.path.join(args.basedir, args.expname, 'evaluate_{}_{}_{:06d}'.format(name, tag, start))
        os.makedirs(savedir, exist_ok=True)
        images, poses, index = _drain(dl)
        print(f'{name} poses shape', poses.shape)
        with torch.no_grad():
            render_path(args, poses, hwf, args.chunk, render_kwargs_test, gt_imgs=images, savedir=savedir,
                        img_ids=index, ret_maps=maps)
        print(f'Saved {name} set')
    return
