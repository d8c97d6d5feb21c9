"""Host-side mirror of /root/reference/script/models/nerfw.py for the HIP render path.

`NeRFW` here is a *parameter container* with the reference's exact state_dict layout (so the
reference's `{:06d}.tar` checkpoints load unchanged) and the reference's initialisation order
(constructor reseeds the global RNG to 0, nerfw.py:245, then builds the Linear layers in the same
sequence, so a no-checkpoint run starts from the same weights).  The arithmetic is not here:
`create_nerf` packs the weights into a `NerfHEngine` (MFMA fragment layout on the GPU) and the
returned render kwargs route `rendering.render` to it.
"""
import os

import torch
import torch.nn as nn

from .engine import NerfHEngine
from . import optim

DEVICE_RECOMMIT = True   # HipQuery.refresh: re-pack the engine from the modules' CUDA parameters on the GPU (False: through the host, load_modules)

img2mse = lambda x, y: torch.mean((x - y) ** 2)
mse2psnr = lambda x: -10. * torch.log(x) / torch.log(torch.Tensor([10.]))


def to8b(x):
    """uint8(255 * clip(x, 0, 1)) — truncation, not rounding (reference models/nerf.py:11)."""
    import numpy as np
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def _act(layer, act):
    return nn.Sequential(layer, act) if act is not None else layer


class NeRFW(nn.Module):
    """Weights of one NeRF-H network ('coarse' or 'fine'); names as nerfw.py:259-295."""

    def __init__(self, typ, D=8, W=256, skips=[4], in_channels_xyz=63, in_channels_dir=27,
                 encode_appearance=False, in_channels_a=48, encode_transient=False, in_channels_t=16,
                 beta_min=0.1, out_ch_size=3):
        super().__init__()
        torch.manual_seed(0)  # reference side effect (nerfw.py:245), part of the contract (quirk Q12)
        if out_ch_size != 3:
            raise NotImplementedError("feature-rendering heads (out_ch_size != 3) are not part of the NeRF-H path")
        self.typ, self.D, self.W, self.skips = typ, D, W, list(skips)
        self.in_channels_xyz, self.in_channels_dir = in_channels_xyz, in_channels_dir
        self.encode_appearance = False if typ == 'coarse' else encode_appearance
        self.in_channels_a = in_channels_a if encode_appearance else 0
        self.encode_transient = False if typ == 'coarse' else encode_transient
        self.in_channels_t = in_channels_t
        self.beta_min = beta_min
        for i in range(D):
            k = in_channels_xyz if i == 0 else (W + in_channels_xyz if i in skips else W)
            setattr(self, f"xyz_encoding_{i + 1}", _act(nn.Linear(k, W), nn.ReLU(True)))
        self.xyz_encoding_final = nn.Linear(W, W)
        self.dir_encoding = _act(nn.Linear(W + in_channels_dir + self.in_channels_a, W // 2), nn.ReLU(True))
        self.static_sigma = _act(nn.Linear(W, 1), nn.Softplus())
        self.static_rgb = _act(nn.Linear(W // 2, 3), nn.Sigmoid())
        if self.encode_transient:
            self.transient_encoding = nn.Sequential(
                nn.Linear(W + in_channels_t, W // 2), nn.ReLU(True), nn.Linear(W // 2, W // 2), nn.ReLU(True),
                nn.Linear(W // 2, W // 2), nn.ReLU(True), nn.Linear(W // 2, W // 2), nn.ReLU(True))
            self.transient_sigma = _act(nn.Linear(W // 2, 1), nn.Softplus())
            self.transient_rgb = _act(nn.Linear(W // 2, 3), nn.Sigmoid())
            self.transient_beta = _act(nn.Linear(W // 2, 1), nn.Softplus())

    def forward(self, *a, **k):
        raise RuntimeError("NeRFW here only holds weights; evaluate it through dfnet_amd.rendering.render "
                           "(the fused HIP kernels take rays, not pre-embedded vectors)")


class _FinePointsFn(torch.autograd.Function):
    """raw [R,N,9] = the fine network at pts [R,N,3] with one view direction per row; backward: d L/d pts and d L/d viewdirs from
    d L/d raw (NerfHEngine.mlp_fine_points / mlp_fine_points_backward: the forward is recomputed inside the gradient kernel)."""

    @staticmethod
    def forward(ctx, pts, viewdirs, eng, hist, prec):
        pts, viewdirs = pts.detach().contiguous().float(), viewdirs.detach().contiguous().float()
        ctx.eng, ctx.prec = eng, prec
        ctx.save_for_backward(pts, viewdirs, hist)
        return eng.mlp_fine_points(pts, viewdirs, hist, precision=prec)

    @staticmethod
    def backward(ctx, g_raw):
        pts, viewdirs, hist = ctx.saved_tensors
        g = ctx.eng.mlp_fine_points_backward(pts, viewdirs, hist, g_raw, precision=ctx.prec)
        g_pts = g[..., :3].contiguous() if ctx.needs_input_grad[0] else None
        g_v = g[..., 3:].sum(dim=1) if ctx.needs_input_grad[1] else None   # one view direction per row of points
        return g_pts, g_v, None, None, None


class _CoarsePointsFn(torch.autograd.Function):
    """sigma [R,N] = the coarse network's density at pts [R,N,3]; backward: d L/d pts from d L/d sigma (NerfHEngine.mlp_coarse_points
    / mlp_coarse_points_backward: the forward is recomputed inside the gradient kernel).  sigma does not see the view direction."""

    @staticmethod
    def forward(ctx, pts, eng, prec):
        pts = pts.detach().contiguous().float()
        ctx.eng, ctx.prec = eng, prec
        ctx.save_for_backward(pts)
        return eng.mlp_coarse_points(pts, precision=prec)

    @staticmethod
    def backward(ctx, g_sigma):
        pts, = ctx.saved_tensors
        return ctx.eng.mlp_coarse_points_backward(pts, g_sigma, precision=ctx.prec), None, None


class _CoarseStaticPointsFn(torch.autograd.Function):
    """raw [R,N,4] = (static_rgb, static_sigma) of the coarse network's training query at pts [R,N,3] with one view direction per row;
    backward: d L/d pts and d L/d viewdirs from d L/d raw (NerfHEngine.mlp_coarse_static_points / mlp_coarse_static_points_backward:
    the forward is recomputed inside the gradient kernel).  The weights receive nothing here: network_query_fn(..., train=True) attaches
    them (nerf_train._PointsTrainFn)."""

    @staticmethod
    def forward(ctx, pts, viewdirs, eng, prec):
        pts, viewdirs = pts.detach().contiguous().float(), viewdirs.detach().contiguous().float()
        ctx.eng, ctx.prec = eng, prec
        ctx.save_for_backward(pts, viewdirs)
        return eng.mlp_coarse_static_points(pts, viewdirs, precision=prec)

    @staticmethod
    def backward(ctx, g_raw):
        pts, viewdirs = ctx.saved_tensors
        g = ctx.eng.mlp_coarse_static_points_backward(pts, viewdirs, g_raw, precision=ctx.prec)
        g_pts = g[..., :3].contiguous() if ctx.needs_input_grad[0] else None
        g_v = g[..., 3:].sum(dim=1) if ctx.needs_input_grad[1] else None   # one view direction per row of points
        return g_pts, g_v, None, None


class HipQuery:
    """Stands in for the reference's `network_query_fn` lambda (nerfw.py:425-434): carries the engine that evaluates both networks,
    and is callable as the reference's is.

    `query(inputs, viewdirs, ts, network_fn, typ, embedding_a, embedding_t, output_transient, test_time)` evaluates a network on
    pre-sampled points (run_network_NeRFW, nerfw.py:15-95) with the register-resident HIP kernels: inputs [..., N, 3] (any points,
    not only samples of a ray), one view direction per row of N points (viewdirs [R, 3]) and one histogram per row or one for all
    (ts [R | 1, hist_bin]).  The result keeps the leading shape of `inputs`:
      typ='coarse', test_time=True          sigma [..., N, 1]            (nerfw.py:37-46)
      typ='coarse', test_time=False, static=True   raw [..., N, 4] = (static_rgb, static_sigma), the training query (nerfw.py:47-60)
      typ='fine',   output_transient=True   raw   [..., N, 9]            (nerfw.py:62-95)
      typ='fine',   output_transient=False  raw[..., :4] = (static_rgb, static_sigma), the four values the reference concatenates
    The networks are the ones packed into the engine: a `network_fn` / `embedding_a` / `embedding_t` that is not the module behind
    it raises ValueError (None is accepted).  With grad enabled and `inputs` or `viewdirs` requiring it, typ='fine' is differentiable
    with respect to both (the weights receive no gradient here: that is `train=True` below, or the training step), in fp32-grade arithmetic as
    `render` under autograd: an engine whose precision is plain f16 differentiates in split-f16.
    typ='coarse' is differentiable on request, as sample_pdf(diff=True) is: with `diff=True`, test_time=True, grad enabled and
    `inputs` requiring grad, sigma is attached to `inputs` (the coarse network's input-gradient kernel, netwidth 128, the precision
    rule above; `viewdirs` receives nothing: sigma does not depend on it).  With nothing to track, or under no_grad, diff=True is the
    plain query; typ='fine' accepts and ignores the keyword.
    The coarse network's TRAINING query (typ='coarse', test_time=False: the 4-channel input of raw2outputs_NeRFW's coarse mode) is
    opt-in through the keyword `static=True`: it needs viewdirs [R, 3], one row per row of points; `ts` is ignored (the reference
    passes None) and output_transient=True raises ValueError (the reference's coarse module has no transient branch either).  With
    grad enabled and `inputs` or `viewdirs` requiring it the result is attached to both (netwidth 128, the precision rule above; the
    weights receive nothing) -- there is no earlier behaviour to preserve, so `diff` is not needed for it.  typ='fine', and
    typ='coarse' with test_time=True, accept and ignore the keyword.
    WEIGHT gradients are opt-in through the keyword `train=True` (without it every call is what it was): the query becomes an autograd
    expression of the network's parameters, as the reference's network_query_fn(..., test_time=False) is (nerfw.py:47-95, 297-354) --
    typ='fine': raw [..., N, 9] (or [..., :4]) attached to network_fine's parameters and both embedding weights; typ='coarse' with
    test_time=False: raw [..., N, 4] attached to network_fn's parameters (static=True is implied, output_transient=True a ValueError).
    With grad enabled the result is attached to `inputs` / `viewdirs` too when they require grad; under no_grad it is the plain forward
    of the same kernels.  It runs the fused training chains on the LIVE master weights (netwidth 128; NerfHTrainer.points_forward /
    points_backward, one workspace per call, so several queries may be live in one graph), at the operand scale of the engine's last
    commit.  Stored operands follow trainer.fused_split: the fine network's default is one f16 plane, whose weight gradients are
    f16-grade (1e-3) on queries of a few hundred points; fused_split = True gives fp32-grade ones.  Refused with NotImplementedError,
    each naming the way out: no trainer behind the query (create_nerf with no_grad_update), a netwidth other than 128, and
    typ='coarse' with test_time=True (the sigma-only query is not a training query).
    Refused with NotImplementedError: typ='coarse' with test_time=False without static=True (the positional call of the reference),
    typ='coarse' with test_time=True under autograd without diff=True, and a netwidth other than 128 or 256 (no register-resident
    kernels)."""

    def __init__(self, engine, netchunk=65536, trainer=None, modules=None):
        self.engine = engine
        self.netchunk = netchunk
        self.trainer = trainer      # NerfHTrainer: the training-mode render and its gradients (nerf_train.py)
        self.modules = modules      # (network_fn, network_fine, embedding_a, embedding_t) behind the engine's packed weights
        self.stale = False          # the master weights moved (optimizer step) since the engine was packed
        self._packed_versions = self._versions()

    def _versions(self):
        """torch's in-place version counters of every master tensor: they move with optimizer.step() / load_state_dict()."""
        if self.modules is None:
            return None
        return tuple(p._version for m in self.modules for p in m.parameters())

    def refresh(self):
        """Re-pack the test-time engine from the (trained) modules — before a validation render — when they moved: either the
        training loop said so (`stale`) or their version counters did."""
        if self.modules is None:
            return
        cur = self._versions()
        if self.stale or cur != self._packed_versions:
            # DEVICE_RECOMMIT: the parameters live on the GPU and the engine has been packed once, so it is re-packed there
            # (NerfHEngine.load_device: no host copy, no host packer); otherwise, and with the switch off, through the host as before
            tensors = self.engine.module_tensors(*self.modules) if DEVICE_RECOMMIT else None
            if self.engine.device_ready(tensors):
                self.engine.load_device(tensors)
            else:
                self.engine.load_modules(*self.modules)
            self.stale = False
            self._packed_versions = cur

    def _check_module(self, given, index, name):
        if given is None:
            return
        if self.modules is None or given is not self.modules[index]:
            raise ValueError(f"network_query_fn: {name} is not the module packed into this engine; the HIP kernels evaluate the "
                             "engine's own weights (pass None, or the module create_nerf returned)")

    def __call__(self, inputs, viewdirs, ts, network_fn=None, typ='fine', embedding_a=None, embedding_t=None, output_transient=True,
                 test_time=True, diff=False, static=False, train=False):
        self.refresh()
        if typ not in ('coarse', 'fine'):
            raise ValueError(f"network_query_fn: typ must be 'coarse' or 'fine', got {typ!r}")
        self._check_module(network_fn, 0 if typ == 'coarse' else 1, "network_fn")
        self._check_module(embedding_a, 2, "embedding_a")
        self._check_module(embedding_t, 3, "embedding_t")
        eng = self.engine
        if train:
            return self._train_query(inputs, viewdirs, ts, typ, output_transient, test_time)
        if not eng.fast:
            raise NotImplementedError(f"network_query_fn: point queries exist for netwidth 128 and 256 (the register-resident "
                                      f"kernels); this engine has netwidth {eng.width}")
        if inputs.shape[-1] != 3 or inputs.dim() < 2:
            raise ValueError(f"network_query_fn: inputs must be [..., N, 3], got {tuple(inputs.shape)}")
        lead = tuple(inputs.shape[:-1])
        pts = inputs.reshape(-1, inputs.shape[-2], 3) if inputs.dim() > 2 else inputs.reshape(-1, 1, 3)
        tracked = torch.is_grad_enabled() and (inputs.requires_grad or (viewdirs is not None and viewdirs.requires_grad))
        if typ == 'coarse':
            if not test_time and static:
                if output_transient:
                    raise ValueError("network_query_fn: typ='coarse' has no transient branch: output_transient must be False")
                if viewdirs is None:
                    raise ValueError("network_query_fn: typ='coarse' with test_time=False needs viewdirs [R, 3]")
                v = viewdirs.reshape(-1, 3)
                if v.shape[0] != pts.shape[0]:
                    raise ValueError(f"network_query_fn: viewdirs must have one row per row of points ({pts.shape[0]}), got "
                                     f"{tuple(viewdirs.shape)}")
                if tracked and eng.width != 128:
                    raise NotImplementedError(f"network_query_fn: the training coarse query is differentiable at netwidth 128 only (the "
                                              f"input-gradient kernels; this engine has netwidth {eng.width}): query under no_grad, or "
                                              "with inputs and viewdirs detached")
                if tracked:
                    raw = _CoarseStaticPointsFn.apply(pts, v, eng, "f16x3" if eng.precision in ("f16", "fp16") else eng.precision)
                else:
                    raw = eng.mlp_coarse_static_points(pts.detach(), v.detach())
                return raw.reshape(lead + (4,))
            if not test_time:
                raise NotImplementedError("network_query_fn: typ='coarse' with test_time=False (the 4-channel training query, "
                                          "nerfw.py:47-60) is opt-in: pass the keyword static=True for raw [..., N, 4] = (static_rgb, "
                                          "static_sigma); without it the training render evaluates it (rendering.render)")
            if diff and torch.is_grad_enabled() and inputs.requires_grad:
                sigma = _CoarsePointsFn.apply(pts, eng, "f16x3" if eng.precision in ("f16", "fp16") else eng.precision)
                return sigma.reshape(lead + (1,))
            if tracked and not diff:
                raise NotImplementedError("network_query_fn: typ='coarse' under autograd is opt-in: pass diff=True for sigma attached "
                                          "to `inputs` (netwidth 128); without it the coarse query builds no graph")
            return eng.mlp_coarse_points(pts.detach()).reshape(lead + (1,))
        if viewdirs is None or ts is None:
            raise ValueError("network_query_fn: typ='fine' needs viewdirs [R, 3] and ts [R | 1, hist_bin]")
        v = viewdirs.reshape(-1, 3)
        if v.shape[0] != pts.shape[0]:
            raise ValueError(f"network_query_fn: viewdirs must have one row per row of points ({pts.shape[0]}), got {tuple(viewdirs.shape)}")
        hist = ts.detach().float().reshape(-1, eng.hist_bin).contiguous()
        if tracked:
            raw = _FinePointsFn.apply(pts, v, eng, hist, "f16x3" if eng.precision in ("f16", "fp16") else eng.precision)
        else:
            raw = eng.mlp_fine_points(pts.detach(), v.detach(), hist)
        raw = raw.reshape(lead + (9,))
        return raw if output_transient else raw[..., :4]

    def _train_query(self, inputs, viewdirs, ts, typ, output_transient, test_time):
        """__call__(..., train=True): the query as an autograd expression of the network's PARAMETERS (and of both embedding tables for
        typ='fine'), as the reference's network_query_fn(..., test_time=False) is (nerfw.py:15-95, 297-354) — nerf_train._PointsTrainFn on
        the fused training chains (netwidth 128).  Attached to `inputs` / `viewdirs` as well when they require grad; under no_grad the
        plain forward of the same kernels."""
        from .nerf_train import _PointsTrainFn
        eng, tr = self.engine, self.trainer
        if typ == 'coarse' and test_time:
            raise NotImplementedError("network_query_fn: train=True with typ='coarse' and test_time=True: the sigma-only query is not a "
                                      "training query (the reference evaluates it under no_grad); pass test_time=False for raw "
                                      "[..., N, 4] = (static_rgb, static_sigma) attached to network_fn's parameters")
        if typ == 'coarse' and output_transient:
            raise ValueError("network_query_fn: typ='coarse' has no transient branch: output_transient must be False")
        if tr is None:
            raise NotImplementedError("network_query_fn: train=True needs the trainer behind the engine (weight gradients): create_nerf "
                                      "without no_grad_update attaches one, or set query.trainer = NerfHTrainer(engine, network_fn, "
                                      "network_fine, embedding_a, embedding_t)")
        if eng.width != 128:
            raise NotImplementedError(f"network_query_fn: train=True runs on the fused training chains, which exist for netwidth 128 only "
                                      f"(this engine has netwidth {eng.width}); train through rendering.render(test_time=False) / "
                                      "NerfHTrainer.train_step, which take any width on the exact step")
        if inputs.shape[-1] != 3 or inputs.dim() < 2:
            raise ValueError(f"network_query_fn: inputs must be [..., N, 3], got {tuple(inputs.shape)}")
        fine = typ == 'fine'
        if viewdirs is None or (fine and ts is None):
            raise ValueError("network_query_fn: train=True needs viewdirs [R, 3]" + (" and ts [R | 1, hist_bin]" if fine else ""))
        lead = tuple(inputs.shape[:-1])
        pts = inputs.reshape(-1, inputs.shape[-2], 3) if inputs.dim() > 2 else inputs.reshape(-1, 1, 3)
        v = viewdirs.reshape(-1, 3)
        if v.shape[0] != pts.shape[0]:
            raise ValueError(f"network_query_fn: viewdirs must have one row per row of points ({pts.shape[0]}), got {tuple(viewdirs.shape)}")
        hist = ts.detach().float().reshape(-1, eng.hist_bin).contiguous() if fine else None
        if torch.is_grad_enabled():
            raw = _PointsTrainFn.apply(typ, tr, pts, v, hist, *tr.net_params(typ))
        else:
            raw, _ = tr.points_forward(typ, pts, v, hist)
        raw = raw.reshape(lead + (9 if fine else 4,))
        return raw if (not fine or output_transient) else raw[..., :4]


def create_nerf(args):
    """Same contract as nerfw.py:356-502: returns (render_kwargs_train, render_kwargs_test, start,
    grad_vars, optimizer).  Differences: the networks live in a NerfHEngine (`network_query_fn.engine`)."""
    if not getattr(args, "NeRFH", False):
        raise NotImplementedError("only the NeRF-H path (--NeRFH) is implemented")
    if not getattr(args, "encode_hist", False):
        raise ValueError("NeRF-H needs --encode_hist (the reference leaves embedding_a/t undefined without it, nerfw.py:385-391)")
    if args.reduce_embedding != -1 or args.i_embed != 0:
        raise NotImplementedError("only the paper-default positional encoding (reduce_embedding=-1, i_embed=0) is implemented")
    if not args.use_viewdirs:
        raise NotImplementedError("use_viewdirs=False is not part of the NeRF-H path")
    if not torch.cuda.is_available():
        raise RuntimeError("create_nerf needs a GPU: the render path is HIP-only, there is no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    input_ch, input_ch_views = 3 + 6 * args.multires, 3 + 6 * args.multires_views
    dim_a, rem_a = divmod(args.in_channels_a, args.hist_bin)
    dim_t, rem_t = divmod(args.in_channels_t, args.hist_bin)
    if rem_a or rem_t or (dim_a, dim_t) != (5, 2):
        raise ValueError("in_channels_a/t must equal hist_bin*5 / hist_bin*2 (nn.Embedding(N_vocab,5)/(N_vocab,2), nerfw.py:386-390)")
    embedding_a = nn.Embedding(args.N_vocab, 5).to(device)
    embedding_t = nn.Embedding(args.N_vocab, 2).to(device)
    model = NeRFW('coarse', D=args.netdepth, W=args.netwidth, skips=[4], in_channels_xyz=input_ch,
                  in_channels_dir=input_ch_views).to(device)
    grad_vars = list(model.parameters())
    model_fine = None
    if args.N_importance > 0:
        model_fine = NeRFW('fine', D=args.netdepth, W=args.netwidth, skips=[4], in_channels_xyz=input_ch,
                           in_channels_dir=input_ch_views, encode_appearance=True, encode_transient=True,
                           in_channels_a=args.in_channels_a, in_channels_t=args.in_channels_t).to(device)
        grad_vars += list(model_fine.parameters()) + list(embedding_a.parameters()) + list(embedding_t.parameters())
    else:
        raise NotImplementedError("N_importance == 0 (no fine network) is not part of the NeRF-H path")

    if args.no_grad_update:
        grad_vars, optimizer = None, None
    else:
        optimizer = optim.Adam(params=grad_vars, lr=args.lrate, betas=(0.9, 0.999))   # torch.optim.Adam, one launch per step

    start = 0
    if args.ft_path is not None and args.ft_path != 'None':
        ckpts = [args.ft_path]
    else:
        d = os.path.join(args.basedir, args.expname)
        ckpts = [os.path.join(d, f) for f in sorted(os.listdir(d)) if 'tar' in f] if os.path.isdir(d) else []
    print('Found ckpts', ckpts)
    if len(ckpts) > 0 and not args.no_reload:
        print('Reloading from', ckpts[-1])
        ckpt = torch.load(ckpts[-1], map_location=device)
        start = ckpt['global_step']
        model.load_state_dict(ckpt['network_fn_state_dict'])
        model_fine.load_state_dict(ckpt['network_fine_state_dict'])
        embedding_a.load_state_dict(ckpt['embedding_a_state_dict'])
        embedding_t.load_state_dict(ckpt['embedding_t_state_dict'])

    engine = NerfHEngine(depth=args.netdepth, width=args.netwidth, multires=args.multires,
                         multires_views=args.multires_views, hist_bin=args.hist_bin, dim_a=dim_a, dim_t=dim_t,
                         n_vocab=args.N_vocab, precision=getattr(args, "precision", "f16x3"))
    engine.load_modules(model, model_fine, embedding_a, embedding_t)
    if engine.fast and getattr(args, "precision", "f16x3") == "f16x3" and getattr(args, "coarse_precision", "same") == "f16":
        engine.set_render_options(coarse_f16=True)   # opt-in: the split-f16 fine network makes the pixel, an f16 coarse network places its samples

    from .nerf_train import NerfHTrainer
    query = HipQuery(engine, args.netchunk, modules=(model, model_fine, embedding_a, embedding_t))
    if not args.no_grad_update:
        query.trainer = NerfHTrainer(engine, model, model_fine, embedding_a, embedding_t)
    render_kwargs_train = {
        'network_query_fn': query, 'perturb': args.perturb,
        'N_importance': args.N_importance, 'network_fine': model_fine, 'N_samples': args.N_samples,
        'network_fn': model, 'use_viewdirs': args.use_viewdirs, 'white_bkgd': args.white_bkgd,
        'raw_noise_std': args.raw_noise_std, 'embedding_a': embedding_a, 'embedding_t': embedding_t,
        'test_time': False,
    }
    if args.dataset_type != 'llff' or args.no_ndc:
        print('Not ndc!')
        render_kwargs_train['ndc'] = False
        render_kwargs_train['lindisp'] = args.lindisp
    render_kwargs_test = dict(render_kwargs_train)
    render_kwargs_test.update(perturb=False, raw_noise_std=0., test_time=True)
    return render_kwargs_train, render_kwargs_test, start, grad_vars, optimizer
