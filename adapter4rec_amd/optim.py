"""FusedAdam / FusedAdamW: torch.optim.Adam's and AdamW's update as ONE kernel launch over the engine's flat parameter / gradient buffers instead of
~4 small kernels per tensor.  Same constructor shape as torch.optim.Adam (param groups, per-group lr and weight_decay).  The reference's setting
(Downstream/Text/run.py:524-529: betas (0.9, 0.999), eps 1e-8, no weight decay) runs a4r_adam_step exactly as it always has; weight decay or clipping
switch to a4r_adamw_step (include/a4r.h)."""
import math

import torch

from . import _lib as L

# torch.optim.Adam arguments that have no fused form here: refused, never silently ignored
_UNSUPPORTED = dict(amsgrad=False, maximize=False, capturable=False, differentiable=False, foreach=None, fused=None)


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam over the engine's flat buffers.

    weight_decay: per param group; coupled (torch Adam: g += wd * p) or, with decoupled_weight_decay=True, decoupled (torch AdamW: p *= 1 - lr * wd).
    max_grad_norm: clip the total gradient norm as torch.nn.utils.clip_grad_norm_(params, max_grad_norm) would before the step, without a host read:
    a deterministic fp64 sum of squares (a4r_grad_sumsq), then the step scales every gradient by min(1, max_norm / (norm + 1e-6)) as it reads it.
    Unlike clip_grad_norm_, p.grad (the flat gradient buffer) is NOT rewritten: after step() it still holds the unclipped gradients.
    last_grad_norm is then a 0-d fp32 device tensor holding the pre-clip total norm (what clip_grad_norm_ returns), a new tensor each step; a
    non-finite norm is not an error (error_if_nonfinite=False): the coefficient becomes NaN or 0 and the update proceeds -- check the norm.
    The gradients are read as (g * grad_scale), so under FlatDDP every rank clips the same all-reduced buffer to the same bits."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False, max_grad_norm=None):
        if max_grad_norm is not None and not (math.isfinite(max_grad_norm) and max_grad_norm > 0):
            raise ValueError(f'max_grad_norm must be a finite positive number or None, got {max_grad_norm}')
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, foreach=foreach, maximize=maximize,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=bool(decoupled_weight_decay))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        super().__init__(params, defaults)
        self._bound = None
        self._step = 0

    @staticmethod
    def _check_group(g):
        for k, off in _UNSUPPORTED.items():
            if g.get(k, off) not in (off, False):
                raise NotImplementedError(f'FusedAdam: {k}={g[k]!r} has no fused form (the update is one native kernel over the flat buffers)')
        if not 0.0 <= float(g['weight_decay']):
            raise ValueError(f'Invalid weight_decay value: {g["weight_decay"]}')

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])

    def __setstate__(self, state):                             # (load_state_dict: the groups take the checkpoint's hyper-parameters)
        super().__setstate__(state)
        for g in self.param_groups:
            for k in ('weight_decay', 'decoupled_weight_decay', *_UNSUPPORTED):
                g.setdefault(k, self.defaults[k])              # a checkpoint of an older FusedAdam holds lr / betas / eps / weight_decay only
            self._check_group(g)

    # -- binding to the engine's flat buffers (parameters become views at the engine's first use)
    def _bind(self):
        plist = [p for g in self.param_groups for p in g['params']]
        if not plist:
            raise RuntimeError('FusedAdam: no parameters')
        metas = [getattr(p, '_a4r_flat', None) for p in plist]
        if any(m is None for m in metas):
            raise RuntimeError('FusedAdam: parameters are not bound to a native engine yet (run one forward first); '
                               'there is no eager fallback')
        eng = metas[0][0]
        if any(m[0] is not eng for m in metas):
            raise RuntimeError('FusedAdam: parameters belong to different engines')
        dev = eng.dev
        segs = sorted((m[1], m[1] + m[2], gi) for gi, g in enumerate(self.param_groups) for p in g['params']
                      for m in [p._a4r_flat])
        seg_end = [e for _, e, _ in segs]
        seg_end[-1] = eng.flat_p.numel()                       # alignment padding at the tail
        self._seg_end = torch.tensor(seg_end, dtype=torch.int32, device=dev)
        self._seg_group = torch.tensor([g for _, _, g in segs], dtype=torch.int32, device=dev)
        self._lr_host = None
        self._lr_dev = torch.zeros(len(self.param_groups), dtype=torch.float32, device=dev)
        self._wd_host = None
        self._wd_dev = torch.zeros(len(self.param_groups), dtype=torch.float32, device=dev)
        self._partials = None
        self._m = torch.zeros_like(eng.flat_p)
        self._v = torch.zeros_like(eng.flat_p)
        covered = sum(m[2] for m in metas)
        if covered != sum(n for _, n in eng.offsets.values()):
            raise RuntimeError('FusedAdam must own every trainable parameter of the engine (the flat buffer is updated as a whole)')
        self._bound = eng
        eng._fused_opt = self
        self._attach_grads()
        self._apply_pending()

    def _attach_grads(self):
        eng = self._bound
        for g in self.param_groups:
            for p in g['params']:
                _, off, n = p._a4r_flat
                view = eng.flat_g[off:off + n].view(p.shape)
                if p.grad is None or p.grad.data_ptr() != view.data_ptr():
                    if p.grad is not None:
                        view.copy_(p.grad)
                    p.grad = view

    def zero_grad(self, set_to_none=False):
        if self._bound is None:
            return super().zero_grad(set_to_none=True)
        self._bound.flat_g.zero_()
        self._bound._flat_clean = True          # the next backward writes straight into flat_g (engine.backward_bound)
        self._attach_grads()

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        if closure is not None:
            raise NotImplementedError('closure')
        if self._bound is None:
            self._bind()
        elif next(p for g in self.param_groups for p in g['params'])._a4r_flat[0] is not self._bound:
            # the model rebuilt its engine (.to(device) / load_state_dict): move the moments over to the new flat buffers
            self._pending = dict(step=self._step, m=self._m, v=self._v)
            old = self._bound
            self._bind()
            self._bound.step_count = max(self._bound.step_count, old.step_count)     # the counter-based dropout stream continues, it does not restart
        else:
            self._attach_grads()
        eng = self._bound
        lrs = [float(g['lr']) for g in self.param_groups]
        if lrs != self._lr_host:
            self._lr_dev.copy_(torch.tensor(lrs, dtype=torch.float32))
            self._lr_host = lrs
        g0 = self.param_groups[0]
        wds = [float(g['weight_decay']) for g in self.param_groups]
        self._step += 1
        if self.max_grad_norm is None and not any(wds):        # the reference's configuration: the plain Adam kernel, as it always ran
            L.adam_step(eng.flat_p, eng.flat_g, self._m, self._v, self._seg_end, self._seg_group, self._lr_dev, self._step,
                        beta1=g0['betas'][0], beta2=g0['betas'][1], eps=g0['eps'], grad_scale=grad_scale)
            return
        modes = {bool(g['decoupled_weight_decay']) for g in self.param_groups}
        if len(modes) > 1:
            raise NotImplementedError('FusedAdam: coupled and decoupled weight decay in one optimizer (one kernel updates every group)')
        if wds != self._wd_host:
            self._wd_dev.copy_(torch.tensor(wds, dtype=torch.float32))
            self._wd_host = wds
        norm = None
        if self.max_grad_norm is not None:
            if self._partials is None:
                self._partials = torch.empty(L.GRAD_NORM_PARTS, dtype=torch.float64, device=eng.dev)
            norm = torch.empty((), dtype=torch.float32, device=eng.dev)
            L.grad_sumsq(eng.flat_g, self._partials, grad_scale=grad_scale)
        L.adamw_step(eng.flat_p, eng.flat_g, self._m, self._v, self._seg_end, self._seg_group, self._lr_dev, self._wd_dev, self._step,
                     beta1=g0['betas'][0], beta2=g0['betas'][1], eps=g0['eps'], grad_scale=grad_scale, decoupled=modes.pop(),
                     partials=self._partials if norm is not None else None, max_norm=self.max_grad_norm or 0.0, norm_out=norm)
        self.last_grad_norm = norm

    # -- checkpoint interchange with the reference (Downstream/Text/run.py:481-492, data_utils/utils.py:109-115): torch.optim.Adam's own
    #    layout -- state[param] = {step, exp_avg, exp_avg_sq} -- written and read; the per-parameter tensors are views of the flat moments
    def _state_views(self):
        for g in self.param_groups:
            for p in g['params']:
                _, off, n = p._a4r_flat
                self.state[p] = dict(step=torch.tensor(float(self._step)), exp_avg=self._m[off:off + n].view(p.shape),
                                     exp_avg_sq=self._v[off:off + n].view(p.shape))

    def state_dict(self):
        if self._bound is not None:
            self._state_views()
        sd = super().state_dict()
        if self._bound is not None:
            sd['a4r'] = dict(engine_step_count=int(self._bound.step_count))      # the counter-based dropout stream resumes where it stopped
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)                                          # the caller's dict is not modified
        extra, legacy = sd.pop('a4r', None), sd.pop('a4r_flat', None)
        super().load_state_dict(sd)                            # a reference checkpoint's exp_avg / exp_avg_sq / step land in self.state
        self._pending = dict(extra=extra, legacy=legacy, late=self._bound is not None)
        if extra:                                               # the engine may not exist yet (built at the first forward): leave the
            for g in self.param_groups:                         # dropout counter on the parameters, TransRecEngine picks it up
                for p in g['params']:
                    if getattr(p, '_a4r_flat', None) is not None:
                        p._a4r_flat[0].step_count = int(extra.get('engine_step_count', 0))
                    else:
                        p._a4r_resume_step = int(extra.get('engine_step_count', 0))
        if self._bound is not None:
            self._apply_pending()

    def _apply_pending(self):
        pend = getattr(self, '_pending', None)
        if pend is None or self._bound is None:
            return
        self._pending = None
        if 'm' in pend:                                        # moments carried over an engine rebuild (step())
            self._step = pend['step']
            self._m.copy_(pend['m'])
            self._v.copy_(pend['v'])
            return
        if pend.get('legacy') is not None:                     # round-1 checkpoints of this package
            self._step = pend['legacy']['step']
            self._m.copy_(pend['legacy']['m'])
            self._v.copy_(pend['legacy']['v'])
        else:
            for g in self.param_groups:
                for p in g['params']:
                    st = self.state.get(p)
                    if st and 'exp_avg' in st:
                        _, off, n = p._a4r_flat
                        self._m[off:off + n].copy_(st['exp_avg'].reshape(-1))
                        self._v[off:off + n].copy_(st['exp_avg_sq'].reshape(-1))
                        self._step = int(float(st['step']))
            self._state_views()
        if pend.get('extra') and pend.get('late'):             # engine existed when the state was loaded; a lazily built
            self._bound.step_count = int(pend['extra'].get('engine_step_count', self._bound.step_count))   # one read p._a4r_resume_step


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW over the engine's flat buffers: FusedAdam with decoupled weight decay and AdamW's default weight_decay=0.01."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None, max_grad_norm=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, foreach=foreach, maximize=maximize,
                         capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=True, max_grad_norm=max_grad_norm)


def from_args(param_groups, args):
    """The optimizer of the entry points' --optimizer / --weight_decay / --max_grad_norm flags; the defaults (adam, 0, 0 = off) give FusedAdam(groups),
    the reference's torch.optim.Adam."""
    name = getattr(args, 'optimizer', 'adam')
    wd = float(getattr(args, 'weight_decay', 0.0))
    clip = float(getattr(args, 'max_grad_norm', 0.0))
    kw = dict(max_grad_norm=clip) if clip > 0 else {}
    if name == 'adamw':
        return FusedAdamW(param_groups, weight_decay=wd, **kw)
    if name != 'adam':
        raise ValueError(f'--optimizer {name!r}: adam or adamw')
    if wd:
        kw['weight_decay'] = wd
    return FusedAdam(param_groups, **kw)
