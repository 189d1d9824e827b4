"""optimizer.step() of the training loop (train.py:48) as ONE HIP launch for the whole model (lamp_optim_step).

`Adam` is torch.optim.Adam as main.py:99 calls it -- betas given by the caller, torch's default eps, no weight decay, no
amsgrad, bias correction from the step count; `SGD` is the plain `-optim sgd` update.  Both are torch.optim.Optimizer
subclasses with torch's own state layout (per parameter: `step` a float32 CPU scalar tensor, `exp_avg`, `exp_avg_sq`), so
`state_dict()` / `load_state_dict()` move optimizer state between them and torch.optim.Adam in both directions, and
`param_groups[i]['lr']` is read on every step: torch.optim.lr_scheduler.StepLR (main.py:100) works unchanged.

The table of (param, grad, exp_avg, exp_avg_sq, numel) is rebuilt from the live pointers on every step -- the deferred weight
gradients of lamp_amd/training.py assign a fresh `.grad` tensor per step -- and travels in the kernel arguments: no device
allocation, no host wait.  Parameters whose `.grad` is None are skipped, as torch does.  There is no CPU path.

Opt-in, all through lamp_optim_step_ext and still one optimizer launch per hyper-parameter set:
  weight_decay            read per param group, handed to the kernel per ENTRY: groups that differ only in their decay share
                          one launch.  Adam: torch's L2 form, or AdamW's with decoupled_weight_decay=True (`AdamW` is that with
                          torch's default 1e-2).  SGD: the L2 form.
  momentum (SGD)          state['momentum_buffer'], as torch.optim.SGD keeps it.  No nesterov, no dampening.
  max_grad_norm           gradient clipping by the GLOBAL norm over every parameter of the optimizer: one lamp_grad_norm
                          (fp64 accumulation, no atomics) writes the device record `optimizer.grad_state` = (norm, scale,
                          finite, 0), and the update uses g * scale in registers.  `.grad` itself is not rewritten.
  skip_nonfinite          when the norm is inf or NaN the update launch writes nothing and the device int32
                          `optimizer.skipped_steps` goes up by one.  step() never reads either tensor.  A skipped step still
                          advances the host-side `step` that Adam's bias correction uses: the host cannot know without a
                          read-back, and one correction factor a step further on is harmless next to a NaN model.
With every option at its default, step() makes exactly the call it has always made (N.optim_step, no norm launch).  What is
not served -- amsgrad, maximize, nesterov, dampening -- is a ValueError at construction.  `grad_norm(params)` is the norm
alone, a device scalar, for use with any optimizer.
"""
import contextlib

import torch

from . import _native as N


def _check(p):
    g = p.grad
    if g.is_sparse:
        raise RuntimeError('lamp_amd.optim does not support sparse gradients')
    if not (p.is_cuda and g.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32):
        raise RuntimeError('lamp_amd.optim updates fp32 parameters on a HIP device only; got %s %s (grad %s %s). There is no '
                           'CPU path.' % (p.device, p.dtype, g.device, g.dtype))
    if not p.is_contiguous():
        raise RuntimeError('lamp_amd.optim expects contiguous parameters')
    return g if g.is_contiguous() else g.contiguous()


def _on(dev):
    """Launches go to the current device's stream: switch only when the tensors live elsewhere."""
    return contextlib.nullcontext() if dev.index == torch.cuda.current_device() else torch.cuda.device(dev)


def _check_common(who, weight_decay, max_grad_norm, unserved):
    if not 0.0 <= weight_decay < float('inf'):
        raise ValueError('%s: invalid weight_decay %r' % (who, weight_decay))
    if max_grad_norm is not None and not 0.0 <= float(max_grad_norm) < float('inf'):
        raise ValueError('%s: max_grad_norm %r: None, or a finite number >= 0' % (who, max_grad_norm))
    on = sorted(k for k, v in unserved.items() if v)
    if on:
        raise ValueError('%s does not serve %s' % (who, ', '.join(on)))


def grad_norm(params):
    """The global L2 norm of the `.grad` of every parameter in `params`, accumulated in fp64 on the device (lamp_grad_norm):
    a 0-dim fp32 DEVICE tensor, nothing read back.  A diagnostic, usable beside torch's optimizers too."""
    entries = [(None, _check(p), None, None) for p in params if p.grad is not None]
    if not entries:
        raise ValueError('grad_norm: no parameter has a gradient')
    dev = entries[0][1].device
    if any(e[1].device != dev for e in entries):
        raise RuntimeError('grad_norm: the gradients live on more than one device')
    rec = torch.empty(4, dtype=torch.float32, device=dev)
    with _on(dev):
        N.grad_norm(entries, None, rec)
    return rec[0]


class _Base(torch.optim.Optimizer):
    KIND = None
    max_grad_norm = None
    skip_nonfinite = False
    grad_state = None        # (4,) fp32 device tensor: (norm, scale, finite, 0) of the last step with clipping or skipping
    skipped_steps = None     # 0-dim int32 device tensor: steps whose norm was not finite

    def _launch(self, by_key):
        """by_key: {(device, step, hyper-parameters...): [(p, g, m, v)]} -> one lamp_optim_step call each.  The tensors' version
        counters are bumped as torch's in-place updates would (weights-only caches of the eval path watch them)."""
        touched = [t for entries in by_key.values() for e in entries for t in (e[0], e[2], e[3]) if t is not None]
        if touched:
            torch.autograd.graph.increment_version(touched)
        for (dev, step, lr, b1, b2, eps), entries in by_key.items():
            if dev.index != torch.cuda.current_device():
                with torch.cuda.device(dev):
                    N.optim_step(entries, self.KIND, step, lr, b1, b2, eps)
            else:
                N.optim_step(entries, self.KIND, step, lr, b1, b2, eps)

    def _extended(self):
        return (self.max_grad_norm is not None or self.skip_nonfinite or
                any(g.get('weight_decay') or g.get('momentum') for g in self.param_groups))

    def _launch_ext(self, by_key):
        """by_key: {(device, step, lr, b1, b2, eps, decoupled, momentum): [((p, g, m, v), weight_decay)]}.  One lamp_grad_norm
        over every entry (when clipping or skipping), then one lamp_optim_step_ext per key."""
        if not by_key:
            return
        touched = [t for rows in by_key.values() for e, _ in rows for t in (e[0], e[2], e[3]) if t is not None]
        torch.autograd.graph.increment_version(touched)
        devs = {k[0] for k in by_key}
        need_norm = self.max_grad_norm is not None or self.skip_nonfinite
        if need_norm and len(devs) > 1:
            raise RuntimeError('lamp_amd.optim: max_grad_norm / skip_nonfinite take the norm on ONE device; the parameters '
                               'live on %d' % len(devs))
        dev = next(iter(devs))
        with _on(dev):
            state = None
            if need_norm:
                if self.grad_state is None or self.grad_state.device != dev:
                    self.grad_state = torch.zeros(4, dtype=torch.float32, device=dev)
                    self.skipped_steps = torch.zeros((), dtype=torch.int32, device=dev)
                state = self.grad_state
                N.grad_norm([e for rows in by_key.values() for e, _ in rows], self.max_grad_norm, state,
                            self.skipped_steps if self.skip_nonfinite else None)
        for (d, step, lr, b1, b2, eps, decoupled, momentum), rows in by_key.items():
            with _on(d):
                N.optim_step_ext([e for e, _ in rows], self.KIND, step, lr, b1, b2, eps, weight_decay=[w for _, w in rows],
                                 decoupled=decoupled, momentum=momentum, grad_state=state, skip_nonfinite=self.skip_nonfinite)


class Adam(_Base):
    KIND = N.LAMP_OPTIM_ADAM

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False,
                 max_grad_norm=None, skip_nonfinite=False, amsgrad=False, maximize=False):
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError('invalid Adam hyper-parameters: lr=%r betas=%r eps=%r' % (lr, betas, eps))
        _check_common('lamp_amd.optim.' + type(self).__name__, weight_decay, max_grad_norm, dict(amsgrad=amsgrad, maximize=maximize))
        # the keys torch.optim.Adam's param_groups carry, so that a state_dict of one loads into the other
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=bool(decoupled_weight_decay))
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._steps = {}    # id(param) -> int mirror of state['step'] (reading the tensor back every step is host work)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._steps = {}

    @torch.no_grad()
    def step(self, closure=None):
        """One update.  With max_grad_norm / skip_nonfinite the device record of this step is `self.grad_state`, and a step
        that was skipped on the device still counts in state['step'] (see the module docstring)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ext = self._extended()
        by_key, steps = {}, []
        for group in self.param_groups:
            if group.get('amsgrad') or group.get('maximize'):
                raise NotImplementedError('lamp_amd.optim.Adam: no amsgrad or maximize')
            lr, (b1, b2), eps = float(group['lr']), group['betas'], group['eps']
            wd = float(group.get('weight_decay') or 0.0)
            if wd < 0.0:
                raise ValueError('lamp_amd.optim.Adam: invalid weight_decay %r' % (wd,))
            decoupled = bool(group.get('decoupled_weight_decay'))
            for p in group['params']:
                if p.grad is None:
                    continue
                g = _check(p)
                st = self.state[p]
                if len(st) == 0:
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                n = self._steps.get(id(p))
                if n is None:
                    n = int(st['step'].item())      # (a CPU scalar: after construction or load_state_dict only)
                n += 1
                self._steps[id(p)] = n
                steps.append(st['step'])
                m, v = st['exp_avg'], st['exp_avg_sq']
                if not (m.is_contiguous() and v.is_contiguous() and m.dtype == torch.float32 and v.dtype == torch.float32 and
                        m.device == p.device and v.device == p.device):
                    raise RuntimeError('lamp_amd.optim.Adam: exp_avg / exp_avg_sq must be contiguous fp32 on the parameter\'s device')
                if ext:
                    by_key.setdefault((p.device, n, lr, b1, b2, eps, decoupled, 0.0), []).append(((p, g, m, v), wd))
                else:
                    by_key.setdefault((p.device, n, lr, b1, b2, eps), []).append((p, g, m, v))
        if steps:
            cpu = [s for s in steps if not s.is_cuda]
            if cpu:
                torch._foreach_add_(cpu, 1)
            for s in steps:
                if s.is_cuda:      # a capturable torch.optim.Adam's state: keep it where it is
                    s.add_(1)
        if ext:
            self._launch_ext(by_key)
        else:
            self._launch(by_key)
        return loss


class AdamW(Adam):
    """torch.optim.AdamW: Adam with the decoupled decay, w = w (1 - lr weight_decay) before the update, default 1e-2."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 skip_nonfinite=False, amsgrad=False, maximize=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=True,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, amsgrad=amsgrad, maximize=maximize)


class SGD(_Base):
    """w -= lr * grad: `-optim sgd`; opt-in momentum (buf = momentum buf + g; w -= lr buf), L2 weight decay, max_grad_norm and
    skip_nonfinite (the module docstring)."""
    KIND = N.LAMP_OPTIM_SGD

    def __init__(self, params, lr=1e-3, momentum=0, weight_decay=0, max_grad_norm=None, skip_nonfinite=False, dampening=0,
                 nesterov=False, maximize=False):
        if lr < 0.0:
            raise ValueError('invalid learning rate: %r' % (lr,))
        if not 0.0 <= momentum < 1.0:
            raise ValueError('lamp_amd.optim.SGD: momentum %r is not in [0, 1)' % (momentum,))
        _check_common('lamp_amd.optim.SGD', weight_decay, max_grad_norm, dict(dampening=dampening, nesterov=nesterov, maximize=maximize))
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False, maximize=False,
                        foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ext = self._extended()
        by_key = {}
        for group in self.param_groups:
            if group.get('nesterov') or group.get('maximize') or group.get('dampening'):
                raise NotImplementedError('lamp_amd.optim.SGD: no nesterov, dampening or maximize')
            lr = float(group['lr'])
            momentum, wd = float(group.get('momentum') or 0.0), float(group.get('weight_decay') or 0.0)
            if not 0.0 <= momentum < 1.0 or wd < 0.0:
                raise ValueError('lamp_amd.optim.SGD: invalid momentum %r / weight_decay %r' % (momentum, wd))
            for p in group['params']:
                if p.grad is None:
                    continue
                g = _check(p)
                if not ext:
                    by_key.setdefault((p.device, 0, lr, 0.0, 0.0, 0.0), []).append((p, g, None, None))
                    continue
                buf = None
                if momentum:
                    st = self.state[p]
                    buf = st.get('momentum_buffer')
                    if buf is None:     # zeros: momentum * 0 + g is torch's "first step copies the gradient"
                        buf = st['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    if not (buf.is_contiguous() and buf.dtype == torch.float32 and buf.device == p.device):
                        raise RuntimeError('lamp_amd.optim.SGD: momentum_buffer must be contiguous fp32 on the parameter\'s device')
                by_key.setdefault((p.device, 0, lr, 0.0, 0.0, 0.0, False, momentum), []).append(((p, g, buf, None), wd))
        if ext:
            self._launch_ext(by_key)
        else:
            self._launch(by_key)
        return loss
