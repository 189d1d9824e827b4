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


def average_weight(kind, decay, warmup, n_averaged):
    """The lerp weight of the update that follows `n_averaged` counted ones, a Python float (double), as torch takes it on the
    host: 1 for the first (a copy); 'ema': 1 - d_t with d_t = decay, or min(decay, (1 + t) / (10 + t)) under warmup, t =
    n_averaged; 'swa': 1 / (n_averaged + 1)."""
    if n_averaged == 0:
        return 1.0
    if kind == 'swa':
        return 1.0 / (n_averaged + 1)
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + n_averaged) / (10.0 + n_averaged))
    return 1.0 - d


class WeightAverage(object):
    """An average of the weights kept beside them: kind 'ema' (a = a + (1 - decay)(p - a), optionally
    with the warmup min(decay, (1 + t) / (10 + t))) or 'swa' (the running mean), torch.optim.swa_utils.AveragedModel's arithmetic
    without its deep copy: one fp32 buffer per parameter, allocated here and never again, and ONE lamp_weight_average launch
    per device and 72 parameters per update.

        avg = WeightAverage(optimizer_params, kind='ema', decay=0.999)
        loss.backward(); optimizer.step(); avg.update()
        with avg.applied():            # the model holds the average: evaluate, save, ...
            evaluate(model)            # (one lamp_weight_swap in, one out; the eval path's cached tables follow)

    update() never looks at the optimizer: after a step that skip_nonfinite left out, the unchanged weights are averaged in, as
    AveragedModel does.  `update_every=k` acts on every k-th call.  There are no running statistics in this model family, so an
    average of the parameters is a complete model.  Not served: fp64 or bf16 averages, per-group decays, averaging of buffers,
    nn.DataParallel replicas, a device-side count."""

    def __init__(self, params, kind='ema', decay=0.999, warmup=False, update_every=1):
        if kind not in ('ema', 'swa'):
            raise ValueError("WeightAverage: kind %r is not 'ema' or 'swa'" % (kind,))
        if not 0.0 <= float(decay) < 1.0:       # (false for NaN)
            raise ValueError('WeightAverage: decay %r is not in [0, 1)' % (decay,))
        if isinstance(update_every, bool) or int(update_every) != update_every or update_every < 1:
            raise ValueError('WeightAverage: update_every %r: an integer >= 1' % (update_every,))
        self.kind, self.decay, self.warmup, self.update_every = kind, float(decay), bool(warmup), int(update_every)
        self.params, seen = [], set()
        for p in params:
            if id(p) in seen:
                continue
            seen.add(id(p))
            if not (p.is_cuda and p.dtype == torch.float32):
                raise RuntimeError('lamp_amd.optim updates fp32 parameters on a HIP device only; got %s %s. There is no CPU path.'
                                   % (p.device, p.dtype))
            if not p.is_contiguous():
                raise RuntimeError('lamp_amd.optim expects contiguous parameters')
            self.params.append(p)
        self.buffers = [torch.zeros_like(p, memory_format=torch.contiguous_format, requires_grad=False) for p in self.params]
        self.n_averaged = 0      # counted updates
        self.n_calls = 0         # calls of update()
        self.last_weight = None  # the weight of the last call of update(), None when update_every left it out
        self._swapped = False
        self._by_device = {}
        for p, a in zip(self.params, self.buffers):
            self._by_device.setdefault(p.device, []).append((p, a))
        self._tables = {}        # device -> (the parameters' pointers, the ctypes table built from them)

    def _launches(self):
        """(device, entries, table) per device.  The buffers never move and the parameters rarely do (.to(), .data =): the
        table is kept and rebuilt when a parameter's pointer is not the one it was built from."""
        for dev, entries in self._by_device.items():
            ptrs = [p.data_ptr() for p, _ in entries]
            kept = self._tables.get(dev)
            if kept is None or kept[0] != ptrs:
                kept = self._tables[dev] = (ptrs, N.average_table('WeightAverage', entries))
            yield dev, entries, kept[1]

    def next_weight(self):
        return average_weight(self.kind, self.decay, self.warmup, self.n_averaged)

    def update(self):
        """Fold the current weights into the average: host integers and one launch per device per 72 parameters."""
        if self._swapped:
            raise RuntimeError('WeightAverage.update() while the average is swapped in: the model holds the average and the '
                               'buffers the trained weights')
        self.n_calls += 1
        if self.n_calls % self.update_every:
            self.last_weight = None
            return
        w = self.last_weight = self.next_weight()
        if self.buffers:
            torch.autograd.graph.increment_version(self.buffers)
        for dev, entries, table in self._launches():
            with _on(dev):
                N.weight_average(entries, w, table)
        self.n_averaged += 1

    def swap(self):
        """Exchange the weights and their averages in place (one launch per device per 72 parameters).  The version counters
        of both sides move, so the eval path's weights-only tables and a learnable label bias's folded buffer are rebuilt by the
        next forward."""
        if self.params:
            torch.autograd.graph.increment_version(self.params + self.buffers)
        for dev, entries, table in self._launches():
            with _on(dev):
                N.weight_swap(entries, table)
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def applied(self):
        """The model holds the average inside the block and the trained weights after it, also after an exception."""
        if self._swapped:
            raise RuntimeError('WeightAverage.applied() does not nest: the average is already swapped in')
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    def _not_swapped(self, who):
        if self._swapped:
            raise RuntimeError('WeightAverage.%s while the average is swapped in: the buffers hold the trained weights' % who)

    def copy_to(self, target):
        """Load the average OUT OF PLACE, by torch copies: into the parameters this average was built over (`target` the
        nn.Module that owns them: the model then holds the average for good, and the buffers keep it), or into an iterable
        of as many parameters in this average's order.  Another module takes load_state_dict(averaged_state_dict(model))."""
        self._not_swapped('copy_to()')
        if isinstance(target, torch.nn.Module):
            own = {id(p): a for p, a in zip(self.params, self.buffers)}
            pairs = [(p, own[id(p)]) for p in target.parameters() if id(p) in own]
            if len(pairs) != len(own):
                raise ValueError('WeightAverage.copy_to: the module owns %d of the %d averaged parameters; load '
                                 'averaged_state_dict(model) into another module' % (len(pairs), len(own)))
        else:
            ps = list(target)
            if len(ps) != len(self.buffers) or any(p.shape != a.shape for p, a in zip(ps, self.buffers)):
                raise ValueError('WeightAverage.copy_to: %d parameters do not match the %d averaged ones in count or shape'
                                 % (len(ps), len(self.buffers)))
            pairs = list(zip(ps, self.buffers))
        with torch.no_grad():
            for p, a in pairs:
                p.copy_(a)

    def averaged_state_dict(self, model):
        """model.state_dict() with the averaged tensors in the places of the parameters this average covers (every name of a
        tied weight).  Nothing is cloned and nothing is swapped: the values are the live tensors, as state_dict()'s are."""
        self._not_swapped('averaged_state_dict()')
        own = {id(p): a for p, a in zip(self.params, self.buffers)}
        sd = model.state_dict()
        for name, p in model.named_parameters(remove_duplicate=False):
            if id(p) in own and name in sd:
                sd[name] = own[id(p)]
        return sd

    def state_dict(self, buffers=True):
        """kind, decay, warmup, update_every, n_averaged, n_calls and (unless buffers=False) the averages in parameter order."""
        self._not_swapped('state_dict()')
        sd = dict(kind=self.kind, decay=self.decay, warmup=self.warmup, update_every=self.update_every,
                  n_averaged=self.n_averaged, n_calls=self.n_calls)
        if buffers:
            sd['buffers'] = list(self.buffers)
        return sd

    def load_state_dict(self, sd):
        """The buffers are written in place (their pointers stay); a state without 'buffers' restores the schedule alone."""
        self._not_swapped('load_state_dict()')
        fresh = WeightAverage([], sd['kind'], sd['decay'], sd['warmup'], sd['update_every'])      # (validates)
        bufs = sd.get('buffers')
        if bufs is not None:
            if len(bufs) != len(self.buffers) or any(b.shape != a.shape for b, a in zip(bufs, self.buffers)):
                raise ValueError('WeightAverage.load_state_dict: %d buffers do not match the %d averaged parameters in count or '
                                 'shape' % (len(bufs), len(self.buffers)))
            with torch.no_grad():
                for b, a in zip(bufs, self.buffers):
                    a.copy_(b)
        self.kind, self.decay, self.warmup, self.update_every = fresh.kind, fresh.decay, fresh.warmup, fresh.update_every
        self.n_averaged, self.n_calls = int(sd['n_averaged']), int(sd['n_calls'])
