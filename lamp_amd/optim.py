"""optimizer.step() of the training loop (train.py:48) as ONE HIP launch for the whole model (lamp_optim_step).

`Adam` is torch.optim.Adam as main.py:99 calls it -- betas given by the caller, torch's default eps, no weight decay, no
amsgrad, bias correction from the step count; `SGD` is the plain `-optim sgd` update.  Both are torch.optim.Optimizer
subclasses with torch's own state layout (per parameter: `step` a float32 CPU scalar tensor, `exp_avg`, `exp_avg_sq`), so
`state_dict()` / `load_state_dict()` move optimizer state between them and torch.optim.Adam in both directions, and
`param_groups[i]['lr']` is read on every step: torch.optim.lr_scheduler.StepLR (main.py:100) works unchanged.

The table of (param, grad, exp_avg, exp_avg_sq, numel) is rebuilt from the live pointers on every step -- the deferred weight
gradients of lamp_amd/training.py assign a fresh `.grad` tensor per step -- and travels in the kernel arguments: no device
allocation, no host wait.  Parameters whose `.grad` is None are skipped, as torch does.  There is no CPU path.
"""
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


class _Base(torch.optim.Optimizer):
    KIND = None

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


class Adam(_Base):
    KIND = N.LAMP_OPTIM_ADAM

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError('invalid Adam hyper-parameters: lr=%r betas=%r eps=%r' % (lr, betas, eps))
        # the keys torch.optim.Adam's param_groups carry, so that a state_dict of one loads into the other
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self._steps = {}    # id(param) -> int mirror of state['step'] (reading the tensor back every step is host work)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._steps = {}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        by_key, steps = {}, []
        for group in self.param_groups:
            if group.get('weight_decay') or group.get('amsgrad') or group.get('maximize'):
                raise NotImplementedError('lamp_amd.optim.Adam is main.py:99\'s Adam: no weight decay, amsgrad or maximize')
            lr, (b1, b2), eps = float(group['lr']), group['betas'], group['eps']
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
                by_key.setdefault((p.device, n, lr, b1, b2, eps), []).append((p, g, m, v))
        if steps:
            cpu = [s for s in steps if not s.is_cuda]
            if cpu:
                torch._foreach_add_(cpu, 1)
            for s in steps:
                if s.is_cuda:      # a capturable torch.optim.Adam's state: keep it where it is
                    s.add_(1)
        self._launch(by_key)
        return loss


class SGD(_Base):
    """w -= lr * grad: `-optim sgd` (no momentum, no weight decay)."""
    KIND = N.LAMP_OPTIM_SGD

    def __init__(self, params, lr=1e-3):
        if lr < 0.0:
            raise ValueError('invalid learning rate: %r' % (lr,))
        defaults = dict(lr=lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, maximize=False, foreach=None,
                        differentiable=False, fused=None)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        by_key = {}
        for group in self.param_groups:
            if group.get('momentum') or group.get('weight_decay') or group.get('nesterov') or group.get('maximize'):
                raise NotImplementedError('lamp_amd.optim.SGD is the plain update: no momentum, weight decay or maximize')
            lr = float(group['lr'])
            for p in group['params']:
                if p.grad is None:
                    continue
                by_key.setdefault((p.device, 0, lr, 0.0, 0.0, 0.0), []).append((p, _check(p), None, None))
        self._launch(by_key)
        return loss
