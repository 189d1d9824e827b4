"""Shared pieces of the lamp_grad_norm / lamp_optim_step_ext tests: the cases, fp64 restatements of the updates with gradient
clipping, weight decay (L2 and decoupled), SGD momentum and the non-finite skip, and torch's own fp32 CPU run of the same
sequence -- clip_grad_norm_ followed by torch.optim.AdamW / Adam(weight_decay=) / SGD(momentum=) -- whose distance to the fp64
formula is the yardstick of train_common.within."""
import math

import torch

import train_common as TC

# 12293 = 3 * 4096 + 5 sits one float past a 16-byte boundary on the device (4-byte aligned only); 0 is skipped
NORM_SIZES = [1, 3, 4095, 4096, 4097, 12293, 0]
MISALIGNED = 12293

# name -> (optimizer, weight_decay, decoupled, momentum)
CONFIGS = {
    'adamw_0.01': ('adam', 0.01, True, 0.0),
    'adamw_0.1': ('adam', 0.1, True, 0.0),
    'adam_l2': ('adam', 0.05, False, 0.0),
    'sgd_momentum': ('sgd', 0.0, False, 0.9),
    'sgd_momentum_decay': ('sgd', 0.05, False, 0.9),
}
CLIPS = ('none', 'binds', 'loose')       # no max_grad_norm; half the first step's fp64 norm; 1e6


def lrs(kind, n_steps):
    """The learning rate changes at step 2."""
    a, b = (2e-3, 5e-4) if kind == 'adam' else (0.05, 0.2)
    return [a if i != 1 else b for i in range(n_steps)]


def norm_case(seed=0, sizes=NORM_SIZES):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in sizes]


def long_table_case(seed=1, n=80):
    """80 entries of 1 to 300 elements: crosses the 72-entry launch boundary."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1 + (i * 37) % 300, generator=g) for i in range(n)]


def norm64(grads):
    """sqrt(sum g^2) in fp64 from the fp32 inputs (a Python float)."""
    return math.sqrt(sum(float((t.double() ** 2).sum()) for t in grads))


def scale32(norm32, max_norm):
    """clip_grad_norm_'s own expression on an fp32 CPU scalar holding the device's norm bits."""
    if max_norm is None:
        return torch.tensor(1.0)
    return torch.clamp(max_norm / (norm32.cpu().float() + 1e-6), max=1.0)


def ext_case(seed, n_steps):
    """train_common.optim_case's tensors plus the norm test's sizes -> (params, grads[step][k])."""
    params, grads = TC.optim_case(seed, n_steps)
    g = torch.Generator().manual_seed(1000 + seed)
    extra = [n for n in NORM_SIZES if n not in [p.numel() for p in params]]
    params = params + [torch.randn(n, generator=g) for n in extra]
    for step in grads:
        step += [torch.randn(n, generator=g) * 0.1 for n in extra]
    return params, grads


def max_norm_of(clip, grads):
    return {'none': None, 'binds': 0.5 * norm64(grads[0]), 'loose': 1e6}[clip]


def reference64(kind, params, grads, lr_seq, wd=0.0, decoupled=False, momentum=0.0, max_norm=None, skip_nonfinite=False,
                betas=TC.ADAM_BETAS, eps=1e-8, wds=None):
    """fp64 evaluation of the update sequence -> [(p, m, v)] per parameter (m = exp_avg or the momentum buffer, v = exp_avg_sq
    or None).  wds: one decay per parameter (default: wd everywhere).  The host-side step count advances on a skipped step."""
    n = len(params)
    wds = [wd] * n if wds is None else wds
    p = [t.detach().cpu().double().clone() for t in params]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    b1, b2 = betas
    for i, lr in enumerate(lr_seq):
        gs = [g.detach().cpu().double() for g in grads[i]]
        step = i + 1
        scale = 1.0
        if max_norm is not None or skip_nonfinite:
            norm = math.sqrt(sum(float((g ** 2).sum()) for g in gs))
            if skip_nonfinite and not math.isfinite(norm):
                continue
            if max_norm is not None:
                coef = max_norm / (norm + 1e-6)
                scale = 1.0 if coef > 1.0 else coef      # (a NaN stays a NaN)
        for k in range(n):
            g = gs[k] * scale if (max_norm is not None) else gs[k]
            if wds[k] and not decoupled:
                g = g + wds[k] * p[k]
            if kind == 'adam':
                if wds[k] and decoupled:
                    p[k] = p[k] * (1 - lr * wds[k])
                m[k] = m[k] + (g - m[k]) * (1 - b1)
                v[k] = v[k] * b2 + (1 - b2) * g * g
                denom = v[k].sqrt() / (1 - b2 ** step) ** 0.5 + eps
                p[k] = p[k] - lr / (1 - b1 ** step) * m[k] / denom
            else:
                if momentum:
                    m[k] = momentum * m[k] + g
                    g = m[k]
                p[k] = p[k] - lr * g
    return [(p[k], m[k], v[k] if kind == 'adam' else None) for k in range(n)]


def torch_fp32(kind, params, grads, lr_seq, wd=0.0, decoupled=False, momentum=0.0, max_norm=None, betas=TC.ADAM_BETAS):
    """torch's own fp32 run on the CPU: clip_grad_norm_ then the optimizer step -> (parameters, optimizer)."""
    cpu = [torch.nn.Parameter(p.clone()) for p in params]
    if kind == 'adam':
        cls = torch.optim.AdamW if decoupled else torch.optim.Adam
        ref = cls(cpu, betas=betas, lr=lr_seq[0], weight_decay=wd, foreach=True)
    else:
        ref = torch.optim.SGD(cpu, lr=lr_seq[0], momentum=momentum, weight_decay=wd, foreach=True)
    for i, lr in enumerate(lr_seq):
        ref.param_groups[0]['lr'] = lr
        for p, gr in zip(cpu, grads[i]):
            p.grad = gr.clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(cpu, max_norm)
        ref.step()
    return cpu, ref


def torch_state(ref, p, kind):
    """(m, v) of one parameter of the torch optimizer, None where it keeps none."""
    st = ref.state[p]
    if kind == 'adam':
        return st['exp_avg'], st['exp_avg_sq']
    return st.get('momentum_buffer'), None


def hand_counted_table():
    """[(numel, chunks of 4096)]: the workspace query is 8 bytes per chunk."""
    return [(1, 1), (4096, 1), (4097, 2), (0, 0), (3 * 4096, 3), (10 * 4096 + 1, 11)]
