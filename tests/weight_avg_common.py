"""Shared pieces of the weight-averaging tests (test_weight_avg_cpu.py, test_weight_avg_gpu.py): an fp64 restatement of
lamp_weight_average (include/lamp_hip.h), of a K-step recurrence over it, and of the host-side weight schedule of
lamp_amd.optim.WeightAverage.  Nothing here imports the library; importable without a GPU.

One update, a = the average, p = the weight, w = the lerp weight AS THE KERNEL SEES IT (a double rounded to fp32 once):

    w < 0.5:   a + w (p - a)            otherwise:   p - (p - a)(1 - w)           (torch's lerp, ATen/native/Lerp.h)

and the three edges, written out in update64 below:
    w == 1   the result is p, bit for bit (a copy: NaN payloads and the sign of zero included)
    w == 0   the result is a, bit for bit (nothing is launched)
    p == a   the result is a (torch would make -inf - -inf = NaN of it; the kernel does not)
"""
import numpy as np
import torch


def f32(w):
    """A Python double rounded to fp32 once, as the host entry rounds `weight`."""
    return float(np.float32(w))


def update64(p, a, w, round_weight=True):
    """One update in fp64 from fp32 (or fp64) tensors p and a and the double w -> fp64 tensor.  Non-finite elements follow
    IEEE arithmetic except for the three edges.  The product w (p - a) is added unrounded (taken in extended precision where
    numpy has one), as torch's CPU lerp does it (vec::fmadd): one rounding less than the plain expression, so the fp64 test
    against AveragedModel compares like with like and the fp32 tests get the better reference.  round_weight=False keeps w a
    double (torch's fp64 AveragedModel)."""
    p64, a64 = p.detach().cpu().double(), a.detach().cpu().double()
    if round_weight:
        w = f32(w)
    if w == 1.0:                      # edge 1: a copy
        return p64.clone()
    if w == 0.0:                      # edge 2: nothing happens
        return a64.clone()
    ext = np.longdouble
    d = (p64 - a64).numpy().astype(ext)
    with np.errstate(invalid='ignore', over='ignore'):
        if w < 0.5:
            out = a64.numpy().astype(ext) + ext(w) * d
        else:
            out = p64.numpy().astype(ext) - d * ext(1.0 - w)
    out = torch.from_numpy(np.ascontiguousarray(out.astype(np.float64))).reshape(p64.shape)
    return torch.where(p64 == a64, a64, out)      # edge 3: equal sides keep the average (also at +-inf)


def schedule_weight(kind, decay, warmup, n_averaged):
    """The weight of the update that follows n_averaged counted ones (a double, as torch takes it on the host)."""
    if n_averaged == 0:
        return 1.0
    if kind == 'swa':
        return 1.0 / (n_averaged + 1)
    assert kind == 'ema'
    d = decay
    if warmup:
        d = min(decay, (1.0 + n_averaged) / (10.0 + n_averaged))
    return 1.0 - d


def schedule(kind, decay, warmup, update_every, n_calls):
    """[(weight or None, n_averaged after, n_calls after)] of n_calls calls of update(): every update_every-th call counts."""
    out, n_avg = [], 0
    for c in range(1, n_calls + 1):
        if c % update_every:
            out.append((None, n_avg, c))
            continue
        out.append((schedule_weight(kind, decay, warmup, n_avg), n_avg + 1, c))
        n_avg += 1
    return out


def recurrence64(weights_seq, kind, decay=0.0, warmup=False, update_every=1, round_weight=True):
    """The fp64 average of a sequence of weight lists: weights_seq[k] = [tensor, ...] after step k -> [fp64 tensor, ...].
    round_weight=False keeps w in double (the restatement of torch's fp64 AveragedModel)."""
    avg, n_avg = None, 0
    for c, ps in enumerate(weights_seq, 1):
        if c % update_every:
            continue
        w = schedule_weight(kind, decay, warmup, n_avg)
        if avg is None:
            avg = [torch.zeros_like(p.detach().cpu().double()) for p in ps]
        avg = [update64(p, a, w, round_weight) for p, a in zip(ps, avg)]
        n_avg += 1
    return avg


def ulp32(x):
    """One fp32 unit in the last place at |x| (fp64 tensor in, fp64 out; the smallest denormal below 2^-126)."""
    a = x.detach().cpu().double().abs().clamp(min=2.0 ** -126, max=3.0e38).float()
    return (torch.nextafter(a, torch.full_like(a, float('inf'))) - a).double()


def planted(n, seed):
    """(p, a) fp32 CPU tensors of n elements: randn with the edge elements planted where n allows -- +-0, a denormal, 1e-30
    beside 1e30, p == a at +-inf, p = +inf against a = -inf, a NaN in p and a NaN in a -- and the mask of the planted NON-FINITE
    elements (compared exactly with the restatement)."""
    g = torch.Generator().manual_seed(seed)
    p, a = torch.randn(n, generator=g), torch.randn(n, generator=g)
    inf, nan = float('inf'), float('nan')
    plants = [(0.0, -0.0), (-0.0, 0.5), (1e-40, 3e-39), (1e-30, 1e30), (1e30, 1e-30), (inf, inf), (-inf, -inf), (inf, -inf),
              (nan, 0.25), (0.25, nan), (1.5, 1.5)]
    hard = torch.zeros(n, dtype=torch.bool)
    if n >= 64:
        for k, (pv, av) in enumerate(plants):
            for i in (7 + 5 * k, n - 3 - 5 * k):          # in the 16-byte body and next to the tail
                p[i], a[i] = pv, av
                hard[i] = not (np.isfinite(pv) and np.isfinite(av))
    elif n >= 3:
        p[0], a[0] = -inf, -inf
        p[n - 1], a[n - 1] = nan, 1.0
        hard[0] = hard[n - 1] = True
    return p, a, hard


def compare(got, p, a, w, hard, what):
    """got (fp32, after the update) against update64(p, a, w): the planted non-finite elements exactly (NaN where NaN, the
    same infinity), every other element within max(1 fp32 ulp at the fp64 value, 4 x the gap of torch's own fp32 CPU lerp
    on the same inputs).  -> the worst used fraction of that bar."""
    got64 = got.detach().cpu().double()
    want = update64(p, a, w)
    nan_w = torch.isnan(want)
    assert torch.equal(torch.isnan(got64), nan_w), '%s: NaNs do not coincide' % what
    inf_w = torch.isinf(want)
    assert torch.equal(got64[inf_w], want[inf_w]) and torch.equal(torch.isinf(got64), inf_w), '%s: infinities differ' % what
    assert torch.equal(got64[hard & ~nan_w], want[hard & ~nan_w]), '%s: a planted non-finite element differs' % what
    ok = ~(nan_w | inf_w | hard)
    t32 = torch.lerp(a.detach().cpu().float(), p.detach().cpu().float(), f32(w)).double()
    # torch's gap is taken per magnitude class, so that the 1e30 plants do not set the bar of the randn elements
    big = (p.detach().cpu().abs() > 1e20) | (a.detach().cpu().abs() > 1e20)
    worst = 0.0
    for cls, name in ((ok & ~big, 'randn'), (ok & big, '1e30')):
        if not bool(cls.any()):
            continue
        fin = cls & torch.isfinite(t32)
        gap = float((t32 - want).abs()[fin].max()) if bool(fin.any()) else 0.0
        err = (got64 - want).abs()[cls]
        tol = torch.maximum(ulp32(want)[cls], torch.full_like(err, 4.0 * gap))
        frac = float((err / tol).max())
        print('%s [%s]: max |err| %.3e, 4 x torch fp32 gap %.3e, worst err / bar %.3f' % (what, name, float(err.max()), 4.0 * gap, frac))
        assert frac <= 1.0, (what, name, frac)
        worst = max(worst, frac)
    return worst
