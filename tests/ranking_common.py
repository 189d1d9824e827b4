"""Shared pieces of the ranking-metric tests: a torch-CPU fp64 restatement of the definitions in include/lamp_hip.h
(lamp_ranking_metrics) and DESIGN.md section 8.2, input generators, fixture access.  Test infrastructure only: nothing under
lamp_amd/ imports it."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ranking.npz')
NAN = float('nan')


def column_ref(p, t, cutoff=0.5):
    """(auc, aupr, fdr_recall, P, N) of one column: p float32 scores, t targets.  Integer numerators, fp64 elsewhere."""
    p, t = p.float(), t.float()
    if bool(torch.isnan(p).any()) or bool(((p < 0) | (p > 1)).any()) or bool(((t != 0) & (t != 1)).any()):
        return NAN, NAN, NAN, 0, 0
    order = torch.argsort(p, descending=True, stable=True)
    ps, ts = p[order], t[order].long()
    n = ps.numel()
    end = torch.ones(n, dtype=torch.bool)
    end[:-1] = ps[1:] != ps[:-1]
    idx = end.nonzero().flatten()
    tp = ts.cumsum(0)[idx]                       # int64, cumulative through each tie group
    cnt = idx + 1
    fp = cnt - tp
    P, N = int(tp[-1]), int(fp[-1])
    zero = torch.zeros(1, dtype=torch.long)
    tp_prev, fp_prev = torch.cat((zero, tp[:-1])), torch.cat((zero, fp[:-1]))
    num = int(((fp - fp_prev) * (tp + tp_prev)).sum())
    auc = float(num) / float(2 * P * N) if P > 0 and N > 0 else NAN
    if P == 0:
        return auc, NAN, NAN, P, N
    q = tp.double() / cnt.double()
    q_prev = torch.cat((torch.ones(1, dtype=torch.float64), q[:-1]))
    r = tp.double() / float(P)
    r_prev = torch.cat((torch.zeros(1, dtype=torch.float64), r[:-1]))
    aupr = float(((r - r_prev) * (q + q_prev) / 2).cumsum(0)[-1])      # summed in group order
    ok = ((1.0 - q) <= cutoff).nonzero().flatten()
    fdr = float(r[ok[-1]]) if ok.numel() else 0.0
    return auc, aupr, fdr, P, N


def ranking_ref(probs, targets, cutoff=0.5):
    """Per-label float64 arrays (auc, aupr, fdr_recall) and int64 (n_pos, n_neg) of (n, L) cpu matrices."""
    L = probs.size(1)
    out = np.empty((3, L), dtype=np.float64)
    cnt = np.empty((2, L), dtype=np.int64)
    for l in range(L):
        a, b, c, P, N = column_ref(probs[:, l], targets[:, l], cutoff)
        out[:, l] = (a, b, c)
        cnt[:, l] = (P, N)
    return out[0], out[1], out[2], cnt[0], cnt[1]


def finite_stats(v):
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v)]
    return (float(np.mean(v)), float(np.median(v))) if v.size else (NAN, NAN)


def make_inputs(n, L, kind='normal', pos_rate=0.1, seed=0, both_classes=False):
    """(probs, targets) float32 cpu.  kind: 'normal' = sigmoid of logits correlated with the target; 'saturated' = the same,
    pushed until many scores are exactly 0.0 / 1.0; 'quantised' = rounded to 1/8 so that ties dominate."""
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(n, L, generator=g) < pos_rate).float()
    if both_classes and n >= 2:
        t[0] = 1
        t[1] = 0
    scale = 40.0 if kind == 'saturated' else 1.5
    z = (torch.randn(n, L, generator=g) + (t - 0.5) * 1.5) * scale
    p = torch.sigmoid(z)
    if kind == 'quantised':
        p = torch.round(p * 8) / 8
    return p.float().contiguous(), t.contiguous()


def fixture_cases():
    """{name: dict of numpy arrays} of tests/golden/ranking.npz (keys '<name>__<field>')."""
    z = np.load(GOLDEN, allow_pickle=False)
    cases = {}
    for k in z.files:
        name, field = k.split('__', 1)
        cases.setdefault(name, {})[field] = z[k]
    return cases


def same_bits(a, b):
    """Equal as fp64 bit patterns (NaN equals NaN)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)) or
                                       (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])))


def max_diff(a, b):
    """max |a - b| with NaN == NaN; inf when the NaN patterns differ."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    if a.shape != b.shape or not np.array_equal(na, nb):
        return float('inf')
    d = np.abs(a[~na] - b[~nb])
    return float(d.max()) if d.size else 0.0
