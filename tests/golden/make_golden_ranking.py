#!/usr/bin/env python3
"""Golden vectors for the ranking metrics the reference computes after an evaluation epoch (utils/evals.py:316-407
compute_metrics with all_metrics=True: compute_auc, compute_aupr, compute_fdr).

Runs ONLY in the build container: imports the reference's own `utils.evals` with ONE shim -- sklearn removed the `reorder`
keyword of metrics.auc that compute_aupr passes (the bare `except` there swallows the TypeError and the mean prints nan); the
shim drops the keyword, nothing else.

"clean" cases (every label has both classes): what the reference's compute_metrics(all_metrics=True) returns.
One "degenerate" case (a label without positives, an all-positive label, a column with a NaN score): per-label sklearn values
for the labels that can be ranked, NaN elsewhere by the rules of include/lamp_hip.h, aggregates over the finite entries.
Data only; scores are stored as float16-exact or quantised values where that keeps the archive small.
"""
import argparse
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get('LAMP_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path = [REF] + [p for p in sys.path if os.path.abspath(p or '.') not in
                    (os.path.abspath(os.path.join(HERE, '..', '..')),
                     os.path.abspath(os.path.join(HERE, '..', '..', 'dropin')), HERE,
                     os.path.abspath(os.path.join(HERE, '..')))]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from sklearn import metrics as skm  # noqa: E402

from utils import evals  # noqa: E402

assert os.path.abspath(evals.__file__).startswith(os.path.abspath(REF))

_auc = skm.auc


def _auc_without_reorder(x, y, reorder=None):
    return _auc(x, y)


class _Metrics(object):
    """sklearn.metrics as utils.evals sees it, with the removed keyword dropped."""

    def __getattr__(self, name):
        return _auc_without_reorder if name == 'auc' else getattr(skm, name)


evals.metrics = _Metrics()


def inputs(n, L, kind, pos_rate, seed):
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(n, L, generator=g) < pos_rate).float()
    if n >= 2:          # clean: both classes in every label
        t[0] = 1
        t[1] = 0
    scale = 40.0 if kind == 'saturated' else 1.5
    p = torch.sigmoid((torch.randn(n, L, generator=g) + (t - 0.5) * 1.5) * scale)
    if kind == 'quantised':
        p = torch.round(p * 8) / 8
    else:
        p = p.half().float()     # fp16-exact fp32 scores: the archive stores them in half the bytes, ties stay rare
    return p.float(), t


def sk_column(p, t):
    auc = skm.roc_auc_score(t, p)
    prec, rec, _ = skm.precision_recall_curve(t, p, pos_label=1)
    aupr = skm.auc(rec, prec)
    fdr = 1 - prec
    i = next(i for i, x in enumerate(fdr) if x <= 0.5)
    return auc, aupr, rec[i]


def main():
    out = {}
    args = argparse.Namespace(br_threshold=0.5, decoder='graph')
    clean = (('n2', 2, 3, 'normal', 0.5), ('n37', 37, 5, 'normal', 0.3), ('n300', 300, 12, 'normal', 0.1),
             ('n300sat', 300, 12, 'saturated', 0.2), ('n257q', 257, 9, 'quantised', 0.3),
             ('reuters', 3019, 90, 'normal', 0.02), ('reutersq', 3019, 90, 'quantised', 0.05))
    for seed, (name, n, L, kind, rate) in enumerate(clean):
        p, t = inputs(n, L, kind, rate, 100 + seed)
        m = evals.compute_metrics(p.clone(), t.clone(), 0.0, args, 0.0, all_metrics=True, verbose=False)
        assert len(m['allAUC']) == L and len(m['allAUPR']) == L
        # compute_fdr keeps its per-label array to itself: the same sklearn calls, label by label
        fdr = np.array([sk_column(p[:, l].numpy(), t[:, l].numpy())[2] for l in range(L)])
        assert abs(np.mean(fdr) - m['meanFDR']) < 1e-15
        out[name + '__probs'] = p.numpy().astype(np.float16)
        assert np.array_equal(out[name + '__probs'].astype(np.float32), p.numpy())
        out[name + '__targets'] = t.numpy().astype(np.uint8)
        out[name + '__auc'] = np.asarray(m['allAUC'], dtype=np.float64)
        out[name + '__aupr'] = np.asarray(m['allAUPR'], dtype=np.float64)
        out[name + '__fdr'] = fdr
        out[name + '__agg'] = np.array([m['meanAUC'], m['medianAUC'], m['meanAUPR'], m['medianAUPR'], m['meanFDR'],
                                        m['medianFDR']], dtype=np.float64)
        out[name + '__thresholded'] = np.array([m['ACC'], m['HA'], m['ebF1'], m['miF1'], m['maF1']], dtype=np.float64)
    # n = 1: nothing can be ranked by AUC (one class); the positive label has AUPR / FDR recall by sklearn
    p1, t1 = torch.tensor([[0.25, 0.75, 0.5]]), torch.tensor([[1., 0., 1.]])
    # degenerate: label 1 without positives, label 3 all positive, label 5 holds a NaN score
    p, t = inputs(200, 7, 'normal', 0.2, 77)
    t[:, 1] = 0
    t[:, 3] = 1
    p[17, 5] = float('nan')
    for name, p, t in (('n1', p1, t1), ('degenerate', p, t)):
        n, L = p.shape
        auc, aupr, fdr = (np.full(L, np.nan) for _ in range(3))
        for l in range(L):
            pc, tc = p[:, l].numpy(), t[:, l].numpy()
            if np.isnan(pc).any() or tc.sum() == 0:
                continue                     # unranked / no positives: NaN in all three
            a, b, c = sk_column(pc, tc) if tc.sum() < n else (np.nan,) + sk_column_one_class(pc, tc)
            auc[l], aupr[l], fdr[l] = a, b, c
        out[name + '__probs'] = p.numpy().astype(np.float16)
        assert np.array_equal(np.nan_to_num(out[name + '__probs'].astype(np.float32), nan=-1), np.nan_to_num(p.numpy(), nan=-1))
        out[name + '__targets'] = t.numpy().astype(np.uint8)
        out[name + '__auc'], out[name + '__aupr'], out[name + '__fdr'] = auc, aupr, fdr
        agg = []
        for v in (auc, aupr, fdr):
            f = v[np.isfinite(v)]
            agg += [np.mean(f), np.median(f)] if f.size else [np.nan, np.nan]
        out[name + '__agg'] = np.array(agg, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, 'ranking.npz'), **out)
    print('wrote ranking.npz (%d bytes):' % os.path.getsize(os.path.join(HERE, 'ranking.npz')),
          {k: out[k] for k in out if k.endswith('__agg')})


def sk_column_one_class(p, t):
    """An all-positive column: roc_auc_score raises (one class), the precision-recall curve is defined."""
    prec, rec, _ = skm.precision_recall_curve(t, p, pos_label=1)
    fdr = 1 - prec
    i = next(i for i, x in enumerate(fdr) if x <= 0.5)
    return skm.auc(rec, prec), rec[i]


if __name__ == '__main__':
    main()
