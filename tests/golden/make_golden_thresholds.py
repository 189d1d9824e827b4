"""Records tests/golden/thresholds.npz: per label column, the threshold at which sklearn's curves have their best Youden J
(roc_curve(drop_intermediate=False): argmax of tpr - fpr) and their best F1 (precision_recall_curve: argmax of
2 p r / (p + r)), with the integer tp / fp behind each (recorded with scikit-learn 1.7.2; the tests need no sklearn).

Every label's optimum is asserted to be unique in exact arithmetic over the integers recovered from sklearn's own curves, and
sklearn's floating-point argmax to be that optimum: the restatement of tests/thresholds_common.py, with whatever tie rule, must
then name the same threshold bit for bit.

    python tests/golden/make_golden_thresholds.py
"""
import os
from fractions import Fraction

import numpy as np
import sklearn
from sklearn.metrics import precision_recall_curve, roc_curve


def unique_argmax(values):
    best = max(values)
    at = [i for i, v in enumerate(values) if v == best]
    assert len(at) == 1, 'the optimum is not unique: %s' % at
    return at[0]


def main():
    rng = np.random.default_rng(20261019)
    n, L = 300, 12
    rates = np.array([0.01, 0.02, 0.03, 0.05, 0.08, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5, 0.7])
    targets = (rng.random((n, L)) < rates[None, :]).astype(np.float32)
    targets[:3, :] = 1.0                                                      # every label has positives ...
    targets[3:6, :] = 0.0                                                     # ... and negatives
    logits = rng.standard_normal((n, L)) * 1.5 + (targets * 2.0 - 1.0) * rng.uniform(0.3, 1.5, size=L)[None, :]
    scores = (1.0 / (1.0 + np.exp(-logits))).astype(np.float32)
    assert all(len(np.unique(scores[:, l])) == n for l in range(L))           # tie-free
    out = {'scores': scores, 'targets': targets, 'sklearn_version': np.asarray(sklearn.__version__)}
    rec = {k: [] for k in ('youden_threshold', 'youden_tp', 'youden_fp', 'f1_threshold', 'f1_tp', 'f1_fp')}
    for l in range(L):
        y, s = targets[:, l], scores[:, l].astype(np.float64)
        P = int(y.sum())
        N = n - P
        # Youden's J
        fpr, tpr, thr = roc_curve(y, s, drop_intermediate=False)
        tp = np.rint(tpr * P).astype(np.int64)
        fp = np.rint(fpr * N).astype(np.int64)
        assert np.array_equal(tp / P, tpr) and np.array_equal(fp / N, fpr)
        at = unique_argmax([int(a) * N - int(b) * P for a, b in zip(tp, fp)])
        assert at == int(np.argmax(tpr - fpr)) and at > 0                     # (entry 0 is sklearn's "predict nothing" point)
        assert np.float32(thr[at]) == thr[at]
        rec['youden_threshold'].append(np.float32(thr[at]))
        rec['youden_tp'].append(tp[at])
        rec['youden_fp'].append(fp[at])
        # F1
        prec, rcl, thr = precision_recall_curve(y, s)
        prec, rcl = prec[:-1], rcl[:-1]                                       # (the last point has no threshold)
        tp = np.rint(rcl * P).astype(np.int64)
        assert np.array_equal(tp / P, rcl)
        pred = np.array([int(round(t / p)) if t > 0 else 0 for t, p in zip(tp, prec)], dtype=np.int64)
        assert all(t == 0 or t / c == p for t, c, p in zip(tp, pred, prec))
        at = unique_argmax([Fraction(2 * int(t), int(c) + P) if t > 0 else Fraction(0) for t, c in zip(tp, pred)])
        with np.errstate(invalid='ignore', divide='ignore'):
            f1 = np.nan_to_num(2.0 * prec * rcl / (prec + rcl), nan=0.0)
        assert at == int(np.argmax(f1))
        assert np.float32(thr[at]) == thr[at]
        rec['f1_threshold'].append(np.float32(thr[at]))
        rec['f1_tp'].append(tp[at])
        rec['f1_fp'].append(pred[at] - tp[at])
    for k, v in rec.items():
        out[k] = np.asarray(v, dtype=np.float32 if k.endswith('threshold') else np.int32)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'thresholds.npz'), **out)
    print({k: (v.shape if v.ndim else v.item()) for k, v in out.items()})
    print({k: out[k].tolist() for k in rec})


if __name__ == '__main__':
    main()
