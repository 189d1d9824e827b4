"""Records tests/golden/label_ranking.npz: sklearn.metrics.label_ranking_average_precision_score, coverage_error,
label_ranking_loss and the mean roc_auc_score over the rows that hold both classes, on a 120 x 37 matrix of which every second
row has scores quantised to 1 / 8 (ties), with empty and full rows (recorded with scikit-learn 1.7.2; the tests need no
sklearn).

    python tests/golden/make_golden_label_ranking.py
"""
import os

import numpy as np
import sklearn
from sklearn.metrics import coverage_error, label_ranking_average_precision_score, label_ranking_loss, roc_auc_score


def main():
    rng = np.random.default_rng(20261021)
    n, L = 120, 37
    scores = rng.standard_normal((n, L)).astype(np.float32)
    scores[::2] = (np.round(scores[::2] * 8.0) / 8.0).astype(np.float32)      # half the rows: ties dominate
    targets = (rng.random((n, L)) < 0.2).astype(np.float32)
    targets[5, :] = 0.0                                                       # empty rows, a quantised and a plain one
    targets[76, :] = 0.0
    targets[9, :] = 1.0                                                       # full rows
    targets[40, :] = 1.0
    s64 = scores.astype(np.float64)
    both = [i for i in range(n) if 0 < targets[i].sum() < L]
    out = {'scores': scores, 'targets': targets, 'sklearn_version': np.asarray(sklearn.__version__),
           'lrap': np.float64(label_ranking_average_precision_score(targets, s64)),
           'coverage_error': np.float64(coverage_error(targets, s64)),
           'ranking_loss': np.float64(label_ranking_loss(targets, s64)),
           'instance_auc': np.float64(np.mean([roc_auc_score(targets[i], s64[i]) for i in both])),
           'n_with_both': np.int64(len(both))}
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'label_ranking.npz'), **out)
    print({k: (v.shape if v.ndim else v.item()) for k, v in out.items()})


if __name__ == '__main__':
    main()
