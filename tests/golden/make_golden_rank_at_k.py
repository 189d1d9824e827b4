"""Records tests/golden/rank_at_k.npz: sklearn.metrics.ndcg_score(targets, scores, k=k, ignore_ties=True) for k = 1, 3, 5, 10
on tie-free scores (recorded with scikit-learn 1.7.2; the tests need no sklearn).

    python tests/golden/make_golden_rank_at_k.py
"""
import os

import numpy as np
import sklearn
from sklearn.metrics import ndcg_score

KS = (1, 3, 5, 10)


def main():
    rng = np.random.default_rng(20261019)
    n, L = 120, 37
    scores = rng.standard_normal((n, L)).astype(np.float32)
    assert all(len(np.unique(row)) == L for row in scores)          # tie-free: ignore_ties=True changes nothing
    targets = (rng.random((n, L)) < 0.12).astype(np.float32)
    targets[5, :] = 0.0                                             # gold-free rows: sklearn gives them an nDCG of 0
    targets[77, :] = 0.0
    targets[9, :] = 1.0                                             # an all-gold row
    out = {'scores': scores, 'targets': targets, 'ks': np.asarray(KS, dtype=np.int64),
           'sklearn_version': np.asarray(sklearn.__version__)}
    for k in KS:
        out['ndcg_%d' % k] = np.float64(ndcg_score(targets, scores.astype(np.float64), k=k, ignore_ties=True))
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rank_at_k.npz'), **out)
    print({k: (v.shape if v.ndim else v.item()) for k, v in out.items()})


if __name__ == '__main__':
    main()
