"""Shared by test_rank_at_k_cpu.py and test_rank_at_k_gpu.py: an fp64 numpy restatement of the row order and of the figures
at k that include/lamp_hip.h defines, and the input generators.  Nothing here imports the code under test."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KINDS = ('normal', 'quantised', 'saturated', 'constant', 'ascending', 'descending', 'special')


def order_ref(scores):
    """(n, L) float32 -> int64 (n, L): every row's columns in rank order -- a number before a NaN, the larger number first
    (+0.0 and -0.0 tied), the lower column on a tie."""
    s = np.asarray(scores, dtype=np.float32)
    isnan = np.isnan(s)
    with np.errstate(invalid='ignore'):      # a signalling NaN among the inputs is quieted by the cast
        key = np.where(isnan, 0.0, s.astype(np.float64) + 0.0)
    col = np.broadcast_to(np.arange(s.shape[1]), s.shape)
    return np.lexsort((col, -key, isnan))


def topk_ref(scores, k):
    """-> (int32 (n, k) columns, uint32 (n, k) bit patterns of the selected scores)."""
    s = np.ascontiguousarray(np.asarray(scores, dtype=np.float32))
    idx = order_ref(s)[:, :k]
    return idx.astype(np.int32), np.take_along_axis(s.view(np.uint32), idx, 1)


def dcg_tables(k):
    d = 1.0 / np.log2(np.arange(k, dtype=np.float64) + 2.0)
    return d, np.concatenate(([0.0], np.cumsum(d)))


def per_sample_ref(idx, targets):
    """-> (hit bool (n, k), ndcg float64 (n, k), recall float64 (n, k), gold int64 (n,)); column j - 1 holds the value at
    rank j.  A sample without a gold label has 0 in both."""
    idx = np.asarray(idx, dtype=np.int64)
    gold_mat = np.asarray(targets) != 0
    gold = gold_mat.sum(1).astype(np.int64)
    k = idx.shape[1]
    hit = np.take_along_axis(gold_mat, idx, 1)
    d, ideal = dcg_tables(k)
    dcg = np.cumsum(hit * d[None, :], axis=1)
    denom = ideal[np.minimum(np.arange(1, k + 1)[None, :], gold[:, None])]
    has = (gold > 0)[:, None]
    ndcg = np.where(has, dcg / np.where(denom > 0, denom, 1.0), 0.0)
    recall = np.where(has, np.cumsum(hit, axis=1) / np.maximum(gold, 1)[:, None].astype(np.float64), 0.0)
    return hit, ndcg, recall, gold


def sums_ref(idx, targets):
    """-> (hits_at_rank int64 (k,), ndcg_sum float64 (k,), recall_sum float64 (k,), n_with_gold)."""
    hit, ndcg, recall, gold = per_sample_ref(idx, targets)
    return hit.sum(0).astype(np.int64), ndcg.sum(0), recall.sum(0), int((gold > 0).sum())


def figures_ref(scores, targets, ks):
    """The dict metrics.rank_at_k returns, from the restatement."""
    n = np.asarray(scores).shape[0]
    k = max(ks)
    hits, ndcg, recall, with_gold = sums_ref(topk_ref(scores, k)[0], targets)
    out = {}
    for j in ks:
        out['P@%d' % j] = float(int(hits[:j].sum())) / float(n * j)
        out['nDCG@%d' % j] = float(ndcg[j - 1]) / n
        out['R@%d' % j] = float(recall[j - 1]) / n
    out['n_with_gold'] = with_gold
    return out


def _bits(words):
    return np.asarray(words, dtype=np.uint32).view(np.float32)


def make_scores(kind, n, L, seed=0):
    """float32 (n, L) of one input kind."""
    rng = np.random.default_rng(seed * 7919 + L * 31 + KINDS.index(kind))
    if kind == 'normal':
        return rng.standard_normal((n, L)).astype(np.float32)
    if kind == 'quantised':        # rounded to 1 / 8: ties dominate
        return (np.round(rng.standard_normal((n, L)) * 8.0) / 8.0).astype(np.float32)
    if kind == 'saturated':        # a sigmoid of large logits: most entries exactly 0 or 1
        x = (rng.standard_normal((n, L)) * 40.0).astype(np.float32)
        return (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)
    if kind == 'constant':
        return np.full((n, L), 0.25, dtype=np.float32)
    ramp = np.arange(L, dtype=np.float32)[None, :] + np.arange(n, dtype=np.float32)[:, None]
    if kind == 'ascending':        # the winners at the very end of the row
        return np.ascontiguousarray(ramp)
    if kind == 'descending':       # ... and at the very start
        return np.ascontiguousarray(-ramp)
    assert kind == 'special'
    s = rng.standard_normal((n, L)).astype(np.float32)
    pool = np.concatenate((_bits([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FC12345]),      # NaNs, payloads and signs
                           np.array([np.inf, -np.inf, 0.0, -0.0], dtype=np.float32),
                           _bits([0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF])))      # denormals
    w = s.view(np.uint32)
    hit = rng.random((n, L)) < 0.3
    w[hit] = pool.view(np.uint32)[rng.integers(0, pool.size, size=int(hit.sum()))]
    for r in (2, 4):               # rows that are entirely NaN
        if r < n:
            w[r, :] = 0x7FC00000
            w[r, ::3] = 0xFFC00001
    return s


def make_targets(n, L, seed=0, density=0.1):
    """float32 0 / 1 (n, L); row 1 has no gold label, row 3 only gold labels (when they exist)."""
    rng = np.random.default_rng(seed * 104729 + L)
    t = (rng.random((n, L)) < density).astype(np.float32)
    if n > 1:
        t[1, :] = 0.0
    if n > 3:
        t[3, :] = 1.0
    return t


def fixture():
    return np.load(os.path.join(GOLDEN, 'rank_at_k.npz'), allow_pickle=False)
