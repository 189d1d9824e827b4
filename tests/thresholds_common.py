"""Shared by test_tune_thresholds_cpu.py and test_tune_thresholds_gpu.py: a brute-force numpy / python-integer restatement of
the definition of lamp_tune_thresholds in include/lamp_hip.h (enumerate the candidates c = 0..G, compare with python integers,
break ties towards the highest threshold), the counts at a threshold vector, and the input generators.  Nothing here imports
the code under test."""
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CRITERIA = ('f1', 'youden', 'balance')
CRITERION_ID = {'f1': 0, 'youden': 1, 'balance': 2}
FAMILIES = ('tiefree', 'ties7', 'constant', 'separable', 'nopos', 'noneg', 'unrankable')
INF_BITS = 0x7F800000
TIE_VALUES = np.array([0.0, 0.125, 0.3, 0.5, 0.75, 0.9, 1.0], dtype=np.float32)


def rankable(scores, targets):
    """The rule of lamp_ranking_metrics for one column: every score a number in [0, 1], every target 0 or 1."""
    s, t = np.asarray(scores, dtype=np.float32), np.asarray(targets, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        return bool(np.all((s >= 0.0) & (s <= 1.0)) and np.all((t == 0.0) | (t == 1.0)))


def candidates(scores, targets):
    """One rankable column -> (bits, tp, cnt): python lists over the candidates c = 0..G.  bits[c] is the threshold's bit
    pattern (+inf for c = 0; the group's score with -0.0 read as +0.0 otherwise), tp[c] / cnt[c] the positives / rows at or
    above it."""
    s = (np.asarray(scores, dtype=np.float32) + np.float32(0.0)).astype(np.float32)     # -0.0 -> +0.0
    t = np.asarray(targets, dtype=np.float32) == 1.0
    order = np.argsort(-s.astype(np.float64), kind='stable')
    s, t = s[order], t[order]
    ends = np.nonzero(np.append(s[1:] != s[:-1], True))[0]                                # last row of every group
    ctp = np.cumsum(t.astype(np.int64))
    bits = [INF_BITS] + s.view(np.uint32)[ends].tolist()
    tp = [0] + ctp[ends].tolist()
    cnt = [0] + (ends + 1).tolist()
    return bits, tp, cnt


def better(criterion, tp_a, cnt_a, tp_b, cnt_b, P, N):
    """Candidate a strictly beats b, in python integers."""
    if criterion == 'f1':
        return tp_a * (cnt_b + P) > tp_b * (cnt_a + P)
    fp_a, fp_b = cnt_a - tp_a, cnt_b - tp_b
    if criterion == 'youden':
        return tp_a * N - fp_a * P > tp_b * N - fp_b * P
    assert criterion == 'balance'
    return abs(tp_a * N + fp_a * P - P * N) < abs(tp_b * N + fp_b * P - P * N)


def choose(criterion, tp, cnt):
    """The chosen candidate: the smallest c no other candidate beats."""
    P, N = tp[-1], cnt[-1] - tp[-1]
    best = 0
    for c in range(1, len(tp)):
        if better(criterion, tp[c], cnt[c], tp[best], cnt[best], P, N):
            best = c
    return best


def tune_column_ref(scores, targets, criterion, fallback=0.5):
    """-> (threshold bits, tp, fp, n_pos, n_neg, tuned) of one column."""
    if not rankable(scores, targets):
        return int(np.array([fallback], dtype=np.float32).view(np.uint32)[0]), 0, 0, 0, 0, 0
    bits, tp, cnt = candidates(scores, targets)
    c = choose(criterion, tp, cnt)
    return bits[c], tp[c], cnt[c] - tp[c], tp[-1], cnt[-1] - tp[-1], 1


def tune_ref(scores, targets, criterion, fallback=0.5):
    """(n, L) matrices -> dict of arrays of length L: 'threshold' as uint32 bit patterns, 'tp', 'fp', 'n_pos', 'n_neg' int32,
    'tuned' bool."""
    scores, targets = np.asarray(scores, dtype=np.float32), np.asarray(targets, dtype=np.float32)
    rows = [tune_column_ref(scores[:, l], targets[:, l], criterion, fallback) for l in range(scores.shape[1])]
    cols = list(zip(*rows))
    out = {'threshold': np.asarray(cols[0], dtype=np.uint32)}
    for i, k in enumerate(('tp', 'fp', 'n_pos', 'n_neg')):
        out[k] = np.asarray(cols[i + 1], dtype=np.int32)
    out['tuned'] = np.asarray(cols[5], dtype=bool)
    return out


def value_ref(criterion, tp, fp, P, N):
    """The criterion's value in fp64, one division of exact integers; NaN where it is undefined."""
    tp, fp, P, N = int(tp), int(fp), int(P), int(N)
    if criterion == 'f1':
        num, den = 2 * tp, tp + fp + P
    elif criterion == 'youden':
        num, den = tp * N - fp * P, P * N
    else:
        num, den = abs(tp * N + fp * P - P * N), P * N
    return num / den if den > 0 else float('nan')


def f1_fraction(tp, fp, P):
    den = tp + fp + P
    return Fraction(2 * tp, den) if den > 0 else Fraction(0)


def counts_ref(scores, targets, thresholds):
    """The seven outputs of lamp_threshold_counts(_vec): prediction = (score, NaN read as 0) >= threshold (a float or a vector
    of length L), gold = target != 0.  -> (label (3, L) int32: tp, fp, fn;  sample (4, n) int32: tp, predicted, gold, mismatch)."""
    s = np.asarray(scores, dtype=np.float32)
    s = np.where(np.isnan(s), np.float32(0.0), s)
    thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float32), (s.shape[1],))
    with np.errstate(invalid='ignore'):
        pred = s >= thr[None, :]
    gold = np.asarray(targets) != 0
    lab = np.stack(((pred & gold).sum(0), (pred & ~gold).sum(0), (~pred & gold).sum(0))).astype(np.int32)
    ex = np.stack(((pred & gold).sum(1), pred.sum(1), gold.sum(1), (pred != gold).sum(1))).astype(np.int32)
    return lab, ex


def make_column(family, n, rng):
    """(scores float32 (n,), targets float32 (n,)) of one family; scores in [0, 1] except the unrankable column's one NaN."""
    if family == 'tiefree':
        s = ((rng.permutation(n) + 1.0) / (n + 1.0)).astype(np.float32)
        assert len(np.unique(s)) == n
        t = rng.random(n) < s
    elif family == 'ties7':      # groups straddle thread, wave and tile boundaries
        s = TIE_VALUES[rng.integers(0, 7, size=n)]
        t = rng.random(n) < 0.15 + 0.6 * s
    elif family == 'constant':
        s = np.full(n, 0.25, dtype=np.float32)
        t = rng.random(n) < 0.3
    elif family == 'separable':  # every positive above every negative
        t = rng.random(n) < 0.2
        u = ((rng.permutation(n) + 1.0) / (2.0 * n + 2.0)).astype(np.float32)
        s = np.where(t, u + np.float32(0.5), u).astype(np.float32)
    elif family == 'nopos':
        s = rng.random(n).astype(np.float32)
        t = np.zeros(n, dtype=bool)
    elif family == 'noneg':
        s = rng.random(n).astype(np.float32)
        t = np.ones(n, dtype=bool)
    else:
        assert family == 'unrankable'
        s = rng.random(n).astype(np.float32)
        t = rng.random(n) < 0.3
        s[int(rng.integers(0, n))] = np.float32('nan')
    return s, t.astype(np.float32)


def make_case(n, L, seed=0, family=None):
    """(scores, targets) float32 (n, L).  family=None: column l is of family FAMILIES[(l + n) % 7], so every shape with L >= 7
    holds all of them, an unrankable column among rankable ones included."""
    rng = np.random.default_rng(seed * 1000003 + n * 131 + L)
    s, t = np.empty((n, L), dtype=np.float32), np.empty((n, L), dtype=np.float32)
    for l in range(L):
        s[:, l], t[:, l] = make_column(family or FAMILIES[(l + n) % len(FAMILIES)], n, rng)
    return s, t


def fixture():
    return np.load(os.path.join(GOLDEN, 'thresholds.npz'), allow_pickle=False)
