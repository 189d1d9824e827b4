"""Shared by test_label_ranking_cpu.py and test_label_ranking_gpu.py: a numpy restatement of the label-ranking metrics that
include/lamp_hip.h defines (lamp_label_ranking), sort-based so that L = 32768 is instant, a brute-force O(L^2) pair count in
float semantics that checks the restatement on small rows, and the input generators.  Nothing here imports the code under
test."""
import os

import numpy as np

import rank_at_k_common as RK

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KINDS = ('normal', 'quantised', 'saturated', 'constant', 'special')
ROW_COUNTS = ('n_pos', 'coverage', 'misordered', 'tied', 'top1_hit', 'has_nan')
U = 2.0 ** -52


def keys_ref(scores):
    """float32 (..., L) -> uint32 keys that order as the row ordering does: +0.0 and -0.0 share a key, every NaN shares one
    key below that of -inf, denormals stay distinct.  Integer arithmetic only."""
    bits = np.ascontiguousarray(np.asarray(scores, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    mag = bits & 0x7FFFFFFF
    neg = (bits >> 31) == 1
    key = np.where(neg, 0xFFFFFFFF - bits, bits | 0x80000000)
    key = np.where(mag == 0, 0x80000000, key)
    key = np.where(mag > 0x7F800000, 1, key)
    return key.astype(np.uint32)


def row_ref(scores, targets, strict=False):
    """One row -> (six integers in the order of ROW_COUNTS, lrap, rloss, auc or None).  strict=True is the MUTANT that counts
    s_j > s_p where the definition counts s_j >= s_p (kept for the test that shows the tie rule is tested)."""
    s = np.asarray(scores, dtype=np.float32)
    L = s.shape[0]
    key = keys_ref(s).astype(np.int64)
    gold = np.asarray(targets) != 0
    n_p = int(gold.sum())
    n_n = L - n_p
    side = 'right' if strict else 'left'
    kp = key[gold]                                              # column order
    rank = L - np.searchsorted(np.sort(key), kp, side)
    pos = n_p - np.searchsorted(np.sort(kp), kp, side)
    other = np.sort(key[~gold])
    tied = int((np.searchsorted(other, kp, 'right') - np.searchsorted(other, kp, 'left')).sum())
    if strict:
        rank, pos = rank + 1, pos + 1                           # p itself
    coverage = int(rank.max()) if n_p else 0
    misordered = int((rank - pos).sum())
    top1 = int(gold[int(np.argmax(key))])                       # the first maximum: the lowest column of a tie
    has_nan = int(np.isnan(s).any())
    quot = pos.astype(np.float64) / rank.astype(np.float64)
    lrap = float(np.cumsum(quot)[-1]) / n_p if n_p else 1.0     # cumsum: a sequential fp64 sum in column order
    pairs = n_p * n_n
    rloss = misordered / pairs if pairs else 0.0
    auc = 1.0 - (misordered - tied / 2) / pairs if pairs else None
    return (n_p, coverage, misordered, tied, top1, has_nan), lrap, rloss, auc


def rows_ref(scores, targets, strict=False):
    """(n, L) -> (int64 (n, 6), lrap float64 (n,), rloss float64 (n,), auc float64 (n,) with NaN where undefined)."""
    n = len(scores)
    ints, lrap, rloss, auc = np.zeros((n, 6), np.int64), np.zeros(n), np.zeros(n), np.full(n, np.nan)
    for i in range(n):
        ints[i], lrap[i], rloss[i], a = row_ref(scores[i], targets[i], strict)
        if a is not None:
            auc[i] = a
    return ints, lrap, rloss, auc


def sums_ref(ints, lrap, rloss, auc):
    """-> (float64 [3] lrap_sum, rloss_sum, auc_sum; int64 [5] coverage_sum, top1_hits, n_with_gold, n_with_both,
    n_rows_with_nan), the fp64 sums sequential in row order."""
    both = np.isfinite(auc)
    sums = np.array([np.cumsum(lrap)[-1], np.cumsum(rloss)[-1], np.cumsum(np.where(both, auc, 0.0))[-1]])
    counts = np.array([ints[:, 1].sum(), ints[:, 4].sum(), (ints[:, 0] > 0).sum(), both.sum(), ints[:, 5].sum()], dtype=np.int64)
    return sums, counts


def figures_ref(scores, targets):
    """The dict metrics.label_ranking returns, from the restatement."""
    ints, lrap, rloss, auc = rows_ref(scores, targets)
    sums, counts = sums_ref(ints, lrap, rloss, auc)
    n = len(scores)
    return {
        'LRAP': float(sums[0]) / n,
        'coverage_error': float(counts[0]) / n,
        'ranking_loss': float(sums[1]) / n,
        'one_error': 1.0 - float(counts[1]) / n,
        'instance_AUC': float(sums[2]) / int(counts[3]) if counts[3] > 0 else float('nan'),
        'n_with_gold': int(counts[2]),
        'n_with_both': int(counts[3]),
        'n_rows_with_nan': int(counts[4]),
    }


def at_or_above(a, b):
    """a >= b in the row ordering, from FLOAT comparisons (no keys): everything is at or above a NaN, a NaN is at or above
    NaNs only, numbers compare as floats (+0.0 == -0.0)."""
    if np.isnan(b):
        return True
    if np.isnan(a):
        return False
    return bool(a >= b)


def brute_row(scores, targets):
    """The six integers and lrap of one row by counting pairs, O(L^2): the check of row_ref on small rows."""
    s = np.asarray(scores, dtype=np.float32)
    L = len(s)
    gold = [bool(t != 0) for t in targets]
    n_p = sum(gold)
    coverage = misordered = tied = 0
    quot = 0.0
    for p in range(L):
        if not gold[p]:
            continue
        rank = sum(at_or_above(s[j], s[p]) for j in range(L))
        pos = sum(at_or_above(s[j], s[p]) for j in range(L) if gold[j])
        tied += sum(at_or_above(s[j], s[p]) and at_or_above(s[p], s[j]) for j in range(L) if not gold[j])
        coverage = max(coverage, rank)
        misordered += rank - pos
        quot += pos / rank
    first = 0
    for j in range(1, L):                      # strictly above only: the lowest column of a tie stays
        if not at_or_above(s[first], s[j]):
            first = j
    has_nan = int(any(np.isnan(v) for v in s))
    return (n_p, coverage, misordered, tied, int(gold[first]), has_nan), (quot / n_p if n_p else 1.0)


def make_scores(kind, n, L, seed=0):
    assert kind in KINDS
    return RK.make_scores(kind, n, L, seed)


def make_targets(n, L, seed=0, density=0.1):
    """rank_at_k_common.make_targets (row 1 empty, row 3 full) with more patterns: row 0 half positive (ceil(L / 2) random
    columns), row 2 a single positive in the first column, row 4 a single positive in the last column."""
    t = RK.make_targets(n, L, seed, density)
    rng = np.random.default_rng(seed * 65537 + L + 1)
    t[0, :] = 0.0
    t[0, rng.permutation(L)[:(L + 1) // 2]] = 1.0
    if n > 2:
        t[2, :] = 0.0
        t[2, 0] = 1.0
    if n > 4:
        t[4, :] = 0.0
        t[4, L - 1] = 1.0
    return t


def rows_with_a_tie(scores, targets):
    """bool (n,): rows in which some gold label shares its key with a label that is not gold."""
    ints = rows_ref(scores, targets)[0]
    return ints[:, 3] > 0


def fixture():
    return np.load(os.path.join(GOLDEN, 'label_ranking.npz'), allow_pickle=False)
