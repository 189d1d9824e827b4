"""The numbers an evaluation reports (reference: utils/evals.py:316-407 compute_metrics), computed on the MI355X.

The reference calls compute_metrics after every test_epoch, on valid and on test, with all_metrics=True: per label column one
roc_auc_score, one precision_recall_curve + auc and a second precision_recall_curve for the recall at FDR <= 0.5 -- three
sklearn sorts of the column on one CPU thread.  Here the prediction matrix stays where evaluate.test_epoch left it: one
key-only segmented sort of all columns and one walk over each sorted column give the three per-label figures
(csrc/metrics.hip: lamp_ranking_metrics), one more pass over the two matrices gives the integer counts behind the five
thresholded figures (lamp_threshold_counts).  The per-label results come back in one copy; the means / medians over L
doubles are taken on the host.

Definitions (include/lamp_hip.h spells them out): today's sklearn without the removed `reorder`
keyword.  Scores are probabilities -- [0, 1] is the contract; a column holding a NaN score, a score outside [0, 1] or a target
other than 0 / 1 is unranked (NaN), as the reference skipped such labels on ValueError.  A label without positives has NaN
AUC / AUPR / FDR recall, one without negatives NaN AUC only; the aggregates run over the finite entries.

Ranking a sample's labels (csrc/rank_at_k.hip) is opt-in beside it: topk_labels gives the k best columns
of every row in the order include/lamp_hip.h defines (a number before a NaN, the larger number first, the lower column on a
tie), rank_at_k and compute_metrics(at_k=...) the precision, nDCG and recall at those ranks from integer hit counts and
fixed-order fp64 sums (lamp_rank_at_k), a sample without a gold label adding 0 as sklearn's ndcg_score(ignore_ties=True) has it.

Fitted decision thresholds (csrc/thresholds.hip) are opt-in too: tune_thresholds walks the same sorted
columns once more and picks, per label, the candidate threshold that is best under F1, Youden's J or the reference's
Find_Optimal_Cutoff balance, compared in integers with ties to the highest threshold (lamp_tune_thresholds); threshold_counts
and compute_metrics(thresholds=...) then take one threshold per label (lamp_threshold_counts_vec).

Label-ranking metrics of whole rows (csrc/rank_at_k.hip) are opt-in as well: label_ranking and
compute_metrics(label_ranking=True) give LRAP, coverage error, ranking loss, one-error and the per-sample AUC from every gold
label's rank among all L labels (lamp_label_ranking: exact integers per row, fixed-order fp64 sums; a tie counts against the
gold label, as sklearn's label_ranking_average_precision_score, coverage_error and label_ranking_loss have it).

There is no CPU path: without a HIP device compute_metrics raises (N.require_device).
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N

RANKING_KEYS = ('meanAUC', 'medianAUC', 'meanAUPR', 'medianAUPR', 'allAUC', 'allAUPR', 'meanFDR', 'medianFDR')


def _matrix(t):
    """fp32 (n, L) device view whose labels are contiguous (a row stride is passed on) -> (tensor, row stride)."""
    if t.dim() != 2:
        raise ValueError('expected an (n, L) matrix, got shape %s' % (tuple(t.shape),))
    if t.dtype != torch.float32:
        t = t.float()
    if t.size(1) > 1 and t.stride(1) != 1 or t.stride(0) < t.size(1):
        t = t.contiguous()
    return t, max(int(t.stride(0)), int(t.size(1)))


def _ranking_buffer(probs, targets, fdr_cutoff):
    """-> float64 (5, L) device buffer: rows auc, aupr, fdr recall, then n_pos and n_neg as int64 bit patterns."""
    N.require_device(probs, targets)
    p, ldp = _matrix(probs)
    t, ldt = _matrix(targets)
    if p.shape != t.shape:
        raise ValueError('predictions %s and targets %s differ in shape' % (tuple(p.shape), tuple(t.shape)))
    n, L = p.shape
    lib = N.lib()
    nbytes = lib.lamp_ranking_metrics_workspace_bytes(n, L)
    if nbytes == 0:
        raise ValueError('ranking metrics: unsupported shape (%d, %d)' % (n, L))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)   # per call: gigabytes at genomics sizes, not worth keeping
    out = torch.empty((5, L), dtype=torch.float64, device=p.device)
    counts = out[3:].view(torch.int64)
    N.check(lib.lamp_ranking_metrics(N.ptr(p), ldp, N.ptr(t), ldt, n, L, float(fdr_cutoff), N.ptr(out[0]), N.ptr(out[1]),
                                     N.ptr(out[2]), N.ptr(counts[0]), N.ptr(counts[1]), N.ptr(ws), nbytes, N.stream()),
            'lamp_ranking_metrics')
    return out


def ranking_metrics(probs, targets, fdr_cutoff=0.5):
    """Per-label (auc, aupr, fdr_recall, n_pos, n_neg) of (n, L) device matrices: float64 / int64 tensors of length L on the
    device (views of one buffer), nothing synchronised."""
    out = _ranking_buffer(probs, targets, fdr_cutoff)
    counts = out[3:].view(torch.int64)
    return out[0], out[1], out[2], counts[0], counts[1]


def _threshold_vector(thresholds, L, device):
    """A length-L tensor of thresholds -> contiguous float32 on `device` (uploaded when it is a host tensor)."""
    thr = thresholds.detach().to(device=device, dtype=torch.float32).contiguous()
    if thr.dim() != 1 or thr.numel() != L:
        raise ValueError('thresholds: expected a tensor of length %d, got shape %s' % (L, tuple(thresholds.shape)))
    return thr


def _counts_buffer(probs, targets, threshold):
    """-> int32 device buffer: the (3, L) label counts, then the (4, n) sample counts.  `threshold`: a python float, or a
    float32 tensor of length L (one threshold per label)."""
    N.require_device(probs, targets)
    p, ldp = _matrix(probs)
    t, ldt = _matrix(targets)
    if p.shape != t.shape:
        raise ValueError('predictions %s and targets %s differ in shape' % (tuple(p.shape), tuple(t.shape)))
    n, L = p.shape
    buf = torch.empty(3 * L + 4 * n, dtype=torch.int32, device=p.device)
    lab, ex = buf[:3 * L].view(3, L), buf[3 * L:].view(4, n)
    if torch.is_tensor(threshold):
        thr = _threshold_vector(threshold, L, p.device)
        N.check(N.lib().lamp_threshold_counts_vec(N.ptr(p), ldp, N.ptr(t), ldt, n, L, N.ptr(thr), N.ptr(lab[0]), N.ptr(lab[1]),
                                                  N.ptr(lab[2]), N.ptr(ex[0]), N.ptr(ex[1]), N.ptr(ex[2]), N.ptr(ex[3]),
                                                  N.stream()), 'lamp_threshold_counts_vec')
        return buf
    N.check(N.lib().lamp_threshold_counts(N.ptr(p), ldp, N.ptr(t), ldt, n, L, float(threshold), N.ptr(lab[0]), N.ptr(lab[1]),
                                          N.ptr(lab[2]), N.ptr(ex[0]), N.ptr(ex[1]), N.ptr(ex[2]), N.ptr(ex[3]), N.stream()),
            'lamp_threshold_counts')
    return buf


def threshold_counts(probs, targets, threshold):
    """-> (label counts int32 (3, L): tp, fp, fn;  sample counts int32 (4, n): tp, predicted, gold, mismatches) on the device.
    `threshold` is a python float for all labels or a float32 tensor of length L."""
    n, L = probs.shape
    buf = _counts_buffer(probs, targets, threshold)
    return buf[:3 * L].view(3, L), buf[3 * L:].view(4, n)


def thresholded_from_counts(lab, ex, n_labels):
    """The five thresholded figures from the integer counts (numpy int arrays (3, L) and (4, n)), with the conventions of
    run_eval.multilabel_metrics: example-based F1 over samples with a gold or a predicted label, macro-F1 over labels with
    tp + fp + fn > 0, NaN where nothing is left."""
    lab, ex = lab.astype(np.int64), ex.astype(np.int64)
    tp, fp, fn = lab
    ex_tp, ex_pred, ex_gold, ex_mis = ex
    n = ex.shape[1]
    nan = float('nan')
    ex_den = ex_pred + ex_gold
    ex_ok = ex_den > 0
    lab_den = 2 * tp + fp + fn
    lab_ok = lab_den > 0
    return {
        'ACC': float(np.count_nonzero(ex_mis == 0)) / n,
        'HA': float(n * n_labels - int(ex_mis.sum())) / float(n * n_labels),
        'ebF1': float(np.mean(2.0 * ex_tp[ex_ok] / ex_den[ex_ok])) if ex_ok.any() else nan,
        'miF1': 2.0 * float(tp.sum()) / float(lab_den.sum()) if lab_den.sum() > 0 else nan,
        'maF1': float(np.mean(2.0 * tp[lab_ok] / lab_den[lab_ok])) if lab_ok.any() else nan,
    }


def aggregate(values):
    """(mean, median, variance) over the finite entries, as compute_auc / compute_aupr / compute_fdr take them over the labels
    they did not skip (utils/evals.py:294-297); NaN when no label could be ranked."""
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    if v.size == 0:
        return float('nan'), float('nan'), float('nan')
    return float(np.mean(v)), float(np.median(v)), float(np.var(v))


TUNE_CRITERIA = {'f1': 0, 'youden': 1, 'balance': 2}   # include/lamp_hip.h: enum lamp_tune_criterion


def tune_thresholds(probs, targets, criterion='f1', fallback=0.5, scope='label'):
    """The decision threshold per label that is best under `criterion` on these rows (include/lamp_hip.h: lamp_tune_thresholds;
    'f1', 'youden' = tpr - fpr, 'balance' = the reference's Find_Optimal_Cutoff quantity |tpr - (1 - fpr)|; ties to the highest
    threshold).  -> a dict of device tensors of length L: 'threshold' float32 (+inf: predict nothing), 'tp', 'fp', 'n_pos',
    'n_neg' int32 (the counts at the chosen threshold and the column's positives / negatives) and 'tuned' bool (False for a
    column that cannot be ranked: its threshold is `fallback`, its counts 0).  Nothing is synchronised.
    scope='global' tunes ONE threshold on the flattened matrix (under 'f1' the micro-F1-optimal cutoff; n L < 2^31): every
    entry of the result is that single column's, broadcast to length L."""
    if criterion not in TUNE_CRITERIA:
        raise ValueError("criterion must be one of 'f1', 'youden', 'balance'; got %r" % (criterion,))
    if scope not in ('label', 'global'):
        raise ValueError("scope must be 'label' or 'global'; got %r" % (scope,))
    N.require_device(probs, targets)
    p, ldp = _matrix(probs)
    t, ldt = _matrix(targets)
    if p.shape != t.shape:
        raise ValueError('predictions %s and targets %s differ in shape' % (tuple(p.shape), tuple(t.shape)))
    n_labels = p.size(1)
    if scope == 'global':
        if p.numel() >= 1 << 31:
            raise ValueError("tune_thresholds(scope='global'): n L = %d is not below 2^31" % p.numel())
        p, t = p.contiguous().view(-1, 1), t.contiguous().view(-1, 1)
        ldp = ldt = 1
    n, L = p.shape
    lib = N.lib()
    nbytes = lib.lamp_tune_thresholds_workspace_bytes(n, L)
    if nbytes == 0:
        raise ValueError('tune_thresholds: unsupported shape (%d, %d)' % (n, L))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    out = torch.empty((6, L), dtype=torch.int32, device=p.device)   # row 0 holds the float32 thresholds
    thr = out[0].view(torch.float32)
    N.check(lib.lamp_tune_thresholds(N.ptr(p), ldp, N.ptr(t), ldt, n, L, TUNE_CRITERIA[criterion], float(fallback), N.ptr(thr),
                                     N.ptr(out[1]), N.ptr(out[2]), N.ptr(out[3]), N.ptr(out[4]), N.ptr(out[5]), N.ptr(ws), nbytes,
                                     N.stream()), 'lamp_tune_thresholds')
    res = {'threshold': thr, 'tp': out[1], 'fp': out[2], 'n_pos': out[3], 'n_neg': out[4], 'tuned': out[5] != 0}
    if scope == 'global':
        res = {k: v.expand(n_labels) for k, v in res.items()}
    return res


def tuned_values(result, criterion):
    """The criterion's value at the chosen threshold of every label, in fp64 from the integers of a tune_thresholds result
    (copied to the host here): 'f1' 2 tp / (tp + fp + n_pos), 'youden' tp / n_pos - fp / n_neg, 'balance'
    |tp / n_pos - (1 - fp / n_neg)|, each as ONE division of exact integers.  NaN where the value is undefined: a label that
    was not tuned, 'f1' with nothing predicted and no positive, 'youden' / 'balance' without a positive or without a negative."""
    if criterion not in TUNE_CRITERIA:
        raise ValueError("criterion must be one of 'f1', 'youden', 'balance'; got %r" % (criterion,))
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in result.items()}
    out = np.full(len(host['tp']), np.nan, dtype=np.float64)
    for l in range(len(out)):
        if not host['tuned'][l]:
            continue
        tp, fp, P, Nn = (int(host[k][l]) for k in ('tp', 'fp', 'n_pos', 'n_neg'))
        if criterion == 'f1':
            num, den = 2 * tp, tp + fp + P
        elif criterion == 'youden':
            num, den = tp * Nn - fp * P, P * Nn
        else:
            num, den = abs(tp * Nn + fp * P - P * Nn), P * Nn
        if den > 0:
            out[l] = num / den
    return out


TOPK_MAX_K, TOPK_MAX_L = 64, 32768   # include/lamp_hip.h: lamp_topk_labels


def topk_labels(scores, k, values=True):
    """The k first-ranked columns of every row of an (n, L) device matrix, in the order include/lamp_hip.h defines (a number
    before a NaN, the larger number first, the lower column on a tie) -> (int32 (n, k) columns, float32 (n, k) selected scores
    or None) on the device, nothing synchronised.  1 <= k <= min(L, 64), L <= 32768."""
    N.require_device(scores)
    s, ld = _matrix(scores)
    n, L = s.shape
    k = int(k)
    idx = torch.empty((n, k), dtype=torch.int32, device=s.device)
    val = torch.empty((n, k), dtype=torch.float32, device=s.device) if values else None
    N.check(N.lib().lamp_topk_labels(N.ptr(s), ld, n, L, k, N.ptr(idx), k, N.ptr(val), k, N.stream()), 'lamp_topk_labels')
    return idx, val


def dcg_tables(k):
    """(discount, ideal) of lamp_rank_at_k in fp64: discount[r] = 1 / log2(r + 2), ideal[m] = the sum of the first m."""
    d = 1.0 / np.log2(np.arange(k, dtype=np.float64) + 2.0)
    ideal = np.concatenate(([0.0], np.cumsum(d)))
    return d, ideal


def _rank_at_k_buffer(scores, targets, k):
    """-> float64 (3 k + 1) device buffer: ndcg_sum, recall_sum, then hits_at_rank and n_with_gold as int64 bit patterns."""
    N.require_device(scores, targets)
    t, ldt = _matrix(targets)
    if tuple(scores.shape) != tuple(t.shape):
        raise ValueError('scores %s and targets %s differ in shape' % (tuple(scores.shape), tuple(t.shape)))
    n, L = t.shape
    idx, _ = topk_labels(scores, k, values=False)
    lib = N.lib()
    nbytes = lib.lamp_rank_at_k_workspace_bytes(n, k)
    if nbytes == 0:
        raise ValueError('rank at k: unsupported request (n = %d, k = %d)' % (n, k))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
    out = torch.empty(3 * k + 1, dtype=torch.float64, device=t.device)
    ints = out[2 * k:].view(torch.int64)
    d, ideal = dcg_tables(k)
    N.check(lib.lamp_rank_at_k(N.ptr(idx), k, N.ptr(t), ldt, n, L, k, d.ctypes.data_as(C.POINTER(C.c_double)),
                               ideal.ctypes.data_as(C.POINTER(C.c_double)), N.ptr(ints[:k]), N.ptr(out[:k]), N.ptr(out[k:2 * k]),
                               N.ptr(ints[k:]), N.ptr(ws), nbytes, N.stream()), 'lamp_rank_at_k')
    return out


def _check_ks(ks, L):
    ks = tuple(int(k) for k in ks)
    if not ks or min(ks) < 1 or max(ks) > min(L, TOPK_MAX_K):
        raise ValueError('rank at k: every k must lie in 1 .. min(L, %d); got %s with L = %d' % (TOPK_MAX_K, ks, L))
    return ks


def rank_at_k_from_sums(buf, n, k, ks):
    """The figures of rank_at_k from the host copy of _rank_at_k_buffer."""
    ints = buf[2 * k:].view(np.int64)
    out = {}
    for j in ks:
        out['P@%d' % j] = float(int(ints[:j].sum())) / float(n * j)
        out['nDCG@%d' % j] = float(buf[j - 1]) / n
        out['R@%d' % j] = float(buf[k + j - 1]) / n
    out['n_with_gold'] = int(ints[k])
    return out


def rank_at_k(scores, targets, ks=(1, 3, 5)):
    """Precision, nDCG and recall at k of (n, L) device matrices, each sample's labels ranked by topk_labels: a dict with
    'P@k', 'nDCG@k' and 'R@k' for every requested k (means over all n samples; a sample without a gold label adds 0, as
    sklearn's ndcg_score(ignore_ties=True) has it) and 'n_with_gold'.  A gold label is a nonzero target.  The scores may be
    logits or probabilities; the figures come back in one copy."""
    ks = _check_ks(ks, scores.size(1))
    k = max(ks)
    buf = _rank_at_k_buffer(scores, targets, k).cpu().numpy()
    return rank_at_k_from_sums(buf, scores.size(0), k, ks)


LABEL_RANKING_KEYS = ('LRAP', 'coverage_error', 'ranking_loss', 'one_error', 'instance_AUC', 'n_with_gold', 'n_with_both',
                      'n_rows_with_nan')
LABEL_RANKING_ROW_COUNTS = ('n_pos', 'coverage', 'misordered', 'tied', 'top1_hit', 'has_nan')   # columns of row_counts


def _label_ranking_buffer(scores, targets, rows=False):
    """-> (float64 (8) device buffer: lrap_sum, rloss_sum, auc_sum, then coverage_sum, top1_hits, n_with_gold, n_with_both and
    n_rows_with_nan as int64 bit patterns; row_counts int32 (n, 6) and row_lrap float64 (n) when `rows`, else None, None)."""
    N.require_device(scores, targets)
    s, lds = _matrix(scores)
    t, ldt = _matrix(targets)
    if s.shape != t.shape:
        raise ValueError('scores %s and targets %s differ in shape' % (tuple(s.shape), tuple(t.shape)))
    n, L = s.shape
    lib = N.lib()
    nbytes = lib.lamp_label_ranking_workspace_bytes(n, L)
    if nbytes == 0:
        raise ValueError('label ranking: unsupported shape (%d, %d); L <= %d' % (n, L, TOPK_MAX_L))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
    out = torch.empty(8, dtype=torch.float64, device=s.device)
    row_counts = torch.empty((n, 6), dtype=torch.int32, device=s.device) if rows else None
    row_lrap = torch.empty(n, dtype=torch.float64, device=s.device) if rows else None
    N.check(lib.lamp_label_ranking(N.ptr(s), lds, N.ptr(t), ldt, n, L, N.ptr(out[:3]), N.ptr(out[3:].view(torch.int64)),
                                   N.ptr(row_counts), N.ptr(row_lrap), N.ptr(ws), nbytes, N.stream()), 'lamp_label_ranking')
    return out, row_counts, row_lrap


def label_ranking_from_sums(buf, n):
    """The figures of label_ranking from the host copy of _label_ranking_buffer's first result and the number of rows."""
    buf = np.ascontiguousarray(buf, dtype=np.float64)
    coverage, top1, with_gold, with_both, with_nan = (int(v) for v in buf[3:].view(np.int64))
    return {
        'LRAP': float(buf[0]) / n,
        'coverage_error': float(coverage) / n,
        'ranking_loss': float(buf[1]) / n,
        'one_error': 1.0 - float(top1) / n,
        'instance_AUC': float(buf[2]) / with_both if with_both > 0 else float('nan'),
        'n_with_gold': with_gold,
        'n_with_both': with_both,
        'n_rows_with_nan': with_nan,
    }


def label_ranking(scores, targets):
    """Label-ranking metrics of (n, L) device matrices, from every gold label's rank among all L labels of its row
    (include/lamp_hip.h: lamp_label_ranking): a dict with 'LRAP', 'coverage_error' and 'ranking_loss' (sklearn's
    label_ranking_average_precision_score, coverage_error and label_ranking_loss: a tie counts against the gold label, a row
    without a gold label has LRAP 1, coverage 0 and loss 0), 'one_error' (1 - P@1 of rank_at_k), 'instance_AUC' (the mean
    roc_auc_score of the rows that hold both classes; NaN when there is none), 'n_with_gold', 'n_with_both' and
    'n_rows_with_nan'.  A gold label is a nonzero target; NaN scores rank lowest.  The figures describe the matrix given:
    probabilities that saturate to exactly 0 or 1 tie where their logits did not.  One copy back."""
    buf, _, _ = _label_ranking_buffer(scores, targets)
    return label_ranking_from_sums(buf.cpu().numpy(), scores.size(0))


def label_ranking_rows(scores, targets):
    """The per-row results of lamp_label_ranking -> (row_counts int32 (n, 6): n_pos, coverage, misordered, tied, top1_hit,
    has_nan; row_lrap float64 (n,)) on the device, nothing synchronised."""
    _, row_counts, row_lrap = _label_ranking_buffer(scores, targets, rows=True)
    return row_counts, row_lrap


def compute_metrics(all_predictions, all_targets, loss, br_threshold=0.5, elapsed=0.0, all_metrics=True, device=None,
                    fdr_cutoff=0.5, at_k=None, thresholds=None, label_ranking=False):
    """utils/evals.py:316-407 for the binary-relevance decoders: a dict with the reference's keys -- ACC, HA, ebF1, miF1, maF1,
    meanAUC, medianAUC, meanAUPR, medianAUPR, allAUC, allAUPR, meanFDR, medianFDR, loss, time.  allAUC / allAUPR are float64
    arrays of length L (NaN for a label that cannot be ranked); all_metrics=False gives 0 for the ranking entries, as the
    reference does.  (n, L) tensors of probabilities in [0, 1] and 0 / 1 targets, on the CPU (uploaded once, to `device` or the
    current HIP device) or on the device; the inputs are not modified.  at_k=(1, 3, 5) adds the keys of rank_at_k for those k
    (P@k, nDCG@k, R@k, n_with_gold); with the default the dict is what it was.  thresholds = a float32 tensor of length L (as
    tune_thresholds fitted it, on another split) makes the five thresholded figures use one threshold per label instead of
    br_threshold; with None not one more launch happens.  label_ranking=True adds the keys of label_ranking (LRAP,
    coverage_error, ranking_loss, one_error, instance_AUC, n_with_gold, n_with_both, n_rows_with_nan) of the predictions as
    given; with the default there is not one more launch, key or copy."""
    if not all_predictions.is_cuda:
        if not torch.cuda.is_available():
            N.require_device(all_predictions)      # raises: HIP device only
        device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        all_predictions = all_predictions.to(device)
    if not all_targets.is_cuda:
        all_targets = all_targets.to(all_predictions.device)
    with torch.cuda.device(all_predictions.device):
        n, L = all_predictions.shape
        counts_d = _counts_buffer(all_predictions, all_targets, br_threshold if thresholds is None else
                                   torch.as_tensor(thresholds, dtype=torch.float32))
        ranked_d = _ranking_buffer(all_predictions, all_targets, fdr_cutoff) if all_metrics else None
        if at_k is not None:
            ks = _check_ks(at_k, L)
            at_k_d = _rank_at_k_buffer(all_predictions, all_targets, max(ks))
        if label_ranking:
            label_ranking_d = _label_ranking_buffer(all_predictions, all_targets)[0]
        counts = counts_d.cpu().numpy()
        out = thresholded_from_counts(counts[:3 * L].reshape(3, L), counts[3 * L:].reshape(4, n), L)
        if all_metrics:
            per_label = ranked_d.cpu().numpy()    # auc, aupr, fdr recall (and the two count rows): one copy
            auc, aupr, fdr = per_label[0].copy(), per_label[1].copy(), per_label[2].copy()
            out['meanAUC'], out['medianAUC'], _ = aggregate(auc)
            out['meanAUPR'], out['medianAUPR'], _ = aggregate(aupr)
            out['allAUC'], out['allAUPR'] = auc, aupr
            out['meanFDR'], out['medianFDR'], _ = aggregate(fdr)
        else:
            for k in RANKING_KEYS:
                out[k] = 0
        if at_k is not None:
            out.update(rank_at_k_from_sums(at_k_d.cpu().numpy(), n, max(ks), ks))
        if label_ranking:
            out.update(label_ranking_from_sums(label_ranking_d.cpu().numpy(), n))
    out['loss'] = loss
    out['time'] = elapsed
    return out
