"""The ranking metrics (AUC, AUPR, recall at FDR <= 0.5; utils/evals.py:208-298,316-407) without a GPU: the test-local fp64
restatement against what the reference / sklearn recorded (tests/golden/ranking.npz), the C ABI's new entry points, the host
side of lamp_amd.metrics, the run_eval flag."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

from lamp_amd import _native as N
from lamp_amd import metrics as M

import ranking_common as RC

CASES = ('n1', 'n2', 'n37', 'n300', 'n300sat', 'n257q', 'reuters', 'reutersq', 'degenerate')


def test_fixture_holds_the_cases_the_definitions_need():
    cases = RC.fixture_cases()
    assert sorted(cases) == sorted(CASES)
    assert cases['reuters']['probs'].shape == (3019, 90) and cases['n1']['probs'].shape[0] == 1
    sat = cases['n300sat']['probs'].astype(np.float32)
    assert (sat == 0.0).any() and (sat == 1.0).any()
    q = cases['n257q']['probs'].astype(np.float32)
    assert np.array_equal(q * 8, np.round(q * 8)) and len(np.unique(q)) <= 9
    dg = cases['degenerate']
    assert dg['targets'][:, 1].sum() == 0 and dg['targets'][:, 3].all() and np.isnan(dg['probs'][:, 5]).any()
    # NaN exactly where the rules say: no positives -> all three; all positive -> AUC only; NaN score -> all three
    assert np.isnan(dg['auc'][[1, 3, 5]]).all() and np.isnan(dg['aupr'][[1, 5]]).all() and np.isnan(dg['fdr'][[1, 5]]).all()
    assert np.isfinite(dg['aupr'][3]) and dg['fdr'][3] == 1.0
    assert np.isfinite(dg['auc'][[0, 2, 4, 6]]).all()


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_the_reference_record(name):
    """Pins tests/ranking_common.ranking_ref (which the GPU tests use at full size) to the reference's own compute_metrics /
    sklearn: AUC and FDR recall within 1e-10 (sklearn's fp64 trapezoid accumulates ~ n 2^-53), AUPR within 1e-9."""
    c = RC.fixture_cases()[name]
    p, t = torch.from_numpy(c['probs'].astype(np.float32)), torch.from_numpy(c['targets'].astype(np.float32))
    auc, aupr, fdr, n_pos, n_neg = RC.ranking_ref(p, t)
    assert RC.max_diff(auc, c['auc']) < 1e-10
    assert RC.max_diff(aupr, c['aupr']) < 1e-9
    assert RC.max_diff(fdr, c['fdr']) < 1e-10
    agg = list(RC.finite_stats(auc)) + list(RC.finite_stats(aupr)) + list(RC.finite_stats(fdr))
    assert RC.max_diff(agg[:2], c['agg'][:2]) < 1e-10 and RC.max_diff(agg[2:4], c['agg'][2:4]) < 1e-9
    assert RC.max_diff(agg[4:], c['agg'][4:]) < 1e-10
    rankable = ~np.isnan(c['aupr'])
    assert np.array_equal((n_pos + n_neg)[rankable], np.full(int(rankable.sum()), p.size(0)))


def test_header_and_ctypes_table_carry_the_new_entry_points():
    text = open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read()
    lib = N.lib()
    for name in ('lamp_ranking_metrics_workspace_bytes', 'lamp_ranking_metrics', 'lamp_threshold_counts'):
        assert re.search(r'\b%s\s*\(' % name, re.sub(r'/\*.*?\*/', '', text, flags=re.S)), name
        assert name in N.PROTOTYPES and hasattr(lib, name)
    assert 'utils/evals.py:283-298' in text and ':208-225' in text and ':228-243' in text
    assert lib.lamp_version() == 5          # additive: the ABI version stays


def test_entry_points_validate_before_any_launch():
    lib = N.lib()
    ws = lib.lamp_ranking_metrics_workspace_bytes
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(1 << 31, 1) == 0
    # LDS route: one key buffer; global route (n > 32768): two + the per-(label, digit, chunk) histograms
    small, large = ws(32768, 10), ws(32769, 10)
    assert 32768 * 10 * 4 <= small < 32768 * 10 * 4 + 4096
    assert large >= 2 * 32769 * 10 * 4 + 10 * 256 * 9 * 4
    assert ws(3019, 90) < ws(3020, 90)
    args = (16, 90, 16, 90, 3019, 90, 0.5, 16, 16, 16, None, None)
    assert lib.lamp_ranking_metrics(*args, 16, ws(3019, 90) - 1, None) == -3          # workspace too small: a status code
    assert lib.lamp_ranking_metrics(None, 90, 16, 90, 3019, 90, 0.5, 16, 16, 16, None, None, 16, 1 << 40, None) == -5
    assert lib.lamp_ranking_metrics(16, 89, 16, 90, 3019, 90, 0.5, 16, 16, 16, None, None, 16, 1 << 40, None) == -1   # ld < L
    assert lib.lamp_ranking_metrics(16, 90, 16, 90, 0, 90, 0.5, 16, 16, 16, None, None, 16, 1 << 40, None) == -1
    assert lib.lamp_ranking_metrics(16, 90, 16, 90, 1 << 31, 90, 0.5, 16, 16, 16, None, None, 16, 1 << 40, None) == -4
    assert lib.lamp_threshold_counts(16, 90, 16, 90, 10, 90, 0.5, 16, 16, 16, 16, 16, 16, None, None) == -5
    assert lib.lamp_threshold_counts(16, 90, 16, 80, 10, 90, 0.5, 16, 16, 16, 16, 16, 16, 16, None) == -1


def test_compute_metrics_has_no_cpu_path(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    p, t = RC.make_inputs(8, 3)
    with pytest.raises(RuntimeError, match='HIP device only'):
        M.compute_metrics(p, t, 0.0)
    with pytest.raises(RuntimeError, match='HIP device only'):
        M.ranking_metrics(p, t)
    with pytest.raises(RuntimeError, match='HIP device only'):
        M.threshold_counts(p, t, 0.5)


def test_no_sklearn_under_the_package():
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'lamp_amd')):
        for f in files:
            if f.endswith('.py'):
                assert not re.search(r'^\s*(import|from)\s+sklearn', open(os.path.join(dirpath, f)).read(), flags=re.M), f


def _counts_on_host(pred, target, threshold):
    p = torch.nan_to_num(pred, nan=0.0) >= threshold
    t = target != 0
    lab = torch.stack(((p & t).sum(0), (p & ~t).sum(0), (~p & t).sum(0))).numpy()
    ex = torch.stack(((p & t).sum(1), p.sum(1), t.sum(1), (p != t).sum(1))).numpy()
    return lab, ex


def test_thresholded_figures_from_integer_counts_match_the_reference():
    """The host half of compute_metrics: the five figures from the integer counts the device returns, against the
    reference's own compute_metrics (tests/golden/evals.npz) and run_eval.multilabel_metrics, empty samples / labels included."""
    from lamp_amd.run_eval import multilabel_metrics
    z = np.load(os.path.join(GOLDEN, 'evals.npz'))
    for i in range(int(z['n_cases'])):
        pred, tgt = torch.from_numpy(z['pred_%d' % i]), torch.from_numpy(z['tgt_%d' % i])
        got = M.thresholded_from_counts(*_counts_on_host(pred, tgt, 0.5), pred.size(1))
        ref = multilabel_metrics(pred, tgt, 0.5)
        for k, r, g in zip(('ACC', 'HA', 'ebF1', 'miF1', 'maF1'), z['ref_%d' % i].tolist(), ref.values()):
            assert abs(got[k] - r) < 1e-6 and abs(got[k] - g) < 1e-12, (i, k, got[k], r, g)
    # nothing predicted, nothing gold: the NaN conventions of multilabel_metrics
    got = M.thresholded_from_counts(*_counts_on_host(torch.zeros(3, 2), torch.zeros(3, 2), 0.5), 2)
    assert got['ACC'] == 1.0 and got['HA'] == 1.0 and all(np.isnan(got[k]) for k in ('ebF1', 'miF1', 'maF1'))


def test_aggregates_run_over_the_finite_entries():
    mean, median, var = M.aggregate([0.5, float('nan'), 1.0, 0.75])
    assert (mean, median) == (0.75, 0.75) and abs(var - np.var([0.5, 1.0, 0.75])) < 1e-15
    assert all(np.isnan(v) for v in M.aggregate([float('nan')]))


def test_run_eval_accepts_all_metrics():
    from lamp_amd import run_eval
    assert run_eval.parse(['-data', 'x.pt']).all_metrics is False
    assert run_eval.parse(['-data', 'x.pt', '-all_metrics']).all_metrics is True


def test_test_epoch_takes_device_results():
    import inspect
    from lamp_amd.evaluate import test_epoch
    assert inspect.signature(test_epoch).parameters['device_results'].default is None
