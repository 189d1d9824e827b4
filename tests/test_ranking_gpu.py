"""The ranking metrics and thresholded counts on the MI355X (csrc/metrics.hip), through the C ABI and through
lamp_amd.metrics.compute_metrics.

Tolerances come from the definitions, not from the code under test:
  * AUC and FDR recall have integer numerators and one fp64 division: bit-equal to the restatement (tests/ranking_common.py),
    within 1e-10 of the sklearn fixtures (sklearn's own fp64 trapezoid accumulates about n 2^-53);
  * AUPR is a sum of <= 5e5 fp64 terms bounded by 1 (4 n 2^-53 ~ 2e-10): within 1e-9 of both;
  * thresholded counts are integers: equal; the five ratios within 1e-12 of run_eval.multilabel_metrics.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

from lamp_amd import _native as N
from lamp_amd import metrics as M
from lamp_amd.run_eval import multilabel_metrics

import ranking_common as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def gpu_ranking(p, t, dev, cutoff=0.5):
    """-> five numpy arrays of the device result for cpu (or device) inputs."""
    out = M.ranking_metrics(p.to(dev), t.to(dev), cutoff)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def check_against_restatement(p, t, got):
    ref = RC.ranking_ref(p, t)
    assert RC.same_bits(got[0], ref[0]), ('auc', RC.max_diff(got[0], ref[0]))
    assert RC.same_bits(got[2], ref[2]), ('fdr', RC.max_diff(got[2], ref[2]))
    assert RC.max_diff(got[1], ref[1]) < 1e-9
    assert np.array_equal(got[3], ref[3]) and np.array_equal(got[4], ref[4])


# ---------------------------------------------------------------------------------------------- fixtures (sklearn / reference)
@pytest.mark.parametrize('name', ['n1', 'n2', 'n37', 'n300', 'n300sat', 'n257q', 'reuters', 'reutersq', 'degenerate'])
def test_fixtures_through_the_c_abi_and_compute_metrics(dev, name):
    c = RC.fixture_cases()[name]
    p, t = torch.from_numpy(c['probs'].astype(np.float32)), torch.from_numpy(c['targets'].astype(np.float32))
    got = gpu_ranking(p, t, dev)
    assert RC.max_diff(got[0], c['auc']) < 1e-10
    assert RC.max_diff(got[1], c['aupr']) < 1e-9
    assert RC.max_diff(got[2], c['fdr']) < 1e-10
    check_against_restatement(p, t, got)
    m = M.compute_metrics(p, t, 1.25, elapsed=2.5, device=dev)
    assert list(m) == ['ACC', 'HA', 'ebF1', 'miF1', 'maF1', 'meanAUC', 'medianAUC', 'meanAUPR', 'medianAUPR', 'allAUC',
                       'allAUPR', 'meanFDR', 'medianFDR', 'loss', 'time'] and m['loss'] == 1.25 and m['time'] == 2.5
    assert RC.same_bits(m['allAUC'], got[0]) and RC.same_bits(m['allAUPR'], got[1])
    agg = [m['meanAUC'], m['medianAUC'], m['meanAUPR'], m['medianAUPR'], m['meanFDR'], m['medianFDR']]
    assert RC.max_diff(agg[:2], c['agg'][:2]) < 1e-10 and RC.max_diff(agg[2:4], c['agg'][2:4]) < 1e-9
    assert RC.max_diff(agg[4:], c['agg'][4:]) < 1e-10
    if 'thresholded' in c:
        # the reference's own five figures for the same matrices: it computes them in float32 (2^-24 ~ 6e-8 per operation),
        # hence 1e-6, the bound tests/test_harness.py holds multilabel_metrics to; the fp64 ratios are held to 1e-12
        for k, r in zip(('ACC', 'HA', 'ebF1', 'miF1', 'maF1'), c['thresholded'].tolist()):
            assert abs(m[k] - r) < 1e-6 or (np.isnan(m[k]) and np.isnan(r)), (k, m[k], r)
        for k, r in zip(('ACC', 'HA', 'ebF1', 'miF1', 'maF1'), multilabel_metrics(torch.nan_to_num(p, nan=0.0), t, 0.5).values()):
            assert abs(m[k] - r) < 1e-12 or (np.isnan(m[k]) and np.isnan(r)), (k, m[k], r)


def test_degenerate_labels_are_nan_where_the_rules_say_and_neighbours_are_unaffected(dev):
    c = RC.fixture_cases()['degenerate']
    p, t = torch.from_numpy(c['probs'].astype(np.float32)), torch.from_numpy(c['targets'].astype(np.float32))
    auc, aupr, fdr, n_pos, n_neg = gpu_ranking(p, t, dev)
    assert np.isnan(auc[[1, 3, 5]]).all() and np.isnan(aupr[[1, 5]]).all() and np.isnan(fdr[[1, 5]]).all()
    assert np.isfinite(aupr[3]) and fdr[3] == 1.0 and n_neg[3] == 0 and n_pos[3] == p.size(0)
    keep = [0, 2, 4, 6]
    clean = gpu_ranking(p[:, keep], t[:, keep], dev)
    for a, b in zip((auc, aupr, fdr), clean):
        assert RC.same_bits(a[keep], b)
    # a score outside [0, 1] and a target other than 0 / 1 unrank their column, and only it
    p2, t2 = p[:, keep].clone(), t[:, keep].clone()
    p2[3, 1] = 1.5
    t2[9, 2] = 2.0
    got = gpu_ranking(p2, t2, dev)
    for a, b in zip(got[:3], clean):
        assert np.isnan(a[[1, 2]]).all() and RC.same_bits(a[[0, 3]], b[[0, 3]])
    check_against_restatement(p2, t2, got)


def test_negative_zero_ranks_like_zero(dev):
    p, t = RC.make_inputs(500, 4, 'saturated', pos_rate=0.3, seed=8)
    assert (p == 0).any()
    want = gpu_ranking(p, t, dev)
    got = gpu_ranking(torch.where(p == 0, torch.full_like(p, -0.0), p), t, dev)
    for a, b in zip(got, want):
        assert RC.same_bits(a.astype(np.float64), b.astype(np.float64))
    assert np.isfinite(got[0]).all()


# ---------------------------------------------------------------------------------------------- shapes against the restatement
SHAPES = [(1, 3, 'normal'), (2, 1, 'normal'), (37, 5, 'normal'), (37, 5, 'quantised'), (3019, 90, 'normal'),
          (3019, 90, 'saturated'), (8000, 919, 'normal'), (300001, 16, 'normal'), (300001, 16, 'quantised'),
          (70000, 5, 'saturated'),
          # either side of the route switch (32768 keys in LDS) and of the global route's 4096-key chunks
          (32767, 3, 'normal'), (32768, 3, 'quantised'), (32769, 3, 'normal'), (36864, 2, 'normal'), (36865, 2, 'quantised'),
          (16384, 2, 'normal'), (16385, 2, 'normal')]


@pytest.mark.parametrize('n,L,kind', SHAPES)
def test_shapes_against_the_restatement(dev, n, L, kind):
    p, t = RC.make_inputs(n, L, kind, pos_rate=0.02 if n > 1000 else 0.3, seed=n + L)
    got = gpu_ranking(p, t, dev)
    check_against_restatement(p, t, got)
    m = M.compute_metrics(p.to(dev), t.to(dev), 0.0)
    assert RC.same_bits(m['allAUC'], got[0]) and RC.same_bits(m['allAUPR'], got[1])
    ref = multilabel_metrics(p, t, 0.5)
    for k, r in zip(('ACC', 'HA', 'ebF1', 'miF1', 'maF1'), ref.values()):
        assert abs(m[k] - r) < 1e-12 or (np.isnan(m[k]) and np.isnan(r)), (k, m[k], r)


@pytest.mark.parametrize('n,L,pad_p,pad_t', [(300, 12, 5, 0), (3019, 90, 38, 6), (40000, 7, 1, 9)])
def test_row_strides_larger_than_L(dev, n, L, pad_p, pad_t):
    p, t = RC.make_inputs(n, L, 'quantised' if n == 300 else 'normal', pos_rate=0.1, seed=5)
    big_p = torch.full((n, L + pad_p), float('nan'), device=dev)      # the padding would unrank a column if it were read
    big_t = torch.full((n, L + pad_t), 7.0, device=dev)
    big_p[:, :L] = p.to(dev)
    big_t[:, :L] = t.to(dev)
    vp, vt = big_p[:, :L], big_t[:, :L]
    assert vp.stride(0) == L + pad_p and (pad_p == 0 or not vp.is_contiguous())
    got = tuple(o.cpu().numpy() for o in M.ranking_metrics(vp, vt))
    want = gpu_ranking(p, t, dev)
    for a, b in zip(got, want):
        assert RC.same_bits(a.astype(np.float64), b.astype(np.float64))
    lab, ex = M.threshold_counts(vp, vt, 0.5)
    lab2, ex2 = M.threshold_counts(p.to(dev), t.to(dev), 0.5)
    assert torch.equal(lab, lab2) and torch.equal(ex, ex2)


# ---------------------------------------------------------------------------------------------- thresholded counts
@pytest.mark.parametrize('n,L', [(1, 3), (37, 5), (3019, 90), (8000, 919), (700, 4200)])
def test_threshold_counts_equal_the_integers_multilabel_metrics_implies(dev, n, L):
    p, t = RC.make_inputs(n, L, 'normal', pos_rate=0.05, seed=n)
    if n > 4:
        p[3] = float('nan')         # a NaN prediction counts as negative
        t[2] = 0
        p[2] = 0                    # an empty sample
        p[:, 1] = 0
        t[:, 1] = 0                 # a label never gold, never predicted
    lab, ex = M.threshold_counts(p.to(dev), t.to(dev), 0.5)
    pb, tb = torch.nan_to_num(p, nan=0.0) >= 0.5, t != 0
    assert torch.equal(lab.cpu().long(), torch.stack(((pb & tb).sum(0), (pb & ~tb).sum(0), (~pb & tb).sum(0))))
    assert torch.equal(ex.cpu().long(), torch.stack(((pb & tb).sum(1), pb.sum(1), tb.sum(1), (pb != tb).sum(1))))
    m = M.compute_metrics(p, t, 0.0, all_metrics=False, device=dev)
    for k, r in zip(('ACC', 'HA', 'ebF1', 'miF1', 'maF1'), multilabel_metrics(p, t, 0.5).values()):
        assert abs(m[k] - r) < 1e-12, (k, m[k], r)
    assert all(m[k] == 0 for k in M.RANKING_KEYS)          # all_metrics=False: zeros, as the reference returns


# ---------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize('n,L,kind', [(3019, 90, 'normal'), (8000, 64, 'quantised'), (100000, 8, 'normal'),
                                      (100000, 8, 'saturated')])
def test_bit_identical_over_runs_and_row_permutations_and_inputs_unchanged(dev, n, L, kind):
    p, t = RC.make_inputs(n, L, kind, pos_rate=0.05, seed=1)
    pd_, td = p.to(dev), t.to(dev)
    p0, t0 = pd_.clone(), td.clone()
    a = tuple(o.cpu().numpy() for o in M.ranking_metrics(pd_, td))
    b = tuple(o.cpu().numpy() for o in M.ranking_metrics(pd_, td))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(dev)
    c = tuple(o.cpu().numpy() for o in M.ranking_metrics(pd_[perm].contiguous(), td[perm].contiguous()))
    for x, y, z in zip(a, b, c):
        assert RC.same_bits(x.astype(np.float64), y.astype(np.float64)) and RC.same_bits(x.astype(np.float64), z.astype(np.float64))
    assert torch.equal(pd_, p0) and torch.equal(td, t0)
    lab, ex = M.threshold_counts(pd_, td, 0.5)
    lab2, ex2 = M.threshold_counts(pd_[perm].contiguous(), td[perm].contiguous(), 0.5)
    assert torch.equal(lab, lab2) and torch.equal(ex[:, perm], ex2) and torch.equal(pd_, p0) and torch.equal(td, t0)


def test_a_too_small_workspace_is_a_status_code(dev):
    lib = N.lib()
    n, L = 40000, 4
    p, t = (x.to(dev) for x in RC.make_inputs(n, L, seed=2))
    need = lib.lamp_ranking_metrics_workspace_bytes(n, L)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.full((3, L), 7.0, dtype=torch.float64, device=dev)
    args = (N.ptr(p), L, N.ptr(t), L, n, L, 0.5, N.ptr(out[0]), N.ptr(out[1]), N.ptr(out[2]), None, None, N.ptr(ws))
    assert lib.lamp_ranking_metrics(*args, need - 1, N.stream()) == -3
    assert lib.lamp_ranking_metrics(*args, 0, N.stream()) == -3
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())          # nothing was launched
    assert lib.lamp_ranking_metrics(*args, need, N.stream()) == 0      # n_pos / n_neg are optional
    torch.cuda.synchronize()
    ref = RC.ranking_ref(p.cpu(), t.cpu())
    assert RC.same_bits(out[0].cpu().numpy(), ref[0]) and RC.max_diff(out[1].cpu().numpy(), ref[1]) < 1e-9


def test_runs_on_the_current_stream(dev):
    """Issued under a side stream and completed by synchronising that stream alone."""
    p, t = (x.to(dev) for x in RC.make_inputs(50000, 8, seed=4))
    ref = RC.ranking_ref(p.cpu(), t.cpu())
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        out = M.ranking_metrics(p, t)
    side.synchronize()
    assert RC.same_bits(out[0].cpu().numpy(), ref[0])


# ---------------------------------------------------------------------------------------------- end to end
def _harness():
    d, sd = load_golden('harness')
    splits = {}
    for name in ('train', 'valid', 'test'):
        splits[name] = {}
        for part in ('src', 'tgt'):
            flat, off = d['%s_%s_flat' % (name, part)], d['%s_%s_off' % (name, part)]
            splits[name][part] = [flat[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
    return d, sd, splits


def test_test_epoch_hands_over_device_matrices(dev):
    from lamp_amd import data as D
    from lamp_amd.Models import LAMP
    from lamp_amd.evaluate import test_epoch
    d, sd, splits = _harness()
    L, dm = sd['decoder.tgt_word_emb.weight'].shape
    h = d['n_head']
    m = LAMP(d['src_vocab_size'], L, d['max_token_seq_len_e'], L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h,
             d_word_vec=dm, d_model=dm, d_inner_hid=2 * dm, d_k=dm // h, d_v=dm // h, encoder='graph', decoder='graph',
             label_adj_matrix=d['label_adj_matrix'].clone(), label_mask='prior', dec_dropout2=False)
    m.load_state_dict(sd)
    m = m.to(dev)
    batches = D.EvalBatcher(splits['test']['src'], splits['test']['tgt'], d['batch_size'])
    plain = test_epoch(m, batches, L, d['batch_size'], dev)
    for streams in (1, 2):
        res = {}
        got = test_epoch(m, batches, L, d['batch_size'], dev, streams=streams, device_results=res)
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and got[2] == plain[2]
        assert res['rows'] == (0, batches.n_insts) and res['probs'].is_cuda and res['targets'].is_cuda
        torch.cuda.synchronize()
        assert torch.equal(res['probs'].cpu(), plain[0]) and torch.equal(res['targets'].cpu(), plain[1])
        on_dev = M.compute_metrics(res['probs'], res['targets'], got[2])
        on_cpu = M.compute_metrics(got[0], got[1], got[2], device=dev)
        assert list(on_dev) == list(on_cpu)
        for k in on_dev:
            assert RC.same_bits(on_dev[k], on_cpu[k]), k
    ref = RC.ranking_ref(plain[0], plain[1])
    assert RC.same_bits(on_dev['allAUC'], ref[0]) and RC.max_diff(on_dev['allAUPR'], ref[1]) < 1e-9


def test_run_eval_all_metrics_prints_every_key(dev, tmp_path):
    """run_eval -all_metrics on the synthetic reuters-shaped dataset of the harness fixture: the JSON keeps its keys and gains
    the ranking ones; without the flag it is what it was."""
    import argparse
    d, sd, splits = _harness()
    src = {('w%d' % i): i for i in range(d['n_src_dict'])}
    tgt = {('l%d' % i): i for i in range(d['n_tgt_dict'])}
    data = {'settings': argparse.Namespace(max_seq_len=d['max_seq_len']), 'dict': {'src': src, 'tgt': tgt}, **splits}
    torch.save(data, tmp_path / 'train_valid_test.pt')
    torch.save({'model': sd, 'epoch': 3}, tmp_path / 'model.chkpt')
    dm = sd['decoder.tgt_word_emb.weight'].size(1)
    args = ['-data', str(tmp_path / 'train_valid_test.pt'), '-checkpoint', str(tmp_path / 'model.chkpt'), '-d_model', str(dm),
            '-d_inner_hid', str(2 * dm), '-n_layers_enc', '2', '-n_head', str(d['n_head']), '-label_mask', 'prior',
            '-batch_size', str(d['batch_size'])]
    env = dict(os.environ, PYTHONPATH=ROOT)
    outs = []
    for extra in ([], ['-all_metrics']):
        r = subprocess.run([sys.executable, '-m', 'lamp_amd.run_eval'] + args + extra, capture_output=True, text=True, env=env,
                           cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    base, full = outs
    assert not any(k in base for k in M.RANKING_KEYS)
    assert set(full) == set(base) | set(M.RANKING_KEYS) | {'metrics_seconds'}
    for k in ('subset_accuracy', 'hamming_accuracy', 'example_f1', 'micro_f1', 'macro_f1', 'bce_total', 'n_samples'):
        assert full[k] == base[k] or (np.isnan(full[k]) and np.isnan(base[k])), k
    L = base['n_labels']
    assert len(full['allAUC']) == L and len(full['allAUPR']) == L
    for k in ('meanAUC', 'medianAUC', 'meanAUPR', 'medianAUPR', 'meanFDR', 'medianFDR'):
        assert 0.0 <= full[k] <= 1.0, (k, full[k])
    assert abs(full['meanAUC'] - RC.finite_stats(full['allAUC'])[0]) < 1e-15
    assert abs(full['medianAUPR'] - RC.finite_stats(full['allAUPR'])[1]) < 1e-15
