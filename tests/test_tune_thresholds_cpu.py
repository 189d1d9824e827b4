"""Fitted decision thresholds without a GPU: the test-local integer restatement against what sklearn
recorded (tests/golden/thresholds.npz), hand cases that pin the tie rule and the degenerate columns, the C ABI's entry points
and their status codes, and the host side of lamp_amd.metrics / run_eval / run_train.  Every comparison is exact."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from lamp_amd import _native as N
from lamp_amd import metrics as M

import thresholds_common as TH

NAMES = ('lamp_tune_thresholds_workspace_bytes', 'lamp_tune_thresholds', 'lamp_threshold_counts_vec')
E_DIMS, E_WORKSPACE, E_UNSUPPORTED, E_NULL = -1, -3, -4, -5
INF = TH.INF_BITS


def f32bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def col(scores, targets, criterion, fallback=0.5):
    return TH.tune_column_ref(np.array(scores, dtype=np.float32), np.array(targets, dtype=np.float32), criterion, fallback)


def test_restatement_matches_the_sklearn_record():
    """Every label's optimum in the fixture is unique (the generator asserts it in exact arithmetic), so sklearn's argmax and
    the restatement's must name the same threshold bit for bit, with the same integers behind the best F1 / J."""
    z = TH.fixture()
    scores, targets = z['scores'], z['targets']
    assert scores.shape == (300, 12) and str(z['sklearn_version']) == '1.7.2'
    assert all(len(np.unique(scores[:, l])) == 300 for l in range(12))
    for criterion in ('f1', 'youden'):
        got = TH.tune_ref(scores, targets, criterion)
        assert got['tuned'].all()
        assert np.array_equal(got['threshold'], z[criterion + '_threshold'].view(np.uint32)), criterion
        assert np.array_equal(got['tp'], z[criterion + '_tp']) and np.array_equal(got['fp'], z[criterion + '_fp']), criterion
        assert np.array_equal(got['n_pos'], targets.sum(0).astype(np.int32))
        for l in range(12):
            want = TH.value_ref(criterion, z[criterion + '_tp'][l], z[criterion + '_fp'][l], got['n_pos'][l], got['n_neg'][l])
            assert TH.value_ref(criterion, got['tp'][l], got['fp'][l], got['n_pos'][l], got['n_neg'][l]) == want


def test_hand_cases_pin_the_tie_rule():
    # candidates: c0 (0, 0), c1 = 0.9 (tp 1, cnt 1), c2 = 0.8 (1, 2), c3 = 0.7 (2, 3), c4 = 0.6 (2, 4); P = N = 2
    s, t = [0.9, 0.8, 0.7, 0.6], [1, 0, 1, 0]
    # F1: 0, 2/3, 2/4, 4/5, 4/6 -> c3
    assert col(s, t, 'f1') == (f32bits(0.7), 2, 1, 2, 2, 1)
    # J scaled by P N: 0, 2, 0, 2, 0 -> c1 and c3 tie: the highest threshold
    assert col(s, t, 'youden') == (f32bits(0.9), 1, 0, 2, 2, 1)
    # |tp N + fp P - P N|: 4, 2, 0, 2, 4 -> c2
    assert col(s, t, 'balance') == (f32bits(0.8), 1, 1, 2, 2, 1)
    # an F1 tie: c1 = 1.0 (tp 1, cnt 1) 2/(1+2), c2 = 0.5 (2, 4) 4/(4+2): equal -> c1
    assert col([1.0, 0.5, 0.5, 0.5], [1, 1, 0, 0], 'f1') == (f32bits(1.0), 1, 0, 2, 2, 1)
    # the balance with P = N = 1: distances 1, 0 (the negative alone: tpr 0 = 1 - fpr), 1
    assert col([0.9, 0.1], [0, 1], 'balance') == (f32bits(0.9), 0, 1, 1, 1, 1)
    # N = 0: every distance is 0, so is every J
    assert col([0.9], [1], 'balance') == (INF, 0, 0, 1, 0, 1)


def test_hand_cases_pin_the_degenerate_columns():
    for criterion in TH.CRITERIA:
        # P = 0: every candidate has tp = 0, all three tie everywhere -> predict nothing
        assert col([0.3, 0.9, 0.1], [0, 0, 0], criterion) == (INF, 0, 0, 0, 3, 1), criterion
        # a NaN score, a score outside [0, 1], a target other than 0 / 1: the fallback, zeros, not tuned
        assert col([0.3, float('nan'), 0.1], [0, 1, 0], criterion, 0.25) == (f32bits(0.25), 0, 0, 0, 0, 0)
        assert col([0.3, 1.5, 0.1], [0, 1, 0], criterion) == (f32bits(0.5), 0, 0, 0, 0, 0)
        assert col([0.3, -0.5, 0.1], [0, 1, 0], criterion) == (f32bits(0.5), 0, 0, 0, 0, 0)
        assert col([0.3, 0.5, 0.1], [0, 2, 0], criterion) == (f32bits(0.5), 0, 0, 0, 0, 0)
    # N = 0: F1 grows with every positive taken -> the lowest score; J and the balance tie everywhere -> predict nothing
    assert col([0.3, 0.9, 0.1], [1, 1, 1], 'f1') == (f32bits(0.1), 3, 0, 3, 0, 1)
    assert col([0.3, 0.9, 0.1], [1, 1, 1], 'youden') == (INF, 0, 0, 3, 0, 1)
    assert col([0.3, 0.9, 0.1], [1, 1, 1], 'balance') == (INF, 0, 0, 3, 0, 1)
    # a constant column: two candidates, nothing or everything
    assert col([0.25] * 4, [1, 0, 0, 1], 'f1') == (f32bits(0.25), 2, 2, 2, 2, 1)
    assert col([0.25] * 4, [1, 0, 0, 1], 'youden') == (INF, 0, 0, 2, 2, 1)          # J = 0 at both
    assert col([0.25] * 4, [1, 0, 0, 1], 'balance') == (INF, 0, 0, 2, 2, 1)         # |0 - 4| = |4 + 4 - 4|
    # one row
    assert col([0.7], [1], 'f1') == (f32bits(0.7), 1, 0, 1, 0, 1)
    assert col([0.7], [0], 'f1') == (INF, 0, 0, 0, 1, 1)
    assert col([0.7], [1], 'youden') == (INF, 0, 0, 1, 0, 1)
    # a score of 1.0 is a threshold like any other (and the key's largest)
    assert col([1.0, 0.2], [1, 0], 'f1') == (0x3F800000, 1, 0, 1, 1, 1)
    assert col([1.0, 0.2], [1, 0], 'youden') == (0x3F800000, 1, 0, 1, 1, 1)
    # -0.0 next to +0.0: one group, and its threshold is +0.0's bits
    assert col([-0.0, 0.0, -0.0], [1, 0, 1], 'f1') == (0x00000000, 2, 1, 2, 1, 1)
    bits, tp, cnt = TH.candidates(np.array([-0.0, 0.0, 0.5], np.float32), np.array([1, 1, 0], np.float32))
    assert bits == [INF, f32bits(0.5), 0] and tp == [0, 0, 2] and cnt == [0, 1, 3]


def test_counts_restatement_reads_nan_and_infinite_thresholds_as_predict_nothing():
    s = np.array([[0.9, 0.9, 0.9, float('nan')], [0.1, 1.0, 0.4, 0.0]], np.float32)
    t = np.array([[1, 1, 0, 1], [0, 1, 1, 0]], np.float32)
    lab, ex = TH.counts_ref(s, t, np.array([0.5, float('inf'), float('nan'), 0.0], np.float32))
    assert lab.tolist() == [[1, 0, 0, 1], [0, 0, 0, 1], [0, 2, 1, 0]]               # a NaN score is 0: predicted at 0.0
    assert ex.tolist() == [[2, 0], [2, 1], [3, 2], [1, 3]]


def test_generators_cover_what_they_name():
    s, t = TH.make_case(1025, 7)
    kinds = [TH.FAMILIES[(l + 1025) % 7] for l in range(7)]
    assert sorted(kinds) == sorted(TH.FAMILIES)
    for l, k in enumerate(kinds):
        assert TH.rankable(s[:, l], t[:, l]) == (k != 'unrankable'), k
    c = kinds.index
    assert len(np.unique(s[:, c('tiefree')])) == 1025 and len(np.unique(s[:, c('ties7')])) == 7
    assert len(np.unique(s[:, c('constant')])) == 1 and t[:, c('nopos')].sum() == 0 and t[:, c('noneg')].sum() == 1025
    sep = c('separable')
    assert s[t[:, sep] == 1, sep].min() > s[t[:, sep] == 0, sep].max()
    for n in (1, 2):
        for fam in TH.FAMILIES:
            s, t = TH.make_case(n, 2, family=fam)
            assert s.shape == (n, 2) and all(len(TH.tune_ref(s, t, cr)['tp']) == 2 for cr in TH.CRITERIA)


def test_header_and_ctypes_table_carry_the_new_entry_points():
    text = open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = N.lib()
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in N.PROTOTYPES and hasattr(lib, name) and name in N.LATE_ENTRY_POINTS
    assert re.search(r'LAMP_TUNE_F1\s*=\s*0\s*,\s*LAMP_TUNE_YOUDEN\s*=\s*1\s*,\s*LAMP_TUNE_BALANCE\s*=\s*2', code)
    assert M.TUNE_CRITERIA == TH.CRITERION_ID
    for phrase in ('A tie goes to the smallest c', 'drop_intermediate', 'NaN threshold', 'P == 0'):
        assert phrase in text, phrase
    assert lib.lamp_version() == N.ABI_VERSION == 5                     # additive: the ABI version stays


def test_build_lists_the_unit_as_lean():
    from lamp_amd import build
    assert 'thresholds.hip' in build.SOURCES and 'thresholds.hip' in build.LEAN_UNITS
    rows = build.kernel_resources('thresholds.hip')
    assert sum('tune_walk_kernel' in k for k in rows) == 3 and any('threshold_counts_vec_kernel' in k for k in rows)
    for name, r in rows.items():
        assert r.get('scratch', 0) == 0 and r.get('agpr', 0) == 0, (name, r)


def _tune(lib, probs=16, ldp=90, targets=16, ldt=90, n=10, L=90, criterion=0, outs=(16, 16, 16, 16, 16), tuned=16, ws=16,
          nbytes=1 << 40):
    return lib.lamp_tune_thresholds(probs, ldp, targets, ldt, n, L, criterion, 0.5, outs[0], outs[1], outs[2], outs[3], outs[4],
                                    tuned, ws, nbytes, None)


def test_tune_thresholds_validates_before_any_launch():
    lib = N.lib()
    ws = lib.lamp_tune_thresholds_workspace_bytes
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(1 << 31, 5) == 0 and ws(-1, 5) == 0
    assert ws(10, 90) == lib.lamp_ranking_metrics_workspace_bytes(10, 90) >= 10 * 90 * 4 + 90 * 4      # the same layout
    assert ws(32768, 3) < ws(32769, 3)                                                                  # the radix route's second buffer
    for bad in (dict(n=0), dict(n=-1), dict(L=0, ldp=0, ldt=0), dict(ldp=89), dict(ldt=89)):
        assert _tune(lib, **bad) == E_DIMS, bad
    for bad in (dict(probs=None), dict(targets=None), dict(ws=None)) + tuple(
            dict(outs=tuple(None if i == j else 16 for i in range(5))) for j in range(5)):
        assert _tune(lib, **bad) == E_NULL, bad
    for bad in (dict(criterion=3), dict(criterion=-1), dict(n=1 << 31)):
        assert _tune(lib, **bad) == E_UNSUPPORTED, bad
    assert _tune(lib, nbytes=ws(10, 90) - 1) == E_WORKSPACE             # one byte short: a status code, nothing launched
    assert _tune(lib, nbytes=0) == E_WORKSPACE
    # the order of the checks: dimensions, pointers, what is not served, the workspace
    assert _tune(lib, probs=None, ldp=89) == E_DIMS
    assert _tune(lib, probs=None, criterion=3) == E_NULL
    assert _tune(lib, criterion=3, nbytes=0) == E_UNSUPPORTED
    assert _tune(lib, n=1 << 31, nbytes=0) == E_UNSUPPORTED
    assert _tune(lib, tuned=None, nbytes=0) == E_WORKSPACE              # `tuned` is nullable


def _vec(lib, probs=16, ldp=90, targets=16, ldt=90, n=10, L=90, thresholds=16, outs=(16,) * 7):
    return lib.lamp_threshold_counts_vec(probs, ldp, targets, ldt, n, L, thresholds, *outs, None)


def test_threshold_counts_vec_validates_before_any_launch():
    lib = N.lib()
    for bad in (dict(n=0), dict(n=-1), dict(L=0, ldp=0, ldt=0), dict(ldp=89), dict(ldt=89)):
        assert _vec(lib, **bad) == E_DIMS, bad
    for bad in (dict(probs=None), dict(targets=None), dict(thresholds=None)) + tuple(
            dict(outs=tuple(None if i == j else 16 for i in range(7))) for j in range(7)):
        assert _vec(lib, **bad) == E_NULL, bad
    assert _vec(lib, n=(1 << 31) * 256) == E_UNSUPPORTED
    assert _vec(lib, thresholds=None, ldp=89) == E_DIMS
    assert _vec(lib, thresholds=None, n=(1 << 31) * 256) == E_NULL


def test_tuned_values_come_from_the_integers():
    res = {'tp': np.array([2, 0, 3, 0, 1], np.int32), 'fp': np.array([1, 0, 0, 0, 1], np.int32),
           'n_pos': np.array([2, 0, 3, 0, 1], np.int32), 'n_neg': np.array([2, 3, 0, 0, 1], np.int32),
           'tuned': np.array([True, True, True, False, True])}
    f1 = M.tuned_values(res, 'f1')
    assert f1[0] == 4 / 5 and np.isnan(f1[1]) and f1[2] == 1.0 and np.isnan(f1[3]) and f1[4] == 2 / 3
    j = M.tuned_values(res, 'youden')
    assert j[0] == (2 * 2 - 1 * 2) / 4 and np.isnan(j[1]) and np.isnan(j[2]) and np.isnan(j[3]) and j[4] == 0.0
    b = M.tuned_values(res, 'balance')
    assert b[0] == abs(4 + 2 - 4) / 4 and np.isnan(b[1]) and np.isnan(b[2]) and b[4] == 1.0
    for l in range(5):
        for c in TH.CRITERIA:
            want = TH.value_ref(c, res['tp'][l], res['fp'][l], res['n_pos'][l], res['n_neg'][l]) if res['tuned'][l] else np.nan
            got = M.tuned_values(res, c)[l]
            assert got == want or (np.isnan(got) and np.isnan(want))
    with pytest.raises(ValueError):
        M.tuned_values(res, 'f2')


def test_arguments_are_checked_on_the_host(monkeypatch):
    p, t = torch.rand(4, 3), torch.zeros(4, 3)
    with pytest.raises(ValueError, match='criterion'):
        M.tune_thresholds(p, t, 'f2')
    with pytest.raises(ValueError, match='scope'):
        M.tune_thresholds(p, t, 'f1', scope='sample')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match='HIP device only'):
        M.tune_thresholds(p, t, 'f1')
    with pytest.raises(RuntimeError, match='HIP device only'):
        M.threshold_counts(p, t, torch.full((3,), 0.5))
    from lamp_amd.Models import LAMP
    m = LAMP(20, 9, 6, 9, n_layers_enc=1, n_layers_dec=1, n_head=2, n_head2=2, d_word_vec=16, d_model=16, d_inner_hid=32, d_k=8,
             d_v=8, encoder='graph', decoder='graph', label_mask='none', dec_dropout2=False)
    seq = torch.randint(1, 20, (2, 6))
    pos = torch.arange(1, 7).repeat(2, 1)
    with pytest.raises(RuntimeError, match='HIP device only'):
        m.predict_labels((seq, pos), 0.5)
    assert m.training                                   # the mode it was in is put back
    assert inspect.signature(LAMP.predict_labels).parameters['thresholds'].default == 0.5


def test_compute_metrics_without_thresholds_makes_the_calls_it_made(monkeypatch):
    """The default: ONE counts call with the python float, no other entry; thresholds=tensor hands the tensor to the same
    call and changes nothing but the five thresholded figures."""
    assert inspect.signature(M.compute_metrics).parameters['thresholds'].default is None
    n, L = 12, 7
    rng = np.random.default_rng(5)
    p = torch.from_numpy(rng.random((n, L)).astype(np.float32))
    t = torch.from_numpy((rng.random((n, L)) < 0.3).astype(np.float32))
    calls = []

    class FakeDev(object):
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return torch.from_numpy(self.a)

    def counts(pp, tt, thr):
        calls.append(thr)
        lab, ex = TH.counts_ref(pp.numpy(), tt.numpy(), thr.numpy() if torch.is_tensor(thr) else thr)
        return FakeDev(np.concatenate((lab.reshape(-1), ex.reshape(-1))))

    class NoDevice(object):
        def __init__(self, *a):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    def forbidden(*a, **k):
        raise AssertionError('an entry the default must not reach')

    monkeypatch.setattr(M, '_counts_buffer', counts)
    monkeypatch.setattr(M, 'tune_thresholds', forbidden)
    monkeypatch.setattr(M, '_threshold_vector', forbidden)
    monkeypatch.setattr(M, '_rank_at_k_buffer', forbidden)
    monkeypatch.setattr(torch.cuda, 'device', NoDevice)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    base = M.compute_metrics(p, t, 0.5, 0.4, all_metrics=False)
    assert list(base) == ['ACC', 'HA', 'ebF1', 'miF1', 'maF1'] + list(M.RANKING_KEYS) + ['loss', 'time']
    assert len(calls) == 1 and isinstance(calls[0], float) and calls[0] == 0.4
    same = M.compute_metrics(p, t, 0.5, 0.9, all_metrics=False, thresholds=torch.full((L,), 0.4))
    assert len(calls) == 2 and torch.is_tensor(calls[1]) and calls[1].dtype == torch.float32
    assert list(same) == list(base) and all(same[k] == base[k] or (np.isnan(same[k]) and np.isnan(base[k])) for k in base)
    thr = torch.tensor([0.1, 0.9, 0.5, float('inf'), 0.3, 0.7, 0.2])
    tuned = M.compute_metrics(p, t, 0.5, all_metrics=False, thresholds=thr)
    lab, ex = TH.counts_ref(p.numpy(), t.numpy(), thr.numpy())
    assert {k: tuned[k] for k in ('ACC', 'HA', 'ebF1', 'miF1', 'maF1')} == M.thresholded_from_counts(lab, ex, L)


def test_run_eval_parses_the_flags():
    from lamp_amd import run_eval
    base = run_eval.parse(['-data', 'x.pt'])
    assert base.tune_thresholds is None and base.tune_split == 'valid' and base.tune_scope == 'label'
    opt = run_eval.parse(['-data', 'x.pt', '-tune_thresholds', 'youden', '-tune_split', 'train', '-tune_scope', 'global'])
    assert (opt.tune_thresholds, opt.tune_split, opt.tune_scope) == ('youden', 'train', 'global')
    assert run_eval.parse(['-data', 'x.pt', '-tune_thresholds', 'checkpoint']).tune_thresholds == 'checkpoint'
    for k, v in vars(base).items():                      # nothing else moves
        if not k.startswith('tune_'):
            assert getattr(opt, k) == v, k
    for bad in (['-tune_thresholds', 'f2'], ['-tune_thresholds', 'f1', '-tune_scope', 'sample'], ['-tune_split', 'dev']):
        with pytest.raises(SystemExit):
            run_eval.parse(['-data', 'x.pt'] + bad)


def test_run_train_parses_the_flag_and_is_unchanged_without_it():
    from lamp_amd import run_train
    base = run_train.parse(['-data', 'x.pt'])
    assert base.tune_thresholds is None
    assert base.model_name == ('results/reuters/enc_graph.dec_graph.512.1024.64.64.nlayers_5_5.nheads_8.proj_share.bsz_64.loss_ce.'
                               'adam.lr_0002.drop_10_10.nonemask')
    assert 'tune_thresholds' not in vars(run_train.checkpoint_settings(base))
    for c in TH.CRITERIA:
        opt = run_train.parse(['-data', 'x.pt', '-tune_thresholds', c, '-name', 'r1'])
        assert opt.tune_thresholds == c and opt.model_name == base.model_name + '.thr_%s.r1' % c
        s = vars(run_train.checkpoint_settings(opt))
        assert s['tune_thresholds'] == c
        assert set(s) - {'tune_thresholds'} == set(vars(run_train.checkpoint_settings(base)))
    with pytest.raises(SystemExit):
        run_train.parse(['-data', 'x.pt', '-tune_thresholds', 'checkpoint'])
    assert inspect.signature(run_train.save_model).parameters['label_thresholds'].default is None
