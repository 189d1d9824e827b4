"""Label-ranking metrics of whole rows (LRAP, coverage error, ranking loss, one-error, per-sample AUC)
without a GPU: the test-local restatement against what sklearn recorded (tests/golden/label_ranking.npz) and against a
brute-force pair count, hand cases that pin the tie rule and the conventions, the generators, the C ABI's entry points and
their status codes, and the host side of lamp_amd.metrics / run_eval / run_train."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from lamp_amd import _native as N
from lamp_amd import metrics as M

import label_ranking_common as LR
import rank_at_k_common as RK

NAMES = ('lamp_label_ranking_workspace_bytes', 'lamp_label_ranking')
E_DIMS, E_WORKSPACE, E_UNSUPPORTED, E_NULL = -1, -3, -4, -5
GPU_LS = (1, 2, 63, 64, 65, 90, 983, 1024, 1025, 4096, 4097, 32768)     # test_label_ranking_gpu.py: LS


# ---------------------------------------------------------------------------------------------- the restatement
def test_restatement_matches_the_sklearn_record():
    """Within 1e-12: fp64 sums of <= 37 terms and a mean of 120 (the gap measured when the record was made: 1e-16)."""
    z = LR.fixture()
    scores, targets = z['scores'], z['targets']
    assert scores.shape == targets.shape == (120, 37) and str(z['sklearn_version']) == '1.7.2'
    assert (targets.sum(1) == 0).sum() >= 2 and (targets.sum(1) == 37).sum() >= 1
    quantised = np.array([np.array_equal(r * 8, np.round(r * 8)) for r in scores])
    assert quantised.sum() == 60 and LR.rows_with_a_tie(scores, targets)[quantised].mean() > 0.5
    got = LR.figures_ref(scores, targets)
    for key, name in (('LRAP', 'lrap'), ('coverage_error', 'coverage_error'), ('ranking_loss', 'ranking_loss'),
                      ('instance_AUC', 'instance_auc')):
        assert abs(got[key] - float(z[name])) < 1e-12, (key, got[key], float(z[name]))
    assert got['n_with_both'] == int(z['n_with_both']) == int(((targets.sum(1) > 0) & (targets.sum(1) < 37)).sum())


@pytest.mark.parametrize('kind', LR.KINDS)
def test_restatement_equals_the_brute_force_pair_count(kind):
    """The sort-based restatement (integer keys) against O(L^2) counting in float semantics, every target pattern."""
    for L in (1, 2, 13, 37):
        n = 9
        s, t = LR.make_scores(kind, n, L), LR.make_targets(n, L, density=0.3)
        for i in range(n):
            ints, lrap, _, _ = LR.row_ref(s[i], t[i])
            b_ints, b_lrap = LR.brute_row(s[i], t[i])
            assert tuple(ints) == tuple(b_ints), (kind, L, i)
            assert abs(lrap - b_lrap) <= (ints[0] + 2) * LR.U, (kind, L, i)


def _row(s, gold):
    s = np.asarray(s, dtype=np.float32)
    t = np.zeros(len(s), np.float32)
    t[list(gold)] = 1.0
    return LR.row_ref(s, t)


def test_hand_cases_pin_the_definitions():
    nan, inf = float('nan'), float('inf')
    ints, lrap, rloss, auc = _row([.5, .5, .1], {0})
    assert ints == (1, 2, 1, 1, 1, 0) and lrap == 0.5 and rloss == 0.5 and auc == 0.75     # a tie counts against the gold label
    assert _row([0.0, -0.0, -1.0], {0})[0] == (1, 2, 1, 1, 1, 0)                          # +0.0 and -0.0 are tied
    assert _row([-0.0, 0.0, -1.0], {1})[0] == (1, 2, 1, 1, 0, 0)                          # ... and the lower column is first
    ints, lrap, rloss, auc = _row([-inf, nan, nan], {1})
    assert ints == (1, 3, 2, 1, 0, 1) and lrap == 1.0 / 3.0 and rloss == 1.0 and auc == 0.25      # NaN below -inf, NaNs tied
    assert _row([nan, -inf], {1})[0] == (1, 1, 0, 0, 1, 1)
    ints, lrap, rloss, auc = _row([.3, .2, .1], ())
    assert ints == (0, 0, 0, 0, 0, 0) and (lrap, rloss, auc) == (1.0, 0.0, None)          # the empty row: 1, 0, 0
    ints, lrap, rloss, auc = _row([.3, .2, .1], {0, 1, 2})
    assert ints == (3, 3, 0, 0, 1, 0) and (lrap, rloss, auc) == (1.0, 0.0, None)          # the full row
    assert _row([2.0], {0}) == ((1, 1, 0, 0, 1, 0), 1.0, 0.0, None)                       # L = 1
    assert _row([nan], ()) == ((0, 0, 0, 0, 0, 1), 1.0, 0.0, None)
    tiny = np.array([1, 0x80000001], dtype=np.uint32).view(np.float32)                   # two denormals of opposite sign
    assert _row(tiny, {1})[0] == (1, 2, 1, 0, 0, 0) and _row(tiny, {0})[0] == (1, 1, 0, 0, 1, 0)
    assert len(set(LR.keys_ref(np.array([tiny[0], tiny[1], 0.0], np.float32)).tolist())) == 3
    f = LR.figures_ref(np.array([[.5, .5, .1], [.3, .2, .1]], np.float32), np.array([[1, 0, 0], [0, 0, 0]], np.float32))
    assert f == {'LRAP': 0.75, 'coverage_error': 1.0, 'ranking_loss': 0.25, 'one_error': 0.5, 'instance_AUC': 0.75,
                 'n_with_gold': 1, 'n_with_both': 1, 'n_rows_with_nan': 0}


def test_generators_put_ties_where_the_tie_rule_is_tested():
    """At the shapes the GPU tests use, a gold label is tied with a label that is not gold in at least a quarter of the
    quantised and of the saturated rows -- at every shape of 67 rows, and over all rows of the kind; the two shapes of 5 rows
    (of which one is empty and one full) have at least the half-positive row -- and a restatement that counts s_j > s_p
    instead of s_j >= s_p differs on every one of those matrices: otherwise the tie rule would not be tested.  The target
    patterns are there."""
    tie_rows = {'quantised': [], 'saturated': []}
    for L in GPU_LS:
        n = 5 if L > 4096 else 67
        t = LR.make_targets(n, L)
        assert t[0].sum() == (L + 1) // 2 and t[1].sum() == 0 and t[3].sum() == L
        assert t[2].nonzero()[0].tolist() == [0] and t[4].nonzero()[0].tolist() == [L - 1]
        if L < 63:
            continue
        for kind in tie_rows:
            s = LR.make_scores(kind, n, L)
            ties = LR.rows_with_a_tie(s, t)
            tie_rows[kind].extend(ties.tolist())
            assert ties[0] and ties.mean() >= (0.25 if n == 67 else 0.2), (kind, L)
            ints, lrap, _, _ = LR.rows_ref(s, t)
            m_ints, m_lrap, _, _ = LR.rows_ref(s, t, strict=True)
            assert np.array_equal(ints[:, 2] != m_ints[:, 2], ties) and (lrap != m_lrap).any(), (kind, L)
    assert all(np.mean(v) >= 0.25 for v in tie_rows.values())
    sp = LR.make_scores('special', 67, 90)
    assert np.isnan(sp[2]).all() and LR.rows_ref(sp, LR.make_targets(67, 90))[0][:, 5].sum() > 2


# ---------------------------------------------------------------------------------------------- ABI and build
def test_header_and_ctypes_table_carry_the_new_entry_points():
    text = open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = N.lib()
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in N.PROTOTYPES and hasattr(lib, name) and name in N.LATE_ENTRY_POINTS
    for phrase in ('THE TIE RULE', 'rank_p = #{j : s_j >= s_p}', '1.0 for an empty row', 'coverage_error row',
                   'rows with 0 < n_p < L only', 'n_rows_with_nan', 'saturate to exactly 0 or 1'):
        assert phrase in text, phrase                                     # the definitions and conventions are written down
    assert lib.lamp_version() == N.ABI_VERSION == 5                       # additive: the ABI version stays


def test_build_lists_the_new_kernels_as_lean():
    from lamp_amd import build
    assert 'rank_at_k.hip' in build.LEAN_UNITS
    rows = build.kernel_resources('rank_at_k.hip')
    assert sum('label_rank_wave_kernel' in k for k in rows) == 5 and sum('label_rank_block_kernel' in k for k in rows) == 5
    assert any('label_rank_chunk_kernel' in k for k in rows) and any('label_rank_final_kernel' in k for k in rows)
    for name, r in rows.items():
        if 'label_rank' in name:
            assert r.get('scratch', 0) == 0 and r.get('agpr', 0) == 0, (name, r)
    big = [r for k, r in rows.items() if 'label_rank_block_kernel<32, 16>' in k]
    assert len(big) == 1 and 128 * 1024 <= big[0]['lds'] <= 160 * 1024    # the whole row's keys, within a workgroup's LDS


def _call(lib, scores=16, lds=90, targets=16, ldt=90, n=10, L=90, sums=16, counts=16, rc=16, rl=16, ws=16, nbytes=1 << 40):
    return lib.lamp_label_ranking(scores, lds, targets, ldt, n, L, sums, counts, rc, rl, ws, nbytes, None)


def test_label_ranking_validates_before_any_launch():
    """Every refusal below comes back with pointers that are not device memory: nothing was launched."""
    lib = N.lib()
    ws = lib.lamp_label_ranking_workspace_bytes
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(-1, 5) == 0 and ws(5, 32769) == 0 and ws(1 << 31, 5) == 0
    assert ws(10, 5) >= 10 * (6 * 4 + 3 * 8) + 8 * 8 and ws((1 << 31) - 1, 32768) > 0
    sizes = [ws(n, 919) for n in (1, 10, 1024, 1025, 3019, 100000, 455024)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1] and ws(1024, 919) < ws(1025, 919)
    assert ws(3019, 90) == ws(3019, 32768)                                  # the per-row terms: no function of L
    for bad in (dict(n=0), dict(n=-1), dict(L=0, lds=0, ldt=0), dict(lds=89), dict(ldt=89)):
        assert _call(lib, **bad) == E_DIMS, bad
    for bad in (dict(scores=None), dict(targets=None), dict(sums=None), dict(counts=None), dict(ws=None)):
        assert _call(lib, **bad) == E_NULL, bad
    assert _call(lib, L=32769, lds=32769, ldt=32769) == E_UNSUPPORTED
    assert _call(lib, n=1 << 31) == E_UNSUPPORTED
    assert _call(lib, nbytes=ws(10, 90) - 1) == E_WORKSPACE                 # one byte short: a status code, nothing launched
    assert _call(lib, rc=None, rl=None, nbytes=ws(10, 90) - 1) == E_WORKSPACE      # the row outputs are nullable
    # the order of the checks: dimensions, then pointers, then what is not served, then the workspace
    assert _call(lib, scores=None, lds=89) == E_DIMS
    assert _call(lib, scores=None, L=32769, lds=32769, ldt=32769) == E_NULL
    assert _call(lib, L=32769, lds=32769, ldt=32769, nbytes=0) == E_UNSUPPORTED
    assert _call(lib, n=1 << 31, nbytes=0) == E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- the host side
def _buffer(sums, counts):
    buf = np.zeros(8)
    buf[:3] = sums
    buf[3:].view(np.int64)[:] = counts
    return buf


def test_figures_from_the_sums():
    out = M.label_ranking_from_sums(_buffer([6.0, 1.5, 4.5], [25, 7, 9, 6, 2]), 10)
    assert out == {'LRAP': 0.6, 'coverage_error': 2.5, 'ranking_loss': 0.15, 'one_error': 1.0 - 0.7, 'instance_AUC': 0.75,
                   'n_with_gold': 9, 'n_with_both': 6, 'n_rows_with_nan': 2}
    assert list(out) == list(M.LABEL_RANKING_KEYS)
    assert all(isinstance(out[k], int) for k in ('n_with_gold', 'n_with_both', 'n_rows_with_nan'))
    none = M.label_ranking_from_sums(_buffer([3.0, 0.0, 0.0], [0, 0, 0, 0, 0]), 3)
    assert none['LRAP'] == 1.0 and np.isnan(none['instance_AUC']) and none['one_error'] == 1.0
    assert M.LABEL_RANKING_ROW_COUNTS == LR.ROW_COUNTS


def test_compute_metrics_without_label_ranking_is_what_it_was(monkeypatch):
    """The default key set and no extra call, from the host half alone: the device buffers replaced by host restatements."""
    assert inspect.signature(M.compute_metrics).parameters['label_ranking'].default is False
    n, L = 12, 7
    rng = np.random.default_rng(3)
    p, t = torch.from_numpy(rng.random((n, L)).astype(np.float32)), torch.from_numpy(RK.make_targets(n, L))
    called = []

    class FakeDev(object):
        """Stands where a device tensor would: .cpu() hands the host buffer over."""
        def __init__(self, a):
            self.a = a

        def cpu(self):
            called.append('copy')
            return torch.from_numpy(self.a)

    def counts(pp, tt, thr):
        pred, gold = (torch.nan_to_num(pp, nan=0.0) >= thr), tt != 0
        lab = torch.stack(((pred & gold).sum(0), (pred & ~gold).sum(0), (~pred & gold).sum(0))).to(torch.int32)
        ex = torch.stack(((pred & gold).sum(1), pred.sum(1), gold.sum(1), (pred != gold).sum(1))).to(torch.int32)
        return FakeDev(torch.cat((lab.reshape(-1), ex.reshape(-1))).numpy())

    def label_ranking(pp, tt, rows=False):
        called.append('label_ranking')
        sums, cnt = LR.sums_ref(*LR.rows_ref(pp.numpy(), tt.numpy()))
        return FakeDev(_buffer(sums, cnt)), None, None

    class NoDevice(object):
        def __init__(self, *a):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    monkeypatch.setattr(M, '_counts_buffer', counts)
    monkeypatch.setattr(M, '_label_ranking_buffer', label_ranking)
    monkeypatch.setattr(torch.cuda, 'device', NoDevice)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    base = M.compute_metrics(p, t, 0.5, all_metrics=False)
    assert list(base) == ['ACC', 'HA', 'ebF1', 'miF1', 'maF1'] + list(M.RANKING_KEYS) + ['loss', 'time']
    assert called == ['copy']                                # the thresholded counts' one copy, and not one call more
    del called[:]
    full = M.compute_metrics(p, t, 0.5, all_metrics=False, label_ranking=True)
    assert list(full) == list(base)[:-2] + list(M.LABEL_RANKING_KEYS) + ['loss', 'time']
    assert called == ['label_ranking', 'copy', 'copy']       # one launch group, one more copy
    for k in base:
        assert full[k] == base[k] or (np.isnan(full[k]) and np.isnan(base[k])), k
    ref = LR.figures_ref(p.numpy(), t.numpy())
    assert {k: full[k] for k in M.LABEL_RANKING_KEYS} == ref


def test_everything_raises_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    s, t = torch.from_numpy(LR.make_scores('normal', 8, 9)), torch.from_numpy(LR.make_targets(8, 9))
    with pytest.raises(RuntimeError, match='HIP device only'):
        M.label_ranking(s, t)
    with pytest.raises(RuntimeError, match='HIP device only'):
        M.label_ranking_rows(s, t)
    with pytest.raises(RuntimeError, match='HIP device only'):
        M.compute_metrics(torch.sigmoid(s), t, 0.0, all_metrics=False, label_ranking=True)


def test_no_sklearn_under_the_package():
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'lamp_amd')):
        for f in files:
            if f.endswith('.py'):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(import|from)\s+sklearn', text, flags=re.M), f


# ---------------------------------------------------------------------------------------------- the runners' flags
def test_run_eval_accepts_label_ranking():
    from lamp_amd import run_eval
    assert run_eval.parse(['-data', 'x.pt']).label_ranking is False
    opt = run_eval.parse(['-data', 'x.pt', '-label_ranking'])
    assert opt.label_ranking is True and opt.all_metrics is False and opt.at_k == ()
    both = run_eval.parse(['-data', 'x.pt', '-label_ranking', '-at_k', '1,3', '-all_metrics'])
    assert both.label_ranking and both.at_k == (1, 3) and both.all_metrics
    assert '-label_ranking' in run_eval.__doc__ and 'label_ranking_seconds' in run_eval.__doc__


BASE = ['-data', 'x.pt', '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-name', 'n1']


def test_run_train_flags_are_reporting_only():
    from lamp_amd import run_train as RT
    plain = RT.parse(BASE)
    assert plain.label_ranking is False and plain.at_k == ()
    opt = RT.parse(BASE + ['-label_ranking', '-at_k', '1,3,5'])
    assert opt.label_ranking is True and opt.at_k == (1, 3, 5)
    assert opt.model_name == plain.model_name                              # no change to the results name
    for o in (plain, opt):
        o.loss_options, o.rank_loss = None, None                            # as run_train.main leaves them for plain BCE
    st, st_plain = RT.checkpoint_settings(opt), RT.checkpoint_settings(plain)
    assert vars(st) == vars(st_plain)                                       # ... nor to the checkpoint's settings
    assert not hasattr(st, 'label_ranking') and not hasattr(st, 'at_k')
    assert 'loss_fn' not in vars(st_plain) and 'tune_thresholds' not in vars(st_plain)
    for bad in ('0', '65', 'a,b'):
        with pytest.raises(SystemExit):
            RT.parse(BASE + ['-at_k', bad])
    assert '-label_ranking' in RT.__doc__ and '-at_k' in RT.__doc__
    assert inspect.signature(RT.save_model).parameters.keys() >= {'opt', 'epoch_i', 'model', 'valid_loss', 'valid_losses'}
