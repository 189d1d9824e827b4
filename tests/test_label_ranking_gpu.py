"""Label-ranking metrics of whole rows on the MI355X (csrc/rank_at_k.hip: lamp_label_ranking) through the C ABI and through
lamp_amd.metrics, compute_metrics(label_ranking=True), run_eval -label_ranking and run_train -label_ranking -at_k.

What is compared, and how closely (U = 2^-52):
  * the six per-row integers and the five dataset counts are defined exactly (include/lamp_hip.h): EQUAL to the restatement
    (tests/label_ranking_common.py), no tolerance;
  * row_lrap: within (n_p + 2) U relative -- a sum of n_p correctly rounded quotients in [0, 1] (any order: at most n_p - 1
    roundings of partial sums that never exceed the total) and one division, on the device and in the restatement;
  * lrap_sum: within (n + 2) U relative on top of the rows' own bounds; rloss_sum and auc_sum: within (n + 2) U relative (a
    row's rloss and auc are one or two correctly rounded operations on exact integers, the same on both sides);
  * the sklearn record (tests/golden/label_ranking.npz) within 1e-12.
The worst used fraction of the bars is printed by test_rows_match_the_restatement.
"""
import gc
import json
import os
import tempfile

import numpy as np
import pytest
import torch

from conftest import load_golden

from lamp_amd import _native as N
from lamp_amd import metrics as M

import label_ranking_common as LR
import large_extent_common as LX
import rank_at_k_common as RK
import redzone_common as RZ
import train_common as TC

pytestmark = pytest.mark.gpu

# both sides of every route switch that matters to the code (64: one ballot chunk; 1024 -> 4 waves per row; 4096 -> 16 waves),
# the issue's sizes, L = 1 and the largest L
LS = (1, 2, 63, 64, 65, 90, 983, 1024, 1025, 4096, 4097, 32768)
U = LR.U
B32_SHAPE = ((1 << 18) + 293, 4096)     # rows x L x 4 bytes crosses 2^31 and 2^32


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _rows_n(L):
    return 5 if L > 4096 else 67


def _call(dev, s, t, rows=True):
    """-> (sums float64 [3], counts int64 [5], row_counts int64 (n, 6) or None, row_lrap float64 (n,) or None), on the host."""
    buf, rc, rl = M._label_ranking_buffer(s, t, rows=rows)
    buf = buf.cpu().numpy()
    return (buf[:3].copy(), buf[3:].view(np.int64).copy(), None if rc is None else rc.cpu().numpy().astype(np.int64),
            None if rl is None else rl.cpu().numpy())


def _used(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 the values must be equal."""
    got, ref, bound = np.atleast_1d(got), np.atleast_1d(ref), np.atleast_1d(bound)
    err = np.abs(got - ref)
    assert np.all(err[bound == 0] == 0), (got, ref)
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def _compare(got, ref_rows, what):
    """The whole result of one call against the restatement of the same matrices -> the worst used fraction of the bars."""
    sums, counts, rc, rl = got
    ints, lrap, rloss, auc = ref_rows
    n = len(lrap)
    r_sums, r_counts = LR.sums_ref(ints, lrap, rloss, auc)
    assert np.array_equal(rc, ints), (what, np.argwhere(rc != ints)[:5].tolist())
    assert np.array_equal(counts, r_counts), (what, counts, r_counts)
    row_bound = (ints[:, 0] + 2) * U * np.abs(lrap)
    used = [_used(rl, lrap, row_bound),
            _used(sums[0], r_sums[0], row_bound.sum() + (n + 2) * U * abs(r_sums[0])),
            _used(sums[1], r_sums[1], (n + 2) * U * abs(r_sums[1])),
            _used(sums[2], r_sums[2], (n + 2) * U * abs(r_sums[2]))]
    assert max(used) <= 1.0, (what, used)
    return max(used)


# ---------------------------------------------------------------------------------------------- rows and sums
@pytest.mark.parametrize('L', LS)
def test_rows_match_the_restatement(dev, L):
    """Every score kind; targets with an empty, a full, a half-positive row and single positives in the first and the last
    column; n = 67 (5 at L = 32768).  Integers equal, fp64 within the bars of the module docstring."""
    n = _rows_n(L)
    t = LR.make_targets(n, L)
    t_d = torch.from_numpy(t).to(dev)
    worst = 0.0
    for kind in LR.KINDS:
        s = LR.make_scores(kind, n, L)
        got = _call(dev, torch.from_numpy(s).to(dev), t_d)
        worst = max(worst, _compare(got, LR.rows_ref(s, t), (kind, L)))
    print('label ranking L %d n %d: worst used fraction of the fp64 bars %.3f' % (L, n, worst))


def test_hand_cases(dev):
    nan, inf = float('nan'), float('inf')
    s = torch.tensor([[.5, .5, .1], [0.0, -0.0, -1.0], [-inf, nan, nan], [1e-45, -1e-45, 0.0], [.3, .2, .1]], device=dev)
    t = torch.tensor([[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 0]], dtype=torch.float32, device=dev)
    rc, rl = M.label_ranking_rows(s, t)
    assert rc.dtype == torch.int32 and rl.dtype == torch.float64 and rc.shape == (5, 6) and rl.shape == (5,)
    assert rc.tolist() == [[1, 2, 1, 1, 1, 0],      # tied with a negative: it counts against the gold label
                           [1, 2, 1, 1, 1, 0],      # +0.0 and -0.0 are tied
                           [1, 3, 2, 1, 0, 1],      # NaN below -inf, the two NaNs tied
                           [1, 3, 2, 0, 0, 0],      # denormals of opposite sign and zero are three distinct keys
                           [0, 0, 0, 0, 0, 0]]      # an empty row
    assert rl.tolist() == [0.5, 0.5, 1.0 / 3.0, 1.0 / 3.0, 1.0]
    f = M.label_ranking(s[:1], t[:1])
    assert f == {'LRAP': 0.5, 'coverage_error': 2.0, 'ranking_loss': 0.5, 'one_error': 0.0, 'instance_AUC': 0.75,
                 'n_with_gold': 1, 'n_with_both': 1, 'n_rows_with_nan': 0}
    one = M.label_ranking(torch.tensor([[2.0], [nan]], device=dev), torch.tensor([[1.0], [0.0]], device=dev))     # L = 1
    assert one['LRAP'] == 1.0 and one['coverage_error'] == 0.5 and one['ranking_loss'] == 0.0 and one['one_error'] == 0.5
    assert np.isnan(one['instance_AUC']) and one['n_with_both'] == 0 and one['n_rows_with_nan'] == 1


@pytest.mark.parametrize('L', [7, 90, 983, 1025, 4097])
def test_row_stride_and_padding(dev, L):
    """Row strides L + 3 / L + 5 with NaN in the padding of the scores and 1.0 in the padding of the targets: the bits of the
    contiguous call, and the inputs are not written."""
    n = 67
    t = torch.from_numpy(LR.make_targets(n, L)).to(dev)
    for kind in ('quantised', 'special'):
        s = torch.from_numpy(LR.make_scores(kind, n, L)).to(dev)
        wide_s = torch.full((n, L + 3), float('nan'), device=dev)
        wide_t = torch.ones((n, L + 5), device=dev)
        wide_s[:, :L] = s
        wide_t[:, :L] = t
        keep_s, keep_t = wide_s.clone(), wide_t.clone()
        assert wide_s[:, :L].stride() == (L + 3, 1) and wide_t[:, :L].stride() == (L + 5, 1)
        buf, rc, rl = M._label_ranking_buffer(wide_s[:, :L], wide_t[:, :L], rows=True)
        ref_buf, ref_rc, ref_rl = M._label_ranking_buffer(s, t, rows=True)
        assert RZ.bit_equal(buf, ref_buf) and torch.equal(rc, ref_rc) and RZ.bit_equal(rl, ref_rl), (kind, L)
        assert RZ.bit_equal(wide_s, keep_s) and RZ.bit_equal(wide_t, keep_t)


@pytest.mark.parametrize('L', [90, 983, 2049, 8193])
def test_rows_are_independent(dev, L):
    """A row's six integers and lrap bits in a batch of 1 and of 67, from run to run, and at another place of the permuted
    batch; the integer dataset counts under that permutation of the rows."""
    n = 67
    s = torch.from_numpy(LR.make_scores('quantised', n, L)).to(dev)
    t = torch.from_numpy(LR.make_targets(n, L)).to(dev)
    buf, rc, rl = M._label_ranking_buffer(s, t, rows=True)
    buf2, rc2, rl2 = M._label_ranking_buffer(s, t, rows=True)
    assert RZ.bit_equal(buf, buf2) and torch.equal(rc, rc2) and RZ.bit_equal(rl, rl2)
    for i in (0, 1, 3, 13, 66):
        _, one_rc, one_rl = M._label_ranking_buffer(s[i:i + 1], t[i:i + 1], rows=True)
        assert torch.equal(one_rc[0], rc[i]) and RZ.bit_equal(one_rl[0], rl[i]), i
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).to(dev)
    p_buf, p_rc, p_rl = M._label_ranking_buffer(s[perm].contiguous(), t[perm].contiguous(), rows=True)
    assert torch.equal(p_rc, rc[perm]) and RZ.bit_equal(p_rl, rl[perm])
    assert torch.equal(p_buf[3:].view(torch.int64), buf[3:].view(torch.int64))


@pytest.mark.parametrize('n', [1024, 1025, 2500])
def test_chunk_boundaries_of_the_reduction(dev, n):
    L = 7
    s, t = LR.make_scores('quantised', n, L, seed=2), RK.make_targets(n, L, seed=2, density=0.3)
    got = _call(dev, torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev))
    used = _compare(got, LR.rows_ref(s, t), n)
    no_rows = _call(dev, torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev), rows=False)
    assert np.array_equal(no_rows[0].view(np.int64), got[0].view(np.int64)) and np.array_equal(no_rows[1], got[1])
    print('label ranking n %d L %d: used %.3f' % (n, L, used))


@pytest.mark.parametrize('kind', LR.KINDS)
def test_top1_hits_are_the_first_rank_of_rank_at_k(dev, kind):
    for L in (5, 90, 1500, 5000):
        n = 67
        s = torch.from_numpy(LR.make_scores(kind, n, L, seed=4)).to(dev)
        t = torch.from_numpy(LR.make_targets(n, L, seed=4)).to(dev)
        at_k = M._rank_at_k_buffer(s, t, 1).cpu().numpy()
        hits = int(at_k[2:].view(np.int64)[0])
        counts = _call(dev, s, t, rows=False)[1]
        assert int(counts[1]) == hits, (kind, L)
        assert M.label_ranking(s, t)['one_error'] == 1.0 - M.rank_at_k(s, t, (1,))['P@1']


# ---------------------------------------------------------------------------------------------- exact buffers
def _sentinel_free(t, fill):
    words = RZ.bits(t).view(torch.int32)
    return not bool((words == RZ._i32(fill)).any())


def _c_call(arena, fill, s, t, n, L, lds=None, ldt=None, rows=True):
    lib = N.lib()
    s_b = arena.inp(s, 'scores', ld=lds)
    t_b = arena.inp(t, 'targets', ld=ldt)
    sums = arena.out((3,), 'sums', dtype=torch.float64)
    counts = arena.out((5,), 'counts', dtype=torch.int64)
    rc = arena.out((n, 6), 'row_counts', dtype=torch.int32) if rows else None
    rl = arena.out((n,), 'row_lrap', dtype=torch.float64) if rows else None
    nbytes = lib.lamp_label_ranking_workspace_bytes(n, L)
    assert nbytes > 0
    ws = arena.scratch(nbytes, 'workspace')
    st = lib.lamp_label_ranking(arena.ptr(s_b), lds or L, arena.ptr(t_b), ldt or L, n, L, arena.ptr(sums), arena.ptr(counts),
                                arena.ptr(rc), arena.ptr(rl), arena.ptr(ws), nbytes, N.stream())
    assert st == 0, st
    arena.check()          # zones, inputs and paddings unchanged; every int32 output element written
    assert _sentinel_free(counts, fill) and (rl is None or _sentinel_free(rl, fill))     # (the 64-bit outputs: checked here)
    return (sums.cpu().numpy().copy(), counts.cpu().numpy().copy(), None if rc is None else rc.cpu().numpy().astype(np.int64),
            None if rl is None else rl.cpu().numpy().copy())


@pytest.mark.parametrize('n,L', [(1, 1), (67, 7), (67, 90), (1025, 159), (67, 983), (13, 1500), (5, 5000)])
def test_exact_buffers_and_sentinels(dev, n, L):
    """Through the C ABI on exactly-sized red-zoned buffers, the workspace exactly *_workspace_bytes(), contiguous and strided,
    both sentinel fills, the row outputs given and absent: nothing outside the outputs changes, every output element is
    written, and all runs give the same bits, which are the restatement's."""
    s, t = LR.make_scores('special', n, L, seed=1), LR.make_targets(n, L, seed=1)
    s_d, t_d = torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev)
    runs = []
    for fill in RZ.FILLS:
        runs.append(_c_call(RZ.Arena(dev, fill), fill, s_d, t_d, n, L))
        runs.append(_c_call(RZ.Arena(dev, fill), fill, s_d, t_d, n, L, lds=L + 3, ldt=L + 5))
        bare = _c_call(RZ.Arena(dev, fill), fill, s_d, t_d, n, L, rows=False)
        assert np.array_equal(bare[0].view(np.int64), runs[0][0].view(np.int64)) and np.array_equal(bare[1], runs[0][1])
    for other in runs[1:]:
        assert np.array_equal(other[0].view(np.int64), runs[0][0].view(np.int64)) and np.array_equal(other[1], runs[0][1])
        assert np.array_equal(other[2], runs[0][2]) and np.array_equal(other[3].view(np.int64), runs[0][3].view(np.int64))
    _compare(runs[0], LR.rows_ref(s, t), (n, L))


# ---------------------------------------------------------------------------------------------- past 2^32 bytes
def test_label_ranking_across_b32(dev):
    """Row offsets in 64 bits: scores and targets of (2^18 + 293) x 4096 fp32 cross 2^31 and 2^32 bytes.  Periodic operands
    (a row's result depends on the row alone, so the row outputs are bit-periodic); the rows in windows around the
    boundaries equal the restatement, the integer counts are what the periodic fill implies."""
    n, L = B32_SHAPE
    nb = n * L * 4
    assert LX.crossings(nb) == ['B31', 'B32']
    ws_bytes = N.lib().lamp_label_ranking_workspace_bytes(n, L)
    assert ws_bytes > 0
    ops = [('row_counts', n * 24), ('row_lrap', n * 8), ('sums', 24), ('counts', 40), ('workspace', ws_bytes), ('scores', nb),
           ('targets', nb)]
    LX.require_memory(LX.need_bytes(ops))
    P = LX.PERIOD
    sp = np.round(np.random.default_rng(23).standard_normal((P, L)) * 8.0).astype(np.float32) / 8.0     # quantised: ties
    cols = np.arange(L)
    tp = np.stack([((cols + r) % 128 == 0) for r in range(P)]).astype(np.float32)                     # 32 positives per row
    sp[7, ::5] = np.nan
    tp[11, :] = 0.0
    tp[13, :] = 1.0
    ints, lrap, rloss, auc = LR.rows_ref(sp, tp)
    sp_t, tp_t = torch.from_numpy(sp), torch.from_numpy(tp)
    ar = None
    try:
        ar = LX.BigArena(dev, LX.FILL_NAN, ops)
        S, T_ = ar.view('scores', shape=(n, L)), ar.view('targets', shape=(n, L))
        LX.fill_periodic_rows(S, sp_t)
        LX.fill_periodic_rows(T_, tp_t)
        st = N.lib().lamp_label_ranking(ar.ptr('scores'), L, ar.ptr('targets'), L, n, L, ar.ptr('sums'), ar.ptr('counts'),
                                        ar.ptr('row_counts'), ar.ptr('row_lrap'), ar.ptr('workspace'), ws_bytes, N.stream())
        assert st == 0
        ar.check_zones()
        for name in ('row_counts', 'row_lrap', 'sums', 'counts'):
            ar.check_written(name)
        RC, RL = ar.view('row_counts', torch.int32, (n, 6)), ar.view('row_lrap', torch.int32, (n, 2))
        LX.assert_bit_periodic(RC, P, 'row_counts')
        LX.assert_bit_periodic(RL, P, 'row_lrap')
        wins = LX.windows(n, L * 4)
        LX.assert_rows_equal_generator(S, sp_t, wins, 'scores')
        LX.assert_rows_equal_generator(T_, tp_t, wins, 'targets')
        idx = LX.window_rows(wins).numpy() % P
        assert np.array_equal(LX.take_rows(RC, wins).numpy().astype(np.int64), ints[idx])
        got_lrap = LX.take_rows(ar.view('row_lrap', torch.float64, (n, 1)), wins).numpy()[:, 0]
        used = _used(got_lrap, lrap[idx], (ints[idx, 0] + 2) * U * np.abs(lrap[idx]))
        assert used <= 1.0, used
        every = np.arange(n) % P
        r_sums, r_counts = LR.sums_ref(ints[every], lrap[every], rloss[every], auc[every])
        assert np.array_equal(ar.view('counts', torch.int64).cpu().numpy(), r_counts)
        sums = ar.view('sums', torch.float64).cpu().numpy()
        row_bound = ((ints[every, 0] + 2) * U * np.abs(lrap[every])).sum()
        used_sums = [_used(sums[0], r_sums[0], row_bound + (n + 2) * U * abs(r_sums[0])),
                     _used(sums[1], r_sums[1], (n + 2) * U * abs(r_sums[1])), _used(sums[2], r_sums[2], (n + 2) * U * abs(r_sums[2]))]
        assert max(used_sums) <= 1.0, used_sums
        print('large-extent used: lamp_label_ranking rows %.3f sums %.3f' % (used, max(used_sums)))
    finally:
        if ar is not None:
            ar.free()
        del ar
        gc.collect()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- sklearn, compute_metrics
def test_the_sklearn_fixture_holds(dev):
    z = LR.fixture()
    s, t = torch.from_numpy(z['scores']).to(dev), torch.from_numpy(z['targets']).to(dev)
    got = M.label_ranking(s, t)
    for key, name in (('LRAP', 'lrap'), ('coverage_error', 'coverage_error'), ('ranking_loss', 'ranking_loss'),
                      ('instance_AUC', 'instance_auc')):
        print('%s: device %.17g, sklearn %.17g' % (key, got[key], float(z[name])))
        assert abs(got[key] - float(z[name])) < 1e-12, key
    assert got['n_with_both'] == int(z['n_with_both']) and got['n_rows_with_nan'] == 0


def test_compute_metrics_adds_the_keys_and_changes_nothing_else(dev):
    n, L = 300, 159
    s = torch.sigmoid(torch.from_numpy(LR.make_scores('quantised', n, L, seed=3))).to(dev)
    t = torch.from_numpy(LR.make_targets(n, L, seed=3, density=0.05)).to(dev)
    ref = M.label_ranking(s, t)
    host = LR.figures_ref(s.cpu().numpy(), t.cpu().numpy())
    assert list(ref) == list(host) == list(M.LABEL_RANKING_KEYS)
    for key in ref:
        if key.startswith('n_') or key in ('coverage_error', 'one_error'):
            assert ref[key] == host[key], key                      # from the integers
        else:
            assert abs(ref[key] - host[key]) <= 1e-12, key
    base = M.compute_metrics(s, t, 0.25)
    full = M.compute_metrics(s, t, 0.25, label_ranking=True)
    assert list(full) == [k for k in base if k not in ('loss', 'time')] + list(ref) + ['loss', 'time']
    assert all(full[k] == ref[k] for k in ref)
    for k in base:
        a, b = np.asarray(full[k], dtype=np.float64), np.asarray(base[k], dtype=np.float64)
        assert np.array_equal(a, b, equal_nan=True), k
    both = M.compute_metrics(s.cpu(), t.cpu(), 0.25, all_metrics=False, at_k=(1, 3), label_ranking=True, device=dev)
    assert all(both[k] == ref[k] for k in ref) and ref['one_error'] == 1.0 - both['P@1']


# ---------------------------------------------------------------------------------------------- the runners
def _harness():
    d, sd = load_golden('harness')
    splits = {}
    for name in ('train', 'valid', 'test'):
        splits[name] = {}
        for part in ('src', 'tgt'):
            flat, off = d['%s_%s_flat' % (name, part)], d['%s_%s_off' % (name, part)]
            splits[name][part] = [flat[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
    return d, sd, splits


def test_run_eval_label_ranking_prints_the_figures_of_label_ranking(dev, tmp_path, capsys):
    """run_eval -label_ranking on the synthetic split of the harness fixture: the figures it prints and returns are those of
    metrics.label_ranking on the matrices test_epoch leaves on the device; without the flag the result is what it was."""
    import argparse
    from lamp_amd import data as D
    from lamp_amd import run_eval
    from lamp_amd.evaluate import test_epoch
    from lamp_amd.Models import LAMP
    d, sd, splits = _harness()
    src = {('w%d' % i): i for i in range(d['n_src_dict'])}
    tgt = {('l%d' % i): i for i in range(d['n_tgt_dict'])}
    data = {'settings': argparse.Namespace(max_seq_len=d['max_seq_len']), 'dict': {'src': src, 'tgt': tgt}, **splits}
    torch.save(data, tmp_path / 'train_valid_test.pt')
    torch.save({'model': sd, 'epoch': 3}, tmp_path / 'model.chkpt')
    L, dm = sd['decoder.tgt_word_emb.weight'].shape
    h = d['n_head']
    args = ['-data', str(tmp_path / 'train_valid_test.pt'), '-checkpoint', str(tmp_path / 'model.chkpt'), '-d_model', str(dm),
            '-d_inner_hid', str(2 * dm), '-n_layers_enc', '2', '-n_head', str(h), '-label_mask', 'prior',
            '-batch_size', str(d['batch_size'])]
    base = run_eval.main(args)
    capsys.readouterr()
    full = run_eval.main(args + ['-label_ranking'])
    printed = capsys.readouterr()
    m = LAMP(d['src_vocab_size'], L, d['max_token_seq_len_e'], L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h,
             d_word_vec=dm, d_model=dm, d_inner_hid=2 * dm, d_k=dm // h, d_v=dm // h, encoder='graph', decoder='graph',
             label_adj_matrix=d['label_adj_matrix'].clone(), label_mask='prior', dec_dropout2=False)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    res = {}
    batches = D.EvalBatcher(splits['test']['src'], splits['test']['tgt'], d['batch_size'])
    test_epoch(m, batches, L, d['batch_size'], dev, device_results=res)
    ref = M.label_ranking(res['probs'], res['targets'])
    host = LR.figures_ref(res['probs'].cpu().numpy(), res['targets'].cpu().numpy())
    assert set(full) == set(base) | set(ref) | {'label_ranking_seconds'} and not any(k in base for k in ref)
    line = json.loads(printed.out.strip().splitlines()[-1])
    for k in ref:
        same = full[k] == ref[k] or (np.isnan(full[k]) and np.isnan(ref[k]))
        assert same and (line[k] == ref[k] or np.isnan(ref[k])), k
        assert abs(ref[k] - host[k]) <= 1e-12 or np.isnan(host[k]), k
        assert (('%s %d' if k.startswith('n_') else '%s %.6f') % (k, ref[k])) in printed.err, k
    for k in ('subset_accuracy', 'micro_f1', 'bce_total', 'n_samples'):
        assert full[k] == base[k] or (np.isnan(full[k]) and np.isnan(base[k])), k


def test_run_train_reports_label_ranking_and_at_k_for_all_splits():
    from lamp_amd import run_train
    with tempfile.TemporaryDirectory(prefix='lamp_run_') as root:   # (save_model writes nothing under a path that contains 'test')
        assert 'test' not in root
        data_path = os.path.join(root, 'train_valid_data.pt')
        torch.save(TC.synthetic_dataset(n_train=64, n_valid=16, n_test=16), data_path)
        args = ['-data', data_path, '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2', '-label_mask',
                'prior', '-batch_size', '16', '-epoch', '1', '-lr', '0.003', '-dropout', '0.0', '-results_dir',
                os.path.join(root, 'res'), '-seed', '1']
        hist = run_train.main(args + ['-label_ranking', '-at_k', '1,3'])
        assert len(hist) == 1
        record = json.loads(json.dumps(hist[0]))
        extra = set(M.LABEL_RANKING_KEYS) | {'P@1', 'nDCG@1', 'R@1', 'P@3', 'nDCG@3', 'R@3'}
        for split in ('train', 'valid', 'test'):
            got = record['metrics'][split]
            assert extra <= set(got), (split, sorted(extra - set(got)))
            assert 0.0 <= got['LRAP'] <= 1.0 and 0.0 <= got['ranking_loss'] <= 1.0 and got['coverage_error'] >= 0.0
            assert got['one_error'] == 1.0 - got['P@1']
        ckpt = torch.load(hist[0]['checkpoint'], map_location='cpu', weights_only=False)
        assert set(ckpt) == {'model', 'settings', 'epoch'}
        assert not hasattr(ckpt['settings'], 'label_ranking') and not hasattr(ckpt['settings'], 'at_k')
        assert 'label_ranking' not in hist[0]['checkpoint'] and 'at_k' not in hist[0]['checkpoint']
