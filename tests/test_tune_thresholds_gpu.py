"""Fitted decision thresholds on the MI355X (csrc/thresholds.hip): lamp_tune_thresholds and lamp_threshold_counts_vec through
the C ABI and through lamp_amd.metrics, LAMP.predict_labels, run_train -tune_thresholds and run_eval -tune_thresholds.

Everything compared here is exact: integer counts, the bit pattern of the chosen threshold, and fp64 values computed from the
same integers on both sides.  The reference is the python-integer restatement of tests/thresholds_common.py (itself checked
against what sklearn recorded, test_tune_thresholds_cpu.py).  No tolerance anywhere."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

from lamp_amd import _native as N
from lamp_amd import metrics as M

import redzone_common as RZ
import thresholds_common as TH
import train_common as TC

pytestmark = pytest.mark.gpu

# the walk's seams: one row, a lone pair, the wave (64), the 1024-key walk tile, two tiles + 1, four tiles + 4; L around the
# 64 x 64 key tile of the key build
NS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4100)
LS = (1, 3, 65, 130)
KEYS = ('threshold', 'tp', 'fp', 'n_pos', 'n_neg', 'tuned')
FIVE = ('ACC', 'HA', 'ebF1', 'miF1', 'maF1')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def case(n, L, family=None):
    return TH.make_case(n, L, family=family)


@functools.lru_cache(maxsize=None)
def ref(n, L, criterion, family=None):
    return TH.tune_ref(*case(n, L, family), criterion)


def host(res):
    """A tune_thresholds result -> numpy, the threshold as its bit pattern."""
    out = {k: res[k].contiguous().cpu().numpy() for k in KEYS}
    out['threshold'] = out['threshold'].view(np.uint32)
    return out


def assert_same(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, '%s: %s differs at labels %s: got %s, want %s' % (what, k, bad[:5].tolist(), got[k][bad[:5]].tolist(),
                                                                              want[k][bad[:5]].tolist())


def tune(dev, s, t, criterion, **kw):
    return host(M.tune_thresholds(torch.from_numpy(np.ascontiguousarray(s)).to(dev), torch.from_numpy(np.ascontiguousarray(t)).to(dev),
                                  criterion, **kw))


# ---------------------------------------------------------------------------------------------- device vs restatement
@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('n', NS)
def test_device_equals_the_restatement(dev, n, L):
    """All six outputs, the three criteria; column l is of family FAMILIES[(l + n) % 7] (tie-free, seven-valued, constant,
    separable, no positive, no negative, one NaN), so the wide shapes hold an unrankable column among rankable ones."""
    s, t = case(n, L)
    for criterion in TH.CRITERIA:
        assert_same(tune(dev, s, t, criterion), ref(n, L, criterion), '%s n=%d L=%d' % (criterion, n, L))


@pytest.mark.parametrize('family', TH.FAMILIES)
def test_every_score_family_across_two_walk_tiles(dev, family):
    n, L = 2049, 5
    s, t = case(n, L, family)
    for criterion in TH.CRITERIA:
        got = tune(dev, s, t, criterion, fallback=0.375)
        assert_same(got, TH.tune_ref(s, t, criterion, 0.375), '%s %s' % (family, criterion))
        assert got['tuned'].all() == (family != 'unrankable')


def test_radix_route(dev):
    """n = 33000 > 32768: the sort goes through global memory; a tie-free, a seven-valued and a separable column."""
    n = 33000
    rng = np.random.default_rng(33)
    cols = [TH.make_column(f, n, rng) for f in ('tiefree', 'ties7', 'separable')]
    s, t = np.stack([c[0] for c in cols], 1), np.stack([c[1] for c in cols], 1)
    for criterion in TH.CRITERIA:
        assert_same(tune(dev, s, t, criterion), TH.tune_ref(s, t, criterion), 'radix %s' % criterion)


def test_strides_permutations_and_repeats_give_the_same_bits(dev):
    n, L = 1025, 65
    s, t = case(n, L)
    perm = np.random.default_rng(1).permutation(n)
    wide_s = torch.full((n, L + 7), float('nan'), device=dev)       # the padding is never read: NaN there changes nothing
    wide_t = torch.full((n, L + 3), 7.0, device=dev)
    wide_s[:, :L] = torch.from_numpy(s).to(dev)
    wide_t[:, :L] = torch.from_numpy(t).to(dev)
    assert wide_s[:, :L].stride(0) == L + 7
    for criterion in TH.CRITERIA:
        want = ref(n, L, criterion)
        assert_same(tune(dev, s, t, criterion), want, 'first run')
        assert_same(tune(dev, s, t, criterion), want, 'second run')
        assert_same(host(M.tune_thresholds(wide_s[:, :L], wide_t[:, :L], criterion)), want, 'strided')
        assert_same(tune(dev, s[perm], t[perm], criterion), want, 'permuted rows')


# ---------------------------------------------------------------------------------------------- closure with the counts
def test_counts_at_the_tuned_thresholds_reproduce_the_tuner(dev):
    """lamp_threshold_counts_vec at the tuned thresholds gives the tuner's tp and fp for every tuned label, and the F1 from
    those counts is >= the F1 at 0.5 and at every other candidate (exact fractions)."""
    n, L = 1025, 14
    s, t = case(n, L)
    s_d, t_d = torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev)
    at_half = M.threshold_counts(s_d, t_d, 0.5)[0].cpu().numpy()
    for criterion in TH.CRITERIA:
        res = M.tune_thresholds(s_d, t_d, criterion)
        lab, ex = M.threshold_counts(s_d, t_d, res['threshold'])
        got, lab, ex = host(res), lab.cpu().numpy(), ex.cpu().numpy()
        rlab, rex = TH.counts_ref(s, t, got['threshold'].view(np.float32))
        assert np.array_equal(lab, rlab) and np.array_equal(ex, rex)
        ok = got['tuned']
        assert ok.sum() == L - 2
        assert np.array_equal(lab[0][ok], got['tp'][ok]) and np.array_equal(lab[1][ok], got['fp'][ok]), criterion
        assert np.array_equal(lab[2][ok], (got['n_pos'] - got['tp'])[ok])
        if criterion != 'f1':
            continue
        for l in np.nonzero(ok)[0]:
            P = int(got['n_pos'][l])
            best = TH.f1_fraction(int(lab[0][l]), int(lab[1][l]), P)
            assert best >= TH.f1_fraction(int(at_half[0][l]), int(at_half[1][l]), P), l
            _, tp, cnt = TH.candidates(s[:, l], t[:, l])
            assert all(best >= TH.f1_fraction(a, c - a, P) for a, c in zip(tp, cnt)), l
        values = M.tuned_values(res, 'f1')
        for l in range(L):
            want = TH.value_ref('f1', got['tp'][l], got['fp'][l], got['n_pos'][l], got['n_neg'][l]) if ok[l] else float('nan')
            assert values[l] == want or (np.isnan(values[l]) and np.isnan(want)), l


@pytest.mark.parametrize('n,L', [(67, 130), (300, 2049), (70, 4100)])
def test_vec_with_a_constant_vector_equals_the_scalar_entry(dev, n, L):
    """All seven outputs, bit for bit; L crosses the vector kernel's slab of 2048 labels and the scalar kernel's of 4096.
    Thresholds that are +inf and NaN predict nothing."""
    rng = np.random.default_rng(n + L)
    s = rng.random((n, L)).astype(np.float32)
    s[rng.random((n, L)) < 0.02] = np.float32('nan')                # read as 0
    t = (rng.random((n, L)) < 0.1).astype(np.float32)
    s_d, t_d = torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev)
    for thr in (0.5, 0.3, 0.0):
        a = M._counts_buffer(s_d, t_d, thr)
        b = M._counts_buffer(s_d, t_d, torch.full((L,), thr, device=dev))
        assert a.dtype == b.dtype == torch.int32 and torch.equal(a, b), thr
        lab, ex = TH.counts_ref(s, t, thr)
        assert np.array_equal(b[:3 * L].view(3, L).cpu().numpy(), lab) and np.array_equal(b[3 * L:].view(4, n).cpu().numpy(), ex)
    nothing = torch.full((L,), float('inf'), device=dev)
    nothing[1::2] = float('nan')
    lab, ex = M.threshold_counts(s_d, t_d, nothing)
    gold = torch.from_numpy(t != 0)
    assert not lab[0].any() and not lab[1].any() and torch.equal(lab[2].cpu(), gold.sum(0).int())
    assert not ex[0].any() and not ex[1].any() and torch.equal(ex[2].cpu(), gold.sum(1).int()) and torch.equal(ex[3], ex[2])
    mixed = torch.from_numpy(rng.random(L).astype(np.float32)).to(dev)
    mixed[::5] = float('inf')
    lab, ex = M.threshold_counts(s_d, t_d, mixed)
    rlab, rex = TH.counts_ref(s, t, mixed.cpu().numpy())
    assert np.array_equal(lab.cpu().numpy(), rlab) and np.array_equal(ex.cpu().numpy(), rex)


def test_global_scope_equals_the_restatement_on_the_flattened_matrix(dev):
    n, L = 300, 6
    cols = [TH.make_column(f, n, np.random.default_rng(i)) for i, f in enumerate(TH.FAMILIES[:6])]
    s, t = np.stack([c[0] for c in cols], 1), np.stack([c[1] for c in cols], 1)
    for criterion in TH.CRITERIA:
        res = M.tune_thresholds(torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev), criterion, scope='global')
        assert all(tuple(res[k].shape) == (L,) for k in KEYS)
        one = TH.tune_ref(s.reshape(-1, 1), t.reshape(-1, 1), criterion)
        assert_same(host(res), {k: np.repeat(v, L) for k, v in one.items()}, 'global %s' % criterion)
        assert one['tuned'][0] and one['n_pos'][0] + one['n_neg'][0] == n * L
    s2 = s.copy()
    s2[17, 3] = np.float32('nan')                                   # one NaN anywhere: the single flattened column is unrankable
    res = host(M.tune_thresholds(torch.from_numpy(s2).to(dev), torch.from_numpy(t).to(dev), 'f1', fallback=0.25, scope='global'))
    assert not res['tuned'].any() and (res['threshold'].view(np.float32) == 0.25).all() and not res['tp'].any()


# ---------------------------------------------------------------------------------------------- buffer contract
def _arena_tune(dev, fill, s, t, criterion, pad):
    n, L = s.shape
    lib = N.lib()
    arena = RZ.Arena(dev, fill)
    p_d = arena.inp(torch.from_numpy(s), 'probs', ld=L + pad if pad else None)
    t_d = arena.inp(torch.from_numpy(t), 'targets', ld=L + 2 * pad if pad else None)
    thr = arena.out((L,), 'threshold')
    ints = [arena.out((L,), name, dtype=torch.int32) for name in ('tp', 'fp', 'n_pos', 'n_neg', 'tuned')]
    nbytes = lib.lamp_tune_thresholds_workspace_bytes(n, L)
    assert nbytes > 0
    ws = arena.scratch(nbytes, 'workspace')
    with torch.cuda.device(dev):
        N.check(lib.lamp_tune_thresholds(arena.ptr(p_d), L + pad, arena.ptr(t_d), L + 2 * pad, n, L, TH.CRITERION_ID[criterion], 0.5,
                                         arena.ptr(thr), *[arena.ptr(v) for v in ints], arena.ptr(ws), nbytes, N.stream()),
                'lamp_tune_thresholds')
    arena.check()
    out = {'threshold': thr.cpu().numpy().view(np.uint32)}
    out.update({k: v.cpu().numpy() for k, v in zip(('tp', 'fp', 'n_pos', 'n_neg'), ints)})
    out['tuned'] = ints[4].cpu().numpy() != 0
    return out


@pytest.mark.parametrize('n,L,pad', [(1025, 67, 3), (65, 130, 0), (33000, 2, 1)])
def test_tune_stays_inside_exactly_sized_buffers(dev, n, L, pad):
    """Exactly-sized, red-zoned buffers, the workspace of exactly lamp_tune_thresholds_workspace_bytes(), two sentinel fills:
    nothing outside the outputs and the workspace changes, every output element is written, the results are bit-equal between
    the fills and equal to the restatement."""
    s, t = case(n, L)
    for criterion in ('f1', 'balance'):
        outs = [_arena_tune(dev, fill, s, t, criterion, pad) for fill in RZ.FILLS]
        assert_same(outs[0], outs[1], 'between the fills')
        assert_same(outs[0], ref(n, L, criterion), 'against the restatement')


@pytest.mark.parametrize('n,L,pad', [(257, 67, 3), (300, 2100, 0)])
def test_counts_vec_stays_inside_exactly_sized_buffers(dev, n, L, pad):
    rng = np.random.default_rng(L)
    s = rng.random((n, L)).astype(np.float32)
    t = (rng.random((n, L)) < 0.2).astype(np.float32)
    v = rng.random(L).astype(np.float32)
    v[::7] = np.float32('inf')
    lib = N.lib()
    results = []
    for fill in RZ.FILLS:
        arena = RZ.Arena(dev, fill)
        p_d = arena.inp(torch.from_numpy(s), 'probs', ld=L + pad if pad else None)
        t_d = arena.inp(torch.from_numpy(t), 'targets', ld=L + 2 * pad if pad else None)
        v_d = arena.inp(torch.from_numpy(v), 'thresholds')
        lab = [arena.out((L,), name, dtype=torch.int32) for name in ('label_tp', 'label_fp', 'label_fn')]
        ex = [arena.out((n,), name, dtype=torch.int32) for name in ('sample_tp', 'sample_pred', 'sample_gold', 'sample_mismatch')]
        with torch.cuda.device(dev):
            N.check(lib.lamp_threshold_counts_vec(arena.ptr(p_d), L + pad, arena.ptr(t_d), L + 2 * pad, n, L, arena.ptr(v_d),
                                                  *[arena.ptr(x) for x in lab + ex], N.stream()), 'lamp_threshold_counts_vec')
        arena.check()
        results.append((np.stack([x.cpu().numpy() for x in lab]), np.stack([x.cpu().numpy() for x in ex])))
    rlab, rex = TH.counts_ref(s, t, v)
    for lab, ex in results:
        assert np.array_equal(lab, rlab) and np.array_equal(ex, rex)


# ---------------------------------------------------------------------------------------------- model and drivers
def test_predict_labels_agrees_with_the_counts(dev):
    from lamp_amd.Models import LAMP
    torch.manual_seed(4)
    L = 9
    model = LAMP(20, L, 6, L, n_layers_enc=1, n_layers_dec=1, n_head=2, n_head2=2, d_word_vec=16, d_model=16, d_inner_hid=32,
                 d_k=8, d_v=8, encoder='graph', decoder='graph', label_mask='none', dec_dropout2=False).to(dev)
    seq = torch.randint(1, 20, (5, 6), device=dev)
    pos = torch.arange(1, 7, device=dev).repeat(5, 1)
    model.eval()
    with torch.no_grad():
        probs = torch.sigmoid(model.forward((seq, pos), None, None, None)[0])
    model.train()
    targets = (torch.rand(5, L, device=dev) < 0.3).float()
    thr = probs.median(0).values.clone()
    thr[2], thr[5] = float('inf'), float('nan')
    for v in (0.5, thr):
        pred = model.predict_labels((seq, pos), v)
        assert pred.dtype == torch.bool and tuple(pred.shape) == (5, L) and model.training
        lab, ex = M.threshold_counts(probs, targets, v)
        assert torch.equal(pred.sum(1).int(), ex[1]) and torch.equal((pred & (targets != 0)).sum(0).int(), lab[0])
        assert torch.equal(pred, probs >= v)
    assert not pred[:, 2].any() and not pred[:, 5].any() and pred.any()
    with pytest.raises(ValueError):
        model.predict_labels((seq, pos), thr[:4])


def test_run_train_stores_thresholds_and_run_eval_applies_them(monkeypatch):
    from lamp_amd import run_eval, run_train
    with tempfile.TemporaryDirectory(prefix='lamp_thr_') as root:   # (save_model writes nothing under a path that contains 'test')
        assert 'test' not in root
        data_path = os.path.join(root, 'train_valid_data.pt')
        torch.save(TC.synthetic_dataset(n_train=96), data_path)
        args = ['-data', data_path, '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2', '-label_mask', 'prior',
                '-batch_size', '16']
        hist = run_train.main(args + ['-epoch', '2', '-lr', '0.003', '-dropout', '0.0', '-results_dir', os.path.join(root, 'res'),
                                      '-name', 'thr', '-seed', '1', '-tune_thresholds', 'f1'])
        assert '.thr_f1.thr' in hist[1]['checkpoint'] and hist[1]['tune_criterion'] == 'f1'
        ckpt = torch.load(hist[1]['checkpoint'], map_location='cpu', weights_only=False)
        assert sorted(ckpt) == ['epoch', 'label_thresholds', 'model', 'settings', 'tune_criterion']
        thr = ckpt['label_thresholds']
        L = 11
        assert not thr.is_cuda and thr.dtype == torch.float32 and tuple(thr.shape) == (L,) and ckpt['tune_criterion'] == 'f1'
        assert ckpt['settings'].tune_thresholds == 'f1' and 0 < hist[1]['n_labels_tuned'] <= L
        test_m = hist[1]['metrics']['test']
        assert all('tuned_' + k in test_m and k in test_m for k in FIVE) and 'tuned_ACC' not in hist[1]['metrics']['valid']

        seen = []
        real = run_eval.test_epoch

        def recording(*a, **k):
            r = real(*a, **k)
            seen.append((r[0].clone(), r[1].clone()))
            return r

        monkeypatch.setattr(run_eval, 'test_epoch', recording)
        dev = torch.device('cuda', torch.cuda.current_device())
        # the checkpoint's thresholds on the test split: what compute_metrics gives on the same predictions, and what the
        # last training epoch reported
        out = run_eval.main(args + ['-checkpoint', hist[1]['checkpoint'], '-split', 'test', '-tune_thresholds', 'checkpoint'])
        assert len(seen) == 1 and out['tune_criterion'] == 'f1'
        assert np.array_equal(np.asarray(out['thresholds'], dtype=np.float32).view(np.uint32), thr.numpy().view(np.uint32))
        want = M.compute_metrics(seen[0][0].to(dev), seen[0][1].to(dev), 0.0, all_metrics=False, thresholds=thr.to(dev))
        for k in FIVE:
            assert out['tuned_' + k] == want[k] or (np.isnan(out['tuned_' + k]) and np.isnan(want[k])), k
            assert out['tuned_' + k] == test_m['tuned_' + k] or (np.isnan(want[k]) and np.isnan(test_m['tuned_' + k])), k
        # tuned here on the valid split; the fixed-threshold keys are those of a run without the flag
        del seen[:]
        plain = run_eval.main(args + ['-checkpoint', hist[1]['checkpoint'], '-split', 'test'])
        tuned = run_eval.main(args + ['-checkpoint', hist[1]['checkpoint'], '-split', 'test', '-tune_thresholds', 'f1',
                                      '-tune_split', 'valid'])
        assert len(seen) == 3                                        # test;  valid, test
        assert not any(k.startswith('tune') or k == 'thresholds' or k == 'n_labels_tuned' for k in plain)
        for k in plain:
            if k not in ('seconds', 'samples_per_s'):
                assert tuned[k] == plain[k] or (isinstance(plain[k], float) and np.isnan(plain[k]) and np.isnan(tuned[k])), k
        assert tuned['tune_criterion'] == 'f1' and tuned['tune_split'] == 'valid' and tuned['tune_seconds'] > 0
        fit = M.tune_thresholds(seen[1][0].to(dev), seen[1][1].to(dev), 'f1', 0.5)
        assert tuned['n_labels_tuned'] == int(fit['tuned'].sum()) and len(tuned['thresholds']) == L
        assert np.array_equal(np.asarray(tuned['thresholds'], dtype=np.float32).view(np.uint32),
                              fit['threshold'].cpu().numpy().view(np.uint32))
        assert np.array_equal(fit['threshold'].cpu().numpy().view(np.uint32), thr.numpy().view(np.uint32))   # the last epoch's fit
        want = M.compute_metrics(seen[2][0].to(dev), seen[2][1].to(dev), 0.0, all_metrics=False, thresholds=fit['threshold'])
        for k in FIVE:
            assert tuned['tuned_' + k] == want[k] or (np.isnan(tuned['tuned_' + k]) and np.isnan(want[k])), k
        # no thresholds in a checkpoint of a run without the flag: a clear error
        bare = os.path.join(root, 'bare.chkpt')
        torch.save({'model': ckpt['model'], 'settings': ckpt['settings'], 'epoch': 1}, bare)
        with pytest.raises(SystemExit, match='label_thresholds'):
            run_eval.main(args + ['-checkpoint', bare, '-tune_thresholds', 'checkpoint'])
