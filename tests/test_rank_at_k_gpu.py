"""Ranking a sample's labels on the MI355X (csrc/rank_at_k.hip): lamp_topk_labels and lamp_rank_at_k through the C ABI and
through lamp_amd.metrics, LAMP.predict_topk and run_eval -at_k.

What is compared, and how closely:
  * the order is defined exactly (include/lamp_hip.h): idx EQUALS the restatement (tests/rank_at_k_common.py) and val is
    BIT-equal to the selected scores; no tolerance;
  * hits_at_rank and n_with_gold are integers: equal;
  * ndcg_sum / recall_sum are fp64 sums of n terms in [0, 1] (error ~ n 2^-53, 3e-13 at n = 3019): within
    1e-12 max(1, sum) of the restatement, bit-equal from run to run;
  * nDCG@k within 1e-12 of what sklearn recorded (tests/golden/rank_at_k.npz).
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

from lamp_amd import _native as N
from lamp_amd import metrics as M

import rank_at_k_common as RK
import redzone_common as RZ

pytestmark = pytest.mark.gpu

# the issue's sizes, and L - 1, L, L + 1 around every L at which lamp_topk_labels changes its kernel: 64, 128, 256, 512 (scores
# per lane of the wave-per-row route), 1024 (-> a workgroup of 4 waves per row), 2048, 4096 (-> 16 waves), 8192, 16384
LS = (1, 2, 63, 64, 65, 90, 127, 128, 129, 159, 255, 256, 257, 511, 512, 513, 983, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096,
      4097, 8191, 8192, 8193, 16383, 16384, 16385, 32768)
NS = (1, 5, 67)
KS = (1, 3, 5, 10, 64)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32))


# ---------------------------------------------------------------------------------------------- the order
@pytest.mark.parametrize('L', LS)
def test_order_equals_the_restatement(dev, L):
    """Every input kind, n in {1, 5, 67}, k in {1, 3, 5, 10, 64} up to L: idx equal, val bit-equal.  L covers one wave per row
    with 1 .. 16 scores per lane, 4 and 16 waves per row, and both sides of every switch (LS above)."""
    kmax = min(64, L)
    for kind in RK.KINDS:
        s = RK.make_scores(kind, max(NS), L)
        ridx, rbits = RK.topk_ref(s, kmax)
        s_d, ridx_d, rbits_d = torch.from_numpy(s).to(dev), torch.from_numpy(ridx).to(dev), _i32(rbits).to(dev)
        for n in NS:
            for k in KS:
                if k > L:
                    continue
                idx, val = M.topk_labels(s_d[:n], k)
                assert idx.dtype == torch.int32 and val.dtype == torch.float32 and idx.shape == val.shape == (n, k)
                assert torch.equal(idx, ridx_d[:n, :k]), (kind, n, k)
                assert torch.equal(val.view(torch.int32), rbits_d[:n, :k]), (kind, n, k)
        only_idx, none = M.topk_labels(s_d, kmax, values=False)
        assert none is None and torch.equal(only_idx, ridx_d)


def test_hand_case(dev):
    nan, inf = float('nan'), float('inf')
    row = torch.tensor([[0.0, -0.0, nan, 1, inf, -inf, 1, nan]], device=dev)
    idx, val = M.topk_labels(row, 8)
    assert idx[0].tolist() == [4, 3, 6, 0, 1, 5, 2, 7]
    assert val.view(torch.int32)[0, 3:5].tolist() == [0, -(1 << 31)]       # +0.0 then -0.0, each with its own bits
    assert M.topk_labels(torch.full((3, 300), 0.25, device=dev), 64)[0].tolist() == [list(range(64))] * 3


# ---------------------------------------------------------------------------------------------- stride, padding, rows
@pytest.mark.parametrize('L', [5, 90, 159, 983, 1025, 4097])
def test_row_stride_and_padding(dev, L):
    """ld = L + 3 with +inf in the padding columns: every index < L and the result bit-equal to the contiguous call."""
    n, k = 67, min(10, L)
    for kind in ('quantised', 'special', 'ascending'):
        s = torch.from_numpy(RK.make_scores(kind, n, L)).to(dev)
        wide = torch.full((n, L + 3), float('inf'), device=dev)
        wide[:, :L] = s
        view = wide[:, :L]
        assert view.stride() == (L + 3, 1)
        idx, val = M.topk_labels(view, k)
        ref_idx, ref_val = M.topk_labels(s, k)
        assert int(idx.max()) < L and int(idx.min()) >= 0
        assert torch.equal(idx, ref_idx) and RZ.bit_equal(val, ref_val)
        assert RZ.bit_equal(wide[:, :L], s) and bool(torch.isinf(wide[:, L:]).all())    # the input is not written


def _c_topk(arena, s, n, L, k, ld=None, ld_idx=None, ld_val=None, with_val=True):
    src = arena.inp(s, 'scores', ld=ld)
    idx = arena.out((n, k), 'idx', dtype=torch.int32, ld=ld_idx)
    val = arena.out((n, k), 'val', ld=ld_val) if with_val else None
    st = N.lib().lamp_topk_labels(arena.ptr(src), ld or L, n, L, k, arena.ptr(idx), ld_idx or k, arena.ptr(val), ld_val or k,
                                  N.stream())
    assert st == 0, st
    arena.check()
    return idx.clone(), (val.clone() if with_val else None)


@pytest.mark.parametrize('L,k', [(7, 7), (90, 5), (159, 64), (983, 10), (1500, 3), (5000, 64)])
def test_exact_buffers_gaps_and_sentinels(dev, L, k):
    """idx and val on exactly-sized red-zoned buffers, contiguous and with ld_idx = k + 2 / ld_val = k + 5 / ld = L + 3: the gaps
    and the zones keep the sentinel, every element is written, the input comes back unchanged, and the result is the same
    bits under both fills."""
    n = 67
    s = torch.from_numpy(RK.make_scores('special', n, L)).to(dev)
    ridx, rbits = RK.topk_ref(s.cpu().numpy(), k)
    got = []
    for fill in RZ.FILLS:
        dense = _c_topk(RZ.Arena(dev, fill), s, n, L, k)
        gaps = _c_topk(RZ.Arena(dev, fill), s, n, L, k, ld=L + 3, ld_idx=k + 2, ld_val=k + 5)
        no_val = _c_topk(RZ.Arena(dev, fill), s, n, L, k, with_val=False)
        assert torch.equal(dense[0], gaps[0]) and RZ.bit_equal(dense[1], gaps[1]) and torch.equal(dense[0], no_val[0])
        got.append(dense)
    assert torch.equal(got[0][0], got[1][0]) and RZ.bit_equal(got[0][1], got[1][1])
    assert torch.equal(got[0][0].cpu(), torch.from_numpy(ridx))
    assert torch.equal(got[0][1].view(torch.int32).cpu(), _i32(rbits))


@pytest.mark.parametrize('L', [90, 983, 2049, 8193])
def test_rows_are_independent(dev, L):
    """Permuted rows give permuted results; a row embedded at another position of a larger batch gives the same bits."""
    n, k = 67, min(64, L)
    s = torch.from_numpy(RK.make_scores('quantised', n, L)).to(dev)
    idx, val = M.topk_labels(s, k)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).to(dev)
    p_idx, p_val = M.topk_labels(s[perm].contiguous(), k)
    assert torch.equal(p_idx, idx[perm]) and RZ.bit_equal(p_val, val[perm])
    big = torch.from_numpy(RK.make_scores('normal', 301, L, seed=9)).to(dev)
    for src_row, at in ((0, 300), (66, 0), (13, 150)):
        big[at] = s[src_row]
    b_idx, b_val = M.topk_labels(big, k)
    for src_row, at in ((0, 300), (66, 0), (13, 150)):
        assert torch.equal(b_idx[at], idx[src_row]) and RZ.bit_equal(b_val[at], val[src_row])
    one_idx, one_val = M.topk_labels(s[13:14], k)
    assert torch.equal(one_idx[0], idx[13]) and RZ.bit_equal(one_val[0], val[13])


def test_runs_on_the_current_stream(dev):
    s = torch.from_numpy(RK.make_scores('normal', 67, 983)).to(dev)
    t = torch.from_numpy(RK.make_targets(67, 983)).to(dev)
    ref = RK.figures_ref(s.cpu().numpy(), t.cpu().numpy(), (1, 5))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        idx, _ = M.topk_labels(s, 5)
        buf = M._rank_at_k_buffer(s, t, 5)
    side.synchronize()
    assert torch.equal(idx.cpu(), torch.from_numpy(RK.topk_ref(s.cpu().numpy(), 5)[0]))
    got = M.rank_at_k_from_sums(buf.cpu().numpy(), 67, 5, (1, 5))
    assert got['P@5'] == ref['P@5'] and got['n_with_gold'] == ref['n_with_gold']


# ---------------------------------------------------------------------------------------------- the figures at k
def _c_rank(arena, idx, t, n, L, k, ld_idx=None, ld_t=None):
    lib = N.lib()
    idx_b = arena.inp(idx, 'idx', ld=ld_idx)
    t_b = arena.inp(t, 'targets', ld=ld_t)
    hits = arena.out((k,), 'hits_at_rank', dtype=torch.int64)
    ndcg = arena.out((k,), 'ndcg_sum', dtype=torch.float64)
    recall = arena.out((k,), 'recall_sum', dtype=torch.float64)
    with_gold = arena.out((1,), 'n_with_gold', dtype=torch.int64)
    nbytes = lib.lamp_rank_at_k_workspace_bytes(n, k)
    assert nbytes > 0
    ws = arena.scratch(nbytes, 'workspace')
    d, ideal = M.dcg_tables(k)
    dp, ip = d.ctypes.data_as(C.POINTER(C.c_double)), ideal.ctypes.data_as(C.POINTER(C.c_double))
    st = lib.lamp_rank_at_k(arena.ptr(idx_b), ld_idx or k, arena.ptr(t_b), ld_t or L, n, L, k, dp, ip, arena.ptr(hits),
                            arena.ptr(ndcg), arena.ptr(recall), arena.ptr(with_gold), arena.ptr(ws), nbytes, N.stream())
    assert st == 0, st
    arena.check()
    return hits.cpu().numpy().copy(), ndcg.cpu().numpy().copy(), recall.cpu().numpy().copy(), int(with_gold.cpu()[0])


def _close(got, ref):
    return bool(np.all(np.abs(got - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref))))


@pytest.mark.parametrize('n,L,k', [(1, 5, 5), (67, 90, 10), (1025, 159, 64), (3019, 90, 5), (3019, 983, 64), (2500, 4097, 3)])
def test_sums_match_the_restatement_on_exact_buffers(dev, n, L, k):
    """Through the C ABI, every buffer (workspace included) exactly sized and red-zoned, contiguous and strided, under both
    fills: integers equal, fp64 sums within 1e-12 max(1, sum), the same bits from run to run and between the fills; the
    integer outputs also under a permutation of the rows.  The targets hold a gold-free and an all-gold row."""
    s = RK.make_scores('quantised', n, L, seed=1)
    t = RK.make_targets(n, L, seed=1)
    idx = RK.topk_ref(s, k)[0]
    r_hits, r_ndcg, r_recall, r_gold = RK.sums_ref(idx, t)
    idx_d, t_d = torch.from_numpy(idx).to(dev), torch.from_numpy(t).to(dev)
    runs = []
    for fill in RZ.FILLS:
        runs.append(_c_rank(RZ.Arena(dev, fill, capacity=64 << 20), idx_d, t_d, n, L, k))
        runs.append(_c_rank(RZ.Arena(dev, fill, capacity=64 << 20), idx_d, t_d, n, L, k, ld_idx=k + 3, ld_t=L + 5))
    hits, ndcg, recall, with_gold = runs[0]
    print('n %d L %d k %d: max |ndcg_sum - ref| %.3e, max |recall_sum - ref| %.3e' %
          (n, L, k, np.abs(ndcg - r_ndcg).max(), np.abs(recall - r_recall).max()))
    assert np.array_equal(hits, r_hits) and with_gold == r_gold
    assert _close(ndcg, r_ndcg) and _close(recall, r_recall)
    for other in runs[1:]:
        assert np.array_equal(other[0], hits) and other[3] == with_gold
        assert np.array_equal(other[1].view(np.int64), ndcg.view(np.int64))
        assert np.array_equal(other[2].view(np.int64), recall.view(np.int64))
    perm = np.random.default_rng(2).permutation(n)
    p = _c_rank(RZ.Arena(dev, RZ.FILL_NAN, capacity=64 << 20), torch.from_numpy(idx[perm]).to(dev),
                torch.from_numpy(t[perm]).to(dev), n, L, k)
    assert np.array_equal(p[0], hits) and p[3] == with_gold and _close(p[1], r_ndcg) and _close(p[2], r_recall)


@pytest.mark.parametrize('kind', ['normal', 'saturated', 'special', 'constant'])
def test_rank_at_k_matches_the_restatement(dev, kind):
    n, L, ks = 300, 159, (1, 3, 5, 10, 64)
    s, t = RK.make_scores(kind, n, L, seed=3), RK.make_targets(n, L, seed=3, density=0.05)
    t[7, ::2] = 2.5                                   # gold is "nonzero", as lamp_threshold_counts has it
    ref = RK.figures_ref(s, t, ks)
    got = M.rank_at_k(torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev), ks)
    assert list(got) == list(ref)
    for key in ref:
        if key.startswith('P@') or key == 'n_with_gold':
            assert got[key] == ref[key], key           # from the integers
        else:
            assert abs(got[key] - ref[key]) <= 1e-12, (key, got[key], ref[key])
    again = M.rank_at_k(torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev), ks)
    assert again == got


def test_the_sklearn_fixture_holds(dev):
    z = RK.fixture()
    s, t = torch.from_numpy(z['scores']).to(dev), torch.from_numpy(z['targets']).to(dev)
    ks = tuple(int(k) for k in z['ks'])
    got = M.rank_at_k(s, t, ks)
    base = M.compute_metrics(s, t, 0.25, all_metrics=False)
    full = M.compute_metrics(s, t, 0.25, all_metrics=False, at_k=ks)
    assert set(full) == set(base) | set(got) and all(full[k] == got[k] for k in got)
    assert all(full[k] == base[k] or (np.isnan(full[k]) and np.isnan(base[k])) for k in base)
    for k in ks:
        print('nDCG@%d: device %.17g, sklearn %.17g' % (k, got['nDCG@%d' % k], float(z['ndcg_%d' % k])))
        assert abs(got['nDCG@%d' % k] - float(z['ndcg_%d' % k])) < 1e-12
    # also from host matrices (uploaded once)
    host = M.compute_metrics(s.cpu(), t.cpu(), 0.25, all_metrics=False, at_k=ks, device=dev)
    assert all(host[k] == got[k] for k in got)


# ---------------------------------------------------------------------------------------------- the model and the runner
def _harness():
    d, sd = load_golden('harness')
    splits = {}
    for name in ('train', 'valid', 'test'):
        splits[name] = {}
        for part in ('src', 'tgt'):
            flat, off = d['%s_%s_flat' % (name, part)], d['%s_%s_off' % (name, part)]
            splits[name][part] = [flat[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
    return d, sd, splits


def _model(d, sd, dev):
    from lamp_amd.Models import LAMP
    L, dm = sd['decoder.tgt_word_emb.weight'].shape
    h = d['n_head']
    m = LAMP(d['src_vocab_size'], L, d['max_token_seq_len_e'], L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h,
             d_word_vec=dm, d_model=dm, d_inner_hid=2 * dm, d_k=dm // h, d_v=dm // h, encoder='graph', decoder='graph',
             label_adj_matrix=d['label_adj_matrix'].clone(), label_mask='prior', dec_dropout2=False)
    m.load_state_dict(sd)
    return m.to(dev), L


def test_predict_topk_on_both_routes(dev):
    from lamp_amd import data as D
    d, sd, splits = _harness()
    seq, pos = D.pad_to_longest(splits['test']['src'][:13])
    src = (seq.to(dev), pos.to(dev))
    results = []
    for fused in (True, False):
        m, L = _model(d, sd, dev)
        m.eval()
        if not fused:
            m._fused = False                       # the module-by-module route, as a model outside the fused launcher takes it
        assert m._fused is fused
        with torch.no_grad():
            logits = m(src, None, None, None)[0]
        for k in (1, 5, min(64, L)):
            probs, labels = m.predict_topk(src, k)
            assert probs.dtype == torch.float32 and labels.dtype == torch.int64 and probs.shape == labels.shape == (13, k)
            ridx = RK.topk_ref(logits.cpu().numpy(), k)[0]
            assert torch.equal(labels.cpu(), torch.from_numpy(ridx).long()), (fused, k)
            assert RZ.bit_equal(probs, torch.sigmoid(torch.gather(logits, 1, labels)))
        m.train()
        t_probs, t_labels = m.predict_topk(src, 5)   # from training mode: the eval forward, and the mode is put back
        assert m.training
        m.eval()
        e_probs, e_labels = m.predict_topk(src, 5)
        assert torch.equal(t_labels, e_labels) and RZ.bit_equal(t_probs, e_probs)
        results.append((logits, e_probs, e_labels))
    if torch.equal(results[0][0], results[1][0]):    # the same logits give the same answer, whichever route made them
        assert torch.equal(results[0][2], results[1][2]) and RZ.bit_equal(results[0][1], results[1][1])
    else:
        assert float((results[0][0] - results[1][0]).abs().max()) < 1e-3


def test_run_eval_at_k_prints_the_figures_of_rank_at_k(dev, tmp_path, capsys):
    """run_eval -at_k 1,3,5 on the synthetic split of the harness fixture: the figures it prints and returns are those of
    rank_at_k on the matrices test_epoch leaves on the device; without the flag the result is what it was."""
    import argparse
    from lamp_amd import data as D
    from lamp_amd import run_eval
    from lamp_amd.evaluate import test_epoch
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
    base = run_eval.main(args)
    capsys.readouterr()
    full = run_eval.main(args + ['-at_k', '1,3,5'])
    printed = capsys.readouterr()
    m, L = _model(d, sd, dev)
    m.eval()
    res = {}
    batches = D.EvalBatcher(splits['test']['src'], splits['test']['tgt'], d['batch_size'])
    test_epoch(m, batches, L, d['batch_size'], dev, device_results=res)
    ref = M.rank_at_k(res['probs'], res['targets'], (1, 3, 5))
    host = RK.figures_ref(res['probs'].cpu().numpy(), res['targets'].cpu().numpy(), (1, 3, 5))
    assert set(full) == set(base) | set(ref) | {'at_k_seconds'} and not any(k in base for k in ref)
    for k in ref:
        assert full[k] == ref[k], k
        assert abs(ref[k] - host[k]) <= 1e-12, k
    line = json.loads(printed.out.strip().splitlines()[-1])
    assert all(line[k] == ref[k] for k in ref)
    for k in ref:
        if k != 'n_with_gold':
            assert '%s %.6f' % (k, ref[k]) in printed.err, k
    for k in ('subset_accuracy', 'micro_f1', 'bce_total', 'n_samples'):
        assert full[k] == base[k] or (np.isnan(full[k]) and np.isnan(base[k])), k
