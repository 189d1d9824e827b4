"""Ranking a sample's labels (top-k, P@k, nDCG@k, R@k) without a GPU: the test-local fp64 restatement
against what sklearn recorded (tests/golden/rank_at_k.npz), hand cases that pin the order, the C ABI's entry points and their
status codes, and the host side of lamp_amd.metrics / Models / run_eval."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from lamp_amd import _native as N
from lamp_amd import metrics as M

import rank_at_k_common as RK

NAMES = ('lamp_topk_labels', 'lamp_rank_at_k_workspace_bytes', 'lamp_rank_at_k')
E_DIMS, E_WORKSPACE, E_UNSUPPORTED, E_NULL = -1, -3, -4, -5


def test_restatement_matches_the_sklearn_record():
    """ndcg_score(ignore_ties=True) is the mean over ALL samples with 0 for a gold-free one: within 1e-12 (two fp64
    evaluations of sums of <= 10 terms, then a mean of 120)."""
    z = RK.fixture()
    scores, targets = z['scores'], z['targets']
    assert scores.shape == (120, 37) and all(len(np.unique(r)) == 37 for r in scores)
    assert (targets.sum(1) == 0).sum() >= 2 and (targets.sum(1) == 37).sum() >= 1
    ks = tuple(int(k) for k in z['ks'])
    assert ks == (1, 3, 5, 10)
    got = RK.figures_ref(scores, targets, ks)
    for k in ks:
        assert abs(got['nDCG@%d' % k] - float(z['ndcg_%d' % k])) < 1e-12, (k, got['nDCG@%d' % k], float(z['ndcg_%d' % k]))
    assert got['n_with_gold'] == int((targets.sum(1) > 0).sum())


def test_hand_cases_pin_the_order():
    nan, inf = float('nan'), float('inf')
    row = np.array([[0.0, -0.0, nan, 1, inf, -inf, 1, nan]], dtype=np.float32)
    assert RK.order_ref(row)[0].tolist() == [4, 3, 6, 0, 1, 5, 2, 7]
    assert RK.order_ref(np.full((1, 9), 0.25, np.float32))[0].tolist() == list(range(9))      # equal scores: columns 0 .. L-1
    assert RK.order_ref(np.full((1, 4), nan, np.float32))[0].tolist() == [0, 1, 2, 3]
    assert RK.order_ref(np.array([[-inf, nan, -3e38]], np.float32))[0].tolist() == [2, 0, 1]  # -inf above every NaN
    assert RK.order_ref(np.array([[1e-45, 0.0, -1e-45, -0.0]], np.float32))[0].tolist() == [0, 1, 3, 2]   # denormals order
    idx, bits = RK.topk_ref(row, 5)
    assert idx.dtype == np.int32 and idx[0].tolist() == [4, 3, 6, 0, 1]
    assert bits[0, 3] == 0x00000000 and bits[0, 4] == 0x80000000          # the selected elements' own bits: -0.0 stays -0.0


def test_hand_case_pins_the_figures():
    # ranks: columns 2, 0, 1; gold {0, 2} -> hits 1 1 0; gold-free second row
    s = np.array([[0.5, 0.1, 0.9], [0.3, 0.2, 0.1]], np.float32)
    t = np.array([[1, 0, 1], [0, 0, 0]], np.float32)
    hits, ndcg, recall, with_gold = RK.sums_ref(RK.topk_ref(s, 3)[0], t)
    d1 = 1.0 / np.log2(3.0)
    assert hits.tolist() == [1, 1, 0] and with_gold == 1
    assert np.allclose(ndcg, [1.0, 1.0, 1.0], atol=1e-15) and np.allclose(recall, [0.5, 1.0, 1.0], atol=1e-15)
    f = RK.figures_ref(s, t, (1, 2, 3))
    assert f['P@1'] == 0.5 and f['P@2'] == 0.5 and f['P@3'] == 2.0 / 6.0 and f['nDCG@3'] == 0.5 and f['R@1'] == 0.25
    # one hit at rank 2 only: nDCG@2 = d_1 / d_0
    hits, ndcg, _, _ = RK.sums_ref(np.array([[1, 0]]), np.array([[1.0, 0.0]], np.float32))
    assert hits.tolist() == [0, 1] and ndcg[0] == 0.0 and abs(ndcg[1] - d1) < 1e-15


def test_generators_cover_what_they_name():
    assert set(RK.KINDS) == {'normal', 'quantised', 'saturated', 'constant', 'ascending', 'descending', 'special'}
    q = RK.make_scores('quantised', 67, 129)
    assert np.array_equal(q * 8, np.round(q * 8)) and len(np.unique(q)) < 80
    sat = RK.make_scores('saturated', 67, 129)
    assert (sat == 0.0).any() and (sat == 1.0).any()
    assert RK.order_ref(RK.make_scores('ascending', 3, 90))[:, 0].tolist() == [89] * 3
    assert RK.order_ref(RK.make_scores('descending', 3, 90))[:, 0].tolist() == [0] * 3
    sp = RK.make_scores('special', 67, 257)
    w = sp.view(np.uint32)
    assert np.isnan(sp[2]).all() and np.isnan(sp[4]).all() and np.isposinf(sp).any() and np.isneginf(sp).any()
    assert (w == 0x80000000).any() and (w == 0).any() and (w == 1).any() and (w == 0x80000001).any()
    t = RK.make_targets(67, 90)
    assert t[1].sum() == 0 and t[3].sum() == 90


def test_header_and_ctypes_table_carry_the_new_entry_points():
    text = open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = N.lib()
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in N.PROTOTYPES and hasattr(lib, name)
    assert 'ranks before' in text and 'ignore_ties=True' in text        # the order and the gold-free rule are written down
    assert lib.lamp_version() == N.ABI_VERSION == 5                     # additive: the ABI version stays


def test_build_lists_the_unit_as_lean():
    from lamp_amd import build
    assert 'rank_at_k.hip' in build.SOURCES and 'rank_at_k.hip' in build.LEAN_UNITS
    rows = build.kernel_resources('rank_at_k.hip')
    assert sum('topk_labels_kernel' in k for k in rows) == 10 and any('rank_rows_kernel' in k for k in rows)
    for name, r in rows.items():
        assert r.get('scratch', 0) == 0 and r.get('agpr', 0) == 0, (name, r)


def _topk(lib, scores=16, ld=90, n=10, L=90, k=5, idx=16, ld_idx=5, val=16, ld_val=5):
    return lib.lamp_topk_labels(scores, ld, n, L, k, idx, ld_idx, val, ld_val, None)


def test_topk_validates_before_any_launch():
    lib = N.lib()
    for bad in (dict(n=0), dict(L=0, ld=0), dict(k=0), dict(n=-1), dict(ld=89), dict(k=91, ld_idx=91, ld_val=91), dict(ld_idx=4),
                dict(ld_val=4)):
        assert _topk(lib, **bad) == E_DIMS, bad
    assert _topk(lib, scores=None) == E_NULL and _topk(lib, idx=None) == E_NULL
    assert _topk(lib, k=65, ld_idx=65, ld_val=65) == E_UNSUPPORTED
    assert _topk(lib, L=32769, ld=32769) == E_UNSUPPORTED
    assert _topk(lib, n=1 << 31) == E_UNSUPPORTED
    # the order of the checks: dimensions, then pointers, then what is not served
    assert _topk(lib, scores=None, ld=89) == E_DIMS
    assert _topk(lib, scores=None, k=65, ld_idx=65, ld_val=65) == E_NULL
    assert _topk(lib, k=65, ld_idx=64) == E_DIMS
    assert _topk(lib, val=None, ld_val=0, scores=None) == E_NULL        # ld_val counts only with val given


def _rank(lib, idx=16, ld_idx=5, targets=16, ld_t=90, n=10, L=90, k=5, tables=True, outs=(16, 16, 16, 16), ws=16, nbytes=1 << 40):
    import ctypes as C
    d, ideal = M.dcg_tables(64)
    dp = d.ctypes.data_as(C.POINTER(C.c_double)) if tables else None
    ip = ideal.ctypes.data_as(C.POINTER(C.c_double)) if tables else None
    return lib.lamp_rank_at_k(idx, ld_idx, targets, ld_t, n, L, k, dp, ip, outs[0], outs[1], outs[2], outs[3], ws, nbytes, None)


def test_rank_at_k_validates_before_any_launch():
    lib = N.lib()
    ws = lib.lamp_rank_at_k_workspace_bytes
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(5, 65) == 0 and ws(1 << 31, 5) == 0
    assert ws(10, 5) >= 10 * 12 + 3 * 5 * 8 + 8 and ws(3019, 5) < ws(3019, 64) and ws(1024, 5) < ws(1025, 5) < ws(100000, 5)
    for bad in (dict(n=0), dict(L=0, ld_t=0), dict(k=0), dict(ld_t=89), dict(k=91, ld_idx=91), dict(ld_idx=4)):
        assert _rank(lib, **bad) == E_DIMS, bad
    for bad in (dict(idx=None), dict(targets=None), dict(tables=False), dict(ws=None), dict(outs=(None, 16, 16, 16)),
                dict(outs=(16, None, 16, 16)), dict(outs=(16, 16, None, 16)), dict(outs=(16, 16, 16, None))):
        assert _rank(lib, **bad) == E_NULL, bad
    assert _rank(lib, k=65, ld_idx=65) == E_UNSUPPORTED
    assert _rank(lib, L=32769, ld_t=32769) == E_UNSUPPORTED
    assert _rank(lib, n=1 << 31) == E_UNSUPPORTED
    assert _rank(lib, nbytes=ws(10, 5) - 1) == E_WORKSPACE              # one byte short: a status code, nothing launched
    assert _rank(lib, idx=None, ld_t=89) == E_DIMS and _rank(lib, idx=None, k=65, ld_idx=65) == E_NULL
    assert _rank(lib, k=65, ld_idx=65, nbytes=0) == E_UNSUPPORTED


def test_dcg_tables_are_the_definition():
    d, ideal = M.dcg_tables(64)
    assert d.dtype == np.float64 and d.shape == (64,) and ideal.shape == (65,)
    assert d[0] == 1.0 and d[2] == 0.5 and ideal[0] == 0.0 and ideal[1] == 1.0
    rd, rideal = RK.dcg_tables(64)
    assert np.array_equal(d, rd) and np.array_equal(ideal, rideal)


def test_figures_from_the_sums():
    k = 3
    buf = np.zeros(3 * k + 1)
    buf[:k] = [4.0, 5.0, 6.0]
    buf[k:2 * k] = [1.0, 2.0, 3.0]
    buf[2 * k:].view(np.int64)[:] = [7, 2, 1, 9]
    out = M.rank_at_k_from_sums(buf, 10, k, (1, 3))
    assert out == {'P@1': 0.7, 'nDCG@1': 0.4, 'R@1': 0.1, 'P@3': 10.0 / 30.0, 'nDCG@3': 0.6, 'R@3': 0.3, 'n_with_gold': 9}
    with pytest.raises(ValueError):
        M._check_ks((1, 65), 100)
    with pytest.raises(ValueError):
        M._check_ks((1, 5), 4)
    with pytest.raises(ValueError):
        M._check_ks((0,), 4)


def test_compute_metrics_without_at_k_is_what_it_was(monkeypatch):
    """The default key set, from the host half alone: the device buffers replaced by host restatements."""
    import inspect
    assert inspect.signature(M.compute_metrics).parameters['at_k'].default is None
    n, L = 12, 7
    rng = np.random.default_rng(3)
    p, t = torch.from_numpy(rng.random((n, L)).astype(np.float32)), torch.from_numpy(RK.make_targets(n, L))
    called = []

    class FakeDev(object):
        """Stands where a device tensor would: .cpu() hands the host buffer over."""
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return torch.from_numpy(self.a)

    def counts(pp, tt, thr):
        pred, gold = (torch.nan_to_num(pp, nan=0.0) >= thr), tt != 0
        lab = torch.stack(((pred & gold).sum(0), (pred & ~gold).sum(0), (~pred & gold).sum(0))).to(torch.int32)
        ex = torch.stack(((pred & gold).sum(1), pred.sum(1), gold.sum(1), (pred != gold).sum(1))).to(torch.int32)
        return FakeDev(torch.cat((lab.reshape(-1), ex.reshape(-1))).numpy())

    def at_k(pp, tt, k):
        called.append(k)
        hits, ndcg, recall, with_gold = RK.sums_ref(RK.topk_ref(pp.numpy(), k)[0], tt.numpy())
        buf = np.zeros(3 * k + 1)
        buf[:k], buf[k:2 * k] = ndcg, recall
        buf[2 * k:].view(np.int64)[:k] = hits
        buf[2 * k:].view(np.int64)[k] = with_gold
        return FakeDev(buf)

    class NoDevice(object):
        def __init__(self, *a):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    monkeypatch.setattr(M, '_counts_buffer', counts)
    monkeypatch.setattr(M, '_rank_at_k_buffer', at_k)
    monkeypatch.setattr(torch.cuda, 'device', NoDevice)
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    base = M.compute_metrics(p, t, 0.5, all_metrics=False)
    assert list(base) == ['ACC', 'HA', 'ebF1', 'miF1', 'maF1'] + list(M.RANKING_KEYS) + ['loss', 'time'] and not called
    full = M.compute_metrics(p, t, 0.5, all_metrics=False, at_k=(1, 3, 5))
    extra = ['P@1', 'nDCG@1', 'R@1', 'P@3', 'nDCG@3', 'R@3', 'P@5', 'nDCG@5', 'R@5', 'n_with_gold']
    assert set(full) == set(base) | set(extra) and called == [5]
    for k in base:
        assert full[k] == base[k] or (np.isnan(full[k]) and np.isnan(base[k])), k
    ref = RK.figures_ref(p.numpy(), t.numpy(), (1, 3, 5))
    assert {k: full[k] for k in extra} == ref


def test_everything_raises_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    s, t = torch.from_numpy(RK.make_scores('normal', 8, 9)), torch.from_numpy(RK.make_targets(8, 9))
    with pytest.raises(RuntimeError, match='HIP device only'):
        M.topk_labels(s, 3)
    with pytest.raises(RuntimeError, match='HIP device only'):
        M.rank_at_k(s, t, (1, 3))
    with pytest.raises(RuntimeError, match='HIP device only'):
        M.compute_metrics(torch.sigmoid(s), t, 0.0, all_metrics=False, at_k=(1, 3))
    from lamp_amd.Models import LAMP
    m = LAMP(20, 9, 6, 9, n_layers_enc=1, n_layers_dec=1, n_head=2, n_head2=2, d_word_vec=16, d_model=16, d_inner_hid=32, d_k=8,
             d_v=8, encoder='graph', decoder='graph', label_mask='none', dec_dropout2=False)
    seq = torch.randint(1, 20, (2, 6))
    pos = torch.arange(1, 7).repeat(2, 1)
    with pytest.raises(RuntimeError, match='HIP device only'):
        m.predict_topk((seq, pos), 3)
    assert m.training                                   # the mode it was in is put back


def test_run_eval_accepts_at_k():
    from lamp_amd import run_eval
    assert run_eval.parse(['-data', 'x.pt']).at_k == ()
    opt = run_eval.parse(['-data', 'x.pt', '-at_k', '1,3,5'])
    assert opt.at_k == (1, 3, 5) and opt.all_metrics is False
    assert run_eval.parse(['-data', 'x.pt', '-at_k', '10', '-all_metrics']).at_k == (10,)
    for bad in ('0', '65', 'a,b'):
        with pytest.raises(SystemExit):
            run_eval.parse(['-data', 'x.pt', '-at_k', bad])
