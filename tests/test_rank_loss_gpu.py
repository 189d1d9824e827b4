"""The ranking losses on the MI355X (lamp_rank_loss_train): the kernels against the fp64 reference of
tests/rank_loss_common.py under the rule of tests/test_train_gpu.py (per element and per row: the larger of one fp32 ulp at the
value and 4 x the gap torch's own fp32 CPU evaluation of the same stable formula shows against fp64 on the same inputs), the
kink rule of the hinge, the probabilities against lamp_bce_logits_train bit for bit, the BCE share, refusals, rows and batches,
placement, a row range past 2^32 bytes, one train_batch through the model against autograd on the fp64 oracle, train_epoch,
and run_train / run_eval end to end."""
import ctypes
import json
import os
import tempfile
import threading

import numpy as np
import pytest
import torch

from conftest import max_abs_diff

from lamp_amd import _native as N
from lamp_amd import optim as O
from lamp_amd import train as T

import large_extent_common as LX
import rank_loss_common as RC
import redzone_common as RZ
import train_common as TC

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BETAS = (0.0, 1.0)


def _same(a, b):
    return RZ.bit_equal(a[0], b[0]) and all(RZ.bit_equal(x, y) for x, y in zip(a[1], b[1])) and RZ.bit_equal(a[2], b[2])


def _margin(kind, margin=None):
    return (1.0 if margin is None else margin) if kind == 'hinge' else 0.0


# ------------------------------------------------------------------ 1. the kernels against fp64
@pytest.mark.parametrize('B,L,n_mats', RC.SHAPES)
@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('kind', RC.KINDS)
def test_rank_kernel_against_fp64(kind, beta, B, L, n_mats):
    logits, weights, targets, margin, (p64, g64, r64), (p32, g32, r32) = RC.reference_case(kind, B, L, n_mats, beta)
    probs, grads, rows = N.rank_loss_train([x.to(DEV) for x in logits], weights, targets.to(DEV), kind, margin, beta)
    torch.cuda.synchronize()
    for a in [probs, rows] + grads:                       # finite inputs, +-1e4 among them: no NaN, no inf anywhere
        assert bool(torch.isfinite(a).all()), kind
    what = '%s beta %g %dx%d x%d' % (kind, beta, B, L, n_mats)
    used = [TC.within(probs, p64, TC.gap(p32, p64), 'probs ' + what),
            TC.within(rows, r64, TC.gap(r32, r64), 'row losses ' + what)]
    for k in range(n_mats):
        used.append(TC.within(grads[k], g64[k], TC.gap(g32[k], g64[k]), 'dlogits[%d] %s' % (k, what)))
    print('%s: worst used fraction of the bar %.3f' % (what, max(used)))


# ------------------------------------------------------------------ 2. the kink of the hinge
def test_hinge_pairs_on_the_kink_are_inactive():
    """Logits on the 2^-10 grid and margin 1: a pair with x_n - x_p = -1 exactly has a_pn = 0 and contributes nothing, neither to
    the loss nor to a gradient.  Everything here is exact in fp32 up to the one division by n_p n_n, so the bar against fp64
    is one fp32 ulp (train_common.within with a zero gap)."""
    L = 12
    x = torch.tensor([[2.0] * 3 + [1.0] * 9,                                   # every pair on the kink
                      [2.0, 2.0, 2.0, 1.0, 1.0, 1.0 + RC.GRID, 1.0 - RC.GRID, 0.0, 3.0, 1.0, 1.0, 1.0],
                      [0.5, 1.5, -0.25, -0.5, 0.5, 1.5, 2.5, -1.5, 0.5 - RC.GRID, 0.5 + RC.GRID, 7.0, -7.0]])
    t = torch.zeros(3, L)
    t[:, :3] = 1.0
    B = x.size(0)
    probs, (g,), rows = N.rank_loss_train([x.to(DEV)], [1.0], t.to(DEV), 'hinge', 1.0)
    torch.cuda.synchronize()
    assert float(rows[0, 0]) == 0.0 and not bool(g[0].any())
    # row 1: of its 27 pairs only those of the negatives 1 + 2^-10 (a = 2^-10) and 3 (a = 2) are active
    want_loss, want = (3 * RC.GRID + 3 * 2.0) / 27.0, torch.zeros(L, dtype=torch.float64)
    want[:3] = -2.0 / 27.0 / B
    want[5] = want[8] = 3.0 / 27.0 / B
    assert abs(float(rows[0, 1]) - want_loss) <= float(TC.ulp32(torch.tensor(want_loss)))
    assert torch.equal(g[1].cpu() == 0, want == 0)                    # the negatives on the kink: exactly nothing
    TC.within(g[1], want, 0.0, 'kink: row 1 by hand')
    p64, g64, r64 = RC.rank_reference([x], [1.0], t, 'hinge', 1.0, 0.0, torch.float64)
    TC.within(rows, r64, 0.0, 'kink: row losses')
    TC.within(g, g64[0], 0.0, 'kink: dlogits')


# ------------------------------------------------------------------ 3. the probabilities
def test_probabilities_are_bce_logits_trains_bits_for_every_kind_and_beta():
    for B, L, n_mats in ((7, 65, 3), (9, 983, 2)):
        logits, weights, targets, _ = RC.rank_case(B, L, n_mats, 'lsep', seed=3)
        xd, td = [x.to(DEV) for x in logits], targets.to(DEV)
        bce = N.bce_logits_train(xd, weights, td)
        for kind in RC.KINDS:
            for beta in (0.0, 1.0, 0.3):
                p, g, r = N.rank_loss_train(xd, weights, td, kind, _margin(kind), beta)
                assert RZ.bit_equal(p, bce[0]), (kind, beta, L)
                assert not torch.equal(r, bce[2]) and not torch.equal(g[0], bce[1][0]), (kind, beta, L)   # ... another objective


# ------------------------------------------------------------------ 4. the BCE share
@pytest.mark.parametrize('kind', RC.KINDS)
def test_beta_zero_is_the_ranking_term_alone_and_beta_adds_the_mean_bce(kind):
    """At beta = 0 rows without a pair have a zero loss and zero gradients: nothing of the BCE leaks in.  row_loss(beta = 1) -
    row_loss(beta = 0) is bce_row / L up to the roundings it inherits: both operands are one rounding each of a sum taken in
    double (half an ulp each), and the BCE share itself gets the rule's bar -- max(1 ulp, 4 x torch's fp32 gap) on bce_row / L
    in fp64 and fp32.  The same for the gradients with (sigmoid(x) - t) w_k / (B L)."""
    B, L, n_mats = 9, 983, 2
    logits, weights, targets, margin = RC.rank_case(B, L, n_mats, kind, seed=B * 1000 + L)
    xd, td = [x.to(DEV) for x in logits], targets.to(DEV)
    p0, g0, r0 = N.rank_loss_train(xd, weights, td, kind, margin, 0.0)
    p1, g1, r1 = N.rank_loss_train(xd, weights, td, kind, margin, 1.0)
    torch.cuda.synchronize()
    for r in (0, B - 1):                                  # the all-zero and the all-one row
        assert not bool(r0[:, r].any()) and not any(bool(g[r].any()) for g in g0), r
    _, _, ref0 = RC.rank_reference(logits, weights, targets, kind, margin, 0.0)
    TC.within(r0, ref0, TC.gap(RC.rank_reference(logits, weights, targets, kind, margin, 0.0, torch.float32)[2], ref0),
              '%s beta 0 row losses' % kind)
    _, gb64, rb64 = TC.bce_reference(logits, weights, targets, torch.float64)
    _, gb32, rb32 = TC.bce_reference(logits, weights, targets, torch.float32)
    share64, share32 = rb64 / L, (rb32 / L).double()
    inherited = 0.5 * (TC.ulp32(r1) + TC.ulp32(r0))
    bar = torch.maximum(TC.ulp32(share64), torch.full_like(share64, 4.0 * TC.gap(share32, share64))) + inherited
    err = ((r1.cpu().double() - r0.cpu().double()) - share64).abs()
    print('%s: BCE share of the row losses: worst err / bar %.3f' % (kind, float((err / bar).max())))
    assert bool((err <= bar).all())
    for k in range(n_mats):                               # bce_reference's gradients carry 1 / (B L): the share's own factor
        inherited = 0.5 * (TC.ulp32(g1[k]) + TC.ulp32(g0[k]))
        bar = torch.maximum(TC.ulp32(gb64[k]), torch.full_like(gb64[k], 4.0 * TC.gap(gb32[k], gb64[k]))) + inherited
        err = ((g1[k].cpu().double() - g0[k].cpu().double()) - gb64[k]).abs()
        print('%s: BCE share of dlogits[%d]: worst err / bar %.3f' % (kind, k, float((err / bar).max())))
        assert bool((err <= bar).all())


# ------------------------------------------------------------------ 5. refusals
SENTINEL = -7.0


def _raw(xs, weights, t, opts, L=None, n_rows=None):
    """lamp_rank_loss_train through ctypes with `opts` as given (None = a NULL pointer) -> (status, probs, grads, rows)."""
    n, (B, width) = len(xs), xs[0].shape
    probs = torch.full((B, width), SENTINEL, device=DEV)
    grads = [torch.full((B, width), SENTINEL, device=DEV) for _ in xs]
    rows = torch.full((n, B), SENTINEL, device=DEV)
    xp = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
    gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
    wp = (ctypes.c_float * n)(*weights)
    st = N.lib().lamp_rank_loss_train(xp, wp, gp, n, t.data_ptr(), B if n_rows is None else n_rows, width if L is None else L,
                                      N.ptr(probs), width, rows.data_ptr(), B, None if opts is None else ctypes.byref(opts),
                                      N.stream())
    torch.cuda.synchronize()
    return st, probs, grads, rows


def test_refusals_come_before_any_launch_in_the_house_order():
    B, L = 3, 20
    logits, weights, targets, _ = RC.rank_case(B, L, 1, 'lsep', seed=2)
    xd, td = [logits[0].to(DEV)], targets.to(DEV)
    E_DIMS, E_UNSUPPORTED, E_NULL = -1, -4, -5
    nan, inf = float('nan'), float('inf')

    def untouched(out):
        return all(bool((a == SENTINEL).all()) for a in [out[0], out[2]] + out[1])

    for opts in (N.RankLossOptions(0, 0, 0, 0), N.RankLossOptions(4, 0, 0, 0), N.RankLossOptions(-1, 0, 0, 0),
                 N.RankLossOptions(2, -1.0, 0, 0), N.RankLossOptions(2, nan, 0, 0), N.RankLossOptions(2, inf, 0, 0),
                 N.RankLossOptions(1, 0, -0.5, 0), N.RankLossOptions(3, 0, nan, 0), N.RankLossOptions(2, 1.0, inf, 0),
                 N.RankLossOptions(1, 1.0, 0, 0), N.RankLossOptions(3, 0.5, 0, 0),          # a margin outside HINGE
                 N.RankLossOptions(1, 0, 0, 1), N.RankLossOptions(2, 1.0, 1.0, 7)):
        st, *out = _raw(xd, weights, td, opts)
        assert st == E_UNSUPPORTED and untouched(out), (opts.kind, opts.margin, opts.bce_weight, opts.reserved)
    st, *out = _raw(xd, weights, td, None)                                            # opts == NULL
    assert st == E_NULL and untouched(out)
    bad, good = N.RankLossOptions(9, 0, 0, 0), N.RankLossOptions(1, 0, 0, 0)
    lib, s = N.lib(), N.stream()
    xp, wp = (ctypes.c_void_p * 1)(xd[0].data_ptr()), (ctypes.c_float * 1)(1.0)
    # a bad size before a missing pointer before a parameter that is not served
    assert lib.lamp_rank_loss_train(xp, wp, None, 1, None, 0, L, None, L, None, B, ctypes.byref(bad), s) == E_DIMS
    assert lib.lamp_rank_loss_train(xp, wp, None, 1, None, B, 0, None, L, None, B, None, s) == E_DIMS
    assert lib.lamp_rank_loss_train(xp, wp, None, 1, td.data_ptr(), B, L, td.data_ptr(), L - 1, None, B, None, s) == E_DIMS
    assert lib.lamp_rank_loss_train(xp, wp, None, 1, None, B, L, None, L, None, B, ctypes.byref(bad), s) == E_NULL
    assert lib.lamp_rank_loss_train(xp, wp, None, 1, td.data_ptr(), B, L, None, L, None, B, None, s) == E_NULL
    assert lib.lamp_rank_loss_train(xp, wp, None, 1, td.data_ptr(), B, L, None, L, None, B, ctypes.byref(bad), s) == E_UNSUPPORTED
    assert lib.lamp_rank_loss_train(xp, wp, None, 1, td.data_ptr(), B, L, None, L, None, B, ctypes.byref(good), s) == 0
    nine = [xd[0]] * 9
    st, *out = _raw(nine, [1.0] * 9, td, good)
    assert st == E_UNSUPPORTED and untouched(out)                                     # 9 matrices: the entry point takes 8
    with pytest.raises(ValueError):
        N.rank_loss_train(nine, [1.0] * 9, td, 'lsep')
    # L > 4096: refused for the two pair kinds (the buffers are never read: the claim alone decides), served for LSEP
    wide_x, wide_t = torch.zeros(1, 4097, device=DEV), torch.zeros(1, 4097, device=DEV)
    for kind in (2, 3):
        st, *out = _raw([wide_x], [1.0], wide_t, N.RankLossOptions(kind, 0, 0, 0))
        assert st == E_UNSUPPORTED and untouched(out), kind
    wide_t[0, 5] = 1.0
    wide_x[0, 5] = 2.0
    st, probs, grads, rows = _raw([wide_x], [1.0], wide_t, good)
    assert st == 0 and not untouched((probs, grads, rows))
    want = RC.rank_reference([wide_x.cpu()], [1.0], wide_t.cpu(), 'lsep')
    want32 = RC.rank_reference([wide_x.cpu()], [1.0], wide_t.cpu(), 'lsep', dtype=torch.float32)
    TC.within(rows, want[2], TC.gap(want32[2], want[2]), 'LSEP at L = 4097: row loss')
    TC.within(grads[0], want[1][0], TC.gap(want32[1][0], want[1][0]), 'LSEP at L = 4097: dlogits')
    with pytest.raises(ValueError):
        N.rank_loss_train([wide_x], [1.0], wide_t, 'hinge', 1.0)


# ------------------------------------------------------------------ 6. rows and batches
@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('kind', RC.KINDS)
def test_rows_do_not_depend_on_their_batch_and_nan_stays_in_its_row(kind, beta):
    B, L = 32, 159
    logits, weights, targets, margin = RC.rank_case(B, L, 3, kind, seed=5)
    targets[7, :80] = 1.0                                 # a dense row among the sparse ones
    targets[3, 10] = 1.0                                  # (row 3 has both classes whatever the draw)
    xd, td = [x.to(DEV) for x in logits], targets.to(DEV)
    probs, grads, rows = N.rank_loss_train(xd, weights, td, kind, margin, beta)
    assert _same(N.rank_loss_train(xd, weights, td, kind, margin, beta), (probs, grads, rows))     # run to run
    for lo, hi in ((4, 8), (0, 4), (28, 32), (0, 16), (5, 12), (31, 32)):
        # the gradient carries 1 / B of the batch the mean is taken over: the same factor through the weights (exact where
        # B / (hi - lo) is a power of two; otherwise probabilities and losses only)
        scale = (hi - lo) / float(B)
        p, g, r = N.rank_loss_train([x[lo:hi] for x in xd], [w * scale for w in weights], td[lo:hi], kind, margin, beta)
        assert RZ.bit_equal(p, probs[lo:hi]) and RZ.bit_equal(r, rows[:, lo:hi].contiguous()), (lo, hi)
        if (hi - lo) & (hi - lo - 1) == 0:
            assert all(RZ.bit_equal(a, b[lo:hi]) for a, b in zip(g, grads)), (lo, hi)
    bad = [x.clone() for x in xd]
    bad[0][3, 7] = float('nan')                           # (row 3: both classes)
    bad[2][9, 0] = float('nan')
    p, g, r = N.rank_loss_train(bad, weights, td, kind, margin, beta)
    torch.cuda.synchronize()
    assert torch.isnan(p[3, 7]) and int(torch.isnan(p).sum()) == 1                    # probs: its own element
    assert torch.isnan(r[0, 3]) and torch.isnan(r[2, 9]) and int(torch.isnan(r).sum()) == 2
    assert bool(torch.isnan(g[0][3]).all()) and bool(torch.isnan(g[2][9]).all())      # the row's loss and all its gradients
    assert int(torch.isnan(g[0]).sum()) == L and int(torch.isnan(g[2]).sum()) == L and not bool(torch.isnan(g[1]).any())
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[3] = False
    assert RZ.bit_equal(p[keep], probs[keep]) and RZ.bit_equal(r[0][keep], rows[0][keep]) and RZ.bit_equal(g[0][keep], grads[0][keep])
    assert RZ.bit_equal(r[1], rows[1]) and RZ.bit_equal(g[1], grads[1])
    keep[3], keep[9] = True, False
    assert RZ.bit_equal(r[2][keep], rows[2][keep]) and RZ.bit_equal(g[2][keep], grads[2][keep])


# ------------------------------------------------------------------ 7. placement
@pytest.mark.parametrize('fill', RZ.FILLS)
@pytest.mark.parametrize('kind', RC.KINDS)
def test_outputs_stay_inside_exactly_sized_buffers(kind, fill):
    B, L, n = 13, 37, 2
    logits, weights, targets, margin = RC.rank_case(B, L, n, kind, seed=9)
    want = N.rank_loss_train([x.to(DEV) for x in logits], weights, targets.to(DEV), kind, margin, 1.0)
    ar = RZ.Arena(DEV, fill, capacity=4 << 20)
    xs = [ar.inp(x, 'logits%d' % k) for k, x in enumerate(logits)]
    t = ar.inp(targets, 'targets')
    gs = [ar.out((B, L), 'dlogits%d' % k) for k in range(n)]
    probs = ar.out((B, L), 'probs', ld=L + 3)
    rows = ar.out((n, B), 'row_loss', ld=B + 11)
    xp = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
    gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in gs])
    wp = (ctypes.c_float * n)(*weights)
    opts = N.RankLossOptions(N.RANK_KINDS[kind], margin, 1.0, 0)
    st = N.lib().lamp_rank_loss_train(xp, wp, gp, n, t.data_ptr(), B, L, probs.data_ptr(), L + 3, rows.data_ptr(), B + 11,
                                      ctypes.byref(opts), N.stream())
    assert st == 0
    ar.check()
    assert RZ.bit_equal(probs.contiguous(), want[0]) and RZ.bit_equal(rows.contiguous(), want[2])
    assert all(RZ.bit_equal(a, b) for a, b in zip(gs, want[1]))


def test_wrapper_places_strided_outputs_and_serves_loss_only_calls():
    B, L = 13, 37
    logits, weights, targets, margin = RC.rank_case(B, L, 2, 'logistic', seed=9)
    xd, td = [x.to(DEV) for x in logits], targets.to(DEV)
    want = N.rank_loss_train(xd, weights, td, 'logistic', 0.0, 0.5)
    guard = 12345.0
    big = torch.full((B + 9, L + 3), guard, device=DEV)
    loss = torch.full((2, B + 11), guard, device=DEV)
    N.rank_loss_train(xd, weights, td, 'logistic', 0.0, 0.5, probs_out=big[4:4 + B, :L], row_loss_out=loss[:, 6:6 + B])
    torch.cuda.synchronize()
    assert torch.equal(big[4:4 + B, :L], want[0]) and torch.equal(loss[:, 6:6 + B], want[2])
    big[4:4 + B, :L] = guard
    loss[:, 6:6 + B] = guard
    assert bool((big == guard).all()) and bool((loss == guard).all())
    for kind in RC.KINDS:
        full = N.rank_loss_train(xd, weights, td, kind, _margin(kind), 0.5)
        p, g, r = N.rank_loss_train(xd, weights, td, kind, _margin(kind), 0.5, want_grads=False, want_probs=False)
        assert p is None and g is None and RZ.bit_equal(r, full[2]), kind


# ------------------------------------------------------------------ 8. a row range past 2^32 bytes
RANK_B32 = ((1 << 18) + 2 * LX.WINDOW + 37, 4096)        # n * L * 4 crosses 2^32 at row 2^18


@pytest.mark.parametrize('kind', ['lsep', 'hinge'])
def test_rank_loss_across_b32(kind):
    """Row offsets in 64 bits: logits, targets and gradients of (2^18 + 293) x 4096 fp32 cross 2^31 and 2^32 bytes.  Periodic
    operands (the order of every sum is fixed by L and the row's own targets, so the outputs are bit-periodic); rows in
    windows around the boundaries against fp64 under the rule of test 1.  Sparse periodic targets: every 128th column, the
    phase moving with the row, 32 positives per row -- 32 x 4064 pairs."""
    import gc
    n, L = RANK_B32
    nb = n * L * 4
    assert LX.crossings(nb) == ['B31', 'B32']
    ops = [('row_loss', n * 4), ('logits', nb), ('targets', nb), ('dlogits', nb)]
    need = LX.need_bytes(ops)
    LX.require_memory(need)
    g = torch.Generator().manual_seed(23)
    P = LX.PERIOD
    xp = torch.randn(P, L, generator=g) * 4.0
    margin = 0.0
    if kind == 'hinge':
        xp = torch.round(xp / RC.GRID) * RC.GRID
        margin = RC.HINGE_MARGIN
    tp = torch.zeros(P, L)
    cols = torch.arange(L)
    for r in range(P):
        tp[r] = ((cols + r) % 128 == 0).float()
    ar = None
    try:
        ar = LX.BigArena(DEV, LX.FILL_NAN, ops)
        X, T_ = ar.view('logits', shape=(n, L)), ar.view('targets', shape=(n, L))
        LX.fill_periodic_rows(X, xp)
        LX.fill_periodic_rows(T_, tp)
        xs = (ctypes.c_void_p * 1)(ar.ptr('logits'))
        gs = (ctypes.c_void_p * 1)(ar.ptr('dlogits'))
        ws = (ctypes.c_float * 1)(1.0)
        opts = N.RankLossOptions(N.RANK_KINDS[kind], margin, 1.0, 0)
        st = N.lib().lamp_rank_loss_train(xs, ws, gs, 1, ar.ptr('targets'), n, L, None, L, ar.ptr('row_loss'), n,
                                          ctypes.byref(opts), N.stream())
        assert st == 0
        ar.check_zones()
        for name in ('dlogits', 'row_loss'):
            ar.check_written(name)
        D, R = ar.view('dlogits', shape=(n, L)), ar.view('row_loss', shape=(n, 1))
        LX.assert_bit_periodic(D, P, 'dlogits')
        LX.assert_bit_periodic(R, P, 'row_loss')
        wins = LX.windows(n, L * 4)
        LX.assert_rows_equal_generator(X, xp, wins, 'logits')
        LX.assert_rows_equal_generator(T_, tp, wins, 'targets')
        idx = LX.window_rows(wins)
        xw, tw = LX.periodic_rows(xp, idx), LX.periodic_rows(tp, idx)
        if kind == 'hinge':
            RC.assert_hinge_inputs([xw], tw, margin)
        wgt = [float(len(idx)) / n]      # the reference takes the mean over the rows it is given: the gradient's 1 / n
        _, g64, r64 = RC.rank_reference([xw], wgt, tw, kind, margin, 1.0, torch.float64)
        _, g32, r32 = RC.rank_reference([xw], wgt, tw, kind, margin, 1.0, torch.float32)
        frac = [TC.within(LX.take_rows(D, wins), g64[0], TC.gap(g32[0], g64[0]), 'lamp_rank_loss_train %s dlogits' % kind),
                TC.within(LX.take_rows(R, wins).view(1, -1), r64, TC.gap(r32, r64), 'lamp_rank_loss_train %s row losses' % kind)]
        print('large-extent used: lamp_rank_loss_train %s: %.3f' % (kind, max(frac)))
    finally:
        if ar is not None:
            ar.free()
        del ar
        gc.collect()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 9. through the model
def _batch0(fx):
    from lamp_amd.data import get_gold_binary
    data = T.TrainBatcher(fx['src'], fx['tgt'], int(fx['batch_size']), shuffle=False, drop_last=False)
    (seq, pos), _, tgt = data.batch(0)
    return seq, pos, get_gold_binary(tgt[:, 1:], int(fx['tgt_vocab_size']))


def test_train_batch_with_lsep_bce_and_int_preds_against_the_fp64_oracle():
    """One train_batch (LSEP + 1 x mean BCE, -int_preds, dropout 0) on the tiny training model: every parameter's gradient
    against torch.autograd on the fp64 oracle with the fp64 loss.  Tolerance: the rule of tests/test_train_gpu.py's training
    comparisons, max(1e-4, 3 x the oracle's own fp32-vs-fp64 gap) -- the gap taken here from the oracle run in fp32."""
    from oracle import lamp_ref as R
    fx = TC.load_fixture()
    L, h = int(fx['tgt_vocab_size']), int(fx['n_head'])
    seq, pos, gold = _batch0(fx)
    B = gold.size(0)
    is_pos = gold > 0.5
    blocked = R.label_block_mask(torch.from_numpy(fx['label_adj_matrix']), 'prior', L)
    weights = T._loss_weights(4, 0.2)

    def oracle(dtype):
        sd = {k: (v.detach().clone().to(dtype).requires_grad_(True) if v.is_floating_point() else v) for k, v in fx['sd'].items()}
        # lamp_ref.forward with int_preds, but the intermediates read out through a DETACHED copy of the read-out weight, as
        # the model does (the reference deep-copies the projection for them: no gradient reaches the weight from there)
        enc, _ = R.encoder_forward(sd, seq, pos, h)
        y, _, _, int_outs = R.decoder_forward(sd, seq, enc, blocked, h, int_preds=True)
        w_out = sd['tgt_word_proj.linear.weight']
        logits = R.readout(y, w_out).reshape(-1, L)
        mats = [logits] + [R.readout(o, w_out.detach()) for o in int_outs[:-1]]
        assert len(mats) == 4
        total = 0.0
        for x, w in zip(mats, weights):
            row = torch.stack([RC.rank_row(x[r], is_pos[r], 'lsep', 0.0) for r in range(B)])
            row = row + RC.bce_elements(x, gold.to(dtype)).sum(1) / L
            total = total + w * row.mean()
        total.backward()
        return sd, logits.detach()

    sd64, logits64 = oracle(torch.float64)
    sd32, _ = oracle(torch.float32)
    torch.manual_seed(0)
    model = TC.fixture_model(fx, int_preds=True).to(DEV)
    model.train()
    opt = TC.train_opt(L, int_preds=True)
    opt.rank_loss = T.RankLossOptions('lsep', bce_weight=1.0)
    probs, rows = torch.zeros(B, L, device=DEV), torch.zeros(4, B, device=DEV)
    sgd = torch.optim.SGD(list(model.get_trainable_parameters()), lr=0.0)            # (a step that moves nothing)
    T.train_batch(model, sgd, opt, (seq.to(DEV), pos.to(DEV)), None, gold.to(DEV), probs, rows)
    torch.cuda.synchronize()
    assert max_abs_diff(probs, torch.sigmoid(logits64)) < 1e-4
    plain = TC.fixture_model(fx, int_preds=True).to(DEV)
    plain.train()
    T.train_batch(plain, torch.optim.SGD(list(plain.get_trainable_parameters()), lr=0.0), TC.train_opt(L, int_preds=True),
                  (seq.to(DEV), pos.to(DEV)), None, gold.to(DEV), torch.zeros_like(probs), torch.zeros_like(rows))
    bce_grads = dict((k, p.grad) for k, p in plain.named_parameters())
    aliases = {}                                   # a shared weight collects the oracle's gradients of every name it has
    for key, v in model.state_dict(keep_vars=True).items():
        aliases.setdefault(id(v), []).append(key)
    checked, worst, moved = 0, 0.0, 0.0
    for pname, p in model.named_parameters():
        keys = [k for k in aliases[id(p)] if k in sd64 and sd64[k].grad is not None]
        if p.grad is None:                         # the frozen table, the reference's dead code (the unused projection copy)
            assert not keys or pname == 'encoder.position_enc.weight', pname
            continue
        ref = sum(sd64[k].grad for k in keys) if keys else None
        ref32 = sum(sd32[k].grad for k in keys) if keys else None
        assert ref is not None, pname
        tol = max(1e-4, 3.0 * TC.gap(ref32, ref))
        err = max_abs_diff(p.grad, ref)
        worst = max(worst, err / tol)
        moved = max(moved, max_abs_diff(p.grad, bce_grads[pname]))
        assert err <= tol, (pname, err, tol, float(ref.abs().max()))
        checked += 1
    print('train_batch lsep + bce, int_preds: %d gradients, worst err / tol %.3f; largest distance from the BCE gradient %.3e'
          % (checked, worst, moved))
    assert checked >= 40 and moved > 1e-3                      # (ten tolerances away from the gradient of plain BCE)


def _epoch(fx, rank_loss='absent', seed=0):
    torch.manual_seed(seed)
    model = TC.fixture_model(fx).to(DEV)
    data = T.TrainBatcher(fx['src'], fx['tgt'], int(fx['batch_size']), shuffle=False, drop_last=False)
    optim = O.Adam(list(model.get_trainable_parameters()), betas=TC.ADAM_BETAS, lr=float(fx['lr']))
    opt = TC.train_opt(int(fx['tgt_vocab_size']))
    if rank_loss != 'absent':
        opt.rank_loss = rank_loss
    dres = {}
    out = T.train_epoch(model, data, optim, opt, device=DEV, device_results=dres)
    torch.cuda.synchronize()
    return model, out, dres


def test_train_epoch_without_rank_loss_is_todays_epoch_and_with_it_the_mean_is_over_rows():
    fx = TC.load_fixture()
    base_model, base, base_res = _epoch(fx)                       # no rank_loss attribute at all: the call of before
    model, out, dres = _epoch(fx, None)
    assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1]) and out[2] == base[2]
    assert torch.equal(dres['row_loss'], base_res['row_loss'])
    for (k, a), b in zip(model.state_dict().items(), base_model.state_dict().values()):
        assert torch.equal(a, b), k
    rl = T.RankLossOptions('lsep', bce_weight=1.0)
    model, out, dres = _epoch(fx, rl)
    assert max(max_abs_diff(a, b) for a, b in zip(model.state_dict().values(), base_model.state_dict().values())) > 1e-5
    # the first batch saw the initial weights: its rows of row_loss are the kernel's output for that batch's logits
    seq, pos, gold = _batch0(fx)
    torch.manual_seed(0)
    fresh = TC.fixture_model(fx).to(DEV).train()
    logits = fresh((seq.to(DEV), pos.to(DEV)), None, None, gold.to(DEV), return_attns=False, int_preds=False)[0].detach()
    _, _, rows = N.rank_loss_train([logits], [1.0], gold.to(DEV), 'lsep', 0.0, 1.0)
    n0 = gold.size(0)
    assert dres['batches'][0] == (0, n0) and torch.equal(dres['row_loss'][0, :n0], rows[0])
    assert max_abs_diff(out[0][:n0], torch.sigmoid(logits)) < 1e-6
    want_total = sum(float(dres['row_loss'][0, lo:lo + real].cpu().double().sum()) / real for lo, real in dres['batches'])
    assert out[2] == want_total                                   # the trained loss, a mean over ROWS: no division by L


def test_train_epoch_with_rank_loss_never_waits_for_the_device(monkeypatch):
    fx = TC.load_fixture()
    rl = T.RankLossOptions('hinge', 1.0, 0.5)
    _epoch(fx, rl)                          # warm: allocations, the pinned ring
    me = threading.get_ident()
    state = {'inside': False, 'batches': 0, 'waits': [], 'launches': 0}
    body, launch = T.issue_stage, N.rank_loss_train

    def wrapped(*a, **k):
        state['inside'] = True
        try:
            return body(*a, **k)
        finally:
            state['inside'] = False
            state['batches'] += len(a[3].items)

    def counted_launch(*a, **k):
        state['launches'] += 1
        return launch(*a, **k)

    def counting(owner, name, cuda_self):
        real = getattr(owner, name)

        def f(*a, **k):
            if state['inside'] and ((a and a[0].is_cuda) if cuda_self else threading.get_ident() == me):
                state['waits'].append(name)
            return real(*a, **k)
        monkeypatch.setattr(owner, name, f)

    monkeypatch.setattr(T, 'issue_stage', wrapped)
    monkeypatch.setattr(N, 'rank_loss_train', counted_launch)
    counting(torch.cuda, 'synchronize', False)
    counting(torch.cuda.Stream, 'synchronize', False)
    counting(torch.cuda.Event, 'synchronize', False)
    for name in ('item', 'cpu', 'tolist', 'numpy', '__bool__', '__float__', '__int__'):
        counting(torch.Tensor, name, True)
    _epoch(fx, rl)
    assert state['batches'] == 3 and state['launches'] == 3 and state['waits'] == [], state      # one loss launch per batch


def test_run_train_with_lsep_end_to_end_and_run_eval_reads_its_checkpoint():
    from lamp_amd import run_eval, run_train
    with tempfile.TemporaryDirectory(prefix='lamp_run_') as root:   # (save_model writes nothing under a path that contains 'test')
        assert 'test' not in root
        data_path = os.path.join(root, 'train_valid_data.pt')
        torch.save(TC.synthetic_dataset(n_train=208), data_path)
        model_args = ['-data', data_path, '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2',
                      '-label_mask', 'prior', '-batch_size', '16']
        run_args = ['-epoch', '1', '-lr', '0.003', '-dropout', '0.0', '-results_dir', os.path.join(root, 'res'), '-name', 'e2e',
                    '-seed', '1', '-optim_impl', 'lamp']
        bce = run_train.main(model_args + run_args)
        hist = run_train.main(model_args + run_args + ['-loss_fn', 'lsep', '-rank_bce_weight', '1'])
        json.dumps(hist)
        assert len(hist) == 1 and np.isfinite(hist[0]['train_loss'])
        run_dir = os.path.dirname(hist[0]['checkpoint'])
        bce_dir = os.path.dirname(bce[0]['checkpoint'])
        assert os.path.basename(bce_dir).endswith('.e2e') and 'lossfn' not in bce_dir
        assert os.path.basename(run_dir) == os.path.basename(bce_dir)[:-len('.e2e')] + '.lossfn_lsep_1.0.e2e'
        ckpt = torch.load(hist[0]['checkpoint'], map_location='cpu', weights_only=False)
        st = ckpt['settings']
        assert sorted(ckpt) == ['epoch', 'model', 'settings']
        assert (st.loss_fn, st.rank_bce_weight) == ('lsep', 1.0)
        plain = torch.load(bce[0]['checkpoint'], map_location='cpu', weights_only=False)['settings']
        assert not any(hasattr(plain, k) for k in ('loss_fn', 'rank_margin', 'rank_bce_weight', 'rank_loss', 'loss_options'))
        assert set(vars(st)) - set(vars(plain)) == {'loss_fn', 'rank_bce_weight'}
        row = open(os.path.join(run_dir, 'losses.csv')).read().split()[0].split(',')
        row_bce = open(os.path.join(bce_dir, 'losses.csv')).read().split()[0].split(',')
        assert float(row[1]) == hist[0]['train_loss'] and float(row[1]) > float(row_bce[1])       # the trained loss: R + BCE
        assert (float(row[2]), float(row[3])) == (hist[0]['valid_loss'], hist[0]['test_loss'])
        print('run_train lsep + bce: train %.6f (BCE run %.6f), valid %.6f, test %.6f'
              % (hist[0]['train_loss'], bce[0]['train_loss'], hist[0]['valid_loss'], hist[0]['test_loss']))
        # the logged valid and test losses are plain BCE of that checkpoint's predictions: run_eval (lamp_sigmoid_bce_fwd)
        # gives exactly them, from the checkpoint alone
        for split in ('valid', 'test'):
            out = run_eval.main(model_args + ['-checkpoint', hist[0]['checkpoint'], '-split', split])
            assert out['bce_total'] / out['n_samples'] == hist[0]['%s_loss' % split], split
