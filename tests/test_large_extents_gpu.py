"""Kernels on operands past 2 GiB, 4 GiB and 2^31 elements (tests/large_extent_common.py has the harness and the four
boundaries B31 / B32 / E31 / E32; DESIGN.md "Addressing limits" has the table every case cites a row of).

Every case carves its operands from one BigArena: exact sizes, 64 KiB sentinel zones, and below the first operand a landing
zone as long as the largest operand, so that a truncated offset stays in memory the test owns and shows as a failed assertion.
Whole-buffer checks (no sentinel left in an output, no sentinel changed outside the operands, bit-periodic outputs of
periodic inputs) run chunked on the device; references are fp64 on the CPU for row windows only: the first 128 rows, 128 rows
on either side of each boundary crossed, the last 128 + ragged-tail rows.  No tolerance is new: each bar is the one the same
op has against fp64 in the file named beside it.

Each case computes its need in Python integers first and skips only when the device has less than need + 2 GiB free; the
peak it reached, its planned need and the used fraction of each bar are printed (run with -s to see them).

Not here (DESIGN.md 5.3 gives each one's row): lamp_embed_bwd (the atomic form), lamp_onehot_front_bwd, and the lamp_mha_*
composites and the training FFN composites, whose launches are the GEMM, attention, LayerNorm, dropout and column-sum cases of
this file one by one."""
import contextlib
import ctypes as C
import gc
import math

import pytest
import torch
import torch.nn.functional as F

import large_extent_common as LX
import train_common as TC
from conftest import max_abs_diff

pytestmark = pytest.mark.gpu

GIB = float(1 << 30)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def N():
    from lamp_amd import _native
    _native.lib()
    return _native


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def rnd(seed):
    return torch.Generator().manual_seed(seed)


def ok(rc, what):
    assert rc == 0, '%s returned %d' % (what, rc)


def used(what, err, bar):
    frac = err / bar
    print('large-extent used: %s: max |err| %.3e of bar %.3e = %.3f' % (what, err, bar, frac))
    assert frac < 1.0, (what, err, bar)
    return frac


@contextlib.contextmanager
def arena(dev, fill, operands, what, extra=0):
    """The case's BigArena.  need = arena + chunked temporaries + extra, checked against the budget and the free memory before
    anything is allocated; everything is released in the finally (the body keeps its views in a function of its own)."""
    need = LX.need_bytes(operands, extra)
    LX.require_memory(need)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ar = None
    try:
        ar = LX.BigArena(dev, fill, operands)
        yield ar
        torch.cuda.synchronize()
    finally:
        peak = torch.cuda.max_memory_allocated() - base
        if ar is not None:
            ar.free()
        del ar
        gc.collect()
        torch.cuda.empty_cache()
        print('large-extent peak: %s: %.2f GiB (planned %.2f GiB)' % (what, peak / GIB, need / GIB))
    assert peak <= need, '%s: peak %d above the planned need %d' % (what, peak, need)


def f32(n):
    return int(n) * 4


# ====================================================================================== G4: lamp_dropout, E31 and E32
# Table row lamp_dropout: x, y through pointers, 64-bit element index e (grid-stride loop), mix32(lo(e), hi(e), seed); no guard.
def _dropout_body(ar, N, n, pdrop, seed):
    P = LX.PERIOD
    vals = torch.randn(P, generator=rnd(7))
    vals = vals + torch.sign(vals) * 0.5                      # no zeros: a dropped element is told from a kept one
    X = ar.view('x=y')
    LX.fill_periodic_rows(X[:n // P * P].view(-1, P), vals.view(1, P))
    X[n // P * P:].copy_(vals[:n - n // P * P])
    ok(N.lib().lamp_dropout(ar.ptr('x=y'), n, pdrop, seed, ar.ptr('x=y'), N.stream()), 'lamp_dropout')
    ar.check_zones()
    ar.check_written('x=y')
    one = torch.tensor(1.0)
    scale = (one / (one - torch.tensor(pdrop))).item()        # the launcher's own fp32 expression, 1.0f / (1.0f - p)
    # whole buffer, on the device: every element is 0 or its own input times the scale; the kept fraction is 1 - p
    k = LX.CHUNK // (4 * P)
    block = (vals.to(ar.device) * scale).repeat(k)
    kept = 0
    for a in range(0, n, k * P):
        yb = X[a:a + k * P]
        keep = yb != 0
        keep &= yb != block[:yb.numel()]
        assert not bool(keep.any()), 'a kept element is not its own input times 1 / (1 - p)'
        kept += int(torch.count_nonzero(yb))
    assert abs(kept / n - (1 - pdrop)) < 3e-3
    # windows (element indices): exact against the restated counter
    xs = vals * scale
    for a, b in LX.windows(n, 4, LX.FLAT_WINDOW):
        keep = N.dropout_keep_mask(b - a, pdrop, seed, start=a)
        want = torch.where(keep, xs[torch.arange(a, b) % P], torch.zeros(()))
        assert torch.equal(X[a:b].cpu(), want), 'lamp_dropout differs from the restated mask in elements [%d, %d)' % (a, b)
    # the window above E32: unbiased at the bar test_gpu_backward.py: test_dropout_is_counter_based_and_unbiased uses for 2^20
    # elements, and a mask of its own, not that of elements 0 .. 2^20 + 2
    m = n - (1 << 32)
    hi = X[1 << 32:n].cpu() != 0
    lo = X[:m].cpu() != 0
    assert abs(hi.float().mean().item() - (1 - pdrop)) < 3e-3
    assert abs((hi & lo).float().mean().item() - (1 - pdrop) ** 2) < 3e-3 and not torch.equal(hi, lo)


@pytest.mark.parametrize('fill', LX.FILLS)
def test_dropout_in_place_across_e31_and_e32(dev, N, fill):
    n = LX.DROPOUT_N
    assert LX.crossings(f32(n)) == ['B31', 'B32', 'E31', 'E32']
    with arena(dev, fill, [('x=y', f32(n))], 'lamp_dropout n = 2^32 + 2^20 + 3') as ar:
        _dropout_body(ar, N, n, 0.1, 1234)


# ====================================================================================== G5: row kernels
def ln_params(d, seed):
    g = rnd(seed)
    return 1 + 0.3 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)


# Table row lamp_layernorm_fwd: x, y, gamma, beta through pointers; row = 4 * blockIdx.x + wave (int64), x + row * d in 64 bits;
# guard (M + 3) / 4 > 0x7fffffff -> LAMP_E_DIMS (pointwise.hip: grid4).  One wave per row: a row's sums do not depend on its
# position, so x is periodic along rows and y must be bit-periodic.
def _layernorm_fwd_body(ar, N, M, d):
    period = torch.randn(LX.PERIOD, d, generator=rnd(3)) * 2 + 0.5
    gamma, beta = ln_params(d, 4)
    X, Y = ar.view('x', shape=(M, d)), ar.view('y', shape=(M, d))
    LX.fill_periodic_rows(X, period)
    ar.view('gamma').copy_(gamma)
    ar.view('beta').copy_(beta)
    ok(N.lib().lamp_layernorm_fwd(ar.ptr('x'), M, d, ar.ptr('gamma'), ar.ptr('beta'), 1e-5, ar.ptr('y'), N.stream()),
       'lamp_layernorm_fwd')
    ar.check_zones()
    ar.check_written('y')
    LX.assert_bit_periodic(Y, LX.PERIOD, 'lamp_layernorm_fwd y')
    wins = LX.windows(M, f32(d))
    LX.assert_rows_equal_generator(X, period, wins, 'lamp_layernorm_fwd x')
    ref = F.layer_norm(LX.periodic_rows(period, LX.window_rows(wins)).double(), (d,), gamma.double(), beta.double(), 1e-5)
    used('lamp_layernorm_fwd (bar: test_buffer_contracts_gpu.py: test_layernorm_fwd)', max_abs_diff(LX.take_rows(Y, wins), ref), 2e-5)


@pytest.mark.parametrize('fill', [LX.FILL_NAN])
def test_layernorm_fwd_across_e31(dev, N, fill):
    M, d = LX.LN_E31
    nb = f32(M * d)
    assert LX.crossings(nb) == ['B31', 'B32', 'E31']
    with arena(dev, fill, [('gamma', f32(d)), ('beta', f32(d)), ('x', nb), ('y', nb)], 'lamp_layernorm_fwd M * d past 2^31') as ar:
        _layernorm_fwd_body(ar, N, M, d)


# Table row lamp_layernorm_residual_fwd: as lamp_layernorm_fwd, plus residual + (row % residual_rows) * d in 64 bits and the
# dropout counter row * d + 4 c as int64 into drop4 (lamp_kernels.h).  The mask depends on the row's position: windows only.
def _layernorm_residual_body(ar, N, M, d, r_rows, pdrop, seed):
    period = torch.randn(LX.PERIOD, d, generator=rnd(5))
    res = torch.randn(r_rows, d, generator=rnd(6))
    gamma, beta = ln_params(d, 8)
    X, Y = ar.view('x', shape=(M, d)), ar.view('y', shape=(M, d))
    LX.fill_periodic_rows(X, period)
    ar.view('residual', shape=(r_rows, d)).copy_(res)
    ar.view('gamma').copy_(gamma)
    ar.view('beta').copy_(beta)
    ok(N.lib().lamp_layernorm_residual_fwd(ar.ptr('x'), ar.ptr('residual'), r_rows, M, d, ar.ptr('gamma'), ar.ptr('beta'), 1e-5,
                                           pdrop, seed, ar.ptr('y'), N.stream()), 'lamp_layernorm_residual_fwd')
    ar.check_zones()
    ar.check_written('y')
    wins = LX.windows(M, f32(d))
    LX.assert_rows_equal_generator(X, period, wins, 'lamp_layernorm_residual_fwd x')
    assert torch.equal(ar.view('residual', shape=(r_rows, d)).cpu(), res)
    worst = 0.0
    for a, b in wins:
        rows = torch.arange(a, b)
        keep = N.dropout_keep_mask((b - a) * d, pdrop, seed, start=a * d).view(b - a, d)
        z = LX.periodic_rows(period, rows).double() * keep / (1 - pdrop) + res[rows % r_rows].double()
        ref = F.layer_norm(z, (d,), gamma.double(), beta.double(), 1e-5)
        worst = max(worst, max_abs_diff(Y[a:b], ref))
    used('lamp_layernorm_residual_fwd, p = %.1f (bar: test_buffer_contracts_gpu.py: test_layernorm_residual_fwd_and_bwd)' % pdrop,
         worst, 3e-5)


def test_layernorm_residual_fwd_with_dropout_across_e31(dev, N):
    M, d = LX.LN_E31
    nb, r_rows = f32(M * d), 520
    ops = [('gamma', f32(d)), ('beta', f32(d)), ('residual', f32(r_rows * d)), ('x', nb), ('y', nb)]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_layernorm_residual_fwd M * d past 2^31') as ar:
        _layernorm_residual_body(ar, N, M, d, r_rows, 0.3, 77)


# Table rows lamp_softmax_bwd / lamp_sigmoid_attn_bwd: P, dP, dS through pointers.  softmax: row = 4 * blockIdx.x + wave (int64),
# P + row * lk in 64 bits, guard (rows + 3) / 4 > 0x7fffffff -> LAMP_E_DIMS.  sigmoid: flat int64 element index in a
# grid-stride loop, also the dropout counter; no guard.  In place (dS = dP).  The softmax form is row-local and takes no
# dropout through this entry point: periodic.  The sigmoid form runs with attention dropout: windows only.
def _attn_bwd_body(ar, N, rows, lk, kind):
    g = rnd(9)
    Pp = torch.softmax(torch.randn(LX.PERIOD, lk, generator=g) * 2, -1)
    Gp = torch.randn(LX.PERIOD, lk, generator=g)
    Pv, Gv = ar.view('P', shape=(rows, lk)), ar.view('dP=dS', shape=(rows, lk))
    LX.fill_periodic_rows(Pv, Pp)
    LX.fill_periodic_rows(Gv, Gp)
    pdrop, seed = 0.2, 4321
    if kind == 'softmax':
        ok(N.lib().lamp_softmax_bwd(ar.ptr('P'), ar.ptr('dP=dS'), rows, lk, 0.25, ar.ptr('dP=dS'), N.stream()), 'lamp_softmax_bwd')
    else:
        ok(N.lib().lamp_sigmoid_attn_bwd(ar.ptr('P'), ar.ptr('dP=dS'), rows, lk, 0.25, pdrop, seed, ar.ptr('dP=dS'), N.stream()),
           'lamp_sigmoid_attn_bwd')
    ar.check_zones()
    ar.check_written('dP=dS')
    wins = LX.windows(rows, f32(lk))
    LX.assert_rows_equal_generator(Pv, Pp, wins, kind + ' P')
    if kind == 'softmax':
        LX.assert_bit_periodic(Gv, LX.PERIOD, 'lamp_softmax_bwd dS')
    worst = 0.0
    for a, b in wins:
        idx = torch.arange(a, b)
        Pw, Gw = LX.periodic_rows(Pp, idx).double(), LX.periodic_rows(Gp, idx).double()
        if kind == 'softmax':
            ref = 0.25 * Pw * (Gw - (Pw * Gw).sum(-1, keepdim=True))
        else:
            keep = N.dropout_keep_mask((b - a) * lk, pdrop, seed, start=a * lk).view(b - a, lk)
            scale = (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(pdrop))).double()
            ref = 0.25 * Pw * (1 - Pw) * (Gw * keep * scale)
        worst = max(worst, max_abs_diff(Gv[a:b], ref))
    used('lamp_%s_bwd in place (bar: test_buffer_contracts_gpu.py: test_softmax_bwd_and_sigmoid_attn_bwd)'
         % ('softmax' if kind == 'softmax' else 'sigmoid_attn'), worst, 1e-5)


@pytest.mark.parametrize('kind', ['softmax', 'sigmoid'])
def test_softmax_and_sigmoid_attn_bwd_in_place_across_e31(dev, N, kind):
    rows, lk = LX.SOFTMAX_E31
    nb = f32(rows * lk)
    assert LX.crossings(nb) == ['B31', 'B32', 'E31']
    with arena(dev, LX.FILL_NAN, [('P', nb), ('dP=dS', nb)], 'lamp_%s bwd rows * lk past 2^31' % kind) as ar:
        _attn_bwd_body(ar, N, rows, lk, kind)


# Table row lamp_colsum: x, out, workspace through pointers; col and row int64, x[(r + u) * ldx + col] in 64 bits; guards
# (N + 255) / 256 and (N + 31) / 32 > 0x7fffffff -> LAMP_E_DIMS.  Workspace of exactly lamp_colsum_workspace_bytes().
# A column's sum runs over ALL rows: the reference is the exact fp64 sum of the periodic operand (every period row times
# the number of times it occurs), for every column.
def _colsum_body(ar, N, M, Nn):
    P = LX.PERIOD
    tall = M > P
    X = ar.view('x', shape=(M, Nn))
    if tall:       # periodic along rows
        period = torch.randn(P, Nn, generator=rnd(11))
        LX.fill_periodic_rows(X, period)
    else:          # wide: every row periodic along its columns
        period = torch.randn(M, P, generator=rnd(12))
        for r in range(M):
            _flat_fill(X[r], period[r])
    nb = ar.nbytes('workspace')
    ok(N.lib().lamp_colsum(ar.ptr('x'), M, Nn, Nn, ar.ptr('out'), ar.ptr('workspace'), nb, N.stream()), 'lamp_colsum')
    ar.check_zones()
    ar.check_written('out')
    if tall:
        LX.assert_rows_equal_generator(X, period, LX.windows(M, f32(Nn)), 'lamp_colsum x')
        count = torch.full((P,), M // P, dtype=torch.float64)
        count[:M % P] += 1
        ref = (period.double() * count[:, None]).sum(0)
    else:
        pd = period.to(ar.device)
        for r in range(M):
            assert bool((X[r, :Nn - P] == X[r, P:]).all()) and torch.equal(X[r, :P], pd[r]), 'lamp_colsum x changed'
        ref = period.double().sum(0)[torch.arange(Nn) % P]
    used('lamp_colsum %d x %d (bar: test_buffer_contracts_gpu.py: test_colsum, 1e-5 * 4 sqrt(M))' % (M, Nn),
         max_abs_diff(ar.view('out'), ref), 1e-5 * max(1.0, M ** 0.5) * 4)


@pytest.mark.parametrize('M,Nn,fill', [LX.COLSUM_TALL + (LX.FILL_NAN,), LX.COLSUM_TALL + (LX.FILL_BIG,),
                                       (37, 29029999, LX.FILL_NAN)])
def test_colsum_tall_and_wide_across_b32(dev, N, M, Nn, fill):
    nb = f32(M * Nn)
    assert 'B32' in LX.crossings(nb)
    ws = N.lib().lamp_colsum_workspace_bytes(M, Nn)
    assert ws == min(512, (M + 63) // 64) * Nn * 4
    with arena(dev, fill, [('out', f32(Nn)), ('workspace', ws), ('x', nb)], 'lamp_colsum %d x %d' % (M, Nn)) as ar:
        _colsum_body(ar, N, M, Nn)


# Table row lamp_attn_bias_bwd: dS [n_slices, lq * lk], the partials and dbias through pointers; the first stage is lamp_colsum's
# kernel over the [n_slices, lq * lk] view (int64 row and column), the second selects the blocked entries of the forward's bias
# (exactly 0 there) and scales.  Guard ((lq * lk + 255) / 256 > 0x7fffffff -> LAMP_E_DIMS) out of reach of two int32.  dS
# crosses B32 through n_slices; the reference is the exact fp64 sum of the periodic operand; scale = 0.5 is exact.
def _attn_bias_bwd_body(ar, N, n, lq, lk, scale):
    P = LX.PERIOD
    g = rnd(17)
    cols = lq * lk
    period = torch.randn(P, cols, generator=g) * 0.05
    bias = torch.randn(lq, lk, generator=g).masked_fill(torch.rand(lq, lk, generator=g) < 0.2, float('-inf'))
    X = ar.view('dS', shape=(n, cols))
    LX.fill_periodic_rows(X, period)
    ar.view('bias', shape=(lq, lk)).copy_(bias)
    ok(N.lib().lamp_attn_bias_bwd(ar.ptr('dS'), n, lq, lk, scale, ar.ptr('bias'), lk, ar.ptr('dbias'), lk, ar.ptr('workspace'),
                                  ar.nbytes('workspace'), N.stream()), 'lamp_attn_bias_bwd')
    ar.check_zones()
    ar.check_written('dbias')
    LX.assert_rows_equal_generator(X, period, LX.windows(n, f32(cols)), 'lamp_attn_bias_bwd dS')
    assert torch.equal(ar.view('bias', shape=(lq, lk)).cpu(), bias)
    count = torch.full((P,), n // P, dtype=torch.float64)
    count[:n % P] += 1
    ref = (scale * (period.double() * count[:, None]).sum(0)).view(lq, lk)
    got = ar.view('dbias', shape=(lq, lk)).cpu()
    dead = torch.isinf(bias)
    assert bool((got[dead] == 0).all()) and not bool(torch.signbit(got[dead]).any())
    used('lamp_attn_bias_bwd %d x %d x %d (bar: test_buffer_contracts_gpu.py: test_colsum, 1e-5 * 4 sqrt(M), its first stage; x scale)'
         % (n, lq, lk), max_abs_diff(got[~dead], ref[~dead]), scale * 0.05 * 1e-5 * n ** 0.5 * 4)


def test_attn_bias_bwd_across_b32(dev, N):
    lq, lk = 90, 92                            # lk a multiple of 4: ld = lk, no pad columns
    n = LX.B32 // f32(lq * lk) + 2 * LX.WINDOW + 37
    assert LX.crossings(f32(n * lq * lk)) == ['B31', 'B32']
    ws = N.lib().lamp_attn_bias_bwd_workspace_bytes(n, lq, lk)
    assert ws == min(512, (n + 63) // 64) * lq * lk * 4
    ops = [('bias', f32(lq * lk)), ('dbias', f32(lq * lk)), ('workspace', ws), ('dS', f32(n * lq * lk))]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_attn_bias_bwd n_slices * lq * lk * 4 past 2^32') as ar:
        _attn_bias_bwd_body(ar, N, n, lq, lk, 0.5)


# Table row lamp_onehot_front_fwd / lamp_conv_window_fwd / lamp_conv_relu_bwd_pad / lamp_conv_pack (conv.hip): every operand
# through pointers, flat int64 item and row indices; guards: conv_window's row tiles > 0x7fffffff -> LAMP_E_DIMS (CPU file).  The
# chain of lamp_amd/training.py: _OnehotFn at B * T2 * d * 4 past 2^32 (xpad and dz, 16 pad rows a sample more, pass it too):
# front end -> conv2 with its epilogue -> the ReLU mask's backward into the padded layout.  A sample's rows depend on its own
# tokens only (dropout off: its counter is the position), so the batch repeats 13 samples and every buffer is bit-periodic
# over samples; 13 samples against the fp64 restatement of test_buffer_contracts_gpu.py: test_onehot_blocks_forward_and_backward.
def _onehot_body(ar, N, B, T, d, enc):
    from onehot_common import make_dna
    V, T2 = 9, T // 2
    Tp = T2 + 16
    seq13, pos13 = make_dna(SLICES, T, [T, 17, T - 1, 3, T, T // 2, 1, T, 40, T - 7, T, 2, 99], seed=7)
    t1 = N.onehot_tap_table(enc.src_word_emb.weight, enc.conv1.weight).detach()
    b1, w2, b2 = enc.conv1.bias.detach(), enc.conv2.weight.detach().contiguous(), enc.conv2.bias.detach()
    pw = enc.position_enc.weight.detach()
    for name, t in (('t1', t1), ('conv1_b', b1), ('conv2_w', w2), ('conv2_b', b2), ('pos_table', pw)):
        ar.view(name).copy_(t.reshape(-1))
    LX.fill_periodic_rows(ar.view('seq', torch.int64, (B, T)), seq13)
    LX.fill_periodic_rows(ar.view('pos', torch.int64, (B, T)), pos13)
    dy13 = torch.randn(SLICES, T2 * d, generator=rnd(5))
    DY = ar.view('dy', shape=(B, T2 * d))
    LX.fill_periodic_rows(DY, dy13)
    L, p = N.lib(), ar.ptr
    ok(L.lamp_conv_pack(p('conv2_w'), d, d, 16, 0, p('pack'), N.stream()), 'lamp_conv_pack')
    fe = N.OnehotFrontend(p('t1'), p('conv1_b'), p('conv2_w'), p('conv2_b'), p('pack'), V, 16)
    ok(L.lamp_onehot_front_fwd(p('seq'), B, T, C.byref(fe), d, 0.0, 0, p('xpad'), N.stream()), 'lamp_onehot_front_fwd')
    ok(L.lamp_conv_window_fwd(p('xpad'), B, T2, Tp, d, p('pack'), d, p('conv2_b'), 1, p('pos_table'), pw.size(0), p('pos'), T,
                              p('out'), p('relu_out'), N.stream()), 'lamp_conv_window_fwd')
    ok(L.lamp_conv_relu_bwd_pad(p('dy'), p('relu_out'), B, T2, d, p('dz'), N.stream()), 'lamp_conv_relu_bwd_pad')
    ar.check_zones()
    views = {}
    for name, rows in (('xpad', Tp), ('out', T2), ('relu_out', T2), ('dz', Tp)):
        ar.check_written(name)
        views[name] = ar.view(name)[:B * rows * d].view(B, rows * d)
        LX.assert_bit_periodic(views[name], SLICES, 'one-hot ' + name)
    for name in ('xpad', 'dz'):                                   # the 16 trailing rows
        assert not bool(ar.view(name)[B * Tp * d:].any()), name + ': trailing rows'
    assert torch.equal(ar.view('pack', shape=(d, 16, d)).cpu(), w2.permute(0, 2, 1))
    wins = LX.windows(B, f32(T2 * d), width=8)
    LX.assert_rows_equal_generator(DY, dy13, wins, 'one-hot dy')
    LX.assert_rows_equal_generator(ar.view('seq', torch.int64, (B, T)), seq13, wins, 'one-hot seq')
    idx = LX.window_rows(wins) % SLICES
    sd = dict((k_, v_.detach().double()) for k_, v_ in enc.state_dict().items())
    y = F.conv1d(F.embedding(seq13, sd['src_word_emb.weight']).transpose(1, 2), sd['conv1.weight'], sd['conv1.bias'], padding=8)[:, :, :-1]
    y = F.max_pool1d(torch.relu(y), 2, 2)
    y2 = torch.relu(F.conv1d(y, sd['conv2.weight'], sd['conv2.bias'], padding=8).transpose(1, 2))[:, :-1, :]
    xp = F.pad(y.transpose(1, 2), (0, 0, 8, 8))
    src = 'tests/test_onehot_gpu.py through test_buffer_contracts_gpu.py: test_onehot_blocks_forward_and_backward'
    got = dict((name, LX.take_rows(v, wins)) for name, v in views.items())
    used('lamp_onehot_front_fwd xpad (bar: %s)' % src, max_abs_diff(got['xpad'].view(-1, Tp, d), xp[idx]), 1e-4)
    used('lamp_conv_window_fwd relu_out (bar: %s)' % src, max_abs_diff(got['relu_out'].view(-1, T2, d), y2[idx]), 1e-4)
    used('lamp_conv_window_fwd out (bar: %s)' % src,
         max_abs_diff(got['out'].view(-1, T2, d), (y2 + F.embedding(pos13[:, :T2], sd['position_enc.weight']))[idx]), 1e-4)
    want_dz = F.pad(torch.where(got['relu_out'] > 0, dy13[idx], torch.zeros(())).view(-1, T2, d), (0, 0, 8, 8))
    assert torch.equal(got['dz'].view(-1, Tp, d), want_dz), 'lamp_conv_relu_bwd_pad: dz is not dy under the ReLU mask, zero-padded'


def test_onehot_blocks_across_b32(dev, N):
    from onehot_common import build_model
    T, d, V = 200, 64, 9
    T2, Tp = T // 2, T // 2 + 16
    B = LX.B32 // f32(T2 * d) + 2 * SLICES + 5
    assert LX.crossings(f32(B * T2 * d)) == ['B31', 'B32']
    enc = build_model(d=d, h=4, L=23, T_max=256).encoder
    assert N.onehot_tap_table(enc.src_word_emb.weight, enc.conv1.weight).numel() == V * 16 * d
    pad, body = f32((B * Tp + 16) * d), f32(B * T2 * d)
    ops = [('t1', f32(V * 16 * d)), ('conv1_b', f32(d)), ('conv2_w', f32(d * d * 16)), ('conv2_b', f32(d)), ('pack', f32(d * 16 * d)),
           ('pos_table', f32(enc.position_enc.weight.numel())), ('seq', 8 * B * T), ('pos', 8 * B * T), ('xpad', pad), ('out', body),
           ('relu_out', body), ('dy', body), ('dz', pad)]
    with arena(dev, LX.FILL_NAN, ops, 'one-hot blocks, B * T2 * d * 4 past 2^32') as ar:
        _onehot_body(ar, N, B, T, d, enc)


# Table row lamp_embed_fwd: tokens, tables, out through pointers; t = 4 * blockIdx.x + wave (int64), out + t * d in 64 bits;
# guard (n_tokens + 3) / 4 > 0x7fffffff -> LAMP_E_DIMS.  A row is a function of its two indices: periodic tokens, periodic out.
def _embed_body(ar, N, n_tok, d, V, n_pos, with_pos):
    g = rnd(13)
    emb, ptab = torch.randn(V, d, generator=g), torch.randn(n_pos, d, generator=g)
    seq_p = torch.randint(0, V, (LX.PERIOD, 1), generator=g)
    pos_p = torch.randint(0, n_pos, (LX.PERIOD, 1), generator=g)
    LX.fill_periodic_rows(ar.view('seq', torch.int64, (n_tok, 1)), seq_p)
    LX.fill_periodic_rows(ar.view('pos', torch.int64, (n_tok, 1)), pos_p)
    ar.view('emb', shape=(V, d)).copy_(emb)
    ar.view('pos_table', shape=(n_pos, d)).copy_(ptab)
    ok(N.lib().lamp_embed_fwd(ar.ptr('seq'), ar.ptr('pos'), n_tok, ar.ptr('emb'), V, ar.ptr('pos_table') if with_pos else None,
                              n_pos if with_pos else 0, d, ar.ptr('out'), N.stream()), 'lamp_embed_fwd')
    ar.check_zones()
    ar.check_written('out')
    out = ar.view('out', shape=(n_tok, d))
    LX.assert_bit_periodic(out, LX.PERIOD, 'lamp_embed_fwd out')
    wins = LX.windows(n_tok, f32(d))
    idx = LX.window_rows(wins) % LX.PERIOD
    ref = emb[seq_p[idx, 0]].double() + (ptab[pos_p[idx, 0]].double() if with_pos else 0.0)
    used('lamp_embed_fwd (bar: test_buffer_contracts_gpu.py: test_embed_fwd_and_bwd_with_pad_rows)',
         max_abs_diff(LX.take_rows(out, wins), ref), 1e-6)
    assert torch.equal(ar.view('emb', shape=(V, d)).cpu(), emb) and torch.equal(ar.view('pos_table', shape=(n_pos, d)).cpu(), ptab)


@pytest.mark.parametrize('with_pos', [True, False])
def test_embed_fwd_across_b32(dev, N, with_pos):
    d, V, n_pos = 512, 1000, 300
    n_tok = (1 << 30) // d + 2 * LX.WINDOW + 37
    assert LX.crossings(f32(n_tok * d)) == ['B31', 'B32']
    ops = [('seq', 8 * n_tok), ('pos', 8 * n_tok), ('emb', f32(V * d)), ('pos_table', f32(n_pos * d)), ('out', f32(n_tok * d))]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_embed_fwd n_tokens * d * 4 past 2^32') as ar:
        _embed_body(ar, N, n_tok, d, V, n_pos, with_pos)


# Table row lamp_embed_bwd_ordered (train_step.hip: embed_bwd_ordered_kernel): one wave per token position t (int64); the wave
# of an id's FIRST position owns d_emb + tok * d and adds dout + (s0 + b) * d of every occurrence in ascending order, 64
# positions a ballot; every other wave leaves at the first 64-position chunk that holds an earlier occurrence.  Guard: grid4.
# The cost is quadratic only for all-distinct ids.  Here the tokens repeat a period of 4099 positions over a vocabulary of
# 1000, so every id occurs early: about 1000 owner waves walk n_tokens / 64 chunks, the others a few ballots.  dout
# [n_tokens, 512] crosses B32 and is periodic too, with the sign turned every 4099 rows: period 8198 (2^21 rows, what a 32-bit
# byte offset would wrap by, is no multiple of it), so d_emb's exact value is base + the count-weighted fp64 sum of one
# period, for every id.  The turned sign keeps an owner's running sum of some 2100 terms at the size of a few terms: with
# the same rows added 512 times over, the sum would grow to 512 times that, and its fp32 rounding with it -- a property of
# the data, which the bar (taken at 115 tokens) does not cover.  PAD (0) occurs and its row stays as it was.
def _embed_bwd_body(ar, N, n_tok, d, V):
    P = LX.PERIOD
    g = rnd(14)
    seq_p = torch.randint(0, V, (P, 1), generator=g)
    assert int((seq_p == 0).sum()) > 0 and len(torch.unique(seq_p)) > V * 0.95
    seq_p = seq_p.repeat(2, 1)
    dout_p = torch.randn(P, d, generator=g) / 32
    dout_p = torch.cat([dout_p, -dout_p])
    P = 2 * P
    base = torch.randn(V, d, generator=g)
    LX.fill_periodic_rows(ar.view('seq', torch.int64, (n_tok, 1)), seq_p)
    D = ar.view('dout', shape=(n_tok, d))
    LX.fill_periodic_rows(D, dout_p)
    ar.view('d_emb', shape=(V, d)).copy_(base)
    ok(N.lib().lamp_embed_bwd_ordered(ar.ptr('seq'), n_tok, ar.ptr('dout'), d, V, 0, ar.ptr('d_emb'), N.stream()),
       'lamp_embed_bwd_ordered')
    ar.check_zones()
    wins = LX.windows(n_tok, f32(d))
    LX.assert_rows_equal_generator(D, dout_p, wins, 'lamp_embed_bwd_ordered dout')
    LX.assert_rows_equal_generator(ar.view('seq', torch.int64, (n_tok, 1)), seq_p, wins, 'lamp_embed_bwd_ordered src_seq')
    count = torch.full((P,), n_tok // P, dtype=torch.float64)
    count[:n_tok % P] += 1
    ref = base.double().index_add(0, seq_p[:, 0], dout_p.double() * count[:, None])
    ref[0] = base[0].double()
    got = ar.view('d_emb', shape=(V, d)).cpu()
    assert torch.equal(got[0], base[0]), 'the PAD row changed'
    used('lamp_embed_bwd_ordered (bar: test_buffer_contracts_gpu.py: test_embed_fwd_and_bwd_with_pad_rows)', max_abs_diff(got, ref), 1e-4)


def test_embed_bwd_ordered_dout_across_b32(dev, N):
    d, V = 512, 1000
    n_tok = (1 << 30) // d + 2 * LX.WINDOW + 37
    assert LX.crossings(f32(n_tok * d)) == ['B31', 'B32'] and (1 << 21) % (2 * LX.PERIOD)
    ops = [('seq', 8 * n_tok), ('d_emb', f32(V * d)), ('dout', f32(n_tok * d))]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_embed_bwd_ordered n_tokens * d * 4 past 2^32') as ar:
        _embed_bwd_body(ar, N, n_tok, d, V)


# Table rows lamp_diag_logits_fwd: y, w_out, logits through pointers; row = 4 * blockIdx.x + wave (int64), y + row * d in 64
# bits, row % L selects the weight row; guard (B * L + 3) / 4 > 0x7fffffff -> LAMP_E_DIMS.  Row-local; the weight row depends
# on the position: windows.
def _diag_body(ar, N, B, L, d):
    g = rnd(15)
    period = torch.randn(LX.PERIOD, d, generator=g)
    w = torch.randn(L, d, generator=g) / d ** 0.5
    rows = B * L
    Y = ar.view('y', shape=(rows, d))
    LX.fill_periodic_rows(Y, period)
    ar.view('w_out', shape=(L, d)).copy_(w)
    ok(N.lib().lamp_diag_logits_fwd(ar.ptr('y'), ar.ptr('w_out'), B, L, d, ar.ptr('logits'), N.stream()), 'lamp_diag_logits_fwd')
    ar.check_zones()
    ar.check_written('logits')
    wins = LX.windows(rows, f32(d))
    LX.assert_rows_equal_generator(Y, period, wins, 'lamp_diag_logits_fwd y')
    idx = LX.window_rows(wins)
    ref = (LX.periodic_rows(period, idx).double() * w[idx % L].double()).sum(-1)
    got = torch.cat([ar.view('logits')[a:b] for a, b in wins])
    used('lamp_diag_logits_fwd (bar: test_buffer_contracts_gpu.py: test_diag_logits_fwd_bwd_and_sigmoid_bce)',
         max_abs_diff(got, ref), 2e-5)


def test_diag_logits_fwd_across_b32(dev, N):
    B, L, d = LX.DIAG_B32
    assert LX.crossings(f32(B * L * d)) == ['B31', 'B32']
    ops = [('w_out', f32(L * d)), ('logits', f32(B * L)), ('y', f32(B * L * d))]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_diag_logits_fwd B * L * d * 4 past 2^32') as ar:
        _diag_body(ar, N, B, L, d)


# ====================================================================================== G6: the fused loss launch
# Table rows lamp_bce_logits_train / lamp_multilabel_loss_train: every matrix through pointers; row = 4 * blockIdx.x + wave
# (int64), logits + row * L in 64 bits; guard (n_rows + 3) / 4 >= 2^31 -> LAMP_E_UNSUPPORTED.  One wave per (matrix, row) and
# an order of summation fixed by L alone: periodic logits and targets give bit-periodic probabilities, gradients and row sums.
def _loss_body(ar, N, n, L, asym):
    import imbalance_loss_common as IC
    g = rnd(17)
    xp = torch.randn(LX.PERIOD, L, generator=g) * 4.0
    tp = (torch.rand(LX.PERIOD, L, generator=g) < 0.1).float()
    pw = (0.5 + 3 * torch.rand(L, generator=g)) if asym else None
    X, T_ = ar.view('logits', shape=(n, L)), ar.view('targets', shape=(n, L))
    LX.fill_periodic_rows(X, xp)
    LX.fill_periodic_rows(T_, tp)
    xs = (C.c_void_p * 1)(ar.ptr('logits'))
    gs = (C.c_void_p * 1)(ar.ptr('dlogits'))
    ws = (C.c_float * 1)(1.0)
    if asym:
        ar.view('pos_weight').copy_(pw)
        opts = N.LossOptions(0.0, 4.0, float(IC.f32(0.05)), 0, ar.ptr('pos_weight'))
        ok(N.lib().lamp_multilabel_loss_train(xs, ws, gs, 1, ar.ptr('targets'), n, L, ar.ptr('probs'), L, ar.ptr('row_loss'), n,
                                              C.byref(opts), N.stream()), 'lamp_multilabel_loss_train')
    else:
        ok(N.lib().lamp_bce_logits_train(xs, ws, gs, 1, ar.ptr('targets'), n, L, ar.ptr('probs'), L, ar.ptr('row_loss'), n,
                                         N.stream()), 'lamp_bce_logits_train')
    ar.check_zones()
    for name in ('dlogits', 'probs', 'row_loss'):
        ar.check_written(name)
    D, Pr, R = ar.view('dlogits', shape=(n, L)), ar.view('probs', shape=(n, L)), ar.view('row_loss', shape=(n, 1))
    for v, name in ((D, 'dlogits'), (Pr, 'probs'), (R, 'row_loss')):
        LX.assert_bit_periodic(v, LX.PERIOD, name)
    wins = LX.windows(n, f32(L))
    LX.assert_rows_equal_generator(X, xp, wins, 'logits')
    LX.assert_rows_equal_generator(T_, tp, wins, 'targets')
    idx = LX.window_rows(wins)
    xw, tw = LX.periodic_rows(xp, idx), LX.periodic_rows(tp, idx)
    wgt = [float(len(idx)) / n]      # the references take the mean over the rows they are given: the gradient's 1 / (n L)
    if asym:
        def ref(dt):
            return IC.loss_reference([xw], wgt, tw, 0.0, 4.0, IC.f32(0.05), pw, dt)
    else:
        def ref(dt):
            return TC.bce_reference([xw], wgt, tw, dt)
    p64, g64, r64 = ref(torch.float64)
    p32, g32, r32 = ref(torch.float32)
    name = 'lamp_multilabel_loss_train' if asym else 'lamp_bce_logits_train'
    src = '(bar: %s, train_common.within)' % ('test_imbalance_loss_gpu.py' if asym else 'test_train_gpu.py')
    frac = [TC.within(LX.take_rows(Pr, wins), p64, TC.gap(p32, p64), name + ' probs'),
            TC.within(LX.take_rows(D, wins), g64[0], TC.gap(g32[0], g64[0]), name + ' dlogits'),
            TC.within(LX.take_rows(R, wins).view(1, -1), r64, TC.gap(r32, r64), name + ' row sums')]
    print('large-extent used: %s %s: %.3f' % (name, src, max(frac)))


@pytest.mark.parametrize('asym,fill', [(False, LX.FILL_NAN), (False, LX.FILL_BIG), (True, LX.FILL_NAN)])
def test_loss_train_across_b32(dev, N, asym, fill):
    n, L = LX.BCE_B32
    nb = f32(n * L)
    assert LX.crossings(nb) == ['B31', 'B32']
    ops = [('pos_weight', f32(L)), ('row_loss', f32(n)), ('logits', nb), ('targets', nb), ('dlogits', nb), ('probs', nb)]
    with arena(dev, fill, ops, 'fused loss launch n * L * 4 past 2^32, asymmetric = %s' % asym) as ar:
        _loss_body(ar, N, n, L, asym)


# ====================================================================================== G7: the optimizer launches
# Table rows lamp_grad_norm / lamp_optim_step / lamp_optim_step_ext: every tensor through pointers; a workgroup owns chunk
# blockIdx.x - chunk_start[entry] of 4096 elements, off = int64(chunk) * 4096; guard: 2^31 chunks in a table ->
# LAMP_E_UNSUPPORTED.  The first entry has 2^30 + 4096 + 3 elements: p, g, m and v each cross B32, the table-order chunk counts
# continue past it into two small entries.  Elementwise: periodic tensors, bit-periodic results.
def _flat_fill(view, vals):
    P = vals.numel()
    n = view.numel()
    LX.fill_periodic_rows(view[:n // P * P].view(-1, P), vals.view(1, P))
    view[n // P * P:].copy_(vals[:n - n // P * P])


def _optim_body(ar, N, numels, ext):
    import optim_ext_common as XC
    g = rnd(19)
    P = LX.PERIOD
    names = ['%s%d' % (k, i) for i in range(len(numels)) for k in 'pgmv']
    per = {}
    for i, n in enumerate(numels):
        per['p%d' % i] = torch.randn(P, generator=g)
        gr = torch.randn(P, generator=g) * 0.1
        gr[::7] *= 1e-7
        gr[::11] = 0.0
        per['g%d' % i] = gr
        per['m%d' % i] = torch.zeros(P) if ext else torch.randn(P, generator=g) * 0.05
        per['v%d' % i] = torch.zeros(P) if ext else torch.rand(P, generator=g) * 0.01
    for name in names:
        _flat_fill(ar.view(name), per[name])
    arr = (N.OptimEntry * len(numels))()
    for i, n in enumerate(numels):
        arr[i] = N.OptimEntry(ar.ptr('p%d' % i), ar.ptr('g%d' % i), ar.ptr('m%d' % i), ar.ptr('v%d' % i), n)
    lr, (b1, b2), eps = 2e-3, TC.ADAM_BETAS, 1e-8
    L = N.lib()
    # the exact norm of the periodic gradients: one period's fp64 sum of squares times the repeat count, plus the remainder
    total = 0.0
    for i, n in enumerate(numels):
        sq = per['g%d' % i].double() ** 2
        total += float(sq.sum()) * (n // P) + float(sq[:n % P].sum())
    norm64 = math.sqrt(total)
    if ext:
        step, wd, max_norm = 1, 0.01, 0.5 * norm64
        nb = L.lamp_grad_norm_workspace_bytes(arr, len(numels))
        assert nb == ar.nbytes('norm_ws') == 8 * sum((n + 4095) // 4096 for n in numels)
        ok(L.lamp_grad_norm(arr, len(numels), max_norm, ar.ptr('norm_ws'), nb, ar.ptr('grad_state'), None, N.stream()), 'lamp_grad_norm')
        rec = ar.view('grad_state').cpu()
        # bar: test_optim_ext_gpu.py: one fp32 ulp of the fp64 norm
        err, ulp = abs(float(rec[0]) - norm64), float(TC.ulp32(torch.tensor([norm64], dtype=torch.float64)))
        used('lamp_grad_norm (bar: test_optim_ext_gpu.py, one fp32 ulp)', err, ulp * (1 + 1e-9))
        assert float(rec[2]) == 1.0 and torch.equal(rec[1:2], XC.scale32(rec[0:1], max_norm)) and float(rec[1]) < 1.0
        wds = (C.c_float * len(numels))(*([wd] * len(numels)))
        x = N.OptimExt(wds, ar.ptr('grad_state'), 0.0, N.LAMP_OPTIM_DECOUPLED_DECAY, 0)
        ok(L.lamp_optim_step_ext(arr, len(numels), N.LAMP_OPTIM_ADAM, step, lr, b1, b2, eps, C.byref(x), N.stream()),
           'lamp_optim_step_ext')
        s32 = rec[1]
    else:
        step = 5
        ok(L.lamp_optim_step(arr, len(numels), N.LAMP_OPTIM_ADAM, step, lr, b1, b2, eps, N.stream()), 'lamp_optim_step')
    ar.check_zones()
    worst = 0.0
    for i, n in enumerate(numels):
        G = ar.view('g%d' % i)
        wins = LX.windows(n, 4, LX.FLAT_WINDOW)
        for k in 'pmv':
            if n > P:
                v = ar.view('%s%d' % (k, i))
                LX.assert_bit_periodic(v[:n // P * P].view(-1, P), 1, '%s%d' % (k, i))
        for a, b in wins:
            idx = torch.arange(a, b) % P
            assert torch.equal(G[a:b].cpu(), per['g%d' % i][idx]), 'the gradient buffer changed'
            q, gr, m0, v0 = (per['%s%d' % (k, i)][idx] for k in 'pgmv')
            if ext:
                coef = max_norm / (norm64 + 1e-6)
                want = XC.reference64('adam', [q], [[gr.double() * min(1.0, coef)]], [lr], wd, True)[0]
                cpu, ref = XC.torch_fp32('adam', [q], [[gr * s32]], [lr], wd, True)
                tm, tv = XC.torch_state(ref, cpu[0], 'adam')
                y32 = (cpu[0].detach(), tm, tv)
            else:
                want = TC.adam_reference(q, [gr], [lr], m=m0, v=v0, step0=step - 1)
                m32 = m0 + (gr - m0) * (1 - b1)
                v32 = v0 * b2 + (1 - b2) * gr * gr
                y32 = (q - lr / (1 - b1 ** step) * m32 / (v32.sqrt() / (1 - b2 ** step) ** 0.5 + eps), m32, v32)
            for k, w64, w32 in zip('pmv', want, y32):
                worst = max(worst, TC.within(ar.view('%s%d' % (k, i))[a:b], w64, TC.gap(w32, w64),
                                             '%s[%d] elements [%d, %d)' % (k, i, a, b)))
    print('large-extent used: %s (bar: %s, train_common.within): %.3f'
          % ('lamp_optim_step_ext AdamW + clip' if ext else 'lamp_optim_step Adam',
             'test_optim_ext_gpu.py' if ext else 'test_train_gpu.py', worst))


@pytest.mark.parametrize('ext,fill', [(False, LX.FILL_NAN), (False, LX.FILL_BIG), (True, LX.FILL_NAN)])
def test_optimizer_table_whose_first_entry_crosses_b32(dev, N, ext, fill):
    numels = LX.OPTIM_NUMEL
    assert LX.crossings(f32(numels[0])) == ['B31', 'B32']
    ops = [('grad_state', 16), ('norm_ws', 8 * sum((n + 4095) // 4096 for n in numels))]
    ops += [('%s%d' % (k, i), f32(n)) for i, n in reversed(list(enumerate(numels))) for k in 'pgmv']
    with arena(dev, fill, ops, 'optimizer table with a 2^30 + 4099 element entry, ext = %s' % ext) as ar:
        _optim_body(ar, N, numels, ext)


# ====================================================================================== G1: tile GEMMs
# Table rows lamp_linear_fwd / lamp_linear_prec_fwd: A, W, residual, bias, C through per-tile buffer descriptors whose base is
# advanced in 64 bits (A + m0 * lda, m0 = int64(tile row) * BM) and whose in-tile byte offsets are 32-bit; guards
# max(lda, ldw, ldc) * max(BM, BN) * 4 >= 0x7fffffff and ldr * BM * 4 >= 0x7fffffff -> LAMP_E_UNSUPPORTED (gemm.hip: launch_cfg2,
# gemm_split.hip: launch_split2), tile count > 0x7fffffff -> LAMP_E_DIMS.  No K split: every output element is accumulated by
# one tile in a k order fixed by (K, BK), so a row's bits do not depend on its position: periodic A (and residual), bit-periodic C.
def _linear_call(N, ar, prec, M, K, Nn, full):
    L = N.lib()
    args = (ar.ptr('A'), M, K, K, ar.ptr('W'), Nn, K, ar.ptr('bias') if full else None, ar.ptr('residual') if full else None, Nn,
            int(full), ar.ptr('C'), Nn)
    if prec:
        return L.lamp_linear_prec_fwd(*(args + (prec, N.stream())))
    return L.lamp_linear_fwd(*(args + (N.stream(),)))


def _linear_body(ar, N, prec, M, K, Nn, full):
    g = rnd(21 + K)
    ap = torch.randn(LX.PERIOD, K, generator=g)
    w = torch.randn(Nn, K, generator=g) / K ** 0.5
    b = torch.randn(Nn, generator=g)
    rp = torch.randn(LX.PERIOD, Nn, generator=g)
    A, Cv = ar.view('A', shape=(M, K)), ar.view('C', shape=(M, Nn))
    LX.fill_periodic_rows(A, ap)
    ar.view('W', shape=(Nn, K)).copy_(w)
    if full:
        ar.view('bias').copy_(b)
        LX.fill_periodic_rows(ar.view('residual', shape=(M, Nn)), rp)
    ok(_linear_call(N, ar, prec, M, K, Nn, full), 'lamp_linear%s_fwd' % ('_prec' if prec else ''))
    ar.check_zones()
    ar.check_written('C')
    LX.assert_bit_periodic(Cv, LX.PERIOD, 'C')
    wins = sorted(set(LX.windows(M, f32(K)) + LX.windows(M, f32(Nn))))
    LX.assert_rows_equal_generator(A, ap, wins, 'A')
    if full:
        LX.assert_rows_equal_generator(ar.view('residual', shape=(M, Nn)), rp, wins, 'residual')
    assert torch.equal(ar.view('W', shape=(Nn, K)).cpu(), w)
    idx = torch.cat([torch.arange(a_, b_) for a_, b_ in wins])
    aw = LX.periodic_rows(ap, idx).double()
    prod = aw @ w.double().t()
    ref = prod
    if full:
        ref = (prod + b.double()).clamp_min(0) + LX.periodic_rows(rp, idx).double()
    got = torch.cat([Cv[a_:b_] for a_, b_ in wins]).cpu()
    if prec:
        # bar: test_matmul_precision_gpu.py: _check -- 2^-14 sum |a w| on the product plus one fp32 ulp per epilogue add
        extra = torch.zeros_like(ref)
        if full:
            extra = TC.ulp32(prod + b.double()) + TC.ulp32(ref)
        ratio = float(((got.double() - ref).abs() / (2.0 ** -14 * (aw.abs() @ w.double().abs().t()) + extra + 1e-300)).max())
        used('lamp_linear_prec_fwd bf16x3 M = %d, K = %d, N = %d (bar: test_matmul_precision_gpu.py)' % (M, K, Nn), ratio, 1.0)
    else:
        used('lamp_linear_fwd M = %d, K = %d, N = %d (bar: test_buffer_contracts_gpu.py: test_linear_fwd)' % (M, K, Nn),
             max_abs_diff(got, ref), 2e-5)


@pytest.mark.parametrize('prec', [0, 1])
def test_linear_fwd_a_across_e31(dev, N, prec):
    M, K, Nn = (1 << 22) + 64 + 37, 512, 48
    assert LX.crossings(f32(M * K)) == ['B31', 'B32', 'E31']
    ops = [('W', f32(Nn * K)), ('C', f32(M * Nn)), ('A', f32(M * K))]
    with arena(dev, LX.FILL_NAN, ops, 'linear forward, A past 2^31 elements, precision %d' % prec) as ar:
        _linear_body(ar, N, prec, M, K, Nn, False)


@pytest.mark.parametrize('prec,fill', [(0, LX.FILL_NAN), (0, LX.FILL_BIG), (1, LX.FILL_NAN)])
def test_linear_fwd_c_and_residual_across_b32_full_epilogue(dev, N, prec, fill):
    M, K, Nn = (1 << 20) + 101, 32, 1028
    assert LX.crossings(f32(M * Nn)) == ['B31', 'B32']
    ops = [('W', f32(Nn * K)), ('bias', f32(Nn)), ('A', f32(M * K)), ('residual', f32(M * Nn)), ('C', f32(M * Nn))]
    with arena(dev, fill, ops, 'linear forward, C and residual past 2^32 bytes, precision %d' % prec) as ar:
        _linear_body(ar, N, prec, M, K, Nn, True)


# The largest leading dimensions the 32 x 64 tile admits: ld * 64 * 4 < 0x7fffffff, i.e. ld <= 8388604 (a multiple of 4) --
# derived from the guard's expression, max(BM, BN) = 64 for the tile launch_gemm picks below 1200 64 x 64 tiles.  M = one 32-row
# tile + 3 rows.  Each operand is a strided view into a sentinel-filled allocation: only the rows touched are filled, and the
# padding between the rows of C must keep its sentinel.  One step further (ld + 4) the call is refused and C is untouched.
def _linear_ld_body(ar, N, M, K, Nn, ld, ldr):
    g = rnd(23)
    a, w = torch.randn(M, K, generator=g), torch.randn(Nn, K, generator=g) / K ** 0.5
    b, r = torch.randn(Nn, generator=g), torch.randn(M, Nn, generator=g)

    def strided(name, rows, cols):
        step = ldr if name == 'residual' else ld
        return ar.view(name)[:(rows - 1) * step + cols].as_strided((rows, cols), (step, 1))
    strided('A', M, K).copy_(a)
    strided('W', Nn, K).copy_(w)
    strided('residual', M, Nn).copy_(r)
    ar.view('bias').copy_(b)
    L = N.lib()
    sent = LX._i32(ar.fill)
    def call(lda, ldw, ldr_, ldc):
        return L.lamp_linear_fwd(ar.ptr('A'), M, K, lda, ar.ptr('W'), Nn, ldw, ar.ptr('bias'), ar.ptr('residual'), ldr_, 1, ar.ptr('C'),
                                 ldc, N.stream())
    for what, rc in (('lda', call(ld + 4, ld, ldr, ld)), ('ldw', call(ld, ld + 4, ldr, ld)), ('ldr', call(ld, ld, ldr + 4, ld)),
                     ('ldc', call(ld, ld, ldr, ld + 4))):
        assert rc == -4, '%s one step past the guard: expected LAMP_E_UNSUPPORTED, got %d' % (what, rc)
    ar.check_untouched('C')
    ok(call(ld, ld, ldr, ld), 'lamp_linear_fwd')
    ar.check_zones()
    Cv = strided('C', M, Nn)
    got = Cv.cpu()
    assert not bool((got.view(torch.int32) == sent).any()), 'an element of C was never written'
    pad = ar.view('C', torch.int32)[:(M - 1) * ld + Nn].as_strided((M - 1, ld - Nn), (ld, 1), ar.view('C', torch.int32).storage_offset() + Nn)
    assert bool((pad == sent).all()), 'the padding between the rows of C was written'
    assert torch.equal(strided('A', M, K).cpu(), a) and torch.equal(strided('residual', M, Nn).cpu(), r)
    ref = (a.double() @ w.double().t() + b.double()).clamp_min(0) + r.double()
    used('lamp_linear_fwd at the largest admitted leading dimensions (bar: test_buffer_contracts_gpu.py: test_linear_fwd)',
         max_abs_diff(got, ref), 2e-5)


def test_linear_fwd_largest_admitted_leading_dimensions(dev, N):
    M, K, Nn = 35, 64, 68
    ld = (0x7fffffff - 1) // (64 * 4) // 4 * 4
    ldr = (0x7fffffff - 1) // (32 * 4) // 4 * 4          # the residual's own guard: ldr * BM * 4, BM = 32
    assert ld * 64 * 4 < 0x7fffffff <= (ld + 4) * 64 * 4 and ld == 8388604
    assert ldr * 32 * 4 < 0x7fffffff <= (ldr + 4) * 32 * 4 and ldr == 16777212
    ops = [('bias', f32(Nn)), ('A', f32((M - 1) * ld + K)), ('residual', f32((M - 1) * ldr + Nn)), ('C', f32((M - 1) * ld + Nn)),
           ('W', f32((Nn - 1) * ld + K))]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_linear_fwd, lda = ldw = ldc = %d, ldr = %d' % (ld, ldr)) as ar:
        _linear_ld_body(ar, N, M, K, Nn, ld, ldr)


# Table row lamp_ffn_fwd (the eval composite: two launches of the tile GEMM and the LayerNorm through one entry point): its
# hidden rows [M, d_inner] live in the caller's workspace of exactly lamp_ffn_workspace_bytes() and cross B32 here; x and out
# are small.  Row-local, no split K: periodic x gives a bit-periodic out.
def _ffn_body(ar, N, M, d, dff):
    g = rnd(47)
    w = dict(w1=torch.randn(dff, d, generator=g) * 0.1, b1=torch.randn(dff, generator=g) * 0.1,
             w2=torch.randn(d, dff, generator=g) * 0.1, b2=torch.randn(d, generator=g) * 0.1,
             ln_g=1 + 0.1 * torch.randn(d, generator=g), ln_b=0.1 * torch.randn(d, generator=g))
    for k, t in w.items():
        ar.view(k).copy_(t.reshape(-1))
    period = torch.randn(LX.PERIOD, d, generator=g)
    X = ar.view('x', shape=(M, d))
    LX.fill_periodic_rows(X, period)
    wts = N.FfnWeights(*[ar.ptr(k) for k in ('w1', 'b1', 'w2', 'b2', 'ln_g', 'ln_b')])
    ok(N.lib().lamp_ffn_fwd(ar.ptr('x'), M, d, dff, C.byref(wts), ar.ptr('out'), ar.ptr('workspace'), ar.nbytes('workspace'),
                            N.stream()), 'lamp_ffn_fwd')
    ar.check_zones()
    ar.check_written('out')
    out = ar.view('out', shape=(M, d))
    LX.assert_bit_periodic(out, LX.PERIOD, 'lamp_ffn_fwd out')
    wins = LX.windows(M, f32(dff))                  # the rows whose hidden rows lie on either side of B31 and B32
    LX.assert_rows_equal_generator(X, period, wins, 'lamp_ffn_fwd x')
    for k, t in w.items():
        assert torch.equal(ar.view(k).cpu(), t.reshape(-1)), k + ' changed'
    x = LX.periodic_rows(period, LX.window_rows(wins)).double()
    h = torch.relu(x @ w['w1'].double().t() + w['b1'].double())
    ref = F.layer_norm(h @ w['w2'].double().t() + w['b2'].double() + x, (d,), w['ln_g'].double(), w['ln_b'].double(), 1e-5)
    used('lamp_ffn_fwd (bar: test_buffer_contracts_gpu.py: test_ffn_fwd_exact_workspace)', max_abs_diff(LX.take_rows(out, wins), ref), 5e-5)


def test_ffn_fwd_hidden_rows_in_the_workspace_across_b32(dev, N):
    M, d, dff = (1 << 20) + 101, 64, 1028
    ws = N.lib().lamp_ffn_workspace_bytes(M, d, dff)
    assert ws == (f32(M * dff) + 255) // 256 * 256 and LX.crossings(f32(M * dff)) == ['B31', 'B32']
    ops = [('w1', f32(dff * d)), ('b1', f32(dff)), ('w2', f32(d * dff)), ('b2', f32(d)), ('ln_g', f32(d)), ('ln_b', f32(d)),
           ('x', f32(M * d)), ('out', f32(M * d)), ('workspace', ws)]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_ffn_fwd, hidden rows past 2^32 bytes') as ar:
        _ffn_body(ar, N, M, d, dff)


# ====================================================================================== G3: attention
# Table rows lamp_sdpa_fwd / lamp_sdpa_fwd_fast_maps / lamp_sdpa_act_fwd: Q, K, V (and a mask or bias) through one buffer
# descriptor per (sample, head) slice whose base is advanced in 64 bits (p.Q + int64(b) * q_b + int64(h) * q_h); O and P through
# pointers, the slice offset (h * P_batch + b) * lq * lk in 64 bits.  Guards (attention.hip: launch_attn): the 32-bit offsets
# inside ONE slice, and the workgroup count > 0x7fffffff -> LAMP_E_DIMS.  The aggregate tensors grow through B * H at small
# per-slice shapes.  A slice's result does not depend on its position (the key split is chosen from the per-sample shape), so
# the operands are periodic over slices with period 13 and O / P must be bit-periodic; head-major contiguous tensors, slice
# index h * B + b as in the maps.
SLICES = 13
ATTN_CASES = {
    # name: (entry, lq, lk, dk, dv, maps, mask, aggregate that crosses, boundary)
    'small16_out': ('sdpa', 100, 40, 32, 32, None, 'none', 'O', LX.B32),         # attention_small.hip, 16-query blocks
    'attn32_out': ('sdpa', 300, 70, 32, 32, None, 'none', 'O', LX.B32),          # attn_kernel<32, 1, 0>
    'attn32_exact_maps': ('sdpa', 300, 300, 32, 32, 'exact', 'u8', 'P', LX.B32),  # attn_kernel<32, 1, 1>: exact two-pass maps
    'attn32_fast_maps': ('sdpa', 300, 300, 32, 32, 'fast', 'u8', 'P', LX.B32),   # attn_kernel<32, 1, 2> + softmax_from_scores
    'small16_fast_maps_e31': ('sdpa', 100, 300, 32, 32, 'fast', 'u8', 'P', LX.E31),  # the 16-query single-pass write-out
    'tile_out': ('sdpa', 300, 300, 128, 128, None, 'none', 'O', LX.B32),         # attention_tile.hip
    'sigmoid_maps': ('act', 300, 300, 32, 32, 'exact', 'u8', 'P', LX.B32),       # attention_sigmoid.hip
    'bias_maps': ('sdpa', 300, 300, 32, 32, 'exact', 'bias', 'P', LX.B32),       # attention_bias.hip
    'general_maps': ('sdpa', 300, 300, 132, 132, 'exact', 'u8', 'P', LX.B32),    # attention_general.hip (d_k > 128)
    # attention_sparse.hip, the pair kernel: a shared bit-packed mask flagged LAMP_MASK_SPARSE_ROWS, heads of exactly 128, at least
    # 1024 keys, no maps.  Q and O cross B32; K and V are ONE [lk, 128] slice that every (sample, head) reads (k_b = k_h = 0), so the
    # aggregate grows through B * H alone
    'pair_out': ('sdpa', 64, 1030, 128, 128, None, 'sparse_bits', 'O', LX.B32),
}


def _attn_shapes(name):
    entry, lq, lk, dk, dv, maps, mask, agg, at = ATTN_CASES[name]
    per_slice = {'O': lq * dv, 'P': lq * lk}[agg] * 4
    H = 4
    B = (at // per_slice + 2 * SLICES) // H + 1
    return entry, lq, lk, dk, dv, maps, mask, agg, at, B, H


def _attn_operands(name):
    entry, lq, lk, dk, dv, maps, mask, agg, at, B, H = _attn_shapes(name)
    n = B * H
    nkv = 1 if mask == 'sparse_bits' else n
    ops = [('mask', lq * lk if mask == 'u8' else f32(lq * ((lk + 3) & ~3)) if mask == 'bias' else
            f32(lq * ((lk + 31) // 32)) if mask == 'sparse_bits' else 0),
           ('lse', f32(n * lq) if maps == 'fast' else 0), ('q', f32(n * lq * dk)), ('k', f32(nkv * lk * dk)), ('v', f32(nkv * lk * dv)),
           ('o', f32(n * lq * dv)), ('attn', f32(n * lq * lk) if maps else 0)]
    return [(k, b) for k, b in ops if b]


def _attn_body(ar, N, name):
    import attn_routes_common as AR
    entry, lq, lk, dk, dv, maps, mask, agg, at, B, H = _attn_shapes(name)
    n = B * H
    g = rnd(31 + lq + lk + dk)
    shared = mask == 'sparse_bits'                  # one K / V slice for every (sample, head)
    nkv = 1 if shared else n
    qp = torch.randn(SLICES, lq * dk, generator=g)
    kp, vp = (torch.randn(1 if shared else SLICES, lk * w, generator=g) for w in (dk, dv))
    LX.fill_periodic_rows(ar.view('q', shape=(n, lq * dk)), qp)
    LX.fill_periodic_rows(ar.view('k', shape=(nkv, lk * dk)), kp)
    LX.fill_periodic_rows(ar.view('v', shape=(nkv, lk * dv)), vp)
    scale = dk ** -0.5
    lay = N.AttnLayout(lq * dk, B * lq * dk, dk, lk * dk, B * lk * dk, dk, lk * dv, B * lk * dv, dv, lq * dv, B * lq * dv, dv)
    if shared:
        lay.k_b = lay.k_h = lay.v_b = lay.v_h = 0
    mp, blocked, bias = None, None, None
    if shared:
        blocked = torch.rand(lq, lk, generator=g) >= 0.05
        blocked[:, 0] = False
        blocked[3, :] = True
        blocked[3, lk - 1] = False                  # a row whose one allowed key is the last
        words = N.pack_mask_bits(blocked.to(torch.uint8))
        ar.view('mask', torch.int32).copy_(words.view(-1))
        mp = N.Mask(N.LAMP_MASK_BITS_U32, N.LAMP_MASK_SPARSE_ROWS, ar.ptr('mask'), 0, words.size(1), None, 0, int((~blocked).sum()))
    if mask == 'u8':
        blocked = torch.rand(lq, lk, generator=g) < 0.3
        blocked[:, 0] = False
        ar.view('mask', torch.uint8).copy_(blocked.to(torch.uint8).view(-1))
        mp = N.Mask(N.LAMP_MASK_U8, 0, ar.ptr('mask'), 0, lk, None, 0, 0)
    elif mask == 'bias':
        ld = (lk + 3) & ~3
        bias = torch.randn(lq, lk, generator=g).masked_fill(torch.rand(lq, lk, generator=g) < 0.2, float('-inf'))
        bias[:, 0] = 0.0
        ar.view('mask', shape=(lq, ld))[:, :lk].copy_(bias)
        mp = N.Mask(N.LAMP_MASK_BIAS_F32, 0, ar.ptr('mask'), 0, ld, None, 0, 0)
    mref = None if mp is None else C.byref(mp)
    L = N.lib()
    pa = ar.ptr('attn') if maps else None
    if entry == 'act':
        ok(L.lamp_sdpa_act_fwd(ar.ptr('q'), ar.ptr('k'), ar.ptr('v'), ar.ptr('o'), pa, B, H, lq, lk, dk, dv, scale, N.LAMP_ATTN_SIGMOID,
                               mref, C.byref(lay), N.stream()), 'lamp_sdpa_act_fwd')
    elif maps == 'fast':
        ok(L.lamp_sdpa_fwd_fast_maps(ar.ptr('q'), ar.ptr('k'), ar.ptr('v'), ar.ptr('o'), pa, ar.ptr('lse'), B, H, lq, lk, dk, dv, scale,
                                     mref, C.byref(lay), N.stream()), 'lamp_sdpa_fwd_fast_maps')
    else:
        if shared:
            N.prof_enable(True)
            N.prof_reset()
        try:
            ok(L.lamp_sdpa_fwd(ar.ptr('q'), ar.ptr('k'), ar.ptr('v'), ar.ptr('o'), pa, B, H, lq, lk, dk, dv, scale, mref, C.byref(lay),
                               N.stream()), 'lamp_sdpa_fwd')
            if shared:      # the route: only the pair kernel counts the allowed pairs as executed, every other one lq * lk
                torch.cuda.synchronize()
                prof = N.prof_read()
                assert sum(int(v['launches']) for v in prof.values()) == 1
                assert sum(v['flops'] for v in prof.values()) == 2.0 * B * H * int((~blocked).sum()) * (dk + dv) < 2.0 * B * H * lq * lk * (dk + dv)
        finally:
            if shared:
                N.prof_enable(False)
    ar.check_zones()
    ar.check_written('o')
    O = ar.view('o', shape=(n, lq * dv))
    LX.assert_bit_periodic(O, SLICES, name + ' O')
    Pm = None
    if maps:
        ar.check_written('attn')
        Pm = ar.view('attn', shape=(n, lq * lk))
        LX.assert_bit_periodic(Pm, SLICES, name + ' maps')
    if maps == 'fast':
        ar.check_written('lse')
        LX.assert_bit_periodic(ar.view('lse', shape=(n, lq)), SLICES, name + ' lse')
    wins = LX.windows(n, {'O': lq * dv, 'P': lq * lk}[agg] * 4, width=2)
    assert len(wins) >= 3
    kv_wins = [(0, 1)] if shared else wins
    for v, per, what, w_ in ((ar.view('q', shape=(n, lq * dk)), qp, 'q', wins), (ar.view('k', shape=(nkv, lk * dk)), kp, 'k', kv_wins),
                             (ar.view('v', shape=(nkv, lk * dv)), vp, 'v', kv_wins)):
        LX.assert_rows_equal_generator(v, per, w_, name + ' ' + what)
    idx = LX.window_rows(wins) % SLICES
    ikv = idx * 0 if shared else idx
    q, k, v = qp[idx].double().view(-1, lq, dk), kp[ikv].double().view(-1, lk, dk), vp[ikv].double().view(-1, lk, dv)
    s = q @ k.transpose(-1, -2) * scale
    if bias is not None:
        s = s + bias.double()
    if blocked is not None:
        s = s.masked_fill(blocked, float('-inf'))
    ref_p = torch.sigmoid(s) if entry == 'act' else torch.softmax(s, -1)
    ref_o = ref_p @ v
    wide = dk > 128
    tol_out, tol_map = (5e-5, 1e-5) if wide else (2e-5, None) if shared else (AR.TOL_OUT, AR.TOL_MAP)
    src = 'test_buffer_contracts_gpu.py: ' + ('test_sdpa_pair_kernel' if shared else 'check_sdpa' + (
        ' (wide heads)' if wide else ', attn_routes_common.TOL_OUT / TOL_MAP'))
    used('%s O (bar: %s)' % (name, src), max_abs_diff(LX.take_rows(O, wins).view(-1, lq, dv), ref_o), tol_out)
    if maps:
        used('%s maps (bar: %s)' % (name, src), max_abs_diff(LX.take_rows(Pm, wins).view(-1, lq, lk), ref_p), tol_map)


@pytest.mark.parametrize('name,fill', [(k, LX.FILL_NAN) for k in sorted(ATTN_CASES)] + [('attn32_exact_maps', LX.FILL_BIG)])
def test_attention_aggregates_across_the_boundaries(dev, N, name, fill):
    ops = _attn_operands(name)
    entry, lq, lk, dk, dv, maps, mask, agg, at, B, H = _attn_shapes(name)
    crossed = dict(ops)['attn' if agg == 'P' else 'o']
    assert crossed > at + 2 * SLICES * 4 and H * B <= 0x7fffffff
    with arena(dev, fill, ops, 'attention %s, B = %d, H = %d' % (name, B, H)) as ar:
        _attn_body(ar, N, name)


# The per-slice guards of the same rows (attention.hip: launch_attn), one step inside, through a large row stride: inside ONE
# (sample, head) slice the byte offsets are 32-bit, so lq * q_r * 4, lk * k_r * 4, lk * v_r * 4, (lq * stride_q + lk) bytes of a u8
# mask (x 4 for bit-packed words) and (lq * stride_q + lk + 3) * 4 of a bias must stay below 0x7fffffff.  The largest admitted
# values follow from those expressions (strides are multiples of 4 floats): with lq = lk = 300, r = 1789568 for Q / K / V
# (300 * 1789568 * 4 = 2147481600; r + 4 gives 2147486400), stride_q = 7158276 for the byte mask (300 * 7158276 + 300 =
# 2147483100; + 4: 2147484300), 1789568 for the bit-packed words and for the bias.  Each case strides ONE of Q, K, V and its
# mask that far: the operand is a strided view into the sentinel-filled arena, only the rows touched are filled.  One step
# further the call is refused and O still holds the sentinel.
STRIDE_CASES = {'u8': ('q', 7158276), 'bits': ('k', 1789568), 'bias': ('v', 1789568)}


def _attn_stride_body(ar, N, kind, lq, lk, dk, H, r_max):
    which, sq = STRIDE_CASES[kind]
    g = rnd(43)
    hd = H * dk
    src = dict((nm, torch.randn(l, hd, generator=g)) for nm, l in (('q', lq), ('k', lk), ('v', lk)))
    ld = dict((nm, r_max if nm == which else hd) for nm in src)

    def strided(nm):
        rows = src[nm].shape[0]
        return ar.view(nm)[:(rows - 1) * ld[nm] + hd].as_strided((rows, hd), (ld[nm], 1))
    for nm in src:
        strided(nm).copy_(src[nm])
    blocked = torch.rand(lq, lk, generator=g) < 0.3
    blocked[:, 0] = False
    bias = None
    if kind == 'u8':
        ar.view('mask', torch.uint8)[:(lq - 1) * sq + lk].as_strided((lq, lk), (sq, 1)).copy_(blocked.to(torch.uint8))
        code = N.LAMP_MASK_U8
    elif kind == 'bits':
        words = N.pack_mask_bits(blocked.to(torch.uint8))
        nw = words.size(1)
        ar.view('mask', torch.int32)[:(lq - 1) * sq + nw].as_strided((lq, nw), (sq, 1)).copy_(words)
        code = N.LAMP_MASK_BITS_U32
    else:
        bias = torch.randn(lq, lk, generator=g).masked_fill(blocked, float('-inf'))
        ar.view('mask')[:(lq - 1) * sq + lk].as_strided((lq, lk), (sq, 1)).copy_(bias)
        code = N.LAMP_MASK_BIAS_F32
    L = N.lib()

    def call(lds, m_sq):
        lay = N.AttnLayout(lq * lds['q'], dk, lds['q'], lk * lds['k'], dk, lds['k'], lk * lds['v'], dk, lds['v'], lq * hd, dk, hd)
        mp = N.Mask(code, 0, ar.ptr('mask'), 0, m_sq, None, 0, 0)
        return L.lamp_sdpa_fwd(ar.ptr('q'), ar.ptr('k'), ar.ptr('v'), ar.ptr('o'), None, 1, H, lq, lk, dk, dk, dk ** -0.5, C.byref(mp),
                               C.byref(lay), N.stream())
    over = dict(ld)
    over[which] = r_max + 4
    for what, rc in (('row stride', call(over, sq)), ('mask stride', call(ld, sq + 4))):
        assert rc == -4, '%s one step past the guard: expected LAMP_E_UNSUPPORTED, got %d' % (what, rc)
    ar.check_untouched('o')
    ok(call(ld, sq), 'lamp_sdpa_fwd')
    ar.check_zones()
    ar.check_written('o')
    for nm in src:
        assert torch.equal(strided(nm).cpu(), src[nm]), nm + ' changed'
    heads = lambda t, l: t.double().view(l, H, dk).permute(1, 0, 2)  # noqa: E731
    s = heads(src['q'], lq) @ heads(src['k'], lk).transpose(-1, -2) * dk ** -0.5
    s = s + bias.double() if bias is not None else s.masked_fill(blocked, float('-inf'))
    ref = (torch.softmax(s, -1) @ heads(src['v'], lk)).permute(1, 0, 2).reshape(lq, hd)
    import attn_routes_common as AR
    used('attention slice guard %s, %s_r = %d, stride_q = %d (bar: test_buffer_contracts_gpu.py: check_sdpa, TOL_OUT)'
         % (kind, which, r_max, sq), max_abs_diff(ar.view('o', shape=(lq, hd)), ref), AR.TOL_OUT)


@pytest.mark.parametrize('kind', sorted(STRIDE_CASES))
def test_attention_slice_guards_one_step_inside_through_a_large_row_stride(dev, N, kind):
    lq = lk = 300
    dk, H, lim = 32, 2, 0x7fffffff
    hd = H * dk
    r_max = (lim - 1) // (4 * lq) // 4 * 4
    which, sq = STRIDE_CASES[kind]
    assert lq * r_max * 4 < lim <= lq * (r_max + 4) * 4 and r_max == 1789568
    unit, extra = {'u8': (1, 0), 'bits': (4, 0), 'bias': (4, 3)}[kind]
    assert (lq * sq + lk + extra) * unit < lim <= (lq * (sq + 4) + lk + extra) * unit and sq % 4 == 0
    cols = (lk + 31) // 32 if kind == 'bits' else lk
    ops = [(nm, f32((l - 1) * (r_max if nm == which else hd) + hd)) for nm, l in (('q', lq), ('k', lk), ('v', lk))]
    ops += [('o', f32(lq * hd)), ('mask', ((lq - 1) * sq + cols) * unit)]
    with arena(dev, LX.FILL_NAN, ops, 'attention slice guards, %s mask' % kind) as ar:
        _attn_stride_body(ar, N, kind, lq, lk, dk, H, r_max)


# ====================================================================================== G2: lamp_gemm / lamp_gemm_grouped
# Table rows lamp_gemm / lamp_gemm_grouped: A, B, C (relu_mask, split-K partials) through per-tile buffer descriptors, bases
# advanced in 64 bits (A + int64(m0) * lda, the batch strides z0 * a_batch0 + z1 * a_batch1), 32-bit offsets inside a tile.
# Guards (gemm_gen.hip: launch_gemm_gen / launch_gemm_group): (64 * ld + K) * 4 of a k-contiguous operand, K * ld * 4 of a
# k-strided one, 64 * ldc * 4, 64 * ld_mask * 4, each >= 0x7fffffff -> LAMP_E_UNSUPPORTED; batch0 * batch1 > 65535 -> LAMP_E_DIMS.
def _gemm(N, ar, M, Nn, K, a, b, c, ldc, ws=None, batch=(1, 1), accumulate=0, mask=None, ld_mask=0):
    """a / b: (operand name, row stride, col stride, batch0 stride, batch1 stride); c: (name, batch0 stride, batch1 stride)."""
    d = N.GemmDesc(ar.ptr(a[0]), ar.ptr(b[0]), ar.ptr(c[0]), M, Nn, K, batch[0], batch[1], accumulate, a[1], a[2], a[3], a[4],
                   b[1], b[2], b[3], b[4], ldc, c[1], c[2], None if mask is None else ar.ptr(mask), ld_mask, 1.0, 0)
    nb = ar.nbytes(ws) if ws else 0
    return N.lib().lamp_gemm(C.byref(d), ar.ptr(ws) if nb else None, nb, N.stream())


def _gemm_row_major_body(ar, N, M, K, Nn):
    """dX = dY . W with its ReLU mask: A = dY [M, K] row-major past 2^32 bytes, B(n, k) = W[k, n] k-strided, no workspace (no K
    split: every tile accumulates k in ascending order whatever its position, so periodic A and mask give a bit-periodic C)."""
    g = rnd(41)
    ap, w = torch.randn(LX.PERIOD, K, generator=g), torch.randn(K, Nn, generator=g) / K ** 0.5
    hp = torch.randn(LX.PERIOD, Nn, generator=g)
    A, Cv = ar.view('A', shape=(M, K)), ar.view('C', shape=(M, Nn))
    LX.fill_periodic_rows(A, ap)
    LX.fill_periodic_rows(ar.view('relu_mask', shape=(M, Nn)), hp)
    ar.view('B', shape=(K, Nn)).copy_(w)
    ok(_gemm(N, ar, M, Nn, K, ('A', K, 1, 0, 0), ('B', 1, Nn, 0, 0), ('C', 0, 0), Nn, mask='relu_mask', ld_mask=Nn), 'lamp_gemm')
    ar.check_zones()
    ar.check_written('C')
    LX.assert_bit_periodic(Cv, LX.PERIOD, 'C')
    wins = LX.windows(M, f32(K))
    LX.assert_rows_equal_generator(A, ap, wins, 'A')
    idx = LX.window_rows(wins)
    ref = (LX.periodic_rows(ap, idx).double() @ w.double()) * (LX.periodic_rows(hp, idx).double() > 0)
    used('lamp_gemm row-major A, relu_mask (bar: test_buffer_contracts_gpu.py: test_gemm_relu_mask_accumulate_alpha_strided)',
         max_abs_diff(LX.take_rows(Cv, wins), ref), 1e-4)


@pytest.mark.parametrize('fill', LX.FILLS)
def test_gemm_row_major_a_across_b32(dev, N, fill):
    M, K, Nn = (1 << 20) + 101, 1028, 64
    assert LX.crossings(f32(M * K)) == ['B31', 'B32']
    ops = [('B', f32(K * Nn)), ('C', f32(M * Nn)), ('relu_mask', f32(M * Nn)), ('A', f32(M * K))]
    with arena(dev, fill, ops, 'lamp_gemm, row-major A past 2^32 bytes') as ar:
        _gemm_row_major_body(ar, N, M, K, Nn)


def _gemm_k_strided_body(ar, N, M, Nn, K, lda):
    """dW = dY^T . X: A(m, k) = dY[k, m] with rows lda floats apart, one step inside K * lda * 4 < 0x7fffffff, and a split-K
    workspace of exactly lamp_gemm_workspace_bytes().  One step further the call is refused and nothing is written."""
    g = rnd(43)
    dy, x = torch.randn(K, M, generator=g), torch.randn(K, Nn, generator=g)
    Av = ar.view('A')[:(K - 1) * lda + M].as_strided((K, M), (lda, 1))
    Av.copy_(dy)
    ar.view('B', shape=(K, Nn)).copy_(x)
    rc = _gemm(N, ar, M, Nn, K, ('A', 1, lda + 1, 0, 0), ('B', 1, Nn, 0, 0), ('C', 0, 0), Nn, ws='workspace')
    assert rc == -4, 'a_col_stride one step past the guard: expected LAMP_E_UNSUPPORTED, got %d' % rc
    ar.check_untouched('C')
    ar.check_untouched('workspace')
    ok(_gemm(N, ar, M, Nn, K, ('A', 1, lda, 0, 0), ('B', 1, Nn, 0, 0), ('C', 0, 0), Nn, ws='workspace'), 'lamp_gemm')
    ar.check_zones()
    ar.check_written('C')
    assert torch.equal(Av.cpu(), dy) and torch.equal(ar.view('B', shape=(K, Nn)).cpu(), x)
    sent = LX._i32(ar.fill)
    w32 = ar.view('A', torch.int32)
    pad = w32[:(K - 1) * lda + M].as_strided((K - 1, lda - M), (lda, 1), w32.storage_offset() + M)
    assert bool((pad == sent).all()), 'the padding between the rows of A changed'
    used('lamp_gemm k-strided A, split K (bar: test_buffer_contracts_gpu.py: test_gemm_split_k_..., 3e-5 sqrt(K))',
         max_abs_diff(ar.view('C', shape=(M, Nn)), dy.double().t() @ x.double()), 3e-5 * K ** 0.5)


def test_gemm_k_strided_one_step_inside_its_guard(dev, N):
    M, Nn, K = 67, 70, 4096
    lda = (0x7fffffff - 1) // 4 // K
    assert K * lda * 4 < 0x7fffffff <= K * (lda + 1) * 4 and lda == 131071
    ws = N.lib().lamp_gemm_workspace_bytes(M, Nn, K, 1)
    assert ws >= 2 * M * Nn * 4
    ops = [('C', f32(M * Nn)), ('workspace', ws), ('B', f32(K * Nn)), ('A', f32((K - 1) * (lda + 1) + M))]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_gemm, k-strided A with lda = %d' % lda) as ar:
        _gemm_k_strided_body(ar, N, M, Nn, K, lda)


def _gemm_batched_body(ar, N, B, H, lq, lk, dv):
    """dV += P^T . dO over (head, sample) views of head-major tensors: the batch strides carry P across 2^32 bytes; accumulate."""
    g = rnd(45)
    n = H * B
    pp = torch.softmax(torch.randn(SLICES, lq, lk, generator=g), -1).view(SLICES, -1)
    gp, cp = torch.randn(SLICES, lq * dv, generator=g), torch.randn(SLICES, lk * dv, generator=g)
    Pv, Gv, Cv = ar.view('P', shape=(n, lq * lk)), ar.view('dO', shape=(n, lq * dv)), ar.view('dV', shape=(n, lk * dv))
    for v, per in ((Pv, pp), (Gv, gp), (Cv, cp)):
        LX.fill_periodic_rows(v, per)
    ok(_gemm(N, ar, lk, dv, lq, ('P', 1, lk, B * lq * lk, lq * lk), ('dO', 1, dv, B * lq * dv, lq * dv),
             ('dV', B * lk * dv, lk * dv), dv, batch=(H, B), accumulate=1), 'lamp_gemm')
    ar.check_zones()
    LX.assert_bit_periodic(Cv, SLICES, 'dV')
    wins = LX.windows(n, f32(lq * lk), width=2)
    LX.assert_rows_equal_generator(Pv, pp, wins, 'P')
    LX.assert_rows_equal_generator(Gv, gp, wins, 'dO')
    idx = LX.window_rows(wins) % SLICES
    ref = pp[idx].double().view(-1, lq, lk).transpose(-1, -2) @ gp[idx].double().view(-1, lq, dv) + cp[idx].double().view(-1, lk, dv)
    used('lamp_gemm batched head views, accumulate (bar: test_buffer_contracts_gpu.py: test_gemm_batched_head_views)',
         max_abs_diff(LX.take_rows(Cv, wins).view(-1, lk, dv), ref), 1e-4)


def test_gemm_batched_head_views_across_b32(dev, N):
    H, lq, lk, dv = 4, 300, 300, 32
    B = (LX.B32 // f32(lq * lk) + 2 * SLICES) // H + 1
    assert H * B <= 65535 and LX.crossings(f32(H * B * lq * lk)) == ['B31', 'B32']
    ops = [('dV', f32(H * B * lk * dv)), ('dO', f32(H * B * lq * dv)), ('P', f32(H * B * lq * lk))]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_gemm, batched views, P past 2^32 bytes') as ar:
        _gemm_batched_body(ar, N, B, H, lq, lk, dv)


def test_gemm_grouped_with_one_description_beyond_a_guard_writes_nothing(dev, N):
    """Three weight-gradient products in one call; the LAST one's k-strided A one step past K * lda * 4 < 0x7fffffff: the whole
    call is refused before its launch and no C holds anything but the sentinel."""
    M, Nn, K = 64, 64, 4096
    lda = (0x7fffffff - 1) // 4 // K + 1
    ops = [('C%d' % i, f32(M * Nn)) for i in range(3)] + [('A', f32(K * M)), ('B', f32(K * Nn))]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_gemm_grouped, refused') as ar:
        ar.view('A').normal_()
        ar.view('B').normal_()
        descs = (N.GemmDesc * 3)()
        for i in range(3):
            descs[i] = N.GemmDesc(ar.ptr('A'), ar.ptr('B'), ar.ptr('C%d' % i), M, Nn, K, 1, 1, 0, 1, lda if i == 2 else M, 0, 0, 1, Nn,
                                  0, 0, Nn, 0, 0, None, 0, 1.0, 0)
        assert N.lib().lamp_gemm_grouped(descs, 3, N.stream()) == -4
        for i in range(3):
            ar.check_untouched('C%d' % i)
        ar.check_zones()
        descs[2].a_col_stride = M
        ok(N.lib().lamp_gemm_grouped(descs, 3, N.stream()), 'lamp_gemm_grouped')
        ref = ar.view('A', shape=(K, M)).double().t() @ ar.view('B', shape=(K, Nn)).double()
        for i in range(3):
            ar.check_written('C%d' % i)
            used('lamp_gemm_grouped C%d (bar: test_buffer_contracts_gpu.py: test_gemm_grouped, 3e-5 x 4 sqrt(K))' % i,
                 max_abs_diff(ar.view('C%d' % i, shape=(M, Nn)), ref), 3e-5 * K ** 0.5 * 4)


# ====================================================================================== G6: the evaluation's metrics
# Table rows lamp_topk_labels / lamp_rank_at_k / lamp_threshold_counts(_vec) / lamp_ranking_metrics / lamp_tune_thresholds:
# the (n, L) matrices through pointers, row offsets r * ld in 64 bits; guards n_rows >= 2^31 -> LAMP_E_UNSUPPORTED.  The (n, 919)
# probability and target matrices are periodic along rows and cross B32.  Per-row outputs are held on row windows (and must be
# bit-periodic); per-label integer counts against the exact count-weighted sums of one period; the sorted-column figures for the
# first, the last and two middle columns, each on its whole column copied back (n floats) in fp64 on the CPU.
def _metric_inputs(ar, n, L):
    g = rnd(51)
    pp = torch.rand(LX.PERIOD, L, generator=g)
    tp = (torch.rand(LX.PERIOD, L, generator=g) < 0.1).float()
    LX.fill_periodic_rows(ar.view('probs', shape=(n, L)), pp)
    LX.fill_periodic_rows(ar.view('targets', shape=(n, L)), tp)
    count = torch.full((LX.PERIOD,), n // LX.PERIOD, dtype=torch.int64)
    count[:n % LX.PERIOD] += 1
    return pp, tp, count


def _metric_inputs_unchanged(ar, n, L, pp, tp):
    wins = LX.windows(n, f32(L))
    LX.assert_rows_equal_generator(ar.view('probs', shape=(n, L)), pp, wins, 'probs')
    LX.assert_rows_equal_generator(ar.view('targets', shape=(n, L)), tp, wins, 'targets')
    return wins


def _topk_rank_body(ar, N, n, L, k):
    import numpy as np
    import rank_at_k_common as RK
    pp, tp, count = _metric_inputs(ar, n, L)
    lib = N.lib()
    ok(lib.lamp_topk_labels(ar.ptr('probs'), L, n, L, k, ar.ptr('idx'), k, ar.ptr('val'), k, N.stream()), 'lamp_topk_labels')
    d, ideal = RK.dcg_tables(k)
    dh, ih = (C.c_double * k)(*d.tolist()), (C.c_double * (k + 1))(*ideal.tolist())
    ok(lib.lamp_rank_at_k(ar.ptr('idx'), k, ar.ptr('targets'), L, n, L, k, dh, ih, ar.ptr('hits'), ar.ptr('ndcg'), ar.ptr('recall'),
                          ar.ptr('with_gold'), ar.ptr('workspace'), ar.nbytes('workspace'), N.stream()), 'lamp_rank_at_k')
    ar.check_zones()
    for name in ('idx', 'val', 'hits', 'ndcg', 'recall', 'with_gold'):
        ar.check_written(name)
    idx, val = ar.view('idx', torch.int32, (n, k)), ar.view('val', shape=(n, k))
    LX.assert_bit_periodic(idx, LX.PERIOD, 'idx')
    LX.assert_bit_periodic(val, LX.PERIOD, 'val')
    wins = _metric_inputs_unchanged(ar, n, L, pp, tp)
    ridx, rbits = RK.topk_ref(pp.numpy(), k)                      # one period: no tolerance (test_rank_at_k_gpu.py)
    rows = (LX.window_rows(wins) % LX.PERIOD).numpy()
    assert np.array_equal(LX.take_rows(idx, wins).numpy(), ridx[rows])
    assert np.array_equal(LX.take_rows(val, wins).view(torch.int32).numpy().view(np.uint32), rbits[rows])
    hit, ndcg, recall, gold = RK.per_sample_ref(ridx, tp.numpy())
    c = count.numpy()
    assert np.array_equal(ar.view('hits', torch.int64).cpu().numpy(), (hit * c[:, None]).sum(0))
    assert int(ar.view('with_gold', torch.int64)[0]) == int(((gold > 0) * c).sum())
    for name, per in (('ndcg', ndcg), ('recall', recall)):
        got, ref = ar.view(name, torch.float64).cpu().numpy(), (per * c[:, None].astype(np.float64)).sum(0)
        used('lamp_rank_at_k %s_sum (bar: test_rank_at_k_gpu.py: _close, 1e-12 relative)' % name,
             float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))), 1e-12)


def test_topk_labels_and_rank_at_k_across_b32(dev, N):
    (n, L), k = LX.BCE_B32, 5
    nb = f32(n * L)
    ws = N.lib().lamp_rank_at_k_workspace_bytes(n, k)
    assert ws > 0 and LX.crossings(nb) == ['B31', 'B32']
    ops = [('hits', 8 * k), ('ndcg', 8 * k), ('recall', 8 * k), ('with_gold', 8), ('idx', f32(n * k)), ('val', f32(n * k)),
           ('workspace', ws), ('targets', nb), ('probs', nb)]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_topk_labels + lamp_rank_at_k, n * L * 4 past 2^32') as ar:
        _topk_rank_body(ar, N, n, L, k)


def _threshold_counts_body(ar, N, n, L, vec):
    import numpy as np
    import thresholds_common as TH
    pp, tp, count = _metric_inputs(ar, n, L)
    thr = torch.rand(L, generator=rnd(53)) if vec else 0.37
    outs = ['label_tp', 'label_fp', 'label_fn', 'sample_tp', 'sample_pred', 'sample_gold', 'sample_mismatch']
    ptrs = [ar.ptr(o) for o in outs]
    if vec:
        ar.view('thresholds').copy_(thr)
        ok(N.lib().lamp_threshold_counts_vec(ar.ptr('probs'), L, ar.ptr('targets'), L, n, L, ar.ptr('thresholds'), *ptrs, N.stream()),
           'lamp_threshold_counts_vec')
    else:
        ok(N.lib().lamp_threshold_counts(ar.ptr('probs'), L, ar.ptr('targets'), L, n, L, thr, *ptrs, N.stream()), 'lamp_threshold_counts')
    ar.check_zones()
    for o in outs:
        ar.check_written(o)
    wins = _metric_inputs_unchanged(ar, n, L, pp, tp)
    lab, ex = TH.counts_ref(pp.numpy(), tp.numpy(), thr.numpy() if vec else np.float32(thr))     # exact integers, one period
    c = count.numpy()
    # a label's count over all n rows: every period row as often as it occurs (fewer than 2^31, so int32 holds it)
    thr_np = thr.numpy() if vec else np.float32(thr)
    pred, gold = pp.numpy() >= (thr_np[None, :] if vec else thr_np), tp.numpy() != 0
    want = np.stack([((pred & gold) * c[:, None]).sum(0), ((pred & ~gold) * c[:, None]).sum(0), ((~pred & gold) * c[:, None]).sum(0)])
    got = np.stack([ar.view(o, torch.int32).cpu().numpy() for o in outs[:3]])
    assert np.array_equal(got, want) and np.array_equal(lab, np.stack([(pred & gold).sum(0), (pred & ~gold).sum(0), (~pred & gold).sum(0)]))
    rows = (LX.window_rows(wins) % LX.PERIOD).numpy()
    for i, o in enumerate(outs[3:]):
        v = ar.view(o, torch.int32, (n, 1))
        LX.assert_bit_periodic(v, LX.PERIOD, o)
        assert np.array_equal(LX.take_rows(v, wins).numpy()[:, 0], ex[i][rows]), o


@pytest.mark.parametrize('vec,fill', [(False, LX.FILL_NAN), (True, LX.FILL_NAN), (True, LX.FILL_BIG)])
def test_threshold_counts_across_b32(dev, N, vec, fill):
    n, L = LX.BCE_B32
    nb = f32(n * L)
    ops = [('thresholds', f32(L))] + [('label_' + k, f32(L)) for k in ('tp', 'fp', 'fn')]
    ops += [('sample_' + k, f32(n)) for k in ('tp', 'pred', 'gold', 'mismatch')] + [('targets', nb), ('probs', nb)]
    with arena(dev, fill, ops, 'lamp_threshold_counts%s, n * L * 4 past 2^32' % ('_vec' if vec else '')) as ar:
        _threshold_counts_body(ar, N, n, L, vec)


def _sorted_column_body(ar, N, n, L, which):
    import numpy as np
    import ranking_common as RC
    import thresholds_common as TH
    pp, tp, count = _metric_inputs(ar, n, L)
    lib = N.lib()
    if which == 'ranking':
        ok(lib.lamp_ranking_metrics(ar.ptr('probs'), L, ar.ptr('targets'), L, n, L, 0.5, ar.ptr('o0'), ar.ptr('o1'), ar.ptr('o2'),
                                    ar.ptr('o3'), ar.ptr('o4'), ar.ptr('workspace'), ar.nbytes('workspace'), N.stream()),
           'lamp_ranking_metrics')
    else:
        ok(lib.lamp_tune_thresholds(ar.ptr('probs'), L, ar.ptr('targets'), L, n, L, 0, 0.5, ar.ptr('o0'), ar.ptr('o1'), ar.ptr('o2'),
                                    ar.ptr('o3'), ar.ptr('o4'), None, ar.ptr('workspace'), ar.nbytes('workspace'), N.stream()),
           'lamp_tune_thresholds')
    ar.check_zones()
    _metric_inputs_unchanged(ar, n, L, pp, tp)
    Pv, Tv = ar.view('probs', shape=(n, L)), ar.view('targets', shape=(n, L))
    cols = [0, L // 3, 2 * L // 3, L - 1]
    if which == 'ranking':
        auc, aupr, fdr = (ar.view('o%d' % i, torch.float64)[:L].cpu().numpy() for i in range(3))
        n_pos, n_neg = (ar.view('o%d' % i, torch.int64)[:L].cpu().numpy() for i in (3, 4))
        assert np.isfinite(auc).all() and np.isfinite(aupr).all()
        for l in cols:
            a, b, c_, Pn, Nn = RC.column_ref(Pv[:, l].cpu(), Tv[:, l].cpu(), 0.5)     # the whole column, fp64 on the CPU
            assert RC.same_bits(auc[l:l + 1], np.array([a])) and RC.same_bits(fdr[l:l + 1], np.array([c_])), l
            used('lamp_ranking_metrics aupr[%d] (bar: test_ranking_gpu.py, 1e-9)' % l, abs(aupr[l] - b), 1e-9)
            assert (n_pos[l], n_neg[l]) == (Pn, Nn)
    else:
        thr = ar.view('o0', torch.int32)[:L].cpu().numpy().view(np.uint32)
        tpv, fpv, n_pos, n_neg = (ar.view('o%d' % i, torch.int32)[:L].cpu().numpy() for i in (1, 2, 3, 4))
        for l in cols:                                                                # exact: no tolerance (test_tune_thresholds_gpu.py)
            want = TH.tune_column_ref(Pv[:, l].cpu().numpy(), Tv[:, l].cpu().numpy(), 'f1')
            assert (int(thr[l]), int(tpv[l]), int(fpv[l]), int(n_pos[l]), int(n_neg[l])) == tuple(int(x) for x in want[:5]), l


@pytest.mark.parametrize('which', ['ranking', 'tune'])
def test_sorted_column_metrics_across_b32(dev, N, which):
    """Both fit the budget at B32 by their own size queries (8.25 GiB of workspace each at 1168664 x 919)."""
    n, L = LX.BCE_B32
    nb = f32(n * L)
    q = N.lib().lamp_ranking_metrics_workspace_bytes if which == 'ranking' else N.lib().lamp_tune_thresholds_workspace_bytes
    ws = q(n, L)
    assert ws >= 2 * nb
    ops = [('o%d' % i, 8 * L) for i in range(5)] + [('targets', nb), ('probs', nb), ('workspace', ws)]
    assert LX.need_bytes(ops) < LX.BUDGET
    with arena(dev, LX.FILL_NAN, ops, 'lamp_%s, n * L * 4 past 2^32' % ('ranking_metrics' if which == 'ranking' else 'tune_thresholds')) as ar:
        _sorted_column_body(ar, N, n, L, which)


# ====================================================================================== G1 (continued): the packed-W route
# Table row lamp_linear_packed_fwd: the weight pack is read whole through ONE 31-bit descriptor; guard (gemm.hip: gemm_packed_ok)
# (N + 64) * K * 4 >= 0x7fffffff -> the pack is ignored.  One step inside it: K = 8192, N = 65456 (a multiple of 16), so that
# (N + 64) * K * 4 = 0x7ff80000; M = 67 rows give 2046 64 x 64 tiles, below 2048: the packed 32 x 64 tile.  The packed tiles are
# chosen by tile count (fewer than 4096 128 x 64 tiles), so no packed TILE can have a C past 2^32 bytes; the entry point itself
# runs at that size in the case after this one.  W is generated on the device; the whole C must
# carry the bits of the row-major route (the header's promise), and the windows of output columns are held against fp64.
def _packed_body(ar, N, M, K, Nn):
    L = N.lib()
    g = rnd(61)
    a, b = torch.randn(M, K, generator=g), torch.randn(Nn, generator=g)
    W = ar.view('W', shape=(Nn, K))
    gen = torch.Generator(device=ar.device).manual_seed(61)
    for r in range(0, Nn, 1024):
        W[r:r + 1024].normal_(generator=gen).mul_(K ** -0.5)
    before = LX.checksum(ar.view('W'))
    ar.view('A', shape=(M, K)).copy_(a)
    ar.view('bias').copy_(b)
    ok(L.lamp_pack_weight(ar.ptr('W'), Nn, K, K, 0, ar.ptr('pack'), N.stream()), 'lamp_pack_weight')
    ar.check_written('pack')
    Ws, Ps, Cs, Bs = ((C.c_void_p * 1)(ar.ptr(k)) for k in ('W', 'pack', 'C', 'bias'))
    ok(L.lamp_linear_packed_fwd(ar.ptr('A'), M, K, K, Ws, Ps, 1, Nn, K, Bs, None, 0, 1, Cs, Nn, None, N.stream()),
       'lamp_linear_packed_fwd')
    ok(L.lamp_linear_fwd(ar.ptr('A'), M, K, K, ar.ptr('W'), Nn, K, ar.ptr('bias'), None, 0, 1, ar.ptr('C_rowmajor'), Nn, N.stream()),
       'lamp_linear_fwd')
    ar.check_zones()
    ar.check_written('C')
    assert LX.checksum(ar.view('W')) == before, 'W changed'
    got = ar.view('C', shape=(M, Nn)).cpu()
    assert torch.equal(got.view(torch.int32), ar.view('C_rowmajor', torch.int32, (M, Nn)).cpu()), 'packed and row-major routes differ'
    cols = LX.window_rows(LX.windows(Nn, f32(K)))
    ref = (a.double() @ W[cols].cpu().double().t() + b[cols].double()).clamp_min(0)
    used('lamp_linear_packed_fwd, pack one step inside its descriptor (bar: test_buffer_contracts_gpu.py: test_linear_fwd)',
         max_abs_diff(got[:, cols], ref), 2e-5)


def test_linear_packed_fwd_pack_one_step_inside_its_descriptor(dev, N):
    M, K = 67, 8192
    Nn = (0x7fffffff - 1) // (4 * K) - 64
    Nn -= Nn % 16
    assert (Nn + 64) * K * 4 < 0x7fffffff <= (Nn + 16 + 64) * K * 4 and Nn == 65456
    assert 1200 <= ((M + 63) // 64) * ((Nn + 63) // 64) < 2048       # gemm.hip: launch_gemm takes the packed 32 x 64 tile
    ops = [('bias', f32(Nn)), ('A', f32(M * K)), ('C', f32(M * Nn)), ('C_rowmajor', f32(M * Nn)), ('W', f32(Nn * K)), ('pack', f32(Nn * K))]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_linear_packed_fwd, (N + 64) * K * 4 = 0x%x' % ((Nn + 64) * K * 4)) as ar:
        _packed_body(ar, N, M, K, Nn)


# The same entry point with C and the residual across B32: M = 2^20 + 101, K = 32, N = 1024 + 16, one segment, the full
# epilogue, a pack, and m_dev = M - 37 in device memory.  At this tile count launch_gemm ignores the pack (the staged kernel
# serves the shape), but the entry point's own path -- the host arrays of segment pointers, the pack's admission, m_dev -- runs
# at size: rows below *m_dev carry the bits of lamp_linear_fwd, rows at and past it keep the sentinel.  Row-local, no split K:
# periodic A and residual.
def _packed_b32_body(ar, N, M, K, Nn, live):
    L = N.lib()
    g = rnd(67)
    w, b = torch.randn(Nn, K, generator=g) / K ** 0.5, torch.randn(Nn, generator=g)
    ap, rp = torch.randn(LX.PERIOD, K, generator=g), torch.randn(LX.PERIOD, Nn, generator=g)
    A, Rv = ar.view('A', shape=(M, K)), ar.view('residual', shape=(M, Nn))
    LX.fill_periodic_rows(A, ap)
    LX.fill_periodic_rows(Rv, rp)
    ar.view('W', shape=(Nn, K)).copy_(w)
    ar.view('bias').copy_(b)
    ar.view('m_dev', torch.int32).fill_(live)
    ok(L.lamp_pack_weight(ar.ptr('W'), Nn, K, K, 0, ar.ptr('pack'), N.stream()), 'lamp_pack_weight')
    Ws, Ps, Cs, Bs = ((C.c_void_p * 1)(ar.ptr(k)) for k in ('W', 'pack', 'C', 'bias'))
    ok(L.lamp_linear_packed_fwd(ar.ptr('A'), M, K, K, Ws, Ps, 1, Nn, K, Bs, ar.ptr('residual'), Nn, 1, Cs, Nn, ar.ptr('m_dev'),
                                N.stream()), 'lamp_linear_packed_fwd')
    ok(L.lamp_linear_fwd(ar.ptr('A'), M, K, K, ar.ptr('W'), Nn, K, ar.ptr('bias'), ar.ptr('residual'), Nn, 1, ar.ptr('C_rowmajor'), Nn,
                         N.stream()), 'lamp_linear_fwd')
    ar.check_zones()
    Cv, Cr = ar.view('C', torch.int32, (M, Nn)), ar.view('C_rowmajor', torch.int32, (M, Nn))
    sent = LX._i32(ar.fill)
    step = LX.CHUNK // f32(Nn)
    for r in range(0, live, step):
        n = min(step, live - r)
        assert bool((Cv[r:r + n] == Cr[r:r + n]).all()), 'packed and row-major routes differ in rows %d..%d' % (r, r + n)
        assert not bool((Cv[r:r + n] == sent).any()), 'a live element of C was never written'
    assert bool((Cv[live:] == sent).all()), 'a row at or past *m_dev was written'
    wins = [(a_, min(b_, live)) for a_, b_ in LX.windows(M, f32(Nn)) if a_ < live]
    LX.assert_rows_equal_generator(A, ap, wins, 'packed A')
    LX.assert_rows_equal_generator(Rv, rp, wins, 'packed residual')
    idx = LX.window_rows(wins)
    ref = (LX.periodic_rows(ap, idx).double() @ w.double().t() + b.double()).clamp_min(0) + LX.periodic_rows(rp, idx).double()
    used('lamp_linear_packed_fwd, C and residual past 2^32 bytes (bar: test_buffer_contracts_gpu.py: test_linear_fwd)',
         max_abs_diff(LX.take_rows(ar.view('C', shape=(M, Nn)), wins), ref), 2e-5)


def test_linear_packed_fwd_c_and_residual_across_b32_with_a_device_row_count(dev, N):
    M, K, Nn = (1 << 20) + 101, 32, 1024 + 16
    assert LX.crossings(f32(M * Nn)) == ['B31', 'B32'] and f32((M - 37) * Nn) > LX.B32
    ops = [('m_dev', 4), ('W', f32(Nn * K)), ('pack', f32(Nn * K)), ('bias', f32(Nn)), ('A', f32(M * K)), ('residual', f32(M * Nn)),
           ('C', f32(M * Nn)), ('C_rowmajor', f32(M * Nn))]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_linear_packed_fwd, C and residual past 2^32 bytes') as ar:
        _packed_b32_body(ar, N, M, K, Nn, M - 37)


# ====================================================================================== G5 (continued): backward row kernels
# Table row lamp_layernorm_bwd: pointers; a grid-stride int64 row over at most 256 workgroups, x + row * d in 64 bits; workspace of
# exactly lamp_layernorm_bwd_workspace_bytes().  p = 0 (dx NULL, dbias NULL).  dz is row-local: windows.  The column sums run over
# ALL rows; their bar (1e-4 sqrt(M / 100)) was set for sums of independent terms, so x and dy get DIFFERENT prime periods (4093 and
# 4099 rows: the pair does not repeat within M rows) and dy has zero column means over its period -- sums that add up coherently
# over 256 repeats would be sixteen times larger and their fp32 rounding with them.  dgamma and dbeta are held for the first, the
# last and two middle columns, each over its whole column in fp64 on the CPU.
def _layernorm_bwd_body(ar, N, M, d):
    g = rnd(63)
    P2 = 4093
    xp, dyp = torch.randn(P2, d, generator=g), torch.randn(LX.PERIOD, d, generator=g)
    dyp -= dyp.mean(0, keepdim=True)
    gamma, _ = ln_params(d, 64)
    X, DY, DZ = (ar.view(k, shape=(M, d)) for k in ('x', 'dy', 'dz'))
    LX.fill_periodic_rows(X, xp)
    LX.fill_periodic_rows(DY, dyp)
    ar.view('gamma').copy_(gamma)
    nb = ar.nbytes('workspace')
    ok(N.lib().lamp_layernorm_bwd(ar.ptr('x'), None, 0, M, d, ar.ptr('gamma'), 1e-5, 0.0, 0, ar.ptr('dy'), ar.ptr('dz'), None,
                                  ar.ptr('dgamma'), ar.ptr('dbeta'), None, ar.ptr('workspace'), nb, N.stream()),
       'lamp_layernorm_bwd')
    ar.check_zones()
    for k in ('dz', 'dgamma', 'dbeta'):
        ar.check_written(k)
    wins = LX.windows(M, f32(d))
    LX.assert_rows_equal_generator(X, xp, wins, 'x')
    LX.assert_rows_equal_generator(DY, dyp, wins, 'dy')
    idx = LX.window_rows(wins)
    xw = xp[idx % P2].double().requires_grad_()
    F.layer_norm(xw, (d,), gamma.double(), None, 1e-5).backward(dyp[idx % LX.PERIOD].double())
    src = 'test_buffer_contracts_gpu.py: test_layernorm_residual_fwd_and_bwd'
    used('lamp_layernorm_bwd dz (bar: %s, 3e-5)' % src, max_abs_diff(LX.take_rows(DZ, wins), xw.grad), 3e-5)
    cols = [0, d // 3, 2 * d // 3, d - 1]
    x64 = xp.double()
    zhat = ((x64 - x64.mean(1, keepdim=True)) / (x64.var(1, unbiased=False, keepdim=True) + 1e-5).sqrt())[:, cols]
    r = torch.arange(M)
    dy_cols = dyp.double()[:, cols][r % LX.PERIOD]
    bar = 1e-4 * max(1.0, (M / 100) ** 0.5)
    used('lamp_layernorm_bwd dgamma (bar: %s, 1e-4 sqrt(M / 100))' % src,
         max_abs_diff(ar.view('dgamma').cpu()[cols], (dy_cols * zhat[r % P2]).sum(0)), bar)
    used('lamp_layernorm_bwd dbeta (bar: %s)' % src, max_abs_diff(ar.view('dbeta').cpu()[cols], dy_cols.sum(0)), bar)


def test_layernorm_bwd_across_b32(dev, N):
    M, d = LX.COLSUM_TALL
    nb = f32(M * d)
    ws = N.lib().lamp_layernorm_bwd_workspace_bytes(M, d)
    assert ws == 256 * 3 * d * 4 and LX.crossings(nb) == ['B31', 'B32']
    ops = [('gamma', f32(d)), ('dgamma', f32(d)), ('dbeta', f32(d)), ('workspace', ws), ('x', nb), ('dy', nb), ('dz', nb)]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_layernorm_bwd M * d * 4 past 2^32') as ar:
        _layernorm_bwd_body(ar, N, M, d)


# Table row lamp_diag_logits_bwd: pointers; one workgroup per four labels walks b = 0 .. B - 1, row = int64(b) * L + i, y + row * d
# in 64 bits.  dy[b, i, :] = dl[b, i] * w[i, :] on row windows; dw[i, :] = sum_b dl[b, i] * y[b, i, :] for the first, the last and
# two middle labels, each over its whole batch column in fp64 (B = 4099 = the period and L is prime to it: a label's rows are
# one full period of y).
def _diag_bwd_body(ar, N, B, L, d):
    g = rnd(65)
    period = torch.randn(LX.PERIOD, d, generator=g)
    w = torch.randn(L, d, generator=g) / d ** 0.5
    dl = torch.randn(B * L, generator=g) / 64       # (dw then is a sum of B terms of order 1 / 64: of order 1)
    rows = B * L
    Y, DYv = ar.view('y', shape=(rows, d)), ar.view('dy', shape=(rows, d))
    LX.fill_periodic_rows(Y, period)
    ar.view('w_out', shape=(L, d)).copy_(w)
    ar.view('dlogits').copy_(dl)
    ok(N.lib().lamp_diag_logits_bwd(ar.ptr('y'), ar.ptr('w_out'), ar.ptr('dlogits'), B, L, d, ar.ptr('dy'), ar.ptr('dw'), N.stream()),
       'lamp_diag_logits_bwd')
    ar.check_zones()
    ar.check_written('dy')
    ar.check_written('dw')
    wins = LX.windows(rows, f32(d))
    LX.assert_rows_equal_generator(Y, period, wins, 'y')
    idx = LX.window_rows(wins)
    src = 'test_buffer_contracts_gpu.py: test_diag_logits_fwd_bwd_and_sigmoid_bce'
    used('lamp_diag_logits_bwd dy (bar: %s)' % src, max_abs_diff(LX.take_rows(DYv, wins), dl[idx, None].double() * w[idx % L].double()), 1e-5)
    dw = ar.view('dw', shape=(L, d)).cpu()
    worst = 0.0
    for i in (0, L // 3, 2 * L // 3, L - 1):
        r = torch.arange(B) * L + i
        worst = max(worst, max_abs_diff(dw[i], (dl[r, None].double() * LX.periodic_rows(period, r).double()).sum(0)))
    used('lamp_diag_logits_bwd dw (bar: %s)' % src, worst, 1e-5)


def test_diag_logits_bwd_across_b32(dev, N):
    B, L, d = LX.DIAG_B32
    nb = f32(B * L * d)
    ops = [('w_out', f32(L * d)), ('dw', f32(L * d)), ('dlogits', f32(B * L)), ('y', nb), ('dy', nb)]
    with arena(dev, LX.FILL_NAN, ops, 'lamp_diag_logits_bwd B * L * d * 4 past 2^32') as ar:
        _diag_bwd_body(ar, N, B, L, d)


# ====================================================================================== G8: the whole forward
# Table row lamp_forward*: every launch above behind one entry point, the batch split into micro-batches that fit the workspace.
# The project's own promise (include/lamp_hip.h: lamp_forward) is that a sample's outputs do not depend on B or on the split, bit
# for bit: a batch of 419451 samples that repeats eight ragged samples must give eight-periodic logits and enc_output, equal to
# the batch of eight.  The padded enc_output [B, T, d] crosses B32; the workspace limit is set to 2 GiB, so the carve runs some
# twenty passes at large B.  'live_packed' is the packed ragged encoder route of the attention table (enc_self_attn=True behind
# use_packed_live_encoder: csrc/attention_ragged.hip on the packed non-PAD rows, which pass B32 as well: 277 of every 320 rows are
# live); it has no public entry point of its own, so the forward is its case.  The operands are the module's own tensors here,
# not an arena: the entry point is reached through LAMP.forward.
def _tiny_model(dev, V, L, T, d, dff, h, **kw):
    from lamp_amd.Models import LAMP
    from oracle import lamp_ref as R
    sd = R.make_state_dict(V, L, T, d, dff, h, 2, 2, pos_emb=True, seed=0)
    adj = R.make_adjacency(L, 0.2, 0)
    m = LAMP(V, L, T, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=dff,
             d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', label_adj_matrix=adj.clone(), label_mask='prior',
             dec_dropout2=False, **kw)
    m.load_state_dict(sd)
    return m.to(dev).eval(), sd, adj


@pytest.mark.parametrize('route', ['dead', 'live_packed'])
def test_whole_forward_batch_whose_enc_output_crosses_b32_is_the_batch_of_eight(dev, N, route):
    from oracle import lamp_ref as R
    V, L, T, d, dff, h = 200, 24, 40, 64, 128, 4
    live = route == 'live_packed'
    lengths = [40, 39, 40, 40, 37, 40, 1, 40] if live else [40, 3, 17, 40, 29, 8, 1, 33]
    B = LX.B32 // f32(T * d) * (320 if live else sum(lengths)) // sum(lengths) + 16 + 5
    assert f32(B // 8 * sum(lengths) * d) > LX.B32 or not live          # the packed rows cross B32 too
    limit = 2 << 30
    need = f32(B * T * d) + limit + 2 * 8 * B * T + f32(B * L) + LX.TEMP + (64 << 20)
    LX.require_memory(need)
    m, sd, adj = _tiny_model(dev, V, L, T, d, dff, h, **(dict(enc_self_attn=True) if live else {}))
    seq8, pos8 = R.make_batch(8, V, T, lengths=lengths, seed=0)
    if live:
        m.use_packed_live_encoder = True
    m.workspace_limit_bytes = limit
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    try:
        with torch.no_grad():
            ref_logits, ref_enc, _ = m((seq8.to(dev), pos8.to(dev)), None, None, None)
            if live:         # the switch does select another route at this T and head size: the padded live encoder's bits differ
                m.use_packed_live_encoder = False
                padded = m((seq8.to(dev), pos8.to(dev)), None, None, None)
                m.use_packed_live_encoder = True
                assert not torch.equal(padded[1], ref_enc) and max_abs_diff(padded[1], ref_enc) < 1e-4
                del padded
            seq = seq8.to(dev).repeat(B // 8 + 1, 1)[:B].contiguous()
            pos = pos8.to(dev).repeat(B // 8 + 1, 1)[:B].contiguous()
            logits, enc, _ = m((seq, pos), None, None, None)
        torch.cuda.synchronize()
        assert enc.shape == (B, T, d) and LX.crossings(f32(enc.numel())) == ['B31', 'B32']
        LX.assert_bit_periodic(enc.view(B, T * d), 8, 'enc_output')
        LX.assert_bit_periodic(logits.view(B, L), 8, 'logits')
        ref_enc, ref_logits = ref_enc.cpu().view(8, T * d), ref_logits.cpu()
        for a, b in LX.windows(B, f32(T * d), width=8):
            idx = torch.arange(a, b) % 8
            assert torch.equal(enc[a:b].cpu().view(-1, T * d).view(torch.int32), ref_enc[idx].view(torch.int32)), (a, b)
            assert torch.equal(logits[a:b].cpu().view(torch.int32), ref_logits[idx].view(torch.int32)), (a, b)
        if not live:     # (the live routes against fp64 at small batches: tests/test_enc_self_attn_gpu.py)
            with torch.no_grad():
                want, want_enc = R.forward(sd, seq8, pos8, h, R.label_block_mask(adj, 'prior', L))[:2]
            used('whole forward logits (bar: __graft_entry__.py: smoke)', max_abs_diff(ref_logits, want), 1e-4)
            used('whole forward enc_output (bar: __graft_entry__.py: smoke)', max_abs_diff(ref_enc.view(8, T, d), want_enc), 1e-4)
        peak = torch.cuda.max_memory_allocated() - base
        print('large-extent peak: whole forward (%s), B = %d: %.2f GiB (planned %.2f GiB)' % (route, B, peak / GIB, need / GIB))
        assert peak <= need
    finally:
        m = None
        gc.collect()
        torch.cuda.empty_cache()


# The same promise with return_attns, at a batch whose decoder self-attention maps [H * B, L, L] cross B32 (slice h * B + b, as
# lamp_sdpa_fwd lays them out), on a model shrunk for it: T = 12, L = 64, so 65536 slices of 16 KiB reach 2^32 bytes at
# B = 16384 x 4 heads.  The workspace is exactly lamp_forward_workspace_bytes(model, micro_batch = 4099, T, want_attn = 1) (a
# prime: no multiple of the eight repeated samples or of a tile).  The launcher derives its split from those bytes: they must
# hold at least 4099 samples a pass, and hold somewhat more, because the query counts the K / V-ahead buffers that a split
# forward does without (api.hip: forward_tokens).  The launch counters show the split that ran.
def test_whole_forward_with_maps_across_b32_in_micro_batches_of_at_least_4099_is_the_batch_of_eight(dev, N):
    from oracle import lamp_ref as R
    V, L, T, d, dff, h, mb = 200, 64, 12, 64, 128, 4, 4099
    B = LX.B32 // f32(h * L * L) + 16 + 5
    maps = 2 * f32(h * B * L * L) + 2 * f32(h * B * L * T) + 2 * f32(h * B * T * T)         # two layers of each kind
    limit_bound = 1 << 30                      # the workspace of 4099 samples of this model, held below once it is known
    need = maps + f32(B * T * d) + limit_bound + 2 * 8 * B * T + f32(B * L) + LX.TEMP + (64 << 20)
    LX.require_memory(need)
    seq8, pos8 = R.make_batch(8, V, T, lengths=[12, 3, 7, 12, 9, 8, 1, 11], seed=0)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = None
    try:
        m, sd, adj = _tiny_model(dev, V, L, T, d, dff, h)
        model = m._native_model()[0]
        q = N.lib().lamp_forward_workspace_bytes
        one, two = q(C.byref(model), 1, T, 1), q(C.byref(model), 2, T, 1)
        per, fixed = two - one, 2 * one - two
        limit = q(C.byref(model), mb, T, 1)
        assert limit == fixed + per * mb and (limit - fixed) // per == mb and B % mb and B > 3 * mb and limit <= limit_bound
        m.workspace_limit_bytes = limit

        def counted(n):      # a forward of the first n samples with the library's launch counters on
            N.prof_enable(True)
            try:
                N.prof_reset()
                with torch.no_grad():
                    out = m((seq[:n], pos[:n]), None, None, None, return_attns=True)
                torch.cuda.synchronize()
                return out, sum(int(v['launches']) for v in N.prof_read().values())
            finally:
                N.prof_enable(False)
        seq = seq8.to(dev).repeat(B // 8 + 1, 1)[:B].contiguous()
        pos = pos8.to(dev).repeat(B // 8 + 1, 1)[:B].contiguous()
        with torch.no_grad():
            ref = m((seq8.to(dev), pos8.to(dev)), None, None, None, return_attns=True)
        # the split that ran: a pass costs the same launches whatever it holds (test_combo_gpu.py).  4100 and 8199 samples cost a
        # and 2 a launches -- one pass and two (were 4100 samples two passes of 4099 and 1, 8199 would be three: 1.5 a) -- and
        # the whole batch a whole number of passes: more than one, and no more than ceil(B / 4099) = 16, each holding at least
        # the 4099 samples the query was asked for
        a_pass, n_two = counted(mb + 1)[1], counted(2 * mb + 1)[1]
        got, n_launches = counted(B)
        passes = n_launches // a_pass
        print('large-extent split: %d launches a pass, %d passes for B = %d (at least %d samples a pass)'
              % (a_pass, passes, B, (B + passes - 1) // passes))
        assert a_pass > 0 and n_two == 2 * a_pass and n_launches == passes * a_pass, (a_pass, n_two, n_launches)
        assert 2 <= passes <= (B + mb - 1) // mb == 16, passes

        def flat(out):       # -> [(name, tensor, rows per head or None)]
            logits, enc, (enc_attns,), (slf, encdec) = out
            named = [('logits', logits), ('enc_output', enc)]
            for kind, maps_ in (('enc_self_attn', enc_attns), ('dec_self_attn', slf), ('dec_enc_attn', encdec)):
                named += [('%s[%d]' % (kind, i), t) for i, t in enumerate(maps_) if t is not None]
            return named
        crossed = []
        for (name, big), (_, small) in zip(flat(got), flat(ref)):
            heads = big.shape[0] // B
            assert heads * B == big.shape[0] and small.shape[0] == heads * 8, name
            cols = big[0].numel()
            big2, small2 = big.reshape(heads, B, cols), small.reshape(heads, 8, cols).cpu()
            crossed += [name] * ('B32' in LX.crossings(f32(big.numel())))
            for hd in range(heads):
                LX.assert_bit_periodic(big2[hd], 8, '%s head %d' % (name, hd))
            for a, b in LX.windows(heads * B, f32(cols), width=8):          # slices h * B + b on either side of each boundary
                s = torch.arange(a, b)
                want = small2[s // B, (s % B) % 8]
                assert torch.equal(big.reshape(heads * B, cols)[a:b].cpu().view(torch.int32), want.view(torch.int32)), (name, a, b)
        assert 'dec_self_attn[0]' in crossed and 'dec_self_attn[1]' in crossed, crossed
        peak = torch.cuda.max_memory_allocated() - base
        print('large-extent peak: whole forward with maps, B = %d, micro-batch %d: %.2f GiB (planned %.2f GiB)'
              % (B, mb, peak / GIB, need / GIB))
        assert peak <= need
    finally:
        m = None
        gc.collect()
        torch.cuda.empty_cache()
