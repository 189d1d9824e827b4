"""-m gpu: the five entry points of the one-hot front end (csrc/conv.hip) each on its own against the fp64 restatements of
tests/conv_common.py (pinned to torch's fp64 conv / pool / autograd in tests/test_conv_kernels_cpu.py), at the shape edges of
their tiles, chunks and grid-stride loops.  Every output buffer is NaN-filled before the launch, so an element a kernel does
not write fails its comparison.  Sums are held to the a-priori bound (n + 2) 2^-24 mag of conv_common.py (no tolerance here
was tuned against the kernels); selections, copies and the padding to the bits.  Every check prints `<what>: worst err /
bound`; all of them must be <= 1.

Worst err / bound, one run on an MI355X (every case passed as the kernels were; no defect found):
  conv_window, shapes (out / relu_out)    4 -> 4, M = 1: 0.002 / 0.002; 8 -> 36: 0.016 / 0.015; 64 -> 128, one full tile: 0.003 /
                                          0.003; 12 -> 132, M = 129: 0.013 / 0.015 (rows_in = rows_out + 15: 0.016 / 0.017, + 40:
                                          0.014 / 0.016); 160 -> 260, K = 2560: 0.002 / 0.002
  conv_window, sixteen option sets        0.011 .. 0.013; the two out-of-table positions give exactly their two NaN rows
  conv2's input gradient                  36 -> 36: 0.003 .. 0.005 (T2 = 1 .. 43); 12 -> 132: <= 0.001
  front_fwd, 24 pairwise shapes           0.012 (T = 2, n_vocab = 1, d = 4) .. 0.141 (T = 17, n_vocab = 4, d = 64)
  front_fwd, other cases                  constant tokens 0.126, invalid tokens 0.117, dropout 0.5: 0.088 / 0.110, second grid
                                          pass (B = 9, T = 2000, d = 1024; 297 rows) 0.189
  front_bwd, dt1                          B T = 255: 0.093 / 0.085 (d = 4 / 36), 256: 0.084 / 0.097, 257: 0.058 / 0.082, 300: 0.046
                                          / 0.082, 513: 0.028 / 0.034; n_vocab = 16: 0.245, n_vocab = 1: 0.038, T = 2: 0.175;
                                          dropout 0.5: 0.072 / 0.033; constant tokens 0.076, invalid tokens 0.131
  front_bwd, colsum(dz)                   <= 0.010 (T = 2: 0.048)
  dz, conv_pack, conv_relu_bwd_pad, every padding row: the reference's bits; no backward case leaves an element out
"""
import ctypes as C
import itertools

import pytest
import torch

import conv_common as CC

pytestmark = pytest.mark.gpu

NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from lamp_amd import _native as N
    N.lib()
    return torch.device('cuda:0')


# ---------------------------------------------------------------- launches into NaN-filled buffers
def _nan(shape, dev):
    return torch.full(shape, NAN, dtype=torch.float32, device=dev)


def _ok(status, where):
    assert status == 0, '%s returned %d' % (where, status)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _pack(w, flip):
    from lamp_amd import _native as N
    co, ci, taps = w.shape
    out = _nan((ci, taps, co) if flip else (co, taps, ci), w.device)
    _ok(N.lib().lamp_conv_pack(_p(w), co, ci, taps, int(flip), _p(out), N.stream()), 'lamp_conv_pack')
    return out


def _front_fwd(seq, t1, b1, p=0.0, seed=0):
    from lamp_amd import _native as N
    B, T = seq.shape
    d = t1.size(2)
    fe = N.onehot_frontend(t1, b1, None, None, None)
    xpad = _nan((B * (T // 2 + 16) + 16, d), seq.device)
    _ok(N.lib().lamp_onehot_front_fwd(_p(seq), B, T, C.byref(fe), d, float(p), seed, _p(xpad), N.stream()),
        'lamp_onehot_front_fwd')
    return xpad


def _conv_window(x, B, rows_out, rows_in, w_pack, bias=None, relu=False, pos_table=None, src_pos=None, relu_out=False):
    from lamp_amd import _native as N
    c_out, taps, c_in = w_pack.shape
    assert taps == 16 and x.is_contiguous() and x.numel() >= ((B - 1) * rows_in + rows_out + 15) * c_in
    out = _nan((B * rows_out, c_out), x.device)
    ro = _nan((B * rows_out, c_out), x.device) if relu_out else None
    _ok(N.lib().lamp_conv_window_fwd(_p(x), B, rows_out, rows_in, c_in, _p(w_pack), c_out, _p(bias), int(relu), _p(pos_table),
                                     pos_table.size(0) if pos_table is not None else 0, _p(src_pos),
                                     src_pos.size(1) if src_pos is not None else 0, _p(out), _p(ro), N.stream()),
        'lamp_conv_window_fwd')
    return out, ro


def _relu_bwd_pad(dy, ro, B, rows):
    from lamp_amd import _native as N
    d = dy.size(1)
    dz = _nan((B * (rows + 16) + 16, d), dy.device)
    _ok(N.lib().lamp_conv_relu_bwd_pad(_p(dy), _p(ro), B, rows, d, _p(dz), N.stream()), 'lamp_conv_relu_bwd_pad')
    return dz


def _front_bwd(seq, t1, b1, dP, p=0.0, seed=0):
    """-> (dz [B, T, d], dt1 [V, 16, d] = lamp_colsum of the partials, the partials)."""
    from lamp_amd import _native as N
    B, T = seq.shape
    V, _, d = t1.shape
    fe = N.onehot_frontend(t1, b1, None, None, None)
    nbytes = N.lib().lamp_onehot_front_bwd_partials_bytes(B, T, V, d)
    assert nbytes == ((B * T + 255) // 256) * V * 16 * d * 4
    dz, part = _nan((B, T, d), seq.device), _nan((nbytes // 4,), seq.device)
    _ok(N.lib().lamp_onehot_front_bwd(_p(seq), B, T, C.byref(fe), d, float(p), seed, _p(dP), _p(dz), _p(part), nbytes,
                                      N.stream()), 'lamp_onehot_front_bwd')
    dt1 = N.colsum(part.view(-1, V * 16 * d)).view(V, 16, d)
    return dz, dt1, part


# ---------------------------------------------------------------- comparisons
def _ratio(what, got, ref, bound):
    """max err / bound over the elements; the NaN patterns must be equal; a bound of 0 asks for the exact value."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), '%s: NaN in %d elements, the reference in %d' % (
        what, int(torch.isnan(got).sum()), int(nan.sum()))
    err = torch.where(nan, torch.zeros_like(ref), (got - ref).abs())
    r = float((err / bound.expand_as(err).clamp_min(1e-300)).max()) if err.numel() else 0.0
    print('%s: worst err / bound %.3f' % (what, r))
    assert r <= 1.0, (what, r)
    return r


def _bits_equal(got, ref32):
    got = got.detach().cpu()
    return got.shape == ref32.shape and torch.equal(got.view(torch.int32), ref32.view(torch.int32))


# ---------------------------------------------------------------- 1. conv_window shapes
def _cw_inputs(B, rows_out, rows_in, c_in, c_out, seed, n_pos=23, pos_ld=None):
    """x with the slack rows between the samples' windows at magnitude 1e3 (a wrong row(m) shows), weights of magnitude
    K^-1/2 so that the sums are O(1), bias, a position table and indices into it."""
    K = 16 * c_in
    x = CC.f32_randn(B, rows_in, c_in, seed=seed)
    x[:, rows_out + 15:] = 1e3 * torch.sign(x[:, rows_out + 15:])
    w = CC.f32_randn(c_out, 16, c_in, seed=seed + 1, scale=K ** -0.5)
    bias = CC.f32_randn(c_out, seed=seed + 2)
    pos = CC.f32_randn(n_pos, c_out, seed=seed + 3)
    pos_ld = pos_ld or rows_in
    src_pos = torch.randint(0, n_pos, (B, pos_ld), generator=CC.gen(seed + 4))
    return x.view(B * rows_in, c_in), w, bias, pos, src_pos


def _cw_check(what, dev, B, rows_out, rows_in, x, w, bias, relu, pos, src_pos, want_ro):
    c_in = x.size(1)
    t = lambda a: None if a is None else a.to(dev)
    d64 = lambda a: None if a is None else a.double()
    out, ro = _conv_window(t(x), B, rows_out, rows_in, t(w), t(bias), relu, t(pos), t(src_pos), want_ro)
    r_out, r_act, mag, mag_out = CC.conv_window_ref(x.double(), B, rows_out, rows_in, w.double(), d64(bias), relu, d64(pos),
                                                    src_pos)
    worst = _ratio(what + ' out', out, r_out, CC.sum_bound(16 * c_in, mag_out))
    if want_ro:
        assert bool(torch.isfinite(ro).all()), what
        worst = max(worst, _ratio(what + ' relu_out', ro, r_act, CC.sum_bound(16 * c_in, mag)))
    return out, r_out, worst


CW_SHAPES = [(1, 1, 4, 4),          # M = 1: every staged row is a clamp
             (2, 5, 8, 36),         # N % 32 != 0
             (2, 64, 64, 128),      # exactly one unguarded tile
             (3, 43, 12, 132),      # M = 129, N = 132: second tiles of one row and four columns, c_in != c_out
             (1, 130, 160, 260)]    # three N tiles, K = 2560


@pytest.mark.parametrize('B,rows_out,c_in,c_out,slack', [s + (16,) for s in CW_SHAPES] + [(3, 43, 12, 132, 15), (3, 43, 12, 132, 40)])
def test_conv_window_shapes(dev, B, rows_out, c_in, c_out, slack):
    rows_in = rows_out + slack
    x, w, bias, pos, src_pos = _cw_inputs(B, rows_out, rows_in, c_in, c_out, seed=1000 + c_out + slack)
    what = 'conv_window B%d q%d+%d %d->%d' % (B, rows_out, slack, c_in, c_out)
    _, r_out, _ = _cw_check(what, dev, B, rows_out, rows_in, x, w, bias, True, pos, src_pos, True)
    assert float(r_out.abs().max()) < 50    # no slack row (1e3) in any window of the reference


# ---------------------------------------------------------------- 2. conv_window options
@pytest.mark.parametrize('has_bias,relu,has_pos,want_ro', list(itertools.product((False, True), repeat=4)))
def test_conv_window_options(dev, has_bias, relu, has_pos, want_ro):
    B, rows_out, c_in, c_out, n_pos = 2, 5, 8, 36, 23
    rows_in, pos_ld = rows_out + 16, 2 * rows_out + 1      # src_pos [B, T] with T = 2 T2 + 1, as the model passes it
    x, w, bias, pos, src_pos = _cw_inputs(B, rows_out, rows_in, c_in, c_out, seed=2000, n_pos=n_pos, pos_ld=pos_ld)
    src_pos[0, 2], src_pos[1, 4] = -1, n_pos
    src_pos[:, rows_out:] = 10 ** 6                        # never read: only q < rows_out is
    what = 'conv_window bias%d relu%d pos%d ro%d' % (has_bias, relu, has_pos, want_ro)
    out, r_out, _ = _cw_check(what, dev, B, rows_out, rows_in, x, w, bias if has_bias else None, relu,
                              pos if has_pos else None, src_pos if has_pos else None, want_ro)
    nan_rows = torch.isnan(out).cpu()
    want = torch.zeros(B * rows_out, dtype=torch.bool)
    if has_pos:
        want[[0 * rows_out + 2, 1 * rows_out + 4]] = True
    assert torch.equal(nan_rows, want[:, None].expand(-1, c_out))


# ---------------------------------------------------------------- 3. conv2's input gradient
def _relu_out_values(M, c, seed):
    """What a forward leaves in relu_out: positives and +0; -0 (a kernel comparing bits instead of values would pass it)."""
    g = CC.gen(seed)
    kind = torch.randint(0, 4, (M, c), generator=g)
    v = torch.rand(M, c, generator=g) + 1e-3
    v[kind == 0] = 0.0
    v[kind == 1] = -0.0
    v[0, 0], v[0, 1], v[0, 2] = 0.0, -0.0, 1e-30          # present at every shape
    return v.float()


@pytest.mark.parametrize('c_in,c_out', [(36, 36), (12, 132)])
@pytest.mark.parametrize('B,T2', [(2, 1), (2, 2), (2, 17), (3, 43)])
def test_conv_input_gradient(dev, B, T2, c_in, c_out):
    seed = 3000 + 10 * T2 + c_in
    w2 = CC.f32_randn(c_out, c_in, 16, seed=seed, scale=(16 * c_out) ** -0.5)
    dy = CC.f32_randn(B * T2, c_out, seed=seed + 1)
    ro = _relu_out_values(B * T2, c_out, seed + 2)
    dzp = _relu_bwd_pad(dy.to(dev), ro.to(dev), B, T2)
    assert _bits_equal(dzp, CC.relu_bwd_pad_ref(dy, ro, B, T2)), 'conv_relu_bwd_pad differs from the selection'
    flip = _pack(w2.to(dev), 1)
    assert _bits_equal(flip, CC.conv_pack_ref(w2, 1))
    dP, _ = _conv_window(dzp[1:], B, T2, T2 + 16, flip)
    want, mag = CC.conv_input_grad_ref(dy.double(), ro.double(), w2.double(), B, T2)
    _ratio('input gradient B%d T2=%d %d->%d' % (B, T2, c_in, c_out), dP, want, CC.sum_bound(16 * c_out, mag))


# ---------------------------------------------------------------- 4. conv_pack
@pytest.mark.parametrize('flip', [0, 1])
@pytest.mark.parametrize('c_out,c_in,taps', [(5, 12, 16), (4, 4, 1), (7, 3, 3), (160, 160, 96)])
def test_conv_pack(dev, c_out, c_in, taps, flip):
    """(160, 160, 96) has 2 457 600 > 8192 * 256 elements: the grid-stride loop takes a second pass."""
    w = CC.f32_randn(c_out, c_in, taps, seed=4000 + taps)
    assert _bits_equal(_pack(w.to(dev), flip), CC.conv_pack_ref(w, flip))


# ---------------------------------------------------------------- 5. front_fwd
def _front_check(what, dev, seq, t1, b1, p=0.0, seed=0):
    B, T = seq.shape
    T2, d = T // 2, t1.size(2)
    keep = CC.front_keep(B, T, d, p, seed)
    scale = 1.0 / (1.0 - p) if p else 1
    xpad = _front_fwd(seq.to(dev), t1.to(dev), b1.to(dev), p, seed)
    fp = CC.front_pairs(seq, t1.double(), b1.double(), keep, scale)
    r = _ratio(what, xpad, CC.to_xpad(fp['P']), CC.to_xpad(fp['bound']))
    pad = torch.ones(xpad.size(0), dtype=torch.bool)
    pad[CC.xpad_data_rows(B, T2)] = False
    assert int(pad.sum()) == 16 * B + 16
    # exactly +0: the next kernel reads these rows as conv2's zero padding
    assert bool((xpad.cpu()[pad].view(torch.int32) == 0).all()), what
    return xpad.cpu(), fp, r


@pytest.mark.parametrize('T,V,d,B', CC.pairwise_front_cases())
def test_front_fwd_shapes(dev, T, V, d, B):
    t1, b1 = CC.front_weights(V, d, seed=5000 + T)
    seq = CC.tokens(B, T, V, seed=5100 + T + V)
    xpad, fp, _ = _front_check('front_fwd T%d V%d d%d B%d' % (T, V, d, B), dev, seq, t1, b1)
    assert xpad.shape == (B * (T // 2 + 16) + 16, d)    # an odd T drops its last position


def test_front_fwd_constant_sequences_tie(dev):
    seq, t1, b1, _ = CC.constant_case()
    T = seq.size(1)
    xpad, fp, _ = _front_check('front_fwd constant tokens', dev, seq, t1, b1)
    q = torch.arange(4, (T - 8) // 2)
    assert torch.equal(fp['z0'][:, q], fp['z1'][:, q])
    # the pooled interior rows of a sample are all the same row, to the bits
    rows = xpad[CC.xpad_data_rows(seq.size(0), T // 2)].view(seq.size(0), T // 2, -1)[:, q]
    assert bool((rows.view(torch.int32) == rows[:, :1].view(torch.int32)).all())


def test_front_fwd_invalid_tokens_poison_their_windows(dev):
    seq, t1, b1, _ = CC.invalid_case()
    B, T = seq.shape
    xpad, fp, _ = _front_check('front_fwd invalid tokens', dev, seq, t1, b1)
    nan = torch.isnan(xpad[CC.xpad_data_rows(B, T // 2)]).view(B, T // 2, -1)
    assert bool((nan.all(-1) == nan.any(-1)).all())
    rows = nan.all(-1)
    # position j poisons y1 at j - 7 .. j + 8, so the pooled rows (j - 7) // 2 .. (j + 8) // 2
    want = torch.zeros(B, T // 2, dtype=torch.bool)
    for b, j in ((0, 0), (0, T - 1), (1, T // 2), (1, T // 2 + 5), (2, 0), (2, T - 1)):
        want[b, max(0, (j - 7) // 2):min(T // 2, (j + 8) // 2 + 1)] = True
    assert torch.equal(rows, want) and not rows[3].any()


@pytest.mark.parametrize('B,T,V,d', [(3, 33, 9, 36), (2, 40, 4, 64)])
def test_front_fwd_dropout_mask_and_scale(dev, B, T, V, d):
    t1, b1 = CC.front_weights(V, d, seed=5500 + T)
    seq = CC.tokens(B, T, V, seed=5600 + T)
    xpad, fp, _ = _front_check('front_fwd dropout 0.5 T%d d%d' % (T, d), dev, seq, t1, b1, 0.5, CC.DROP_SEED)
    # it is this mask and no other: without it, or with the mask of another seed, the reference is far off
    other = CC.front_pairs(seq, t1.double(), b1.double(), CC.front_keep(B, T, d, 0.5, CC.DROP_SEED + 1), 2.0)['P']
    assert float((other - fp['P']).abs().max()) > 0.1


def test_front_fwd_second_grid_pass(dev):
    """(9 * 1016 + 16) * 256 = 2 344 960 float4 items > 8192 * 256: the grid-stride loop takes a second pass.  Every padding
    row, and every 37th pooled row plus each sample's first and last against the reference."""
    B, T, V, d = 9, 2000, 9, 1024
    T2 = T // 2
    t1, b1 = CC.front_weights(V, d, seed=5900)
    seq = CC.tokens(B, T, V, seed=5901)
    xpad = _front_fwd(seq.to(dev), t1.to(dev), b1.to(dev))
    assert (B * (T2 + 16) + 16) * (d // 4) > 8192 * 256
    pad = torch.ones(xpad.size(0), dtype=torch.bool)
    pad[CC.xpad_data_rows(B, T2)] = False
    assert bool((xpad[pad.to(dev)].view(torch.int32) == 0).all())
    qs = torch.unique(torch.cat([torch.arange(0, T2, 37), torch.tensor([0, 1, 3, 4, T2 - 5, T2 - 4, T2 - 1])]))
    fp = CC.front_pairs(seq, t1.double(), b1.double(), qs=qs)
    rows = (torch.arange(B)[:, None] * (T2 + 16) + 8 + qs[None, :]).reshape(-1)
    got = xpad[rows.to(dev)].view(B, qs.numel(), d)
    _ratio('front_fwd B9 T2000 d1024, %d rows' % rows.numel(), got, fp['P'], fp['bound'])


# ---------------------------------------------------------------- 6. front_bwd
def _bwd_check(what, dev, seq, t1, b1, dP, p=0.0, keep=None, scale=1):
    B, T = seq.shape
    d = t1.size(2)
    from lamp_amd import _native as N
    args = (seq.to(dev), t1.to(dev), b1.to(dev), dP.to(dev), p, CC.DROP_SEED)
    dz, dt1, part = _front_bwd(*args)
    r = CC.front_bwd_ref(seq, t1.double(), b1.double(), dP.double(), keep, scale)
    unsafe = r['unsafe']
    share = float(unsafe.double().mean())
    assert share <= 0.01, share
    assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(part).all())
    got, want = dz.cpu(), r['dz'].float()
    same = got.view(torch.int32) == want.view(torch.int32)
    assert bool((same | unsafe).all()), '%s: dz differs in %d safe elements' % (what, int((~same & ~unsafe).sum()))
    worst = 0.0
    if share == 0.0:    # (every case of conv_common: test_conv_kernels_cpu.py asserts it)
        worst = _ratio(what + ' dt1', dt1, r['dt1'], CC.sum_bound(r['dt1_n'], r['dt1_mag']))
        # conv1's bias gradient is dz's column sum
        db = N.colsum(dz.view(B * T, d))
        worst = max(worst, _ratio(what + ' colsum(dz)', db, r['dz'].sum((0, 1)), CC.sum_bound(B * T, r['dz'].abs().sum((0, 1)))))
    # "Deterministic": a second run gives the same bits, partials included
    dz2, dt12, part2 = _front_bwd(*args)
    assert torch.equal(dz.view(torch.int32), dz2.view(torch.int32))
    assert torch.equal(part.view(torch.int32), part2.view(torch.int32))
    assert torch.equal(dt1.view(torch.int32), dt12.view(torch.int32))
    return got, r, share


@pytest.mark.parametrize('case', CC.BWD_CASES, ids=CC.bwd_case_id)
def test_front_bwd(dev, case):
    seq, t1, b1, dP, p, keep, scale = CC.front_bwd_case(case)
    _, _, share = _bwd_check('front_bwd ' + CC.bwd_case_id(case), dev, seq, t1, b1, dP, p, keep, scale)
    assert share == 0.0


def test_front_bwd_constant_sequences_send_ties_to_the_first(dev):
    seq, t1, b1, dP = CC.constant_case()
    T = seq.size(1)
    dz, r, share = _bwd_check('front_bwd constant tokens', dev, seq, t1, b1, dP)
    assert share == 0.0
    P = r['pairs']['P'][:, 4:(T - 8) // 2]
    first, second = dz[:, 8:T - 8:2], dz[:, 9:T - 8:2]
    up = dP[:, 4:(T - 8) // 2]
    assert torch.equal(first, torch.where(P > 0, up, torch.zeros_like(up)))
    assert not second.any() and bool((P > 0).any()) and bool((P == 0).any())


def test_front_bwd_invalid_tokens_give_finite_gradients(dev):
    seq, t1, b1, dP = CC.invalid_case()
    dz, r, share = _bwd_check('front_bwd invalid tokens', dev, seq, t1, b1, dP)
    assert share == 0.0
    poisoned = torch.isnan(r['pairs']['P'])
    assert bool(poisoned.any()) and not dz[:, 0:2 * (seq.size(1) // 2):2][poisoned].any()
