"""matmul_precision='high' / 'bf16x6' on the GPU: the split GEMM kernel (csrc/gemm_split.hip) through lamp_linear_prec_fwd against
an fp64 product of the same fp32 inputs, its bit rule, and the tiny model against oracle/lamp_ref.py.

Bounds (none of them taken from what the kernel gives):
  x3   |C - C64| <= 2^-14 sum_k |a_k w_k| per element.  bf16 has a unit roundoff of 2^-8, so each of the dropped terms m.m, h.l,
       l.h is at most 2^-16 |a w| (3 x 2^-16 together); the rest of 2^-14 covers the fp32 accumulation at K <= 512.  A kernel that
       loses an h.m term is off by 2^-8 and fails.
  x6   within max(one fp32 ulp at the value, 4 x the gap torch's fp32 CPU product shows on the same inputs): train_common.within
       over the matrix; the row-by-row figure (each row's own gap) is printed beside it.
  epilogue  with a bias or a residual the x3 bound grows by one fp32 ulp at each add's own result (the fp32 epilogue rounds once
       per add whatever computed the product); the bare product keeps the strict bound on every shape.
  model  1e-4 on logits and enc_output, the project's own contract.
"""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F

import enc_live_common as EC
import train_common as TC
from conftest import max_abs_diff
from oracle import lamp_ref as R

pytestmark = pytest.mark.gpu

MS, NS, KS = (1, 17, 130, 257), (4, 6, 64, 132), (4, 36, 64, 512)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _N():
    from lamp_amd import _native as N
    return N


def prec_linear(dev, A, W, prec, bias=None, res=None, relu=False, lda=None, ldc=None, fn='prec'):
    """lamp_linear_prec_fwd (fn='prec') or lamp_linear_fwd (fn='plain') on CPU tensors A [M, K], W [N, K] -> C [M, N] on the CPU.
    lda / ldc: leading dimensions larger than K / N (the gaps hold NaN on the way in; what the call leaves there is returned too)."""
    N = _N()
    M, K = A.shape
    Nn = W.size(0)
    lda, ldc = lda or K, ldc or Nn
    Ad = torch.full((M, lda), float('nan'), device=dev)
    Ad[:, :K] = A.to(dev)
    Cd = torch.full((M, ldc), float('nan'), device=dev)
    Wd = W.contiguous().to(dev)
    bd = bias.to(dev) if bias is not None else None
    rd = res.contiguous().to(dev) if res is not None else None
    args = [N.ptr(Ad), M, K, lda, N.ptr(Wd), Nn, K, N.ptr(bd), N.ptr(rd), Nn if rd is not None else 0, int(relu), N.ptr(Cd), ldc]
    if fn == 'prec':
        st = N.lib().lamp_linear_prec_fwd(*args, prec, N.stream())
    else:
        st = N.lib().lamp_linear_fwd(*args, N.stream())
    torch.cuda.synchronize()
    assert st == 0, st
    full = Cd.cpu()
    return full[:, :Nn], full[:, Nn:]


def _inputs(M, N, K, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + M * 131 + N * 17 + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g)
    A[M // 2] *= 1e3          # one row scaled up, one down
    A[(M // 2 + 1) % M] *= 1e-3 if M > 1 else 1.0
    return A, W, torch.randn(N, generator=g), torch.randn(M, N, generator=g)


def _ref64(A, W, bias, res, relu):
    c = A.double() @ W.double().t()
    if bias is not None:
        c = c + bias.double()
    if relu:
        c = c.clamp(min=0)
    if res is not None:
        c = c + res.double()
    return c


def _ref32(A, W, bias, res, relu):
    c = A @ W.t()
    if bias is not None:
        c = c + bias
    if relu:
        c = c.clamp(min=0)
    if res is not None:
        c = c + res
    return c


def _check(dev, A, W, bias, res, relu, what, **ld):
    want = _ref64(A, W, bias, res, relu)
    scale = A.double().abs() @ W.double().abs().t()    # sum_k |a_k w_k|
    c3, pad3 = prec_linear(dev, A, W, 1, bias, res, relu, **ld)
    # The issue's bound is on the product.  The fp32 epilogue then rounds once per add (bias, residual), which no fp32-out kernel
    # can avoid: one fp32 ulp at each add's own result on top (else an element with sum|a w| << |bias| fails in ANY arithmetic).
    prod = A.double() @ W.double().t()
    extra = torch.zeros_like(want)
    if bias is not None:
        extra = extra + TC.ulp32(prod + bias.double())
    if res is not None:
        extra = extra + TC.ulp32(want)
    err3 = (c3.double() - want).abs()
    ratio = float((err3 / (2.0 ** -14 * scale + extra + 1e-300)).max())
    print('%s x3: max |err| / sum|a w| %.3e (bound %.3e), worst err / bound %.3f' % (what, float((err3 / (scale + 1e-300)).max()),
                                                                                      2.0 ** -14, ratio))
    assert ratio <= 1.0, (what, ratio)
    c6, pad6 = prec_linear(dev, A, W, 2, bias, res, relu, **ld)
    gap = float((_ref32(A, W, bias, res, relu).double() - want).abs().max())
    TC.within(c6, want, gap, what + ' x6')
    # printed, not asserted: the same rule row by row, each row against ITS OWN torch fp32 gap (the row scaled by 1e3 sets the
    # matrix-wide gap above; a single row's gap can be 0 by chance, so it is no bound)
    row_gap = (_ref32(A, W, bias, res, relu).double() - want).abs().amax(1, keepdim=True)
    row_tol = torch.maximum(TC.ulp32(want), 4.0 * row_gap.expand_as(want))
    row_worst = float(((c6.double() - want).abs() / row_tol).max())
    print('%s x6 per row: worst err / max(ulp, 4 x the row\'s own torch fp32 gap) %.3f' % (what, row_worst))
    assert torch.isnan(pad3).all() and torch.isnan(pad6).all()   # nothing written between the rows
    return c3, c6


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('N', NS)
def test_kernel_sweep_against_the_fp64_product(dev, N, K):
    """Every M of the sweep per (N, K); epilogues rotate through all eight bias / ReLU / residual combinations across the
    sweep's cases, and the full-epilogue and bare cases run for every shape."""
    combos = list(itertools.product((False, True), repeat=3))
    for i, M in enumerate(MS):
        A, W, bias, res = _inputs(M, N, K)
        picks = {combos[(i + NS.index(N) + 2 * KS.index(K)) % 8], (False, False, False), (True, True, True)}
        for use_b, relu, use_r in sorted(picks):
            _check(dev, A, W, bias if use_b else None, res if use_r else None, relu,
                   'M%d N%d K%d b%d relu%d r%d' % (M, N, K, use_b, relu, use_r))


def test_every_epilogue_combination(dev):
    A, W, bias, res = _inputs(130, 132, 36, seed=1)
    for use_b, relu, use_r in itertools.product((False, True), repeat=3):
        _check(dev, A, W, bias if use_b else None, res if use_r else None, relu, 'epilogue b%d relu%d r%d' % (use_b, relu, use_r))
    A, W, bias, res = _inputs(17, 6, 36, seed=1)   # the scalar epilogue (N % 4 != 0)
    for use_b, relu, use_r in itertools.product((False, True), repeat=3):
        _check(dev, A, W, bias if use_b else None, res if use_r else None, relu, 'scalar b%d relu%d r%d' % (use_b, relu, use_r))


def test_leading_dimensions_larger_than_the_rows(dev):
    A, W, bias, res = _inputs(130, 64, 36, seed=2)
    padded = _check(dev, A, W, bias, res, True, 'lda 44 ldc 72', lda=44, ldc=72)
    dense = _check(dev, A, W, bias, res, True, 'dense')
    assert torch.equal(padded[0], dense[0]) and torch.equal(padded[1], dense[1])
    odd = _check(dev, A, W[:6], bias[:6], res[:, :6].contiguous(), False, 'ldc 7 (scalar epilogue)', lda=40, ldc=7)
    assert torch.equal(odd[0], _check(dev, A, W[:6], bias[:6], res[:, :6].contiguous(), False, 'N 6 dense')[0])


def test_precision_0_is_lamp_linear_fwd_and_x3_is_another_kernel(dev):
    A, W, bias, res = _inputs(257, 132, 512, seed=3)
    plain = prec_linear(dev, A, W, 0, bias, res, True, fn='plain')[0]
    assert torch.equal(prec_linear(dev, A, W, 0, bias, res, True)[0], plain)
    x3 = prec_linear(dev, A, W, 1, bias, res, True)[0]
    x6 = prec_linear(dev, A, W, 2, bias, res, True)[0]
    assert not torch.equal(x3, plain) and not torch.equal(x3, x6)
    N = _N()
    assert N.lib().lamp_linear_prec_fwd(16, 4, 8, 8, 16, 4, 8, None, None, 0, 0, 16, 4, 3, None) == -4
    # the Python wrapper takes the attribute's names
    got = N.linear(A.to(dev), W.to(dev), bias.to(dev), res.to(dev), relu=True, precision='high')
    assert torch.equal(got.cpu(), x3)


@pytest.mark.parametrize('prec', [1, 2])
def test_bit_rule_rows_do_not_depend_on_m_or_the_segment_count(dev, prec):
    """An element's bits depend on (K, precision) only: a row alone (M = 1, the small tile), inside M = 257, and inside a launch
    large enough for each larger tile of the menu.  lamp_linear_prec_fwd launches one segment; the segment count is covered by
    test_model_bit_identity_under_high (the whole batch projects K/V of both decoder layers as ONE 4-segment launch, the
    micro-batched run as one 2-segment launch per layer, the live encoder's Q/K/V as 3 segments)."""
    K, N = 512, 64
    A, W, bias, _ = _inputs(257, N, K, seed=4)
    whole = prec_linear(dev, A, W, prec, bias)[0]
    for i in (0, 128, 129, 256):
        assert torch.equal(prec_linear(dev, A[i:i + 1], W, prec, bias)[0], whole[i:i + 1]), i
    # 64 x 64 tiles (>= 512 of them) and 128 x 128 tiles (>= 512 of them): the same rows and weight rows, repeated
    for reps_m, reps_n in ((9, 16), (17, 32)):
        big = prec_linear(dev, A.repeat(reps_m, 1), W.repeat(reps_n, 1), prec, bias.repeat(reps_n))[0]
        assert torch.equal(big[:257, :N], whole) and torch.equal(big[-257:, -N:], whole), (reps_m, reps_n)
    # a NaN in one row of A stays in that row
    An = A.clone()
    An[7, 3] = float('nan')
    poisoned = prec_linear(dev, An, W, prec, bias)[0]
    keep = [i for i in range(257) if i != 7]
    assert torch.isnan(poisoned[7]).all() and torch.equal(poisoned[keep], whole[keep])
    # an inf operand gives NaN: the mode's one semantic deviation (fp32 arithmetic gives inf)
    Ai = A.clone()
    Ai[9, 0] = float('inf')
    got = prec_linear(dev, Ai, W, prec, bias)[0]
    others = [i for i in range(257) if i != 9]
    assert torch.isnan(got[9]).all() and torch.equal(got[others], whole[others])


TINY = dict(V=50, L=10, d=64, h=2, dff=128, T=12, lengths=[12, 7, 3])


def _run(m, seq, pos, dev, **kw):
    with torch.no_grad():
        return m((seq.to(dev), pos.to(dev)), None, None, None, **kw)


def _gaps(dev, m, seq, spos, ref_logits, ref_enc, what, **kw):
    """Runs the three precisions; prints each gap; asserts the contract on both modes."""
    out = {}
    for mode in ('highest', 'high', 'bf16x6'):
        m.matmul_precision = mode
        r = _run(m, seq, spos, dev, **kw)
        out[mode] = r
        print('%s %-7s: logits %.3e enc %.3e' % (what, mode, max_abs_diff(r[0], ref_logits), max_abs_diff(r[1], ref_enc)))
    for mode in ('high', 'bf16x6'):
        assert max_abs_diff(out[mode][0], ref_logits) <= 1e-4, (what, mode)
        assert max_abs_diff(out[mode][1], ref_enc) <= 1e-4, (what, mode)
    assert not torch.equal(out['high'][0], out['highest'][0])   # the flag reaches the kernels
    return out


@pytest.mark.parametrize('mask', ['prior', 'none'])
def test_model_against_the_oracle(dev, mask):
    m, sd, blocked, seq, spos, h = EC.build(TINY, mask, True, live=False)
    with torch.no_grad():
        ref_logits, ref_enc, _ = R.forward(sd, seq, spos, h, blocked)
    _gaps(dev, m.to(dev).eval(), seq, spos, ref_logits, ref_enc, 'mask=' + mask)


def test_model_int_preds(dev):
    m, sd, blocked, seq, spos, h = EC.build(TINY, 'prior', True, live=False, int_preds=True)
    with torch.no_grad():
        ref_logits, ref_enc, ref_int = R.forward(sd, seq, spos, h, blocked, int_preds=True)
    out = _gaps(dev, m.to(dev).eval(), seq, spos, ref_logits, ref_enc, 'int_preds', int_preds=True)
    for mode in ('high', 'bf16x6'):
        assert len(out[mode][2]) == len(ref_int) == 3
        for got, want in zip(out[mode][2], ref_int):
            assert max_abs_diff(got, want) <= 1e-4, mode


def test_model_live_encoder(dev):
    m, sd, blocked, seq, spos, h = EC.build(TINY, 'prior', True, live=True)
    with torch.no_grad():
        ref = EC.live_forward_ref(sd, seq, spos, h, blocked)
    m = m.to(dev).eval()
    _gaps(dev, m, seq, spos, ref[0], ref[1], 'enc_self_attn padded')
    m.use_packed_live_encoder = True   # the 3-segment Q/K/V launch over device-counted rows and the separate-launch tail
    _gaps(dev, m, seq, spos, ref[0], ref[1], 'enc_self_attn packed')


def test_model_sigmoid_decoder(dev, monkeypatch):
    from sigmoid_common import sigmoid_sdpa
    m, sd, blocked, seq, spos, h = EC.build(TINY, 'prior', True, live=False, dec_attn_type='sigmoid')
    with torch.no_grad():
        enc = R.encoder_forward(sd, seq, spos, h)[0]
        with monkeypatch.context() as mp:
            mp.setattr(R, 'sdpa', sigmoid_sdpa)
            y = R.decoder_forward(sd, seq, enc, blocked, h)[0]
        ref_logits = R.readout(y, sd['tgt_word_proj.linear.weight'])
    _gaps(dev, m.to(dev).eval(), seq, spos, ref_logits, enc, 'dec_attn_type=sigmoid')


def test_model_onehot(dev):
    import onehot_common as OC
    m = OC.build_model(d=64, h=2, L=10, T_max=16, mask='none')
    sd = OC.fp64_state(m)
    seq, pos = OC.make_dna(3, 2, None)   # T = 2: the smallest the front end accepts (one encoder row per sample)
    ref_logits, ref_enc, _ = OC.onehot_forward_ref(sd, seq, pos, 2, None)
    _gaps(dev, m.to(dev).eval(), seq, pos, ref_logits, ref_enc, 'onehot T=2')


def test_model_bit_identity_under_high(dev):
    """A sample's logits: alone, in the batch, re-padded to a longer T, permuted, with a micro-batch of 1 (which also turns the
    4-segment K/V launch into 2-segment launches); and the padded route
    (maps requested: residual materialised, rows counted on the host) against the packed one (gathered residual, device-side row
    count, A_dense when nothing was skipped)."""
    N = _N()
    m, sd, blocked, seq, spos, h = EC.build(TINY, 'prior', True, live=False)
    m = m.to(dev).eval()
    m.matmul_precision = 'high'
    n, T = seq.shape
    logits, enc, _ = _run(m, seq, spos, dev)
    assert torch.equal(_run(m, seq, spos, dev)[0], logits)
    for b in range(n):
        one = _run(m, seq[b:b + 1], spos[b:b + 1], dev)
        assert torch.equal(one[0], logits[b:b + 1]) and torch.equal(one[1], enc[b:b + 1]), b
    perm = list(reversed(range(n)))
    assert torch.equal(_run(m, seq[perm], spos[perm], dev)[0][perm], logits)
    r_seq, r_pos = F.pad(seq, (0, EC.PAD_EXTRA)), F.pad(spos, (0, EC.PAD_EXTRA))
    assert torch.equal(_run(m, r_seq, r_pos, dev)[0], logits)
    built = m._native_model()
    opts = N.FwdOptions(0, N.LAMP_FWD_MATMUL_BF16X3, None, None)
    per = N.lib().lamp_forward_opts_workspace_bytes(C.byref(built[0]), C.byref(opts), 1, T, 0)
    m.workspace_limit_bytes = per + 4096
    try:
        split = _run(m, seq, spos, dev)
    finally:
        del m.workspace_limit_bytes
    assert torch.equal(split[0], logits) and torch.equal(split[1], enc)
    # gathered residual + m_dev (+ A_dense for the full-length batch) against the materialised residual and host row counts
    for s_, p_ in ((seq, spos), (seq[:1], spos[:1])):
        packed = _run(m, s_, p_, dev)
        padded = _run(m, s_, p_, dev, return_attns=True)
        assert torch.equal(packed[0], padded[0])
        live = s_.ne(0)
        assert torch.equal(packed[1][live], padded[1][live])


def test_highest_is_bit_equal_to_a_model_that_never_touched_the_attribute(dev):
    a, _, _, seq, spos, _ = EC.build(TINY, 'prior', True, live=False)
    b = EC.build(TINY, 'prior', True, live=False)[0]
    a, b = a.to(dev).eval(), b.to(dev).eval()
    b.matmul_precision = 'high'
    changed = _run(b, seq, spos, dev)
    b.matmul_precision = 'highest'
    want, got = _run(a, seq, spos, dev), _run(b, seq, spos, dev)
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    assert not torch.equal(changed[0], want[0])
    # model.train() and the module-by-module route stay fp32 whatever the attribute says
    b.matmul_precision = 'high'
    src = (seq.to(dev), spos.to(dev))
    a.matmul_precision = 'highest'
    with torch.no_grad():
        assert torch.equal(a._forward_composite(src, None, None, False, False)[0], b._forward_composite(src, None, None, False, False)[0])
    with pytest.raises(ValueError):
        b.matmul_precision = 'medium'
