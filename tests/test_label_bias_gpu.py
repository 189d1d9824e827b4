"""The weighted label graph on the GPU: the fused bias kernel (csrc/attention_bias.hip, lamp_mask kind LAMP_MASK_BIAS_F32)
against the fp64 restatement of tests/label_bias_common.py on the same fp32 inputs, in its three output modes; mask
equivalence, bit-identity, wide heads, the module in eval and training, the model against the oracle composition with the
restatement substituted for ``oracle.lamp_ref.sdpa``, every gradient, and run_train / run_eval end to end.

Kernel tolerance (the rule of tests/test_sigmoid_attn_gpu.py): the error against fp64 is at most the larger of one fp32 ulp and
4 x the matrix-wide gap of torch's own fp32 CPU evaluation of the same restatement.  Maps: absolute (values in [0, 1]); outputs:
row-relative, |O - O64| / sum_k p_k |v_k|.  Every case prints both figures before it asserts.

Module and model tolerances are those of the sibling tests of the sigmoid opt-in (same compositions, same shapes): maps 1e-5
(dropped training maps 2e-6 at |bias| <= ~8), eval logits 1e-4 (the project's contract), encoder output 5e-5, gradients
3e-4 of the gradient's largest entry.
"""
import ctypes as C
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

import enc_live_common as EC
import train_common as TC
from conftest import max_abs_diff
from label_bias_common import ULP, bias_sdpa, brute_counts, flat, random_bias, row_rel, sdpa_with_label_bias, toy_split
from oracle import lamp_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _N():
    from lamp_amd import _native as N
    return N


def fuse(t):
    """[B, H, l, d] -> [B, l, H * d], the layout of the fused projections."""
    B, H, l, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, l, H * d).contiguous()


def unfuse(t, H):
    B, l, hd = t.shape
    return t.view(B, l, H, hd // H).permute(0, 2, 1, 3)


def run_kernel(dev, q, k, v, bias, mode):
    """mode 'o': no maps; 'p': exactly normalised maps (lamp_sdpa_fwd); 'lse': single-pass maps (lamp_sdpa_fwd_fast_maps).
    -> (O [B, H, lq, dv] cpu, P [H * B, lq, lk] cpu | None)."""
    N = _N()
    B, H, lq, _ = q.shape
    lk = k.size(2)
    ms, keep = N.make_bias_mask(bias.to(dev), B, lq, lk)
    assert ms.kind == N.LAMP_MASK_BIAS_F32 and ms.stride_q % 4 == 0 and ms.stride_q >= lk
    out = N.sdpa_fused(fuse(q).to(dev), fuse(k).to(dev), fuse(v).to(dev), H, ms, 1.0 / float(q.size(3)) ** 0.5,
                       need_attn=mode != 'o', fast_maps=mode == 'lse')
    torch.cuda.synchronize()
    del keep
    return unfuse(out[0].cpu(), H), (out[1].cpu() if out[1] is not None else None)


def reference(q, k, v, bias):
    """-> (o64, p64, cpu fp32 gap of P, cpu fp32 row-relative gap of O, cpu fp32 gap of the row sums), NaN rows left out."""
    H = q.size(1)
    b = bias if bias.dim() == 2 else bias.repeat(H, 1, 1)
    o64, p64 = bias_sdpa(flat(q).double(), flat(k).double(), flat(v).double(), b.double())
    o32, p32 = bias_sdpa(flat(q), flat(k), flat(v), b)
    ok = ~torch.isnan(p64).any(dim=2)
    gap_p = (p32.double() - p64)[ok].abs().max().item()
    gap_sum = (p32.sum(dim=2).double() - 1.0)[ok].abs().max().item()
    return o64, p64, gap_p, row_rel(o32, o64, p64, flat(v).double()), gap_sum


def check_case(dev, q, k, v, bias, what, nan_rows=None):
    """All three output modes of one case against the restatement.  nan_rows: bool [H * B, lq], the rows that must be NaN."""
    o64, p64, gap_p, gap_o, gap_sum = reference(q, k, v, bias)
    ok = ~torch.isnan(p64).any(dim=2)
    if nan_rows is None:
        assert ok.all()
    else:
        assert torch.equal(~ok, nan_rows)
    bound_p, bound_o, bound_sum = max(ULP, 4.0 * gap_p), max(ULP, 4.0 * gap_o), max(ULP, 4.0 * gap_sum)
    outs = {}
    for mode in ('o', 'p', 'lse'):
        O, P = run_kernel(dev, q, k, v, bias, mode)
        outs[mode] = O
        fo = flat(O)
        assert torch.equal(torch.isnan(fo).any(dim=2), ~ok) and torch.equal(torch.isnan(fo).all(dim=2), ~ok), (what, mode)
        rel = row_rel(fo, o64, p64, flat(v).double())
        perr = serr = 0.0
        if P is not None:
            assert torch.equal(torch.isnan(P).any(dim=2), ~ok) and torch.equal(torch.isnan(P).all(dim=2), ~ok), (what, mode)
            perr = (P.double() - p64)[ok].abs().max().item()
            serr = (P.double().sum(dim=2) - 1.0)[ok].abs().max().item()
            assert (P[ok][torch.isinf(bias_rows(bias, q.size(1), ok))] == 0).all(), (what, mode)
        print('%s mode=%s: O cpu fp32 %.2e hip %.2e | P cpu fp32 %.2e hip %.2e | row sums cpu %.2e hip %.2e' %
              (what, mode, gap_o, rel, gap_p, perr, gap_sum, serr))
        assert rel <= bound_o, (what, mode, rel, bound_o)
        assert perr <= bound_p, (what, mode, perr, bound_p)
        if mode == 'p':
            assert serr <= bound_sum, (what, mode, serr, bound_sum)
    # the map write-out does not change the output: the single-pass kernel walks the same keys in the same order
    assert torch.equal(torch.nan_to_num(outs['o']), torch.nan_to_num(outs['lse'])), what
    return outs


def bias_rows(bias, H, ok):
    """The bias rows [n_ok, lk] that belong to the rows `ok` of an [H * B, lq, lk] map."""
    HB, lq = ok.shape
    b = bias.unsqueeze(0).expand(HB, -1, -1) if bias.dim() == 2 else bias.repeat(H, 1, 1)
    return b[ok]


def qkv(B, H, lq, lk, dk, dv, g):
    return (torch.randn(B, H, lq, dk, generator=g), torch.randn(B, H, lk, dk, generator=g), torch.randn(B, H, lk, dv, generator=g))


# ------------------------------------------------------------------ 1. the kernel against fp64
# the key split is bias_key_shares(lk) of attention_bias.hip: 1 share up to 48 keys (3 tiles), 2 up to 176 (11 tiles), 4 beyond
SHAPES = [(1, 1), (15, 17), (16, 16), (17, 15), (90, 90), (33, 64), (33, 65), (33, 48), (33, 49), (33, 176), (33, 177), (257, 200)]
WIDTHS = [(32, 32), (64, 64), (128, 128), (64, 32), (20, 12)]


@pytest.mark.parametrize('dk,dv', WIDTHS)
@pytest.mark.parametrize('lq,lk', SHAPES)
def test_kernel_against_fp64(dev, lq, lk, dk, dv):
    B, H = 3, 2
    g = torch.Generator().manual_seed(lq * 1000 + lk * 7 + dk)
    q, k, v = qkv(B, H, lq, lk, dk, dv, g)
    check_case(dev, q, k, v, random_bias(lq, lk, g), '%dx%d d%d/%d' % (lq, lk, dk, dv))


def test_fully_blocked_row_is_nan_in_exactly_that_row(dev):
    B, H, lq, lk, d = 3, 2, 33, 65, 64
    g = torch.Generator().manual_seed(11)
    q, k, v = qkv(B, H, lq, lk, d, d, g)
    bias = random_bias(lq, lk, g, full_row=20)            # shared: row 20 of every sample and head
    nan_rows = torch.zeros(H * B, lq, dtype=torch.bool)
    nan_rows[:, 20] = True
    check_case(dev, q, k, v, bias, 'blocked row, shared', nan_rows)
    per = random_bias(lq, lk, g, B=B, full_row=5)         # per sample: row 5 of sample 0 only
    nan_rows = torch.zeros(H, B, lq, dtype=torch.bool)
    nan_rows[:, 0, 5] = True
    check_case(dev, q, k, v, per, 'blocked row, per sample', nan_rows.view(H * B, lq))


def test_per_sample_bias(dev):
    B, H, lq, lk, d = 3, 2, 17, 50, 32
    g = torch.Generator().manual_seed(12)
    q, k, v = qkv(B, H, lq, lk, d, d, g)
    per = random_bias(lq, lk, g, B=B)
    outs = check_case(dev, q, k, v, per, 'per-sample bias')
    shared = check_case(dev, q, k, v, per[1], 'shared bias')
    assert torch.equal(outs['o'][1], shared['o'][1]) and not torch.equal(outs['o'][0], shared['o'][0])


def test_maps_only(dev):
    """lamp_sdpa_fwd with neither v nor out: the exactly normalised maps alone."""
    N = _N()
    B, H, lq, lk, d = 3, 2, 33, 65, 64
    g = torch.Generator().manual_seed(13)
    q, k, v = qkv(B, H, lq, lk, d, d, g)
    bias = random_bias(lq, lk, g)
    ms, keep = N.make_bias_mask(bias.to(dev), B, lq, lk)
    qd, kd = fuse(q).to(dev), fuse(k).to(dev)
    P = torch.full((H * B, lq, lk), float('nan'), device=dev)
    lay = N.AttnLayout(lq * H * d, d, H * d, lk * H * d, d, H * d, lk * H * d, d, H * d, lq * H * d, d, H * d)
    st = N.lib().lamp_sdpa_fwd(N.ptr(qd), N.ptr(kd), None, None, N.ptr(P), B, H, lq, lk, d, d, 1.0 / d ** 0.5, C.byref(ms),
                               C.byref(lay), N.stream())
    torch.cuda.synchronize()
    assert st == 0
    _, P2 = run_kernel(dev, q, k, v, bias, 'p')
    assert torch.equal(P.cpu(), P2)


# ------------------------------------------------------------------ 2. mask equivalence, bits, wide heads
@pytest.mark.parametrize('lq,lk,d', [(90, 90, 64), (33, 177, 128), (257, 200, 32)])
def test_a_zero_and_minus_inf_bias_is_the_mask(dev, lq, lk, d):
    N = _N()
    B, H = 3, 2
    g = torch.Generator().manual_seed(lq + lk + d)
    q, k, v = qkv(B, H, lq, lk, d, d, g)
    blocked = torch.rand(lq, lk, generator=g) < 0.5
    blocked[:, 3 % lk] = False
    bias = torch.zeros(lq, lk).masked_fill(blocked, float('-inf'))
    o64, p64, gap_p, gap_o, _ = reference(q, k, v, bias)
    ms, keep = N.make_mask(blocked.to(dev), B, lq, lk)
    assert ms.kind == N.LAMP_MASK_U8
    for mode in ('o', 'lse'):
        Ob, Pb = run_kernel(dev, q, k, v, bias, mode)
        out = N.sdpa_fused(fuse(q).to(dev), fuse(k).to(dev), fuse(v).to(dev), H, ms, 1.0 / d ** 0.5, need_attn=mode != 'o',
                           fast_maps=mode == 'lse')
        Om = unfuse(out[0].cpu(), H)
        rb, rm = row_rel(flat(Ob), o64, p64, flat(v).double()), row_rel(flat(Om), o64, p64, flat(v).double())
        print('%dx%d d%d %s: cpu fp32 %.2e bias kernel %.2e mask kernel %.2e' % (lq, lk, d, mode, gap_o, rb, rm))
        bound = max(ULP, 4.0 * gap_o)
        assert rb <= bound and rm <= bound        # each within the tolerance of the same fp64 result ...
        apart = row_rel(flat(Ob), flat(Om).double(), p64, flat(v).double())     # ... and of each other
        print('   bias kernel against mask kernel: O %.2e (bound %.2e)' % (apart, bound))
        assert apart <= bound, (mode, apart, bound)
        if Pb is not None:
            p_apart = (Pb.double() - out[1].cpu().double()).abs().max().item()
            print('   bias kernel against mask kernel: P %.2e (bound %.2e)' % (p_apart, max(ULP, 4.0 * gap_p)))
            assert p_apart <= max(ULP, 4.0 * gap_p), (mode, p_apart)
            assert (Pb[blocked.expand(H * B, lq, lk)] == 0).all()


@pytest.mark.parametrize('lk', [40, 90, 200])
def test_a_samples_bits_do_not_depend_on_its_batch(dev, lk):
    H, lq, d = 2, 90, 64
    g = torch.Generator().manual_seed(lk)
    q, k, v = qkv(5, H, lq, lk, d, d, g)
    bias = random_bias(lq, lk, g)
    for mode in ('o', 'lse'):
        O5, P5 = run_kernel(dev, q, k, v, bias, mode)
        O1, P1 = run_kernel(dev, q[2:3], k[2:3], v[2:3], bias, mode)
        assert torch.equal(O1[0], O5[2]), (lk, mode)
        if P5 is not None:
            assert torch.equal(P1.view(H, 1, lq, lk)[:, 0], P5.view(H, 5, lq, lk)[:, 2])


def test_wide_heads(dev):
    B, H, lq, lk, d = 3, 2, 24, 24, 192
    g = torch.Generator().manual_seed(14)
    q, k, v = qkv(B, H, lq, lk, d, d, g)
    bias = random_bias(lq, lk, g)
    o64, p64, gap_p, gap_o, _ = reference(q, k, v, bias)
    O, P = run_kernel(dev, q, k, v, bias, 'p')
    rel, perr = row_rel(flat(O), o64, p64, flat(v).double()), (P.double() - p64).abs().max().item()
    print('wide heads: O cpu fp32 %.2e hip %.2e | P cpu fp32 %.2e hip %.2e' % (gap_o, rel, gap_p, perr))
    assert rel <= max(ULP, 4.0 * gap_o) and perr <= max(ULP, 4.0 * gap_p)
    assert (P[torch.isinf(bias).expand(H * B, lq, lk)] == 0).all()


def test_cooccurrence_counts_on_the_device(dev):
    from lamp_amd import data as D
    rows, n_dict = toy_split()
    Cd = D.label_cooccurrence(rows, n_dict, dev)
    assert Cd.is_cuda and Cd.dtype == torch.float32 and torch.equal(Cd.cpu(), brute_counts(rows, n_dict - 4))
    rows, n_dict = toy_split(seed=9, n=203, L=24)
    assert torch.equal(D.label_cooccurrence(rows, n_dict, dev).cpu(), brute_counts(rows, 24))


# ------------------------------------------------------------------ 3. the module
def _module_bias(lq, lk, g, B=None):
    """N(0, 2) with ~30 % -inf and no +-30 entries (the sibling tolerances of the training maps assume |bias| <= ~8)."""
    shape = (lq, lk) if B is None else (B, lq, lk)
    bias = 2.0 * torch.randn(shape, generator=g)
    drop = torch.rand(shape, generator=g) < 0.3
    drop[..., 1] = False
    return bias.masked_fill(drop, float('-inf'))


def _mha_ref(sd, xq, xkv, bias, H, d, keep=None, p=0.0):
    B, lq, _ = xq.shape
    lk = xkv.size(1)
    split = lambda x, w, l: F.linear(x, w).view(B, l, H, d).permute(2, 0, 1, 3).reshape(H * B, l, d)   # noqa: E731
    q, k, v = split(xq, sd['w_qs.weight'], lq), split(xkv, sd['w_ks.weight'], lk), split(xkv, sd['w_vs.weight'], lk)
    P = bias_sdpa(q, k, v, bias.double())[1]
    Pd = P * keep / (1 - p) if keep is not None else P
    a = torch.bmm(Pd, v).view(H, B, lq, d).permute(1, 2, 0, 3).reshape(B, lq, H * d)
    return R.layer_norm(F.linear(a, sd['fc.weight']) + xq, sd['layer_norm.weight'], sd['layer_norm.bias']), Pd


@pytest.mark.parametrize('d', [32, 192])
def test_module_eval_and_train(dev, d):
    N = _N()
    from lamp_amd import training
    from lamp_amd.SubLayers import MultiHeadAttention
    H, B, lq, lk, dm, p = 2, 2, 24, 40, 64, 0.2
    torch.manual_seed(3)
    mod = MultiHeadAttention(H, dm, d, d, dropout=0.0, dropout2=p).to(dev)
    g = torch.Generator().manual_seed(4)
    xq, xkv = torch.randn(B, lq, dm, generator=g), torch.randn(B, lk, dm, generator=g)
    bias = _module_bias(lq, lk, g)
    ms, keepalive = N.make_bias_mask(bias.to(dev), B, lq, lk)
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mod.state_dict().items()}
    x64 = xq.double().requires_grad_(True)
    # eval
    mod.eval()
    with torch.no_grad():
        out, attn = mod(xq.to(dev), xkv.to(dev), xkv.to(dev), attn_mask=ms)
        ref, P = _mha_ref(sd, x64, xkv.double(), bias, H, d)
    assert max_abs_diff(attn, P) <= 1e-5 and max_abs_diff(out, ref) <= 1e-4
    # train: probability dropout 0.2, the returned map is the dropped one
    mod.train()
    torch.manual_seed(11)
    seed_attn = training._Seeds().next()
    torch.manual_seed(11)
    xq_d, xkv_d = xq.to(dev).requires_grad_(True), xkv.to(dev)
    out, attn = mod(xq_d, xkv_d, xkv_d, attn_mask=ms)
    w = torch.randn(B, lq, dm, generator=g)
    (out * w.to(dev)).sum().backward()
    keep = N.dropout_keep_mask(H * B * lq * lk, p, seed_attn).view(H * B, lq, lk).double()
    ref, Pd = _mha_ref(sd, x64, xkv.double(), bias, H, d, keep, p)
    (ref * w.double()).sum().backward()
    assert max_abs_diff(attn, Pd.detach()) <= 2e-6 and torch.isfinite(out).all()
    assert max_abs_diff(out, ref.detach()) <= 1e-4
    for name, prm in mod.named_parameters():
        r = sd[name].grad
        assert max_abs_diff(prm.grad, r) <= 3e-4 * r.abs().max().item() + 1e-9, name
    assert max_abs_diff(xq_d.grad, x64.grad) <= 3e-4 * x64.grad.abs().max().item() + 1e-9
    del keepalive


# ------------------------------------------------------------------ 4. the model
L_A = EC.SHAPES['A']['L']
assert L_A != EC.SHAPES['A']['T']      # the restatement recognises the label self-attention by its square L x L shape


def _model_bias(kind, blocked):
    """(L, L) bias of a model case.  'random': N(0, 2), ~20 % -inf, never the first key a row's mask allows (no NaN row);
    'logp': label_bias_from_counts of a toy split (finite everywhere)."""
    from lamp_amd import data as D
    if kind == 'logp':
        rows, n_dict = toy_split(seed=21, n=60, L=L_A)
        return D.label_bias_from_counts(brute_counts(rows, L_A), 'logp', 1.0)
    g = torch.Generator().manual_seed(31)
    bias = 2.0 * torch.randn(L_A, L_A, generator=g)
    drop = torch.rand(L_A, L_A, generator=g) < 0.2
    allowed = ~blocked if blocked is not None else torch.ones(L_A, L_A, dtype=torch.bool)
    first = allowed.float().argmax(dim=1)
    assert allowed[torch.arange(L_A), first].all()
    drop[torch.arange(L_A), first] = False
    return bias.masked_fill(drop, float('-inf'))


_CASES = {}


def _case(mask, kind, live=False, int_preds=False):
    """-> (model on the CPU, sd, blocked, seq, pos, h, bias, fp64 reference tuple); the reference is computed once per case."""
    key = (mask, kind, live)
    blocked = EC.build('A', mask, True, live=live)[2]
    bias = _model_bias(kind, blocked)
    m, sd, blocked, seq, spos, h = EC.build('A', mask, True, live=live, int_preds=int_preds, label_bias=bias)
    if key not in _CASES:
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        mp = pytest.MonkeyPatch()
        try:
            with torch.no_grad():
                enc = EC.live_encoder_ref(sd64, seq, spos, h)[0] if live else R.encoder_forward(sd64, seq, spos, h)[0]
                mp.setattr(R, 'sdpa', sdpa_with_label_bias(bias.double(), L_A))
                y, slf, encdec, int_outs = R.decoder_forward(sd64, seq, enc, blocked, h)
        finally:
            mp.undo()
        w = sd64['tgt_word_proj.linear.weight']
        _CASES[key] = (R.readout(y, w), enc, slf, encdec, [R.readout(o, w) for o in int_outs[:-1]])
    return m, sd, blocked, seq, spos, h, bias, _CASES[key]


def _run(m, seq, pos, dev, **kw):
    with torch.no_grad():
        return m((seq.to(dev), pos.to(dev)), None, None, None, **kw)


@pytest.mark.parametrize('kind', ['random', 'logp'])
@pytest.mark.parametrize('mask', ['none', 'prior'])
def test_model_against_the_oracle_composition(dev, mask, kind):
    m, sd, blocked, seq, spos, h, bias, (ref_logits, ref_enc, ref_slf, ref_encdec, _) = _case(mask, kind)
    m = m.to(dev).eval()
    logits, enc, extra = _run(m, seq, spos, dev)
    print('%s %s: logits %.3e enc %.3e' % (mask, kind, max_abs_diff(logits, ref_logits), max_abs_diff(enc, ref_enc)))
    assert extra is None and max_abs_diff(logits, ref_logits) <= 1e-4 and max_abs_diff(enc, ref_enc) <= 5e-5
    l2, e2, _, (slf, encdec) = _run(m, seq, spos, dev, return_attns=True)
    assert max_abs_diff(l2, ref_logits) <= 1e-4
    for got, want in zip(slf + encdec, ref_slf + ref_encdec):
        assert max_abs_diff(got, want) <= 1e-5
    for a in slf:   # a blocked pair, by the mask or by the bias, gets exactly no attention
        gone = torch.isinf(m.decoder.label_bias_f32[:, :L_A].cpu())
        assert (a.cpu()[gone.expand_as(a)] == 0).all()
    # the module-by-module route: the same function
    with torch.no_grad():
        comp = m._forward_composite((seq.to(dev), spos.to(dev)), None, None, True, False)
    assert max_abs_diff(comp[0], ref_logits) <= 1e-4 and max_abs_diff(comp[0], logits) <= 2e-4
    for got, want in zip(comp[3][0] + comp[3][1], ref_slf + ref_encdec):
        assert max_abs_diff(got, want) <= 1e-5
    # the same weights without the bias: another function
    plain = EC.build('A', mask, True, live=False)[0].to(dev).eval()
    assert max_abs_diff(_run(plain, seq, spos, dev)[0], ref_logits) > 1e-3


def test_model_int_preds(dev):
    m, sd, blocked, seq, spos, h, bias, ref = _case('prior', 'random', int_preds=True)
    m = m.to(dev).eval()
    logits, enc, ipreds = _run(m, seq, spos, dev, int_preds=True)
    assert max_abs_diff(logits, ref[0]) <= 1e-4 and len(ipreds) == len(ref[4]) == 3
    for got, want in zip(ipreds, ref[4]):
        assert max_abs_diff(got, want) <= 1e-4


def test_model_live_encoder_and_matmul_precision(dev):
    m, sd, blocked, seq, spos, h, bias, ref = _case('prior', 'logp', live=True)
    logits, enc, _ = _run(m.to(dev).eval(), seq, spos, dev)
    assert max_abs_diff(logits, ref[0]) <= 1e-4 and max_abs_diff(enc, ref[1]) <= 5e-5
    m, sd, blocked, seq, spos, h, bias, ref = _case('prior', 'random')
    m = m.to(dev).eval()
    highest = _run(m, seq, spos, dev)[0]
    m.matmul_precision = 'high'
    high = _run(m, seq, spos, dev)[0]
    assert max_abs_diff(high, ref[0]) <= 1e-4 and not torch.equal(high, highest)


def test_model_bits_under_a_micro_batch_split_and_reordering(dev):
    N = _N()
    m, sd, blocked, seq, spos, h, bias, ref = _case('prior', 'random')
    m = m.to(dev).eval()
    n, T = seq.shape
    logits, enc, _, (slf, encdec) = _run(m, seq, spos, dev, return_attns=True)
    assert torch.equal(_run(m, seq, spos, dev)[0], logits)
    for b0 in range(n):
        assert torch.equal(_run(m, seq[b0:b0 + 1], spos[b0:b0 + 1], dev)[0], logits[b0:b0 + 1]), b0
    perm = list(reversed(range(n)))
    assert torch.equal(_run(m, seq[perm], spos[perm], dev)[0][perm], logits)
    built = m._native_model()
    opts = N.FwdOptions(0, N.LAMP_FWD_LABEL_BIAS, None, None)
    per = N.lib().lamp_forward_opts_workspace_bytes(C.byref(built[0]), C.byref(opts), 1, T, 1)
    assert per == N.lib().lamp_forward_workspace_bytes(C.byref(built[0]), 1, T, 1)
    m.workspace_limit_bytes = per + 4096          # room for one sample: a forced split
    try:
        s_logits, s_enc, _, (s_slf, s_encdec) = _run(m, seq, spos, dev, return_attns=True)
    finally:
        del m.workspace_limit_bytes
    assert torch.equal(s_logits, logits) and torch.equal(s_enc, enc)
    for got, want in zip(s_slf + s_encdec, slf + encdec):
        assert torch.equal(got, want)


def test_onehot_model(dev):
    import onehot_common as OC
    m = OC.build_model(mask='none')
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    L = 23
    g = torch.Generator().manual_seed(41)
    bias = (2.0 * torch.randn(L, L, generator=g)).masked_fill(torch.rand(L, L, generator=g) < 0.2, float('-inf'))
    bias.fill_diagonal_(0.3)
    from lamp_amd.Models import LAMP
    torch.manual_seed(0)
    mb = LAMP(9, L, 64, L, n_layers_enc=2, n_layers_dec=2, n_head=4, n_head2=4, d_word_vec=64, d_model=64, d_inner_hid=128,
              d_k=16, d_v=16, encoder='graph', decoder='graph', dropout=0.0, dec_dropout=0.0, dec_dropout2=0.0, onehot=True,
              label_mask='none', label_bias=bias)
    mb.load_state_dict(sd)
    seq, pos = OC.make_dna(3, 32, lengths=[32, 21, 9])
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    mp = pytest.MonkeyPatch()
    try:
        with torch.no_grad():
            enc, seq2 = OC.onehot_encoder_ref(sd64, seq, pos)
            assert enc.size(1) != L
            mp.setattr(R, 'sdpa', sdpa_with_label_bias(bias.double(), L))
            y = R.decoder_forward(sd64, seq2, enc, None, 4)[0]
    finally:
        mp.undo()
    ref = R.readout(y, sd64['tgt_word_proj.linear.weight'])
    logits = _run(mb.to(dev).eval(), seq, pos, dev)[0]
    assert max_abs_diff(logits, ref) <= 1e-4
    assert max_abs_diff(_run(m.to(dev).eval(), seq, pos, dev)[0], ref) > 1e-3       # without the bias: another function


def test_make_mask_still_reads_a_float_tensor_as_nonzero_blocked(dev):
    N = _N()
    B, H, lq, lk, d = 2, 2, 17, 33, 32
    g = torch.Generator().manual_seed(42)
    q, k, v = qkv(B, H, lq, lk, d, d, g)
    blocked = torch.rand(lq, lk, generator=g) < 0.4
    blocked[:, 0] = False
    as_float = torch.where(blocked, -2.5 * torch.ones(lq, lk), torch.zeros(lq, lk))     # the reference's format: nonzero = blocked
    ms, keep = N.make_mask(as_float.to(dev), B, lq, lk)
    assert ms.kind == N.LAMP_MASK_U8
    out = N.sdpa_fused(fuse(q).to(dev), fuse(k).to(dev), fuse(v).to(dev), H, ms, 1.0 / d ** 0.5, need_attn=True)
    P = out[1].cpu()
    assert (P[blocked.expand(H * B, lq, lk)] == 0).all() and (P[~blocked.expand(H * B, lq, lk)] > 0).all()


def test_data_parallel_replicas_carry_the_bias(dev):
    m, sd, blocked, seq, spos, h, bias, ref = _case('prior', 'random')
    m = m.to(dev).eval()
    rep = torch.nn.parallel.replicate(m, [dev])[0]
    assert rep.decoder.label_bias_f32 is not None
    with torch.no_grad():
        logits = rep((seq.to(dev), spos.to(dev)), None, None, None)[0]
    assert max_abs_diff(logits, ref[0]) <= 1e-4


def test_a_zero_bias_changes_nothing_that_matters(dev):
    plain, sd, blocked, seq, spos, h = EC.build('A', 'prior', True, live=False)
    zero = EC.build('A', 'prior', True, live=False, label_bias=torch.zeros(L_A, L_A))[0]
    a, b = _run(plain.to(dev).eval(), seq, spos, dev), _run(zero.to(dev).eval(), seq, spos, dev)
    ref = R.forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, seq, spos, h, blocked)[0]
    ea, eb = max_abs_diff(a[0], ref), max_abs_diff(b[0], ref)
    # "within rounding" by the kernel tests' rule: 4 x the gap of torch's own fp32 CPU evaluation of the same composition against
    # fp64, at least one fp32 ulp of the largest logit
    gap = max_abs_diff(R.forward(sd, seq, spos, h, blocked)[0], ref)
    bound = max(ULP * float(ref.abs().max()), 4.0 * gap)
    apart = max_abs_diff(a[0], b[0])
    print('zero bias: without %.3e with %.3e apart %.3e (cpu fp32 gap %.3e, bound %.3e)' % (ea, eb, apart, gap, bound))
    assert ea <= 1e-4 and eb <= 1e-4 and torch.equal(a[1], b[1])       # the encoder never sees the bias
    assert apart <= bound, (apart, bound)


@pytest.mark.parametrize('mask,kind', [('prior', 'random'), ('none', 'logp')])
def test_every_parameter_gradient_matches_oracle_autograd(dev, mask, kind):
    m, sd, blocked, seq, spos, h, bias, _ = _case(mask, kind)
    m = m.to(dev)
    tgt = (torch.rand(seq.size(0), L_A, generator=torch.Generator().manual_seed(1)) < 0.2).float()
    sd64 = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    enc64 = R.encoder_forward(sd64, seq, spos, h)[0]
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(R, 'sdpa', sdpa_with_label_bias(bias.double(), L_A))
        y = R.decoder_forward(sd64, seq, enc64, blocked, h)[0]
    finally:
        mp.undo()
    ref_logits = R.readout(y, sd64['tgt_word_proj.linear.weight'])
    ref_loss = F.binary_cross_entropy_with_logits(ref_logits, tgt.double())
    ref_loss.backward()
    m.train()
    logits, enc, extra = m((seq.to(dev), spos.to(dev)), None, None, tgt.to(dev))
    assert max_abs_diff(logits, ref_logits.detach()) < 1e-4 and max_abs_diff(enc, enc64.detach()) < 5e-5
    loss = F.binary_cross_entropy_with_logits(logits, tgt.to(dev))
    loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-5
    checked = 0
    for pname, p in m.named_parameters():
        ref = sd64[pname].grad
        if pname == 'encoder.position_enc.weight' or ('encoder.layer_stack' in pname and 'slf_attn' in pname):
            assert p.grad is None
            continue
        if pname == 'decoder.tgt_word_emb.weight' and sd64['tgt_word_proj.weight'].grad is not None:
            ref = ref + sd64['tgt_word_proj.weight'].grad
        assert p.grad is not None and ref is not None, pname
        scale = ref.abs().max().item()
        assert max_abs_diff(p.grad, ref) <= 3e-4 * scale + 1e-9, (pname, max_abs_diff(p.grad, ref), scale)
        checked += 1
    assert checked >= 35
    assert not m.decoder.label_bias_f32.requires_grad          # a constant: nothing flows to it


# ------------------------------------------------------------------ 5. end to end
def test_run_train_with_a_label_bias_and_run_eval_reads_the_setting():
    from lamp_amd import run_eval, run_train
    with tempfile.TemporaryDirectory(prefix='lamp_run_') as root:
        assert 'test' not in root
        data_path = os.path.join(root, 'train_valid_data.pt')
        torch.save(TC.synthetic_dataset(n_train=64, n_valid=16, n_test=16), data_path)
        args = ['-data', data_path, '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2', '-label_mask',
                'prior', '-batch_size', '16']
        hist = run_train.main(args + ['-epoch', '1', '-lr', '0.003', '-dropout', '0.0', '-results_dir', os.path.join(root, 'res'),
                                      '-name', 'lb', '-seed', '1', '-label_bias', 'logp', '-label_bias_scale', '0.5'])
        assert len(hist) == 1 and hist[0]['train_loss'] == hist[0]['train_loss']
        assert '.lbias_logp_0.5' in hist[0]['checkpoint']
        ckpt = torch.load(hist[0]['checkpoint'], map_location='cpu', weights_only=False)
        assert ckpt['settings'].label_bias == 'logp' and ckpt['settings'].label_bias_scale == 0.5
        assert not any('label_bias' in k for k in ckpt['model'])
        out = run_eval.main(args + ['-checkpoint', hist[0]['checkpoint'], '-split', 'test'])
        assert out['bce_total'] / out['n_samples'] == hist[0]['test_loss']    # the bias is rebuilt: the epoch's own test loss
        bare = os.path.join(root, 'bare.chkpt')
        torch.save(ckpt['model'], bare)                                        # a bare state dict: no bias unless the flags say so
        off = run_eval.main(args + ['-checkpoint', bare, '-split', 'test'])
        on = run_eval.main(args + ['-checkpoint', bare, '-split', 'test', '-label_bias', 'logp', '-label_bias_scale', '0.5'])
        assert on['bce_total'] == out['bce_total'] and off['bce_total'] != out['bce_total']
