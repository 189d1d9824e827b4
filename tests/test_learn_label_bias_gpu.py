"""The learnable label graph on the GPU (LAMP(learn_label_bias=True)): lamp_attn_bias_bwd against the fp64 sum,
lamp_label_bias_fold against the host's fold, the bias gradient of the model against fp64 autograd through the restatement of
tests/label_bias_common.py on both backward routes, the untouched forward, the refresh of the folded buffer after optimizer
steps and load_state_dict, dropout, and run_train / run_eval end to end.

Tolerances are the project's own rules.  Kernel: elementwise, max(one fp32 ulp at the value, 4 x the gap that torch's fp32 CPU
evaluation of the same sum shows against fp64 on the same inputs) -- train_common.within, which prints both figures.  Model
gradients: 3e-4 x the reference gradient's largest entry + 1e-9.  Logits: 1e-4."""
import ctypes as C
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

import enc_live_common as EC
import train_common as TC
from conftest import max_abs_diff
from label_bias_common import brute_counts, random_bias, sdpa_with_label_bias, toy_split
from oracle import lamp_ref as R
from redzone_common import FILL_NAN, Arena, bit_equal

pytestmark = pytest.mark.gpu

NEG_INF = float('-inf')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _N():
    from lamp_amd import _native as N
    return N


# ------------------------------------------------------------------ 1. lamp_attn_bias_bwd against the fp64 sum
# 64 / 65 / 130 slices: one, two and three first-stage chunks; 33 x 40: lq != lk; 257 columns: more than one 256-thread group a row
BWD_SHAPES = [(1, 1, 1), (3, 7, 7), (8, 33, 40), (64, 24, 24), (65, 24, 24), (130, 90, 90), (8, 257, 257)]


def _bwd_call(N, arena, dS, folded, n, lq, lk, ld, scale):
    """One lamp_attn_bias_bwd call on exactly-sized buffers between red zones -> the (lq, lk) view of dbias [lq, ld]."""
    dS_d = arena.inp(dS, 'dS')
    bias_d = arena.inp(folded, 'bias')
    out = arena.out((lq, lk), 'dbias', ld=ld)
    nb = N.lib().lamp_attn_bias_bwd_workspace_bytes(n, lq, lk)
    ws = arena.scratch(nb, 'workspace')
    st = N.lib().lamp_attn_bias_bwd(dS_d.data_ptr(), n, lq, lk, scale, bias_d.data_ptr(), folded.size(1), out.data_ptr(), ld,
                                    ws.data_ptr(), nb, N.stream())
    assert st == 0
    arena.check()          # nothing outside dbias and the workspace changed, the row padding included; every element written
    return out.cpu()


@pytest.mark.parametrize('pad', [0, 3])
@pytest.mark.parametrize('n,lq,lk', BWD_SHAPES)
def test_attn_bias_bwd_against_the_fp64_sum(dev, n, lq, lk, pad):
    N = _N()
    g = torch.Generator().manual_seed(n * 1000 + lq * 7 + lk)
    dS = torch.randn(n, lq, lk, generator=g) * 0.05
    bias = random_bias(lq, lk, g)
    folded = N.pad_bias_rows(bias)
    blocked = torch.isinf(bias)
    scale = 8.0 if lk != 40 else float(torch.tensor(20.0).sqrt())     # sqrt(d_k): a power of two and one that rounds
    ld = lk + pad
    # a NaN behind a blocked entry comes out 0; behind an allowed entry it stays, in that element only
    allowed_at = (~blocked).nonzero()[len((~blocked).nonzero()) // 2].tolist()
    dS[n // 2, allowed_at[0], allowed_at[1]] = float('nan')
    if blocked.any():
        blocked_at = blocked.nonzero()[len(blocked.nonzero()) // 2].tolist()
        dS[n - 1, blocked_at[0], blocked_at[1]] = float('nan')
    else:
        assert (lq, lk) == (1, 1)
    want64 = (scale * dS.double().sum(dim=0)).masked_fill(blocked, 0.0)
    cpu32 = (torch.tensor(scale) * dS.sum(dim=0)).masked_fill(blocked, 0.0)
    ok = ~torch.isnan(want64)
    assert int((~ok).sum()) == 1 and not ok[allowed_at[0], allowed_at[1]]
    gap = float((cpu32.double() - want64)[ok].abs().max()) if ok.any() else 0.0
    got = _bwd_call(N, Arena(dev, FILL_NAN, 8 << 20), dS, folded, n, lq, lk, ld, scale)
    TC.within(got, want64, gap, 'attn_bias_bwd %dx%dx%d ld %d' % (n, lq, lk, ld))
    assert (got[blocked] == 0).all() and not torch.signbit(got[blocked]).any()       # exactly 0 whatever dS holds there
    again = _bwd_call(N, Arena(dev, FILL_NAN, 8 << 20), dS, folded, n, lq, lk, ld, scale)
    assert bit_equal(got, again)                                                     # a fixed summation order
    # without a bias nothing is selected: the planted NaN behind the (formerly) blocked entry shows
    arena = Arena(dev, FILL_NAN, 8 << 20)
    dS_d, out = arena.inp(dS, 'dS'), arena.out((lq, lk), 'dbias', ld=ld)
    nb = N.lib().lamp_attn_bias_bwd_workspace_bytes(n, lq, lk)
    ws = arena.scratch(nb, 'workspace')
    assert N.lib().lamp_attn_bias_bwd(dS_d.data_ptr(), n, lq, lk, scale, None, 0, out.data_ptr(), ld, ws.data_ptr(), nb,
                                      N.stream()) == 0
    arena.check()
    TC.within(out.cpu(), scale * dS.double().sum(dim=0), gap, 'attn_bias_bwd %dx%dx%d no bias' % (n, lq, lk))


def test_attn_bias_bwd_wrapper_equals_the_column_sum(dev):
    """The first stage IS lamp_colsum's: with scale 1 and no bias the result is lamp_colsum's, bit for bit."""
    N = _N()
    g = torch.Generator().manual_seed(5)
    dS = torch.randn(130, 24, 24, generator=g).to(dev)
    a = N.attn_bias_bwd(dS, 1.0)
    b = N.colsum(dS.view(130, 24 * 24)).view(24, 24)
    assert tuple(a.shape) == (24, 24) and torch.equal(a, b)
    assert torch.equal(N.attn_bias_bwd(dS.view(2, 65, 24, 24), 1.0), a)               # (H, B, lq, lk), as the per-launch route has it


# ------------------------------------------------------------------ 2. lamp_label_bias_fold against the host's fold
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('L', [7, 24, 33])
def test_label_bias_fold_equals_the_hosts_fold(dev, L, masked):
    N = _N()
    g = torch.Generator().manual_seed(L)
    param = random_bias(L, L, g)
    mask = (torch.rand(L, L, generator=g) < 0.4).to(torch.uint8) if masked else None
    want = N.pad_bias_rows(param.masked_fill(mask != 0, NEG_INF) if masked else param)
    arena = Arena(dev, FILL_NAN, 1 << 20)
    p_d = arena.inp(param, 'param')
    m_d = arena.inp(mask, 'mask') if masked else None
    out = arena.out(tuple(want.shape), 'out')
    assert N.lib().lamp_label_bias_fold(p_d.data_ptr(), L, N.ptr(m_d), L, out.data_ptr(), N.stream()) == 0
    arena.check()
    assert bit_equal(out.cpu(), want)
    # the wrapper, in place, from a parameter with padded rows
    wide = torch.full((L, L + 5), 9.0)
    wide[:, :L] = param
    buf = torch.full(tuple(want.shape), 3.0, device=dev)
    ptr = buf.data_ptr()
    N.label_bias_fold(wide.to(dev)[:, :L], mask.to(dev) if masked else None, buf)
    assert buf.data_ptr() == ptr and bit_equal(buf.cpu(), want)


# ------------------------------------------------------------------ 3. the model's gradients
L_A = EC.SHAPES['A']['L']
WIDE = dict(EC.SHAPES['A'], d=384, dff=256)          # d_k = d_v = 192 > 128: the general attention route, per-launch backward
assert L_A != EC.SHAPES['A']['T']                    # the restatement recognises the label self-attention by its square shape


def _model_bias(kind, blocked):
    """As the constant-bias tests build theirs.  'random': N(0, 2), ~20 % -inf, never the first key a row's mask allows."""
    from lamp_amd import data as D
    if kind == 'logp':
        rows, n_dict = toy_split(seed=21, n=60, L=L_A)
        return D.label_bias_from_counts(brute_counts(rows, L_A), 'logp', 1.0)
    g = torch.Generator().manual_seed(31)
    bias = 2.0 * torch.randn(L_A, L_A, generator=g)
    drop = torch.rand(L_A, L_A, generator=g) < 0.2
    allowed = ~blocked if blocked is not None else torch.ones(L_A, L_A, dtype=torch.bool)
    first = allowed.float().argmax(dim=1)
    drop[torch.arange(L_A), first] = False
    return bias.masked_fill(drop, NEG_INF)


_REFS = {}


def _case(mask, kind, shape='A', **kw):
    """-> (learnable model on the CPU, sd, blocked, seq, pos, h, bias, tgt, (ref logits, {name: fp64 gradient})); the fp64
    reference -- autograd through sdpa_with_label_bias(bias64.requires_grad_(), L) around the oracle composition, BCE loss --
    is computed once per (mask, kind, shape) and shared."""
    s = WIDE if shape == 'wide' else shape
    blocked = EC.build(s, mask, True, live=False)[2]
    bias = _model_bias(kind, blocked)
    m, sd, blocked, seq, spos, h = EC.build(s, mask, True, live=False, label_bias=bias, learn_label_bias=True, **kw)
    tgt = (torch.rand(seq.size(0), L_A, generator=torch.Generator().manual_seed(1)) < 0.2).float()
    key = (mask, kind, shape)
    if key not in _REFS:
        sd64 = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
        bias64 = bias.double().requires_grad_()
        enc64 = R.encoder_forward(sd64, seq, spos, h)[0]
        mp = pytest.MonkeyPatch()
        try:
            mp.setattr(R, 'sdpa', sdpa_with_label_bias(bias64, L_A))
            y = R.decoder_forward(sd64, seq, enc64, blocked, h)[0]
        finally:
            mp.undo()
        logits = R.readout(y, sd64['tgt_word_proj.linear.weight'])
        F.binary_cross_entropy_with_logits(logits, tgt.double()).backward()
        grads = {k: v.grad for k, v in sd64.items() if v.requires_grad}
        grads['decoder.label_bias'] = bias64.grad
        _REFS[key] = (logits.detach(), grads)
    return m, sd, blocked, seq, spos, h, bias, tgt, _REFS[key]


def _check_gradients(m, seq, spos, tgt, ref, dev):
    ref_logits, grads = ref
    m = m.to(dev).train()
    logits, enc, extra = m((seq.to(dev), spos.to(dev)), None, None, tgt.to(dev))
    assert max_abs_diff(logits, ref_logits) <= 1e-4
    F.binary_cross_entropy_with_logits(logits, tgt.to(dev)).backward()
    got, want = m.decoder.label_bias.grad, grads['decoder.label_bias']
    assert got is not None and tuple(got.shape) == (L_A, L_A) and torch.isfinite(want).all()
    gone = torch.isinf(m.decoder.label_bias_f32[:, :L_A])
    assert (got[gone] == 0).all() and (want[gone.cpu()] == 0).all()                  # exactly 0 where the folded bias blocks
    assert got[~gone].abs().min() > 0                                                # ... and only there
    scale = want.abs().max().item()
    print('d label_bias: max |err| %.3e, bound %.3e (largest entry %.3e)' % (max_abs_diff(got, want), 3e-4 * scale + 1e-9, scale))
    assert scale > 0 and max_abs_diff(got, want) <= 3e-4 * scale + 1e-9
    checked = 0
    for pname, p in m.named_parameters():
        if pname == 'decoder.label_bias':
            continue
        if pname == 'encoder.position_enc.weight' or ('encoder.layer_stack' in pname and 'slf_attn' in pname):
            assert p.grad is None
            continue
        r = grads[pname]
        if pname == 'decoder.tgt_word_emb.weight' and grads.get('tgt_word_proj.weight') is not None:
            r = r + grads['tgt_word_proj.weight']
        assert p.grad is not None and r is not None, pname
        s = r.abs().max().item()
        assert max_abs_diff(p.grad, r) <= 3e-4 * s + 1e-9, (pname, max_abs_diff(p.grad, r), s)
        checked += 1
    assert checked >= 35
    return got


@pytest.mark.parametrize('composite', [True, False])
@pytest.mark.parametrize('kind', ['random', 'logp'])
@pytest.mark.parametrize('mask', ['prior', 'none'])
def test_bias_gradient_matches_fp64_autograd(dev, mask, kind, composite, monkeypatch):
    from lamp_amd import training
    monkeypatch.setattr(training, 'COMPOSITE_CALLS', composite)
    m, sd, blocked, seq, spos, h, bias, tgt, ref = _case(mask, kind)
    if kind == 'random':
        assert torch.isinf(bias).any()
    if mask == 'prior':
        assert blocked.any() and torch.isfinite(m.decoder.label_bias.detach()[blocked.view(L_A, L_A)]).any()
    _check_gradients(m, seq, spos, tgt, ref, dev)


def test_bias_gradient_with_heads_wider_than_128(dev):
    m, sd, blocked, seq, spos, h, bias, tgt, ref = _case('prior', 'random', shape='wide')
    assert m.d_k == 192
    _check_gradients(m, seq, spos, tgt, ref, dev)


def test_both_routes_give_the_same_bias_gradient_bits(dev, monkeypatch):
    """lamp_mha_bwd's dP buffer and the per-launch route's lamp_softmax_bwd output are the same dS, reduced by the same call."""
    from lamp_amd import training
    grads = []
    for composite in (True, False):
        monkeypatch.setattr(training, 'COMPOSITE_CALLS', composite)
        m, sd, blocked, seq, spos, h, bias, tgt, ref = _case('prior', 'random')
        m = m.to(dev).train()
        logits = m((seq.to(dev), spos.to(dev)), None, None, tgt.to(dev))[0]
        F.binary_cross_entropy_with_logits(logits, tgt.to(dev)).backward()
        grads.append(m.decoder.label_bias.grad.clone())
    assert torch.equal(grads[0], grads[1])


def test_a_frozen_parameter_and_autograd_grad(dev):
    m, sd, blocked, seq, spos, h, bias, tgt, ref = _case('none', 'logp')
    m = m.to(dev).train()
    src = (seq.to(dev), spos.to(dev))
    loss = F.binary_cross_entropy_with_logits(m(src, None, None, tgt.to(dev))[0], tgt.to(dev))
    (g,) = torch.autograd.grad(loss, [m.decoder.label_bias])                          # captured, not accumulated
    want = ref[1]['decoder.label_bias']
    assert m.decoder.label_bias.grad is None and max_abs_diff(g, want) <= 3e-4 * want.abs().max().item() + 1e-9
    m.decoder.label_bias.requires_grad_(False)
    F.binary_cross_entropy_with_logits(m(src, None, None, tgt.to(dev))[0], tgt.to(dev)).backward()
    assert m.decoder.label_bias.grad is None and m.decoder.tgt_word_emb.weight.grad is not None


def test_the_module_by_module_route_trains_the_bias(dev):
    """A graph decoder over a vector encoder (enc_transform='mean') runs GraphDecoder.forward: the parameter gets a gradient
    there too, finite and 0 at blocked entries."""
    blocked = EC.build('A', 'prior', True, live=False)[2]
    bias = _model_bias('random', blocked)
    m, sd, blocked, seq, spos, h = EC.build('A', 'prior', True, live=False, label_bias=bias, learn_label_bias=True,
                                            enc_transform='mean')
    tgt = (torch.rand(seq.size(0), L_A, generator=torch.Generator().manual_seed(1)) < 0.2).float()
    m = m.to(dev).train()
    assert not m._fused
    logits = m((seq.to(dev), spos.to(dev)), None, None, tgt.to(dev))[0]
    F.binary_cross_entropy_with_logits(logits, tgt.to(dev)).backward()
    g = m.decoder.label_bias.grad
    gone = torch.isinf(m.decoder.label_bias_f32[:, :L_A])
    assert g is not None and torch.isfinite(g).all() and (g[gone] == 0).all() and g[~gone].abs().min() > 0


# ------------------------------------------------------------------ 4. the forward is untouched
def _run(m, seq, pos, dev, **kw):
    with torch.no_grad():
        return m((seq.to(dev), pos.to(dev)), None, None, None, **kw)


def _constant_twin(learnable, mask, bias=None, **kw):
    """A constant-bias model on the learnable model's weights, its bias taken from the parameter as it is now."""
    if bias is None:
        bias = learnable.decoder.label_bias.detach().cpu().clone()
    twin = EC.build('A', mask, True, live=False, label_bias=bias, **kw)[0]
    state = {k: v for k, v in learnable.state_dict().items() if k != 'decoder.label_bias'}
    twin.load_state_dict(state, strict='int_preds' not in kw)
    assert twin.decoder.label_bias is None
    return twin


@pytest.mark.parametrize('mask', ['prior', 'none'])
def test_logits_equal_the_constant_bias_models_bit_for_bit(dev, mask):
    m, sd, blocked, seq, spos, h, bias, tgt, (ref_logits, _) = _case(mask, 'random')
    m = m.to(dev).eval()
    twin = _constant_twin(m, mask).to(dev).eval()
    assert bit_equal(m.decoder.label_bias_f32, twin.decoder.label_bias_f32)
    a, b = _run(m, seq, spos, dev), _run(twin, seq, spos, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and max_abs_diff(a[0], ref_logits) <= 1e-4
    ra, rb = _run(m, seq, spos, dev, return_attns=True), _run(twin, seq, spos, dev, return_attns=True)
    assert torch.equal(ra[0], rb[0]) and all(torch.equal(x, y) for x, y in zip(ra[3][0] + ra[3][1], rb[3][0] + rb[3][1]))
    with torch.no_grad():      # the module-by-module route agrees with the fused one as it does for a constant bias
        comp = m._forward_composite((seq.to(dev), spos.to(dev)), None, None, False, False)
        comp_twin = twin._forward_composite((seq.to(dev), spos.to(dev)), None, None, False, False)
    assert torch.equal(comp[0], comp_twin[0]) and max_abs_diff(comp[0], a[0]) <= 2e-4 and max_abs_diff(comp[0], ref_logits) <= 1e-4
    m.train()
    twin.train()
    ta, tb = _run(m, seq, spos, dev), _run(twin, seq, spos, dev)                      # dropout 0: training mode is deterministic
    assert torch.equal(ta[0], tb[0]) and max_abs_diff(ta[0], ref_logits) <= 1e-4


def test_int_preds_live_encoder_onehot_and_matmul_precision(dev):
    blocked = EC.build('A', 'prior', True, live=False)[2]
    bias = _model_bias('random', blocked)
    for kw in (dict(int_preds=True), dict(live=True)):
        live = kw.pop('live', False)
        m = EC.build('A', 'prior', True, live=live, label_bias=bias, learn_label_bias=True, **kw)[0].to(dev).eval()
        seq, spos = EC.build('A', 'prior', True, live=live)[3:5]
        twin = EC.build('A', 'prior', True, live=live, label_bias=bias, **kw)[0].to(dev).eval()
        a, b = _run(m, seq, spos, dev, **kw), _run(twin, seq, spos, dev, **kw)
        assert torch.equal(a[0], b[0])
        if kw:
            assert len(a[2]) == 3 and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    m.matmul_precision = twin.matmul_precision = 'high'
    assert torch.equal(_run(m, seq, spos, dev)[0], _run(twin, seq, spos, dev)[0])
    import onehot_common as OC
    from lamp_amd.Models import LAMP
    sd = OC.build_model(mask='none').state_dict()
    g = torch.Generator().manual_seed(41)
    ob = (2.0 * torch.randn(23, 23, generator=g)).masked_fill(torch.rand(23, 23, generator=g) < 0.2, NEG_INF)
    ob.fill_diagonal_(0.3)
    seq, pos = OC.make_dna(3, 32, lengths=[32, 21, 9])
    outs = []
    for learn in (False, True):
        mb = LAMP(9, 23, 64, 23, n_layers_enc=2, n_layers_dec=2, n_head=4, n_head2=4, d_word_vec=64, d_model=64, d_inner_hid=128,
                  d_k=16, d_v=16, encoder='graph', decoder='graph', dropout=0.0, dec_dropout=0.0, dec_dropout2=0.0, onehot=True,
                  label_mask='none', label_bias=ob, learn_label_bias=learn)
        mb.load_state_dict(sd)
        outs.append(_run(mb.to(dev).eval(), seq, pos, dev)[0])
        if learn:     # ... and the one-hot encoder's training route reaches the bias
            mb.train()
            mb((seq.to(dev), pos.to(dev)), None, None, None)[0].sum().backward()
            assert torch.isfinite(mb.decoder.label_bias.grad).all() and (mb.decoder.label_bias.grad[torch.isinf(ob)] == 0).all()
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------ 5. the refresh
@pytest.mark.parametrize('impl', ['lamp', 'torch'])
def test_an_optimizer_step_moves_allowed_entries_and_the_next_forward_sees_it(dev, impl):
    from lamp_amd import optim as O
    m, sd, blocked, seq, spos, h, bias, tgt, ref = _case('prior', 'random')
    m = m.to(dev)
    params = list(m.get_trainable_parameters())
    assert any(p is m.decoder.label_bias for p in params)
    opt = (O.Adam(params, betas=TC.ADAM_BETAS, lr=1e-2) if impl == 'lamp' else
           torch.optim.Adam(params, betas=TC.ADAM_BETAS, lr=1e-2))
    m.eval()
    before_logits = _run(m, seq, spos, dev)[0]
    buf_ptr = m.decoder.label_bias_f32.data_ptr()
    before = m.decoder.label_bias.detach().clone()
    m.train()
    opt.zero_grad()
    F.binary_cross_entropy_with_logits(m((seq.to(dev), spos.to(dev)), None, None, tgt.to(dev))[0], tgt.to(dev)).backward()
    opt.step()
    after = m.decoder.label_bias.detach()
    gone = torch.isinf(m.decoder.label_bias_f32[:, :L_A])
    minus_inf = torch.isinf(before)
    assert minus_inf.any() and torch.equal(after[minus_inf], before[minus_inf])       # -inf stays -inf
    assert torch.equal(after[gone], before[gone])                                     # entries under the mask do not move either
    assert (after[~gone] != before[~gone]).all() and torch.isfinite(after[~minus_inf]).all()
    m.eval()
    logits = _run(m, seq, spos, dev)[0]
    assert m.decoder.label_bias_f32.data_ptr() == buf_ptr and not torch.equal(logits, before_logits)
    twin = _constant_twin(m, 'prior').to(dev).eval()
    assert bit_equal(m.decoder.label_bias_f32, twin.decoder.label_bias_f32)
    assert torch.equal(logits, _run(twin, seq, spos, dev)[0])
    # the module-by-module route reads the same refreshed buffer
    with torch.no_grad():
        a = m._forward_composite((seq.to(dev), spos.to(dev)), None, None, False, False)[0]
        b = twin._forward_composite((seq.to(dev), spos.to(dev)), None, None, False, False)[0]
    assert torch.equal(a, b)
    # a second step, eval in between: training reads the refreshed buffer as well
    m.train()
    twin.train()
    assert torch.equal(_run(m, seq, spos, dev)[0], _run(twin, seq, spos, dev)[0])


def test_load_state_dict_refreshes_the_buffer(dev):
    m, sd, blocked, seq, spos, h, bias, tgt, ref = _case('prior', 'random')
    m = m.to(dev).eval()
    first = _run(m, seq, spos, dev)[0]
    g = torch.Generator().manual_seed(77)
    new_bias = (bias + 0.5 * torch.randn(L_A, L_A, generator=g))
    state = {k: v.clone() for k, v in m.state_dict().items()}
    state['decoder.label_bias'] = new_bias
    ptr = m.decoder.label_bias_f32.data_ptr()
    m.load_state_dict(state)
    logits = _run(m, seq, spos, dev)[0]
    twin = _constant_twin(m, 'prior', bias=new_bias).to(dev).eval()
    assert m.decoder.label_bias_f32.data_ptr() == ptr and not torch.equal(logits, first)
    assert torch.equal(logits, _run(twin, seq, spos, dev)[0])
    with torch.no_grad():      # an in-place edit bumps the parameter's version: the next forward folds again
        m.decoder.label_bias.add_(0.25)
    twin2 = _constant_twin(m, 'prior').to(dev).eval()
    assert torch.equal(_run(m, seq, spos, dev)[0], _run(twin2, seq, spos, dev)[0])


def test_data_parallel_on_one_device(dev):
    m, sd, blocked, seq, spos, h, bias, tgt, ref = _case('prior', 'random')
    m = m.to(dev).eval()
    want = _run(m, seq, spos, dev)[0]
    dp = torch.nn.DataParallel(m, device_ids=[dev.index])
    with torch.no_grad():
        got = dp((seq.to(dev), spos.to(dev)), None, None, None)[0]
    assert torch.equal(got, want)
    # (one device: the wrapper calls the module itself.)  A real replica folds its own copy of the parameter and never trusts
    # the broadcast buffer: same bits as a replica of the constant-bias twin (replicas skip the weights-only caches, so
    # their logits differ from the original's by a re-association)
    twin_rep = torch.nn.parallel.replicate(_constant_twin(m, 'prior').to(dev).eval(), [dev])[0]
    rep = torch.nn.parallel.replicate(m, [dev])[0]
    rep.decoder.label_bias_f32 = torch.full_like(m.decoder.label_bias_f32, 5.0)
    with torch.no_grad():
        got = rep((seq.to(dev), spos.to(dev)), None, None, None)[0]
        assert torch.equal(got, twin_rep((seq.to(dev), spos.to(dev)), None, None, None)[0])
    assert max_abs_diff(got, want) <= 1e-4
    assert rep.decoder.label_bias_f32.data_ptr() != m.decoder.label_bias_f32.data_ptr()
    # ... and in training the gradient comes back through the replica to the original's parameter
    m.train()
    rep = torch.nn.parallel.replicate(m, [dev])[0]
    logits = rep((seq.to(dev), spos.to(dev)), None, None, tgt.to(dev))[0]
    F.binary_cross_entropy_with_logits(logits, tgt.to(dev)).backward()
    r = ref[1]['decoder.label_bias']
    assert max_abs_diff(m.decoder.label_bias.grad, r) <= 3e-4 * r.abs().max().item() + 1e-9


# ------------------------------------------------------------------ 6. dropout
def test_dropout_gives_a_reproducible_finite_gradient(dev):
    blocked = EC.build('A', 'prior', True, live=False)[2]
    bias = _model_bias('random', blocked)
    m, sd, blocked, seq, spos, h = EC.build('A', 'prior', True, live=False, dropout=0.1, label_bias=bias, learn_label_bias=True)
    tgt = (torch.rand(seq.size(0), L_A, generator=torch.Generator().manual_seed(1)) < 0.2).float()
    m = m.to(dev).train()
    grads = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        torch.manual_seed(17)
        logits = m((seq.to(dev), spos.to(dev)), None, None, tgt.to(dev))[0]
        F.binary_cross_entropy_with_logits(logits, tgt.to(dev)).backward()
        grads.append(m.decoder.label_bias.grad.clone())
    gone = torch.isinf(m.decoder.label_bias_f32[:, :L_A])
    assert torch.equal(grads[0], grads[1]) and torch.isfinite(grads[0]).all()
    assert (grads[0][gone] == 0).all() and grads[0][~gone].abs().max() > 0


# ------------------------------------------------------------------ 7. end to end
def test_run_train_learns_the_bias_and_run_eval_takes_it_from_the_checkpoint(dev):
    from lamp_amd import data as D
    from lamp_amd import run_eval, run_train
    with tempfile.TemporaryDirectory(prefix='lamp_run_') as root:
        assert 'test' not in root
        data_path = os.path.join(root, 'train_valid_data.pt')
        data = TC.synthetic_dataset(n_train=64, n_valid=16, n_test=16)
        torch.save(data, data_path)
        args = ['-data', data_path, '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2', '-label_mask',
                'prior', '-batch_size', '16']
        train = args + ['-epoch', '1', '-lr', '0.003', '-dropout', '0.0', '-results_dir', os.path.join(root, 'res'), '-seed', '1',
                        '-label_bias', 'logp']
        hist = run_train.main(train + ['-name', 'learn', '-learn_label_bias'])
        assert len(hist) == 1 and hist[0]['train_loss'] == hist[0]['train_loss']
        assert '.lbias_logp_1.0.lbias_learn.learn' in hist[0]['checkpoint']
        ckpt = torch.load(hist[0]['checkpoint'], map_location='cpu', weights_only=False)
        assert ckpt['settings'].learn_label_bias is True and ckpt['settings'].label_bias == 'logp'
        learned = ckpt['model']['decoder.label_bias']
        initial = D.build_label_bias(data, 'logp', 1.0, dev)
        assert tuple(learned.shape) == tuple(initial.shape) and torch.isfinite(learned).all() and not torch.equal(learned, initial)
        out = run_eval.main(args + ['-checkpoint', hist[0]['checkpoint'], '-split', 'test'])
        assert out['bce_total'] / out['n_samples'] == hist[0]['test_loss']           # the epoch's own test loss, exactly
        bare = os.path.join(root, 'bare.chkpt')
        torch.save(ckpt['model'], bare)                                               # a bare state dict: the key says it all
        assert run_eval.main(args + ['-checkpoint', bare, '-split', 'test'])['bce_total'] == out['bce_total']
        # the same arguments without the flag: today's name, settings and checkpoint keys
        hist0 = run_train.main(train + ['-name', 'const'])
        ckpt0 = torch.load(hist0[0]['checkpoint'], map_location='cpu', weights_only=False)
        assert '.lbias_logp_1.0.const' in hist0[0]['checkpoint'] and 'lbias_learn' not in hist0[0]['checkpoint']
        assert not hasattr(ckpt0['settings'], 'learn_label_bias')
        assert set(ckpt['model']) - set(ckpt0['model']) == {'decoder.label_bias'} and set(ckpt0['model']) <= set(ckpt['model'])
        assert not any('label_bias' in k for k in ckpt0['model'])


def test_two_identical_epochs_end_in_bit_equal_weights(dev):
    from lamp_amd import optim as O
    from lamp_amd import train as T
    s = dict(EC.SHAPES['A'], V=4 + 2 * L_A)          # the synthetic dataset marks every label with two words
    data = TC.synthetic_dataset(n_train=32, n_labels=L_A, n_words=s['V'] - 4, max_len=s['T'] - 2, seed=5)
    blocked = EC.build(s, 'prior', True, live=False)[2]
    bias = _model_bias('random', blocked)

    def epoch():
        m = EC.build(s, 'prior', True, live=False, dropout=0.1, label_bias=bias, learn_label_bias=True)[0].to(dev)
        batches = T.TrainBatcher(data['train']['src'], data['train']['tgt'], 16, shuffle=False, drop_last=False)
        assert len(batches) == 2
        opt = O.Adam(list(m.get_trainable_parameters()), betas=TC.ADAM_BETAS, lr=1e-3)
        torch.manual_seed(3)
        preds, _, loss = T.train_epoch(m, batches, opt, TC.train_opt(L_A), device=dev)
        torch.cuda.synchronize()
        assert loss == loss, 'NaN loss'
        return {k: v.clone() for k, v in m.state_dict().items()}, preds

    (after1, preds1), (after2, preds2) = epoch(), epoch()
    assert torch.equal(preds1, preds2) and all(torch.equal(after1[k], after2[k]) for k in after1)
    moved = after1['decoder.label_bias'].cpu()
    assert torch.equal(torch.isinf(moved), torch.isinf(bias)) and not torch.equal(moved, bias)
