"""Sigmoid attention (attn_type='sigmoid', LAMP(dec_attn_type='sigmoid')) on the GPU: the fused kernel against the reference's
fixture and an fp64 restatement, 0-not-NaN, wide heads, bit-identity, the model against the oracle composition with
``sigmoid_common.sigmoid_sdpa`` substituted for ``oracle.lamp_ref.sdpa``, training gradients, status codes.

Kernel sweep, measured on an MI355X (B = 2, H = 2, every shape, head width, mask kind, layout and maps mode of
test_kernel_sweep): maps within 1e-6 of the fp64 restatement in every case; row-relative output error
|O - O64| / sum_k p_k |v_k|, maximum over the sweep: fp32 torch CPU evaluation of the restatement 3.1e-07, HIP kernel 2.6e-07
(largest HIP / max(CPU, floor / 4) ratio of any case: 1.05, against the 4 the test allows).  Wide heads (d = 192, general
route): CPU fp32 1.8e-07, HIP 1.8e-07.  test_kernel_sweep prints both figures for every case.
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
from oracle import lamp_ref as R
from sigmoid_common import MASKS, load_fixture, mha_state, sigmoid_sdpa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _N():
    from lamp_amd import _native as N
    return N


def raw_sdpa(dev, q, k, v, mask=None, act=1, maps=True, out=True, fused=False):
    """lamp_sdpa_act_fwd on q [B, H, lq, dk], k [B, H, lk, dk], v [B, H, lk, dv] (CPU tensors) -> (status, O [B, H, lq, dv] |
    None, P [H * B, lq, lk] | None).  fused: operands stored [B, l, H * d] (non-contiguous lamp_attn_layout strides).
    mask: None or a dict(kind, ptr tensor, stride_b, stride_q, tiles tensor | None, flags)."""
    N = _N()
    B, H, lq, dk = q.shape
    lk, dv = k.size(2), v.size(3)

    def place(t):
        return (t.permute(0, 2, 1, 3).contiguous() if fused else t.contiguous()).to(dev)
    qd, kd, vd = place(q), place(k), place(v)
    O = torch.full((B, lq, H, dv) if fused else (B, H, lq, dv), float('nan'), device=dev) if out else None
    P = torch.full((H * B, lq, lk), float('nan'), device=dev) if maps else None

    def strides(l, d):
        return (l * H * d, d, H * d) if fused else (H * l * d, l * d, d)
    lay = N.AttnLayout(*(strides(lq, dk) + strides(lk, dk) + strides(lk, dv) + strides(lq, dv)))
    ms, keep = None, []
    if mask is not None:
        mt = mask['ptr'].to(dev) if mask.get('ptr') is not None else None
        tl = mask['tiles'].to(dev) if mask.get('tiles') is not None else None
        keep += [mt, tl]
        ms = N.Mask(mask['kind'], mask.get('flags', 0), N.ptr(mt), mask.get('stride_b', 0), mask.get('stride_q', 0),
                    N.ptr(tl) if tl is not None else None, tl.size(1) if tl is not None else 0, 0)
    st = N.lib().lamp_sdpa_act_fwd(N.ptr(qd), N.ptr(kd), N.ptr(vd) if out else None, N.ptr(O), N.ptr(P), B, H, lq, lk, dk, dv,
                                   1.0 / float(dk) ** 0.5, act, C.byref(ms) if ms is not None else None, C.byref(lay),
                                   N.stream())
    torch.cuda.synchronize()
    if O is not None and fused:
        O = O.permute(0, 2, 1, 3)
    return st, (O.cpu() if O is not None else None), (P.cpu() if P is not None else None)


# ------------------------------------------------------------------ 1. the reference's fixture through the C ABI
@pytest.mark.parametrize('mask', MASKS)
def test_fixture_sdpa_through_the_c_abi(dev, mask):
    fx = load_fixture()
    from lamp_amd.SubLayers import ScaledDotProductAttention
    mod = ScaledDotProductAttention(temperature=4.0, attn_type='sigmoid').eval()
    m = fx.get('sdpa_mask_' + mask)
    out, attn = mod(fx['sdpa_q'].to(dev), fx['sdpa_k'].to(dev), fx['sdpa_v'].to(dev), attn_mask=m.to(dev) if m is not None else None)
    assert max_abs_diff(attn, fx['sdpa_attn_' + mask]) <= 1e-6
    assert max_abs_diff(out, fx['sdpa_out_' + mask]) <= 1e-5


@pytest.mark.parametrize('h', (1, 4))
@pytest.mark.parametrize('mask', MASKS)
def test_fixture_mha_through_the_c_abi(dev, h, mask):
    fx = load_fixture()
    from lamp_amd.SubLayers import MultiHeadAttention
    mod = MultiHeadAttention(h, 64, 64 // h, 64 // h, attn_type='sigmoid')
    mod.load_state_dict(mha_state(fx, h))
    mod = mod.to(dev).eval()
    pre = 'mha%d_' % h
    m = fx.get(pre + 'mask_' + mask)
    xq, xkv = fx[pre + 'xq'].to(dev), fx[pre + 'xkv'].to(dev)
    with torch.no_grad():
        out, attn = mod(xq, xkv, xkv, attn_mask=m.to(dev) if m is not None else None)
    assert max_abs_diff(attn, fx[pre + 'attn_' + mask]) <= 1e-6
    assert max_abs_diff(out, fx[pre + 'out_' + mask]) <= 1e-5


# ------------------------------------------------------------------ 2. kernel sweep against the fp64 restatement
SWEEP_SHAPES = [(16, 16, False), (24, 40, False), (90, 302, False), (128, 96, False), (129, 97, False), (257, 65, False),
                (300, 300, False), (300, 300, True)]
SWEEP_D = [(20, 20), (32, 32), (64, 64), (128, 128), (64, 32)]


def _masks(B, lq, lk, g, ragged):
    """name -> (blocked [B, lq, lk] bool, mask dict for raw_sdpa).  The bit-packed graph has an empty 32 x 32 tile when the
    shape has more than one tile."""
    N = _N()
    flags = N.LAMP_MASK_SELF_RAGGED if ragged else 0
    out = {'none': (None, dict(kind=N.LAMP_MASK_NONE, flags=flags) if ragged else None)}
    shared = torch.rand(lq, lk, generator=g) < 0.6
    shared[:, 0] = False
    if lq > 32 and lk > 32:
        shared[:32, 32:64] = True
    u8 = shared.to(torch.uint8)
    out['u8_shared'] = (shared.expand(B, lq, lk), dict(kind=N.LAMP_MASK_U8, ptr=u8, stride_b=0, stride_q=lk, flags=flags))
    per = torch.rand(B, lq, lk, generator=g) < 0.5
    per[:, :, 1] = False
    out['u8_per_sample'] = (per, dict(kind=N.LAMP_MASK_U8, ptr=per.to(torch.uint8), stride_b=lq * lk, stride_q=lk, flags=flags))
    tok = torch.randint(1, 9, (B, lk), generator=g)
    for b in range(B):
        tok[b, lk - 1 - (3 * b) % max(1, lk // 2):] = 0
    out['key_tokens'] = (tok.eq(0).unsqueeze(1).expand(B, lq, lk), dict(kind=N.LAMP_MASK_KEY_TOKENS_I64, ptr=tok, stride_b=lk,
                                                                        flags=flags))
    bits, words = N.pack_mask_bits(u8), (lk + 31) // 32
    out['bits'] = (shared.expand(B, lq, lk), dict(kind=N.LAMP_MASK_BITS_U32, ptr=bits, stride_b=0, stride_q=words, flags=flags))
    out['bits_tiles'] = (shared.expand(B, lq, lk), dict(kind=N.LAMP_MASK_BITS_U32, ptr=bits, stride_b=0, stride_q=words,
                                                        tiles=N.active_tile_list(u8), flags=flags))
    return out


def _row_rel(o, o64, p64, v64):
    """max over rows and columns of |O - O64| / sum_k p_k |v_k| (a fully blocked row: 0 / 0 -> its |O - O64| must be 0)."""
    scale = torch.bmm(p64, v64.abs())
    err = (o.double() - o64).abs()
    assert (err[scale == 0] == 0).all()
    return (err / scale.clamp_min(1e-30)).max().item()


@pytest.mark.parametrize('dk,dv', SWEEP_D)
@pytest.mark.parametrize('lq,lk,ragged', SWEEP_SHAPES)
def test_kernel_sweep(dev, lq, lk, ragged, dk, dv):
    B, H = 2, 2
    g = torch.Generator().manual_seed(lq * 1000 + lk + dk)
    q, k = torch.randn(B, H, lq, dk, generator=g), torch.randn(B, H, lk, dk, generator=g)
    v = torch.randn(B, H, lk, dv, generator=g)
    flat = lambda t: t.permute(1, 0, 2, 3).reshape(H * B, t.size(2), t.size(3))   # noqa: E731  (index h * B + b)
    for name, (blocked, md) in _masks(B, lq, lk, g, ragged).items():
        bl = blocked.unsqueeze(0).expand(H, B, lq, lk).reshape(H * B, lq, lk) if blocked is not None else None
        o64, p64 = sigmoid_sdpa(flat(q).double(), flat(k).double(), flat(v).double(), bl)
        o32, p32 = sigmoid_sdpa(flat(q), flat(k), flat(v), bl)
        cpu_rel = _row_rel(o32, o64, p64, flat(v).double())
        bound = max(4.0 * cpu_rel, 1e-6)
        fused_layouts = (False, True) if name in ('none', 'bits') else (False,)
        for fused in fused_layouts:
            for maps, out in ((True, True), (False, True), (True, False)):
                st, O, P = raw_sdpa(dev, q, k, v, md, maps=maps, out=out, fused=fused)
                assert st == 0, (name, st)
                if P is not None:
                    perr = (P.double() - p64).abs().max().item()
                    assert perr <= 1e-6, (name, maps, out, perr)
                    if bl is not None:
                        assert (P[bl] == 0).all()
                if O is not None:
                    rel = _row_rel(flat(O), o64, p64, flat(v).double())
                    print('%dx%d d%d/%d %s fused=%d maps=%d: cpu fp32 %.2e hip %.2e' % (lq, lk, dk, dv, name, fused, maps, cpu_rel, rel))
                    assert rel <= bound, (name, maps, fused, rel, bound)


# ------------------------------------------------------------------ 3. zero, not NaN
def test_fully_blocked_row_is_zero_where_softmax_is_nan(dev):
    N = _N()
    B, H, lq, lk, d = 2, 2, 24, 40, 32
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(B, H, l, d, generator=g) for l in (lq, lk, lk))
    blocked = torch.rand(B, lq, lk, generator=g) < 0.4
    blocked[1, 7, :] = True
    md = dict(kind=N.LAMP_MASK_U8, ptr=blocked.to(torch.uint8), stride_b=lq * lk, stride_q=lk)
    st, O, P = raw_sdpa(dev, q, k, v, md, act=N.LAMP_ATTN_SIGMOID)
    assert st == 0
    assert (O[1, :, 7] == 0).all() and (P.view(H, B, lq, lk)[:, 1, 7] == 0).all()
    flat = lambda t: t.permute(1, 0, 2, 3).reshape(H * B, t.size(2), t.size(3))   # noqa: E731
    o64, p64 = sigmoid_sdpa(flat(q).double(), flat(k).double(), flat(v).double(), blocked.repeat(H, 1, 1))
    assert torch.isfinite(O).all() and (P.double() - p64).abs().max().item() <= 1e-6
    assert (flat(O).double() - o64).abs().max().item() <= 1e-4
    st, O, P = raw_sdpa(dev, q, k, v, md, act=N.LAMP_ATTN_SOFTMAX)     # the softmax route: NaN there, finite elsewhere
    assert st == 0 and torch.isnan(O[1, :, 7]).all() and torch.isnan(P.view(H, B, lq, lk)[:, 1, 7]).all()
    keep = torch.ones(B, H, lq, dtype=torch.bool)
    keep[1, :, 7] = False
    assert torch.isfinite(O[keep]).all()


# ------------------------------------------------------------------ 4. wide heads: the general route
def test_wide_heads_go_through_the_general_route(dev):
    N = _N()
    B, H, lq, lk, d = 2, 2, 24, 40, 192
    g = torch.Generator().manual_seed(6)
    q, k, v = (torch.randn(B, H, l, d, generator=g) for l in (lq, lk, lk))
    blocked = torch.rand(B, lq, lk, generator=g) < 0.4
    blocked[0, 3, :] = True
    md = dict(kind=N.LAMP_MASK_U8, ptr=blocked.to(torch.uint8), stride_b=lq * lk, stride_q=lk)
    flat = lambda t: t.permute(1, 0, 2, 3).reshape(H * B, t.size(2), t.size(3))   # noqa: E731
    bl = blocked.repeat(H, 1, 1)
    o64, p64 = sigmoid_sdpa(flat(q).double(), flat(k).double(), flat(v).double(), bl)
    o32, _ = sigmoid_sdpa(flat(q), flat(k), flat(v), bl)
    st, O, P = raw_sdpa(dev, q, k, v, md)
    assert st == 0
    assert (P.double() - p64).abs().max().item() <= 1e-6 and (P[bl] == 0).all() and (O[0, :, 3] == 0).all()
    rel = lambda o: _row_rel(o, o64, p64, flat(v).double())  # noqa: E731
    print('wide heads: cpu fp32 %.2e hip %.2e' % (rel(o32), rel(flat(O))))
    assert rel(flat(O)) <= max(4.0 * rel(o32), 1e-6)
    st, _, _ = raw_sdpa(dev, q, k, v, md, maps=False)    # the general route keeps its scores in the map buffer
    assert st == -3


# ------------------------------------------------------------------ 5 / 6. the model
def _run(m, seq, pos, dev, **kw):
    with torch.no_grad():
        return m((seq.to(dev), pos.to(dev)), None, None, None, **kw)


_REF = {}


def _ref(shape, mask, live, monkeypatch, no_dec_self_att=False):
    key = (shape, mask, live, no_dec_self_att)
    if key not in _REF:
        _, sd, blocked, seq, spos, h = EC.build(shape, mask, True, live=live)
        if no_dec_self_att:
            sd = {k: v for k, v in sd.items() if '.slf_attn.' not in k or k.startswith('encoder.')}
        with torch.no_grad():
            enc = EC.live_encoder_ref(sd, seq, spos, h)[0] if live else R.encoder_forward(sd, seq, spos, h)[0]   # softmax
            with monkeypatch.context() as mp:
                mp.setattr(R, 'sdpa', sigmoid_sdpa)
                y, slf, encdec, int_outs = R.decoder_forward(sd, seq, enc, blocked, h)
            w = sd['tgt_word_proj.linear.weight']
            _REF[key] = (R.readout(y, w), enc, slf, encdec, [R.readout(o, w) for o in int_outs[:-1]])
    return _REF[key]


@pytest.mark.parametrize('live', [False, True])
@pytest.mark.parametrize('mask', ['prior', 'none', 'inveye'])
@pytest.mark.parametrize('shape', ['A', 'B', 'C'])
def test_model_against_the_oracle_composition(dev, monkeypatch, shape, mask, live):
    ref_logits, ref_enc, ref_slf, ref_encdec, ref_int = _ref(shape, mask, live, monkeypatch)
    m, sd, blocked, seq, spos, h = EC.build(shape, mask, True, live=live, dec_attn_type='sigmoid')
    m = m.to(dev).eval()
    logits, enc, extra = _run(m, seq, spos, dev)
    print('%s %s live=%s: logits %.3e enc %.3e' % (shape, mask, live, max_abs_diff(logits, ref_logits), max_abs_diff(enc, ref_enc)))
    assert extra is None and max_abs_diff(logits, ref_logits) <= 1e-4 and max_abs_diff(enc, ref_enc) <= 5e-5
    l2, e2, _, (slf, encdec) = _run(m, seq, spos, dev, return_attns=True)
    assert max_abs_diff(l2, ref_logits) <= 1e-4
    for got, want in zip(slf + encdec, ref_slf + ref_encdec):
        assert max_abs_diff(got, want) <= 1e-5
    src = (seq.to(dev), spos.to(dev))
    with torch.no_grad():
        comp = m._forward_composite(src, None, None, True, False)
    assert max_abs_diff(comp[0], ref_logits) <= 1e-4
    for got, want in zip(comp[3][0] + comp[3][1], ref_slf + ref_encdec):
        assert max_abs_diff(got, want) <= 1e-5
    # softmax model of the same weights: another function
    soft = EC.build(shape, mask, True, live=live)[0].to(dev).eval()
    assert max_abs_diff(_run(soft, seq, spos, dev)[0], ref_logits) > 1e-3


@pytest.mark.parametrize('shape', ['A', 'C'])
def test_model_int_preds_and_no_dec_self_att(dev, monkeypatch, shape):
    ref = _ref(shape, 'prior', False, monkeypatch)
    m, sd, blocked, seq, spos, h = EC.build(shape, 'prior', True, live=False, int_preds=True, dec_attn_type='sigmoid')
    m = m.to(dev).eval()
    logits, enc, ipreds = _run(m, seq, spos, dev, int_preds=True)
    assert max_abs_diff(logits, ref[0]) <= 1e-4 and len(ipreds) == len(ref[4]) == 3
    for got, want in zip(ipreds, ref[4]):
        assert max_abs_diff(got, want) <= 1e-4
    ref = _ref(shape, 'none', False, monkeypatch, no_dec_self_att=True)
    s = EC.SHAPES[shape]
    from lamp_amd.Models import LAMP
    m2 = LAMP(s['V'], s['L'], s['T'] + EC.PAD_EXTRA, s['L'], n_layers_enc=2, n_layers_dec=2, n_head=s['h'], n_head2=s['h'],
              d_word_vec=s['d'], d_model=s['d'], d_inner_hid=s['dff'], d_k=s['d'] // s['h'], d_v=s['d'] // s['h'], encoder='graph',
              decoder='graph', dropout=0.0, dec_dropout=0.0, label_mask='none', no_dec_self_att=True, dec_dropout2=False,
              dec_attn_type='sigmoid')
    sd2 = {k: v for k, v in EC.build(shape, 'none', True, live=False)[1].items() if '.slf_attn.' not in k or k.startswith('encoder.')}
    m2.load_state_dict(sd2)
    logits = _run(m2.to(dev).eval(), seq, spos, dev)[0]
    assert max_abs_diff(logits, ref[0]) <= 1e-4


def test_option_off_is_bit_equal_to_a_model_without_the_keyword(dev):
    a = EC.build('A', 'prior', True, live=False)[0].to(dev).eval()
    b, _, _, seq, spos, _ = EC.build('A', 'prior', True, live=False, dec_attn_type=None, attn_type='sigmoid')
    b = b.to(dev).eval()
    assert torch.equal(_run(a, seq, spos, dev)[0], _run(b, seq, spos, dev)[0])


def test_onehot_model(dev, monkeypatch):
    import onehot_common as OC
    m = OC.build_model(mask='none')
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    from lamp_amd.Models import LAMP
    torch.manual_seed(0)
    ms = LAMP(9, 23, 64, 23, n_layers_enc=2, n_layers_dec=2, n_head=4, n_head2=4, d_word_vec=64, d_model=64, d_inner_hid=128,
              d_k=16, d_v=16, encoder='graph', decoder='graph', dropout=0.0, dec_dropout=0.0, dec_dropout2=0.0, onehot=True,
              label_mask='none', dec_attn_type='sigmoid')
    ms.load_state_dict(sd)
    seq, pos = OC.make_dna(3, 32, lengths=[32, 21, 9])
    with torch.no_grad():
        enc, seq2 = OC.onehot_encoder_ref(sd, seq, pos)
        with monkeypatch.context() as mp:
            mp.setattr(R, 'sdpa', sigmoid_sdpa)
            y = R.decoder_forward(sd, seq2, enc, None, 4)[0]
        ref = R.readout(y, sd['tgt_word_proj.linear.weight'])
    logits = _run(ms.to(dev).eval(), seq, pos, dev)[0]
    assert max_abs_diff(logits, ref) <= 1e-4


def test_a_samples_bits_do_not_depend_on_its_batch(dev):
    m, sd, blocked, seq, spos, h = EC.build('B', 'prior', True, live=False, dec_attn_type='sigmoid')
    m = m.to(dev).eval()
    n = seq.size(0)
    logits, enc, _, (slf, encdec) = _run(m, seq, spos, dev, return_attns=True)
    assert torch.equal(_run(m, seq, spos, dev)[0], logits)
    for bs in (1, 2):
        for b0 in range(0, n, bs):
            part = _run(m, seq[b0:b0 + bs], spos[b0:b0 + bs], dev)[0]
            assert torch.equal(part, logits[b0:b0 + bs]), (bs, b0)
    perm = list(reversed(range(n)))
    assert torch.equal(_run(m, seq[perm], spos[perm], dev)[0][perm], logits)
    T = seq.size(1)
    r_seq, r_pos = F.pad(seq, (0, EC.PAD_EXTRA)), F.pad(spos, (0, EC.PAD_EXTRA))
    assert torch.equal(_run(m, r_seq, r_pos, dev)[0], logits)
    # a forced micro-batch split: workspace for one sample
    N = _N()
    built = m._native_model()
    opts = N.FwdOptions(0, N.LAMP_FWD_DEC_SIGMOID, None, None)
    per = N.lib().lamp_forward_opts_workspace_bytes(C.byref(built[0]), C.byref(opts), 1, T, 1)
    m.workspace_limit_bytes = per + 4096
    try:
        s_logits, s_enc, _, (s_slf, s_encdec) = _run(m, seq, spos, dev, return_attns=True)
    finally:
        del m.workspace_limit_bytes
    assert torch.equal(s_logits, logits) and torch.equal(s_enc, enc)
    for got, want in zip(s_slf + s_encdec, slf + encdec):
        assert torch.equal(got, want)


# ------------------------------------------------------------------ 7. training
@pytest.mark.parametrize('wide', [False, True])
def test_every_parameter_gradient_matches_oracle_autograd(dev, monkeypatch, wide):
    shape = dict(V=50, L=24, d=192, h=1, dff=256, T=40, lengths=[40, 17, 1]) if wide else 'A'   # wide: d_k = d_v = 192
    m, sd, blocked, seq, spos, h = EC.build(shape, 'prior', True, live=False, dec_attn_type='sigmoid')
    m = m.to(dev)
    L = 24
    tgt = (torch.rand(seq.size(0), L, generator=torch.Generator().manual_seed(1)) < 0.2).float()
    sd64 = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    enc64 = R.encoder_forward(sd64, seq, spos, h)[0]
    with monkeypatch.context() as mp:
        mp.setattr(R, 'sdpa', sigmoid_sdpa)
        y = R.decoder_forward(sd64, seq, enc64, blocked, h)[0]
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


@pytest.mark.parametrize('d', [32, 192])
def test_attention_dropout_matches_the_torch_restatement_with_the_librarys_mask(dev, d):
    """MultiHeadAttention(attn_type='sigmoid') in train mode, probability dropout 0.2 (the composite route at d_k = 32, the
    per-launch route at d_k = 192): output, dropped map and every gradient against fp64 torch with the library's own keep mask."""
    N = _N()
    from lamp_amd import training
    from lamp_amd.SubLayers import MultiHeadAttention
    H, B, lq, lk, dm, p = 2, 2, 24, 40, 64, 0.2
    torch.manual_seed(3)
    mod = MultiHeadAttention(H, dm, d, d, dropout=0.0, dropout2=p, attn_type='sigmoid').to(dev).train()
    g = torch.Generator().manual_seed(4)
    xq, xkv = torch.randn(B, lq, dm, generator=g), torch.randn(B, lk, dm, generator=g)
    blocked = torch.rand(B, lq, lk, generator=g) < 0.3
    blocked[1, 5, :] = True
    torch.manual_seed(11)
    seeds = training._Seeds()
    seed_attn = seeds.next()
    torch.manual_seed(11)
    xq_d, xkv_d = xq.to(dev).requires_grad_(True), xkv.to(dev)
    out, attn = mod(xq_d, xkv_d, xkv_d, attn_mask=blocked.to(dev))
    w = torch.randn(B, lq, dm, generator=g)
    (out * w.to(dev)).sum().backward()
    keep = N.dropout_keep_mask(H * B * lq * lk, p, seed_attn).view(H * B, lq, lk).double()
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mod.state_dict().items()}
    x64 = xq.double().requires_grad_(True)
    q = F.linear(x64, sd['w_qs.weight']).view(B, lq, H, d).permute(2, 0, 1, 3).reshape(H * B, lq, d)
    k = F.linear(xkv.double(), sd['w_ks.weight']).view(B, lk, H, d).permute(2, 0, 1, 3).reshape(H * B, lk, d)
    v = F.linear(xkv.double(), sd['w_vs.weight']).view(B, lk, H, d).permute(2, 0, 1, 3).reshape(H * B, lk, d)
    P = sigmoid_sdpa(q, k, v, blocked.repeat(H, 1, 1))[1]
    Pd = P * keep / (1 - p)
    a = torch.bmm(Pd, v).view(H, B, lq, d).permute(1, 2, 0, 3).reshape(B, lq, H * d)
    ref = R.layer_norm(F.linear(a, sd['fc.weight']) + x64, sd['layer_norm.weight'], sd['layer_norm.bias'])
    (ref * w.double()).sum().backward()
    assert max_abs_diff(attn, Pd.detach()) <= 2e-6 and torch.isfinite(out).all()
    assert max_abs_diff(out, ref.detach()) <= 1e-4
    for name, prm in mod.named_parameters():
        r = sd[name].grad
        assert max_abs_diff(prm.grad, r) <= 3e-4 * r.abs().max().item() + 1e-9, name
    assert max_abs_diff(xq_d.grad, x64.grad) <= 3e-4 * x64.grad.abs().max().item() + 1e-9


def test_run_train_with_sigmoid_attention_and_run_eval_reads_the_setting():
    from lamp_amd import run_eval, run_train
    with tempfile.TemporaryDirectory(prefix='lamp_run_') as root:
        assert 'test' not in root
        data_path = os.path.join(root, 'train_valid_data.pt')
        torch.save(TC.synthetic_dataset(n_train=64, n_valid=16, n_test=16), data_path)
        args = ['-data', data_path, '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2', '-label_mask',
                'prior', '-batch_size', '16']
        hist = run_train.main(args + ['-epoch', '2', '-lr', '0.003', '-dropout', '0.0', '-results_dir', os.path.join(root, 'res'),
                                      '-name', 'sg', '-seed', '1', '-attn_type', 'sigmoid'])
        assert len(hist) == 2 and hist[1]['train_loss'] == hist[1]['train_loss'] and hist[1]['train_loss'] < hist[0]['train_loss']
        assert '.attn_sigmoid' in hist[1]['checkpoint']
        ckpt = torch.load(hist[1]['checkpoint'], map_location='cpu', weights_only=False)
        assert ckpt['settings'].attn_type == 'sigmoid'
        out = run_eval.main(args + ['-checkpoint', hist[1]['checkpoint'], '-split', 'test'])
        assert out['bce_total'] / out['n_samples'] == hist[1]['test_loss']    # read as a sigmoid model: the epoch's own test loss


# ------------------------------------------------------------------ 8. status codes
def test_status_codes(dev):
    N = _N()
    g = torch.Generator().manual_seed(8)
    q, k, v = (torch.randn(1, 1, 16, 32, generator=g) for _ in range(3))
    assert raw_sdpa(dev, q, k, v, act=2)[0] == -4 and raw_sdpa(dev, q, k, v, act=-1)[0] == -4
    q, k, v = (torch.randn(1, 1, 16, 30, generator=g) for _ in range(3))
    assert raw_sdpa(dev, q, k, v)[0] == -4
    x = torch.randn(1, 4, 32, device=dev)
    from lamp_amd.SubLayers import MultiHeadAttention
    w = N.mha_weights(MultiHeadAttention(2, 32, 16, 16).to(dev))
    ws = N.workspace(N.lib().lamp_mha_workspace_bytes(1, 4, 4, 32, 2, 16, 16), dev)
    out = torch.empty_like(x)
    st = N.lib().lamp_mha_act_fwd(N.ptr(x), N.ptr(x), 1, 4, 4, 32, 16, 16, C.byref(w), 7, None, N.ptr(out), None, N.ptr(ws),
                                  ws.numel(), N.stream())
    assert st == -4
    P = torch.rand(8, 16, device=dev)
    assert N.lib().lamp_sigmoid_attn_bwd(N.ptr(P), N.ptr(P), 8, 16, 1.0, 1.5, 0, N.ptr(P), N.stream()) == -4
    dS = N.sigmoid_attn_bwd(P, torch.ones_like(P), 0.5)
    assert max_abs_diff(dS, 0.5 * P.cpu() * (1 - P.cpu())) <= 1e-7
    torch.cuda.synchronize()
