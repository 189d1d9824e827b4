"""Shared pieces of the head-geometry tests: models whose ``n_head``, ``n_head2``, ``d_k`` and ``d_v`` are chosen independently
of each other and of ``d_model`` (every other test builds on ``d_k = d_v = d_model / n_head`` and ``n_head2 = n_head``).

``make_state_dict`` follows the initialisation rule of lamp_amd/synthetic.py (std sqrt(2 / (d_model + d_k)) for q and k, the same
with d_v for v, ``fc`` only where the block has more than one head) on a random stream of its own: synthetic.py keeps the stream
bench.py draws from.  ``oracle_forward`` and its variants are the existing oracle compositions with ``n_head2`` passed through.

``python tests/head_geometry_common.py`` re-runs, without a GPU, the seed choice of the gradient cases: the first seed for which
the fp32 CPU oracle's own autograd stays inside the gradient bar against the fp64 oracle (the ReLU-kink caveat of
tests/fuzz_parity.py: a pre-activation within fp32 rounding of zero cannot fake a mismatch)."""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:     # run as a script (under pytest, conftest.py has done this)
    sys.path.insert(0, ROOT)

import enc_live_common as EC  # noqa: E402
from label_bias_common import sdpa_with_label_bias  # noqa: E402
from lamp_amd import Constants  # noqa: E402
from lamp_amd.utils import position_encoding_init  # noqa: E402
from oracle import lamp_ref as R  # noqa: E402
from sigmoid_common import sigmoid_sdpa  # noqa: E402

GRAD_RTOL, GRAD_ATOL = 3e-4, 1e-9     # tests/test_gpu_training.py::test_gradients_with_wide_heads

SMALL = dict(V=50, L=24, T=40, lengths=[40, 17, 1], n_enc=2, n_dec=2)
CHAIN = dict(V=60, L=90, T=24, n_enc=1, n_dec=2)     # G5: B x 90 decoder rows; `lengths` per test
# name: widths and head counts (every width a multiple of 4: the kernels refuse others) and what the geometry reaches
GEOMS = {
    # hdk = 72, hdv = 120 (enc-attention) / 48, 80 (self-attention), none equal to d; K and V are two launches; the blocks differ
    # in head count, so the K/V-ahead projection runs per layer and the workspace is carved for the larger count
    'G1': dict(d=64, dff=96, h=3, h2=2, dk=24, dv=40, mask='prior', **SMALL),
    'G2': dict(d=64, dff=96, h=1, h2=2, dk=48, dv=64, mask='none', **SMALL),      # enc-attention without fc (d_v = d_model)
    'G3': dict(d=64, dff=96, h=2, h2=1, dk=16, dv=64, mask='inveye', **SMALL),    # the mirror: self-attention without fc
    'G4a': dict(d=64, dff=96, h=2, h2=2, dk=160, dv=32, mask='prior', **SMALL),   # the general route because of d_k alone
    'G4b': dict(d=64, dff=96, h=2, h2=2, dk=32, dv=160, mask='inveye', **SMALL),  # ... because of d_v alone
    'G5a': dict(d=512, dff=512, h=4, h2=8, dk=32, dv=64, mask='prior', **CHAIN),  # chain k_h = 256 (enc-attention), 512 (self)
    'G5b': dict(d=512, dff=512, h=8, h2=4, dk=64, dv=128, mask='prior', **CHAIN),  # k_h = 1024 and 512
    'G5b_ff1024': dict(d=512, dff=1024, h=8, h2=4, dk=64, dv=128, mask='prior', **CHAIN),
    'G5c': dict(d=512, dff=512, h=6, h2=6, dk=128, dv=128, mask='none', **CHAIN),  # k_h = 768
    # the 32-query kernel and the LDS-tile kernel (max(d_k, d_v) > 64, lq > 256, lk >= 256) on layouts with q_r != v_r
    'G6': dict(d=128, dff=128, h=2, h2=2, dk=32, dv=128, mask='none', V=50, L=260, T=70, lengths=[70, 33, 1], n_enc=2, n_dec=2),
}
CHAIN_LENGTHS = [24, 3, 17, 9, 24, 11]     # repeated to the batch size of a G5 case

# gradient cases: name -> (geometry, kind); seeds: the first for which fp32_oracle_is_inside() holds (see __main__)
GRAD_CASES = {
    'G1': ('G1', 'softmax'), 'G2': ('G2', 'softmax'), 'G3': ('G3', 'softmax'), 'G4a': ('G4a', 'softmax'),
    'G4b': ('G4b', 'softmax'), 'G6': ('G6', 'softmax'), 'G1_live': ('G1', 'live'), 'G1_sigmoid': ('G1', 'sigmoid'),
}
GRAD_SEEDS = {'G1': 0, 'G2': 0, 'G3': 0, 'G4a': 0, 'G4b': 0, 'G6': 0, 'G1_live': 0, 'G1_sigmoid': 0}


def geometry(name, **over):
    g = dict(GEOMS[name]) if isinstance(name, str) else dict(name)
    g.update(over)
    return g


def make_state_dict(n_src_vocab, n_labels, n_max_seq, d_model, d_inner, n_head, n_head2, d_k, d_v, n_layers_enc, n_layers_dec,
                    pos_emb=True, seed=0, no_dec_self_att=False):
    """The key layout of the reference's graph model with every attention block (n_head * d_k, d_model) for q and k,
    (n_head * d_v, d_model) for v; the encoder's and the enc-attention blocks have n_head heads, the label self-attention n_head2."""
    g = torch.Generator().manual_seed(7919 + seed)

    def normal(shape, std):
        return torch.randn(shape, generator=g) * std

    def uniform(shape, bound):
        return (torch.rand(shape, generator=g) * 2 - 1) * bound

    sd = {}
    emb = normal((n_src_vocab, d_model), 1.0)
    emb[Constants.PAD] = 0
    sd['encoder.src_word_emb.weight'] = emb
    if pos_emb:
        sd['encoder.position_enc.weight'] = position_encoding_init(n_max_seq + 1, d_model)

    def add_mha(p, h):
        sd[p + 'w_qs.weight'] = normal((h * d_k, d_model), math.sqrt(2.0 / (d_model + d_k)))
        sd[p + 'w_ks.weight'] = normal((h * d_k, d_model), math.sqrt(2.0 / (d_model + d_k)))
        sd[p + 'w_vs.weight'] = normal((h * d_v, d_model), math.sqrt(2.0 / (d_model + d_v)))
        sd[p + 'layer_norm.weight'] = torch.ones(d_model) + normal((d_model,), 0.05)
        sd[p + 'layer_norm.bias'] = normal((d_model,), 0.05)
        if h > 1:
            sd[p + 'fc.weight'] = normal((d_model, h * d_v), math.sqrt(2.0 / (d_model + h * d_v)))

    def add_ffn(p):
        sd[p + 'w_1.weight'] = uniform((d_inner, d_model, 1), 1.0 / math.sqrt(d_model))
        sd[p + 'w_1.bias'] = uniform((d_inner,), 1.0 / math.sqrt(d_model))
        sd[p + 'w_2.weight'] = uniform((d_model, d_inner, 1), 1.0 / math.sqrt(d_inner))
        sd[p + 'w_2.bias'] = uniform((d_model,), 1.0 / math.sqrt(d_inner))
        sd[p + 'layer_norm.weight'] = torch.ones(d_model) + normal((d_model,), 0.05)
        sd[p + 'layer_norm.bias'] = normal((d_model,), 0.05)

    for i in range(n_layers_enc):
        add_mha('encoder.layer_stack.%d.slf_attn.' % i, n_head)
        add_ffn('encoder.layer_stack.%d.pos_ffn.' % i)
    sd['decoder.tgt_word_emb.weight'] = normal((n_labels, d_model), 1.0)
    for i in range(n_layers_dec):
        add_mha('decoder.layer_stack.%d.enc_attn.' % i, n_head)
        add_ffn('decoder.layer_stack.%d.pos_ffn1.' % i)
        if not no_dec_self_att:
            add_mha('decoder.layer_stack.%d.slf_attn.' % i, n_head2)
        add_ffn('decoder.layer_stack.%d.pos_ffn2.' % i)
    sd['tgt_word_proj.weight'] = sd['decoder.tgt_word_emb.weight']
    sd['tgt_word_proj.linear.weight'] = normal((n_labels, d_model), math.sqrt(2.0 / (d_model + n_labels)))
    return sd


def build_model(g, sd, adj=None, n_max_seq=None, **kw):
    """LAMP on the CPU at geometry ``g`` (a dict of GEOMS' fields), loaded with ``sd``.  ``kw``: further LAMP keywords."""
    from lamp_amd.Models import LAMP
    L = g['L']
    args = dict(n_layers_enc=g['n_enc'], n_layers_dec=g['n_dec'], n_head=g['h'], n_head2=g['h2'], d_word_vec=g['d'],
                d_model=g['d'], d_inner_hid=g['dff'], d_k=g['dk'], d_v=g['dv'], encoder='graph', decoder='graph', dropout=0.0,
                dec_dropout=0.0, no_enc_pos_embedding=not g.get('pos', True), no_dec_self_att=g.get('no_dec_self_att', False),
                label_adj_matrix=adj.clone() if adj is not None else None, label_mask=g['mask'], dec_dropout2=False)
    args.update(kw)
    m = LAMP(g['V'], L, g['T'] if n_max_seq is None else n_max_seq, L, **args)
    m.load_state_dict(sd)
    return m


def build(name, seed=0, lengths=None, n_max_seq=None, **kw):
    """-> (LAMP on the CPU, state_dict, label block mask, src_seq, src_pos, geometry dict).  ``kw``: geometry overrides
    (``mask``, ``pos``, ``no_dec_self_att``, ``dff`` ...) and, for anything else, LAMP keywords."""
    over = {k: kw.pop(k) for k in list(kw) if k in ('mask', 'pos', 'no_dec_self_att', 'dff', 'L', 'T', 'n_enc', 'n_dec', 'V')}
    g = geometry(name, **over)
    if lengths is not None:
        g['lengths'] = list(lengths)
    n_max = g['T'] if n_max_seq is None else n_max_seq
    sd = make_state_dict(g['V'], g['L'], n_max, g['d'], g['dff'], g['h'], g['h2'], g['dk'], g['dv'], g['n_enc'], g['n_dec'],
                         pos_emb=g.get('pos', True), seed=seed, no_dec_self_att=g.get('no_dec_self_att', False))
    adj = R.make_adjacency(g['L'], 0.2, seed) if g['mask'] == 'prior' else None
    seq, spos = R.make_batch(len(g['lengths']), g['V'], g['T'], lengths=g['lengths'], seed=seed)
    if seq.size(1) < g['T']:
        seq, spos = F.pad(seq, (0, g['T'] - seq.size(1))), F.pad(spos, (0, g['T'] - spos.size(1)))
    m = build_model(g, sd, adj, n_max_seq=n_max, **kw)
    return m, sd, R.label_block_mask(adj, g['mask'], g['L']), seq, spos, g


def chain_lengths(B):
    return [CHAIN_LENGTHS[i % len(CHAIN_LENGTHS)] for i in range(B)]


def load_golden_geometry(name):
    """tests/golden/geometry.npz (the reference's own modules at G1 / G2, tests/golden/make_golden_geometry.py)
    -> (dict of tensors / scalars, state_dict, geometry dict, label block mask)."""
    import numpy as np
    data, sd = {}, {}
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'geometry.npz'), allow_pickle=False) as z:
        for key in z.files:
            if not key.startswith(name + '__'):
                continue
            k, a = key[len(name) + 2:], z[key]
            if k.startswith('sd__'):
                sd[k[4:]] = torch.from_numpy(a).float()     # weights on the fp16 grid are stored as float16, exactly
            elif a.dtype.kind in 'US':
                data[k] = str(a)
            elif a.ndim == 0:
                data[k] = a.item()
            else:
                data[k] = torch.from_numpy(a)
    L, T = sd['decoder.tgt_word_emb.weight'].size(0), sd['encoder.position_enc.weight'].size(0) - 1
    g = dict(d=data['d'], dff=data['dff'], h=data['h'], h2=data['h2'], dk=data['dk'], dv=data['dv'], mask=data['label_mask'],
             V=sd['encoder.src_word_emb.weight'].size(0), L=L, T=T, n_enc=R.count_layers(sd, 'encoder'),
             n_dec=R.count_layers(sd, 'decoder'))
    return data, sd, g, R.label_block_mask(data.get('label_adj_matrix'), data['label_mask'], L)


# ------------------------------------------------------------------ oracle compositions, n_head2 passed through
def oracle_forward(sd, seq, spos, g, blocked, dtype=torch.float64, **kw):
    """oracle.lamp_ref.forward at the geometry's head counts; ``dtype`` converts the weights first."""
    sdx = sd if dtype is None else R.to_dtype(sd, dtype)
    with torch.no_grad():
        return R.forward(sdx, seq, spos, g['h'], blocked, n_head2=g['h2'], **kw)


def _decoder(sd, seq, enc, g, blocked, sdpa=None):
    """decoder_forward + read-outs, with ``sdpa`` substituted for oracle.lamp_ref.sdpa (``mha`` looks it up at call time)."""
    saved = R.sdpa
    if sdpa is not None:
        R.sdpa = sdpa
    try:
        y, slf, encdec, int_outs = R.decoder_forward(sd, seq, enc, blocked, g['h'], g['h2'])
    finally:
        R.sdpa = saved
    w = sd['tgt_word_proj.linear.weight']
    return R.readout(y, w), (slf, encdec), [R.readout(o, w) for o in int_outs[:-1]]


def live_forward_ref(sd, seq, spos, g, blocked, adj=None):
    """tests/enc_live_common.py's composition: the encoder's self-attention live (n_head heads), then the decoder.
    -> (logits, enc_output, encoder maps, (decoder self maps, enc-dec maps), intermediate predictions)."""
    return EC.live_forward_ref(sd, seq, spos, g['h'], blocked, adj=adj, n_head2=g['h2'])


def sigmoid_forward_ref(sd, seq, spos, g, blocked):
    """tests/sigmoid_common.py's restatement in both decoder attention blocks; the encoder stays softmax."""
    enc, enc_attns = R.encoder_forward(sd, seq, spos, g['h'], return_attns=True)
    logits, maps, ips = _decoder(sd, seq, enc, g, blocked, sigmoid_sdpa)
    return logits, enc, enc_attns, maps, ips


def label_bias_forward_ref(sd, seq, spos, g, blocked, bias):
    """tests/label_bias_common.py's restatement: ``bias`` (L, L) added to the label self-attention's scores (L != T), on top of
    the label mask ``blocked``."""
    assert g['L'] != seq.size(1)
    enc, enc_attns = R.encoder_forward(sd, seq, spos, g['h'], return_attns=True)
    logits, maps, ips = _decoder(sd, seq, enc, g, blocked, sdpa_with_label_bias(bias.to(enc.dtype), g['L']))
    return logits, enc, enc_attns, maps, ips


# ------------------------------------------------------------------ gradient cases
def grad_case(name, seed=None):
    """-> (LAMP on the CPU, state_dict, label block mask, src_seq, src_pos, geometry, targets, kind)."""
    gname, kind = GRAD_CASES[name]
    seed = GRAD_SEEDS[name] if seed is None else seed
    extra = {'live': dict(enc_self_attn=True), 'sigmoid': dict(dec_attn_type='sigmoid'), 'softmax': {}}[kind]
    m, sd, blocked, seq, spos, g = build(gname, seed=seed, **extra)
    tgt = (torch.rand(seq.size(0), g['L'], generator=torch.Generator().manual_seed(seed + 1)) < 0.2).float()
    return m, sd, blocked, seq, spos, g, tgt, kind


def oracle_run(kind, sd, seq, spos, g, blocked, tgt, dtype=torch.float64):
    """The oracle's forward, BCE loss and autograd in ``dtype`` -> (logits, enc, loss, {parameter name: gradient or None})."""
    sdx = {k: v.detach().clone().to(dtype).requires_grad_(True) if v.is_floating_point() else v for k, v in sd.items()}
    if kind == 'live':
        logits, enc = live_forward_ref(sdx, seq, spos, g, blocked)[:2]
    elif kind == 'sigmoid':
        logits, enc = sigmoid_forward_ref(sdx, seq, spos, g, blocked)[:2]
    else:
        logits, enc, _ = R.forward(sdx, seq, spos, g['h'], blocked, n_head2=g['h2'])
    loss = F.binary_cross_entropy_with_logits(logits, tgt.to(dtype))
    loss.backward()
    return logits.detach(), enc.detach(), loss.item(), {k: (v.grad if v.is_floating_point() else None) for k, v in sdx.items()}


def reference_gradient(grads, pname):
    """The oracle's gradient of a model parameter (the label embedding is tied to the read-out projection)."""
    ref = grads[pname]
    if pname == 'decoder.tgt_word_emb.weight' and grads.get('tgt_word_proj.weight') is not None:
        ref = ref + grads['tgt_word_proj.weight']
    return ref


def fp32_oracle_is_inside(name, seed):
    """The ReLU-kink condition (tests/attn_routes_common.py): the fp32 CPU oracle's own logits and autograd agree with the fp64
    oracle within the very bars the GPU is held to.  -> (bool, worst gradient error as a fraction of its bar)."""
    m, sd, blocked, seq, spos, g, tgt, kind = grad_case(name, seed)
    l64, e64, loss64, g64 = oracle_run(kind, sd, seq, spos, g, blocked, tgt, torch.float64)
    l32, e32, loss32, g32 = oracle_run(kind, sd, seq, spos, g, blocked, tgt, torch.float32)
    ok = (l32.double() - l64).abs().max().item() < 1e-4
    worst = 0.0
    for pname in g64:
        if g64[pname] is None:
            continue
        ref = reference_gradient(g64, pname)
        bar = GRAD_RTOL * ref.abs().max().item() + GRAD_ATOL
        worst = max(worst, (reference_gradient(g32, pname).double() - ref).abs().max().item() / bar)
    return ok and worst <= 1.0, worst


if __name__ == '__main__':
    for case in sorted(GRAD_CASES):
        for s in range(8):
            inside, frac = fp32_oracle_is_inside(case, s)
            print('%-12s seed %d: fp32 CPU oracle %s (worst gradient error %.3f of the bar)%s' % (
                case, s, 'inside' if inside else 'OUTSIDE', frac, '  <- chosen' if s == GRAD_SEEDS[case] else ''))
            if inside:
                break
