"""Shared pieces of tests/test_attention_train_routes_gpu.py: the training-side attention routes beyond 256 queries.

Where a call with maps AND lse (the single-pass write-out, PM == 2) goes -- launch_attn, lamp_amd/csrc/attention.hip:
    16-query kernel (attention_small.hip)   lq <= 256, or lk <= 64 without per-sample key counts, or LAMP_MASK_SELF_RAGGED,
                                            or bit 7 of the tuning hook
    32-query kernel (attn_kernel<DP, KS, 2>) everything else: lq > 256 and lk > 64; KS = 2 only when forced (tuning hook)
``route`` restates that rule so a parameter list can assert, by construction, which kernel it reaches.

Section 1 (kernel level): ``sdpa_case`` builds head-fused operands with every edge the issue names, ``sdpa_reference`` the fp64
softmax(masked_fill(Q K^T * scale, -inf)), P V and row logsumexp / ln 2 in plain torch on the CPU (computed once per case and
shared), ``check_fast_maps`` the assertions.  Section 3 (whole model): ``model_case`` / ``oracle_run`` / ``fp32_oracle_is_inside``.

``python tests/attn_routes_common.py`` re-runs, without a GPU, the seed choice of section 3: the seeds for which the fp32 CPU
oracle's own autograd stays inside the gradient tolerance against the fp64 oracle (a ReLU kink cannot fake a mismatch)."""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:     # run as a script (under pytest, conftest.py has done this)
    sys.path.insert(0, ROOT)

import enc_live_common as EC  # noqa: E402
from oracle import lamp_ref as R  # noqa: E402
from sigmoid_common import sigmoid_sdpa  # noqa: E402

SPIKE_NAT = 40.0    # the late spike's score (natural units): 57.7 in the kernels' log2 domain, past their 2^32 lazy-rescale threshold
TOL_MAP, TOL_OUT, TOL_ROWSUM = 5e-6, 2e-5, 1e-5     # the bars of test_sdpa_vs_oracle_shapes / test_fast_maps_attention_equals_exact_two_pass
LSE_FACTOR = 4.0    # the kernel may miss fp64 by 4x what fp32 torch on the CPU misses it by (the rule of tests/fuzz_parity.py)
GRAD_RTOL, GRAD_ATOL = 3e-4, 1e-9                   # tests/test_gpu_training.py


def route(lq, lk, self_ragged=False, force=0):
    """The kernel a P && lse call reaches (no per-sample key counts: what lamp_sdpa_fwd_fast_maps / lamp_mha_train_fwd pass)."""
    return 'small16' if (lq <= 256 or lk <= 64 or self_ragged or (force & 0x80)) else 'attn32'


# ------------------------------------------------------------------ section 1: operands, reference, assertions
_CASES = {}


def sdpa_case(lq, lk, dk, dv, kind, H=2):
    """Head-fused q (B, lq, H*dk), k (B, lk, H*dk), v (B, lk, H*dv) and a mask of ``kind``:
      'none'    no mask
      'u8'      a per-sample byte mask; sample 0's LAST query row is fully blocked (a dead row in the tail query block)
      'shared'  one [lq, lk] mask for every sample; its last row is fully blocked
      'keys'    a key-token mask, B = 3: sample 0 half padding, sample 1 ALL padding (every row dead), sample 2 whole
    plus one late spike: key lk - 1 (alone or nearly alone in the last partial key tile) scores SPIKE_NAT for query lq - 2 of
    the last sample, in every head, so the running maximum jumps after nearly the whole row sum has accumulated.
    -> dict, cached: the reference is computed once per case and never modified."""
    key = (lq, lk, dk, dv, kind, H)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(lq * 1009 + lk * 31 + dk * 7 + dv + len(kind))
    B = 3 if kind == 'keys' else 2
    q, k, v = torch.randn(B, lq, H * dk, generator=g), torch.randn(B, lk, H * dk, generator=g), torch.randn(B, lk, H * dv, generator=g)
    seq = shared = None
    blocked = torch.zeros(B, lq, lk, dtype=torch.bool)
    dead = torch.zeros(B, lq, dtype=torch.bool)
    sb, sr, sk = B - 1, lq - 2, lk - 1            # the spike's sample, query, key
    if kind == 'u8':
        blocked = torch.rand(B, lq, lk, generator=g) < 0.35
        blocked[:, :, 0] = False
        blocked[sb, sr, sk] = False
        blocked[0, lq - 1, :] = True
        dead[0, lq - 1] = True
    elif kind == 'shared':
        shared = torch.rand(lq, lk, generator=g) < 0.6
        shared[:, 0] = False
        shared[sr, sk] = False
        shared[lq - 1, :] = True
        blocked = shared.unsqueeze(0).expand(B, lq, lk).clone()
        dead[:, lq - 1] = True
    elif kind == 'keys':
        seq = torch.randint(1, 50, (B, lk), generator=g)
        seq[0, lk // 2:] = 0
        seq[1, :] = 0
        blocked = seq.eq(0).unsqueeze(1).expand(B, lq, lk).clone()
        dead[1, :] = True
    else:
        assert kind == 'none'
    for h in range(H):
        qv = q[sb, sr, h * dk:(h + 1) * dk]
        k[sb, sk, h * dk:(h + 1) * dk] = qv * (SPIKE_NAT * dk ** 0.5 / float(qv @ qv))
    assert torch.equal(dead, blocked.all(-1))     # the dead rows are the ones built in on purpose, nothing else
    c = dict(lq=lq, lk=lk, dk=dk, dv=dv, kind=kind, H=H, B=B, q=q, k=k, v=v, seq=seq, shared=shared, blocked=blocked, dead=dead,
             scale=1.0 / dk ** 0.5, spike=(sb, sr, sk))
    c.update(sdpa_reference(c))
    _CASES[key] = c
    return c


def _scores(c, dtype):
    B, H, lq, lk, dk = c['B'], c['H'], c['lq'], c['lk'], c['dk']
    qh = c['q'].to(dtype).view(B, lq, H, dk).permute(2, 0, 1, 3)
    kh = c['k'].to(dtype).view(B, lk, H, dk).permute(2, 0, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) * c['scale']
    return s.masked_fill(c['blocked'].unsqueeze(0), float('-inf'))       # (H, B, lq, lk)


def sdpa_reference(c):
    """fp64: maps (H*B, lq, lk) [index head*B + b], output (B, lq, H*dv), lse2 = logsumexp(masked scores) / ln 2 (H*B, lq);
    and the gap of the same lse2 computed in fp32 torch on the CPU, over the live rows."""
    B, H, lq, lk, dv = c['B'], c['H'], c['lq'], c['lk'], c['dv']
    s = _scores(c, torch.float64)
    P = torch.softmax(s, -1)
    vh = c['v'].double().view(B, lk, H, dv).permute(2, 0, 1, 3)
    O = (P @ vh).permute(1, 2, 0, 3).reshape(B, lq, H * dv)
    lse = torch.logsumexp(s, -1) / math.log(2.0)
    lse32 = torch.logsumexp(_scores(c, torch.float32), -1) / math.log(2.0)
    live = ~c['dead'].unsqueeze(0).expand(H, B, lq)
    assert torch.isinf(lse[~live]).all() and torch.isfinite(lse[live]).all()
    gap = (lse32.double() - lse)[live].abs().max().item()
    # the spike does what it is there for: its score leads every earlier key of its row by more than the rescale threshold (log2)
    sb, sr, sk = c['spike']
    row = s[:, sb, sr, :] / math.log(2.0)
    assert (row[:, sk] - row[:, :sk].max(-1).values).min().item() > 32.0
    return dict(ref_P=P.reshape(H * B, lq, lk), ref_O=O, ref_lse=lse.reshape(H * B, lq), lse_gap_fp32=gap,
                live=live.reshape(H * B, lq))


def device_mask(N, c, dev, self_ragged=False):
    """-> (N.Mask or None, keepalive tensor)."""
    B, lq, lk = c['B'], c['lq'], c['lk']
    if c['kind'] == 'none':
        assert not self_ragged, 'the flag travels in a mask'
        return None, None
    if c['kind'] == 'u8':
        m, keep = N.make_mask(c['blocked'].to(dev), B, lq, lk)
    elif c['kind'] == 'shared':
        m, keep = N.make_mask(c['shared'].to(dev), B, lq, lk)
    else:
        m, keep = N.key_token_mask(c['seq'].to(dev), lk)
    if self_ragged:
        m.flags |= N.LAMP_MASK_SELF_RAGGED
    return m, keep


def run_fast_maps(N, c, dev, self_ragged=False, _lib=None):
    """lamp_sdpa_fwd_fast_maps on the case -> (out, maps, lse) on the device."""
    m, keep = device_mask(N, c, dev, self_ragged)
    out, P, lse = N.sdpa_fused(c['q'].to(dev), c['k'].to(dev), c['v'].to(dev), c['H'], m, c['scale'], need_attn=True,
                               fast_maps=True, return_lse=True, _lib=_lib)
    torch.cuda.synchronize()
    del keep
    return out, P, lse


_GAPS = {}


def lse_gap_fp32(case_keys):
    """The yardstick for lse: the worst gap to fp64 of the same quantity computed in fp32 torch on the CPU, over ALL the inputs
    of a test -- ``case_keys``, the argument tuples of sdpa_case for every case of the test function.  A property of the
    inputs and of CPU arithmetic alone (no kernel result enters), computed once per test function.
    Why not one gap per case: a case's gap is the maximum over its two spike rows (lse = 57.7, one fp32 ulp = 3.8e-6) of an
    error that is a small whole number of ulps -- it spans 2.7e-6 .. 2.5e-5 over this file's cases, a yardstick ten times
    noisier than what it measures."""
    key = tuple(case_keys)
    if key not in _GAPS:
        _GAPS[key] = max(sdpa_case(*k)['lse_gap_fp32'] for k in key)
    return _GAPS[key]


def check_fast_maps(c, out, P, lse, gap, tag=''):
    """Every assertion of section 1; prints the measured figures first (pytest -s shows them).  ``gap``: lse_gap_fp32 over the
    calling test's inputs.  -> the figures."""
    H, B, lq, lk = c['H'], c['B'], c['lq'], c['lk']
    out, P, lse = out.detach().double().cpu(), P.detach().double().cpu(), lse.detach().double().cpu()
    live = c['live']                                     # (H*B, lq)
    n_live = int(live.sum())
    n_dead = H * int(c['dead'].sum())
    live_o = ~c['dead']                                  # (B, lq): an output row is NaN in every head's columns or in none
    blocked = c['blocked'].unsqueeze(0).expand(H, B, lq, lk).reshape(H * B, lq, lk)
    fig = dict(
        maps=(P[live] - c['ref_P'][live]).abs().max().item(),
        out=(out[live_o] - c['ref_O'][live_o]).abs().max().item(),
        rowsum=(P[live].sum(-1) - 1.0).abs().max().item(),
        lse=(lse[live] - c['ref_lse'][live]).abs().max().item(),
        lse_gap_fp32=gap)
    print('%s %dx%d dk=%d dv=%d %-6s maps %.2e out %.2e rowsum %.2e lse %.2e = %.2f x the fp32 CPU gap %.2e (this case alone: '
          '%.2e, x%.2f)' % (tag, lq, lk, c['dk'], c['dv'], c['kind'], fig['maps'], fig['out'], fig['rowsum'], fig['lse'],
                            fig['lse'] / gap, gap, c['lse_gap_fp32'], fig['lse'] / c['lse_gap_fp32']))
    # NaN exactly where the reference has it -- the dead rows built in on purpose -- and every other entry is compared
    assert torch.equal(torch.isnan(P), torch.isnan(c['ref_P'])) and torch.equal(torch.isnan(out), torch.isnan(c['ref_O']))
    assert torch.equal(torch.isnan(P).all(-1), ~live) and torch.equal(torch.isnan(out).all(-1), c['dead'])
    assert n_live == H * B * lq - n_dead and P[live].numel() == n_live * lk and not torch.isnan(P[live]).any()
    assert n_dead == {'none': 0, 'u8': H, 'shared': H * B, 'keys': H * lq}[c['kind']]
    assert fig['maps'] < TOL_MAP and fig['out'] < TOL_OUT
    assert (P[live.unsqueeze(-1) & blocked] == 0).all()                  # blocked entries of live rows: exactly 0
    assert fig['rowsum'] < TOL_ROWSUM
    assert torch.isfinite(lse[live]).all() and fig['lse'] <= LSE_FACTOR * fig['lse_gap_fp32']
    # a fully blocked row: l = 0, lse = log2(0) = -inf (include/lamp_hip.h); exp2(-inf - -inf) is the row's NaN
    assert (lse[~live] == float('-inf')).all()
    return fig


# ------------------------------------------------------------------ section 3: whole models
# name: (kind, cfg).  'softmax' / 'sigmoid': V, L, T, d, dff, h, mask, pos_emb, B, p_adj, lengths as tests/test_gpu_training.py::CASES;
# 'live': a shape of tests/enc_live_common.py.  The seeds are the first for which fp32_oracle_is_inside() holds (see __main__).
TINY260 = (50, 260, 23, 64, 96, 2, None, True, 2, 0.1, [23, 9])
MODEL_CASES = {
    'labels260_prior': ('softmax', TINY260[:6] + ('prior',) + TINY260[7:]),
    'labels260_inveye': ('softmax', TINY260[:6] + ('inveye',) + TINY260[7:]),
    'labels260_sigmoid': ('sigmoid', TINY260[:6] + ('prior',) + TINY260[7:]),
    'live_T300': ('live', 'B'),
}
MODEL_SEEDS = {'labels260_prior': 0, 'labels260_inveye': 0, 'labels260_sigmoid': 0, 'live_T300': 0}


def model_case(name, seed=None):
    """-> (LAMP on the CPU, state_dict, label block mask, src_seq, src_pos, n_head, targets, kind)."""
    from lamp_amd.Models import LAMP
    kind, cfg = MODEL_CASES[name]
    seed = MODEL_SEEDS[name] if seed is None else seed
    if kind == 'live':
        m, sd, blocked, seq, spos, h = EC.build(cfg, 'prior', True, seed=seed)
        L = EC.SHAPES[cfg]['L']
    else:
        V, L, T, d, dff, h, mask, pos, B, p, lengths = cfg
        sd = R.make_state_dict(V, L, T, d, dff, h, 2, 2, pos_emb=pos, seed=seed)
        adj = R.make_adjacency(L, p, seed) if mask == 'prior' else None
        seq, spos = R.make_batch(B, V, T, lengths=lengths, seed=seed)
        extra = dict(dec_attn_type='sigmoid') if kind == 'sigmoid' else {}
        m = LAMP(V, L, T, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=dff,
                 d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', dropout=0.0, dec_dropout=0.0,
                 no_enc_pos_embedding=not pos, label_adj_matrix=adj.clone() if adj is not None else None, label_mask=mask,
                 dec_dropout2=False, **extra)
        m.load_state_dict(sd)
        blocked = R.label_block_mask(adj, mask, L)
    tgt = (torch.rand(seq.size(0), L, generator=torch.Generator().manual_seed(seed + 1)) < 0.2).float()
    return m, sd, blocked, seq, spos, h, tgt, kind


def oracle_run(kind, sd, seq, spos, h, blocked, tgt, dtype=torch.float64):
    """The oracle's forward, BCE loss and autograd in ``dtype`` -> (logits, enc, loss, {parameter name: gradient or None})."""
    sdx = {k: v.detach().clone().to(dtype).requires_grad_(True) if v.is_floating_point() else v for k, v in sd.items()}
    if kind == 'live':
        logits, enc = EC.live_forward_ref(sdx, seq, spos, h, blocked)[:2]
    elif kind == 'sigmoid':     # the restatement of tests/sigmoid_common.py in the decoder (mha looks sdpa up at call time)
        enc = R.encoder_forward(sdx, seq, spos, h)[0]
        saved = R.sdpa
        R.sdpa = sigmoid_sdpa
        try:
            y = R.decoder_forward(sdx, seq, enc, blocked, h)[0]
        finally:
            R.sdpa = saved
        logits = R.readout(y, sdx['tgt_word_proj.linear.weight'])
    else:
        logits, enc, _ = R.forward(sdx, seq, spos, h, blocked)
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
    """The ReLU-kink condition: the fp32 CPU oracle's own logits, loss and autograd agree with the fp64 oracle within the very
    bars the GPU is held to.  -> (bool, worst gradient error as a fraction of its bar)."""
    m, sd, blocked, seq, spos, h, tgt, kind = model_case(name, seed)
    l64, e64, loss64, g64 = oracle_run(kind, sd, seq, spos, h, blocked, tgt, torch.float64)
    l32, e32, loss32, g32 = oracle_run(kind, sd, seq, spos, h, blocked, tgt, torch.float32)
    ok = (l32.double() - l64).abs().max().item() < 1e-4 and (e32.double() - e64).abs().max().item() < 5e-5
    ok = ok and abs(loss32 - loss64) < 1e-5
    worst = 0.0
    for pname in g64:
        if g64[pname] is None:
            continue
        ref = reference_gradient(g64, pname)
        bar = GRAD_RTOL * ref.abs().max().item() + GRAD_ATOL
        worst = max(worst, (reference_gradient(g32, pname).double() - ref).abs().max().item() / bar)
    return ok and worst <= 1.0, worst


if __name__ == '__main__':
    for case in sorted(MODEL_CASES):
        for s in range(8):
            inside, frac = fp32_oracle_is_inside(case, s)
            print('%-18s seed %d: fp32 CPU oracle %s (worst gradient error %.3f of the bar)%s' % (
                case, s, 'inside' if inside else 'OUTSIDE', frac, '  <- chosen' if s == MODEL_SEEDS[case] else ''))
            if inside:
                break
