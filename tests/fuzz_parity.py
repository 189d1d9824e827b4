#!/usr/bin/env python3
"""Randomised differential campaign on the MI355X (not part of the pytest suite: minutes, not seconds).

    python tests/fuzz_parity.py <n_eval_cases> <n_train_cases>

(Lives under tests/ because it uses the oracle, which only test code may import.)

Eval: random model shapes (1-8 heads, d_k 4..256 incl. widths beyond the fused attention kernel, 1-3 + 1-3 layers,
every mask kind, L and T from 1 to 300 / 150, ragged lengths, with / without decoder self-attention; beyond the slice
tests/test_gpu_fuzz.py runs -- eval cases 60 on, training cases 6 on -- four cases in ten draw d_k, d_v and n_head2 independently
of each other and of d_model / n_head, from a generator of their own, and are built by tests/head_geometry_common.py): logits and
enc_output against the fp64 oracle (bar: max(1e-4, 4 x the oracle's own fp32-vs-fp64 gap)), every attention map against
the fp32 oracle (1e-5), logits bit-identical with and without return_attns (= packed vs padded encoder), and one sample
of the batch run alone at its own length bit-identical to its rows in the batch.
Train: dropout 0, BCE loss, every parameter's gradient against torch.autograd on the fp64 oracle (relative 2e-3 of
the gradient's max; a larger gap on one layer's FFN is what a ReLU pre-activation of ~1e-7 flipping sign between fp32
and fp64 looks like -- check the sub-layer in isolation before calling it a bug).
Round 1: 300 eval cases, 0 mismatches; 80 train cases, 1 flagged = such a ReLU kink (the sub-layer's backward, given
its own input and output gradient, agreed with fp64 to 3e-7).
"""
import sys, random, torch, traceback
import torch.nn.functional as F
import os
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT); sys.path.insert(0, os.path.join(_ROOT, 'tests'))
from oracle import lamp_ref as R
from lamp_amd.Models import LAMP
dev = torch.device('cuda:0')

def mad(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if a.numel() == 0: return 0.0
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb): return float('inf')
    return (torch.nan_to_num(a) - torch.nan_to_num(b)).abs().max().item()

def case(i):
    rng = random.Random(5000 + i)
    h = rng.choice([1, 2, 3, 4, 8])
    dk = rng.choice([4, 8, 12, 16, 20, 32, 36, 64, 128, 132, 160, 256])
    if h >= 4 and dk > 64: dk = 64
    d = h * dk
    if h == 1: d = rng.choice([4, 8, 20, 64, 128, 200])
    dff = rng.choice([4, 12, 64, 100, 200, 516])
    L = rng.choice([1, 2, 17, 31, 32, 33, 64, 95, 129, 300])
    T = rng.choice([1, 2, 5, 31, 32, 33, 97, 150, 200, 302])   # 200 / 302: four key shares in the small-shape attention
    B = rng.randint(1, 6)
    mask = rng.choice(['prior', 'none', 'inveye'])
    pos = rng.random() < 0.5
    n_enc, n_dec = rng.randint(1, 3), rng.randint(1, 3)
    no_slf = rng.random() < 0.2
    lengths = [rng.randint(1, T) for _ in range(B)]
    lengths[rng.randrange(B)] = T
    c = dict(h=h, d=d, dff=dff, L=L, T=T, B=B, mask=mask, pos=pos, n_enc=n_enc, n_dec=n_dec, no_slf=no_slf, lengths=lengths, V=rng.choice([5, 40, 1000]))
    # A general head geometry: only beyond the cases tests/test_gpu_fuzz.py runs (eval 0..59, training 10000..10005 keep the
    # shapes they always had), and from a second generator, so that the first one's stream does not move for any index.
    rng2 = random.Random(77000 + i)
    if (60 <= i < 10000 or i >= 10006) and rng2.random() < 0.4:
        h2 = rng2.choice([1, 2, 3, 4, 8])
        widths = [4, 8, 12, 16, 24, 32, 40, 64] + ([128, 160] if max(h, h2) < 4 else [])
        dk2, dv2 = rng2.choice(widths), rng2.choice(widths)
        if h == 1 or h2 == 1:
            dv2 = d           # a block of one head has no fc: its value width IS d_model
        c.update(h2=h2, dk=dk2, dv=dv2)
    return c

def build(c, i):
    h, d = c['h'], c['d']
    if 'h2' in c:
        import head_geometry_common as HG
        g = dict(V=c['V'], L=c['L'], T=c['T'], d=d, dff=c['dff'], h=h, h2=c['h2'], dk=c['dk'], dv=c['dv'], n_enc=c['n_enc'],
                 n_dec=c['n_dec'], mask=c['mask'], pos=c['pos'], no_dec_self_att=c['no_slf'])
        sd = HG.make_state_dict(c['V'], c['L'], c['T'], d, c['dff'], h, c['h2'], c['dk'], c['dv'], c['n_enc'], c['n_dec'],
                                pos_emb=c['pos'], seed=i, no_dec_self_att=c['no_slf'])
        adj = R.make_adjacency(c['L'], 0.2, i) if c['mask'] == 'prior' else None
        seq, spos = R.make_batch(c['B'], c['V'], c['T'], lengths=c['lengths'], seed=i)
        return HG.build_model(g, sd, adj).to(dev), sd, R.label_block_mask(adj, c['mask'], c['L']), seq, spos
    sd = R.make_state_dict(c['V'], c['L'], c['T'], d, c['dff'], h, c['n_enc'], c['n_dec'], pos_emb=c['pos'], seed=i, no_dec_self_att=c['no_slf'])
    adj = R.make_adjacency(c['L'], 0.2, i) if c['mask'] == 'prior' else None
    seq, spos = R.make_batch(c['B'], c['V'], c['T'], lengths=c['lengths'], seed=i)
    m = LAMP(c['V'], c['L'], c['T'], c['L'], n_layers_enc=c['n_enc'], n_layers_dec=c['n_dec'], n_head=h, n_head2=h, d_word_vec=d, d_model=d,
             d_inner_hid=c['dff'], d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', dropout=0.0, dec_dropout=0.0,
             no_enc_pos_embedding=not c['pos'], no_dec_self_att=c['no_slf'], label_adj_matrix=adj.clone() if adj is not None else None,
             label_mask=c['mask'], dec_dropout2=False)
    m.load_state_dict(sd)
    return m.to(dev), sd, R.label_block_mask(adj, c['mask'], c['L']), seq, spos

n_eval, n_train, bad = int(sys.argv[1]), int(sys.argv[2]), 0
for i in range(n_eval):
    c = case(i)
    try:
        m, sd, blocked, seq, spos = build(c, i)
        m.eval()
        with torch.no_grad():
            ref = R.forward(sd, seq, spos, c['h'], blocked, n_head2=c.get('h2'), return_attns=True)
            ref64, _, _ = R.forward(R.to_dtype(sd, torch.float64), seq, spos, c['h'], blocked, n_head2=c.get('h2'))
            lg, enc, _ = m((seq.to(dev), spos.to(dev)), None, None, None)
            got = m((seq.to(dev), spos.to(dev)), None, None, None, return_attns=True)
        gap = mad(ref[0], ref64)
        tol = max(1e-4, 4 * gap)
        errs = [mad(enc, ref[1]) < 5e-5, mad(lg, ref64) < tol, torch.equal(got[0], lg)]
        # a sample alone, padded to its own length: the same bits as inside the batch (packed encoder, per-sample key split)
        b = i % c['B']; n = c['lengths'][b]
        with torch.no_grad():
            one, enc_one, _ = m((seq[b:b + 1, :n].to(dev), spos[b:b + 1, :n].to(dev)), None, None, None)
        errs.append(torch.equal(one, lg[b:b + 1]) and torch.equal(enc_one, enc[b:b + 1, :n]))
        for a, b in zip(got[3][1], ref[3][1]): errs.append(mad(a, b) < 1e-5)
        for a, b in zip(got[3][0], ref[3][0]):
            if a is not None: errs.append(mad(a, b) < 1e-5)
        for a, b in zip(got[2][0], ref[2][0]): errs.append(mad(a, b) < 1e-5)
        if not all(errs):
            bad += 1; print('EVAL MISMATCH', i, c, errs, mad(lg, ref64), tol)
    except Exception as e:
        bad += 1; print('EVAL ERROR', i, c, repr(e)); traceback.print_exc()
print('eval cases', n_eval, 'bad', bad)
bad_t = flips = 0
for i in range(n_train):
    c = case(10000 + i)
    c['L'] = min(c['L'], 95); c['T'] = min(c['T'], 97)
    c['lengths'] = [min(x, c['T']) for x in c['lengths']]; c['lengths'][0] = c['T']
    try:
        m, sd, blocked, seq, spos = build(c, i)
        tgt = (torch.rand(c['B'], c['L'], generator=torch.Generator().manual_seed(i)) < 0.3).float()
        sd64 = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
        rl, _, _ = R.forward(sd64, seq, spos, c['h'], blocked, n_head2=c.get('h2'))
        F.binary_cross_entropy_with_logits(rl, tgt.double()).backward()
        m.train()
        lg, _, _ = m((seq.to(dev), spos.to(dev)), None, None, tgt.to(dev))
        F.binary_cross_entropy_with_logits(lg, tgt.to(dev)).backward()
        worst, worst_name = 0.0, None
        for n, p in m.named_parameters():
            if p.grad is None: continue
            ref = sd64[n].grad
            if n == 'decoder.tgt_word_emb.weight' and 'tgt_word_proj.weight' in sd64 and sd64['tgt_word_proj.weight'].grad is not None:
                ref = ref + sd64['tgt_word_proj.weight'].grad
            scale = ref.abs().max().item()
            rel = mad(p.grad, ref) / (scale + 1e-12) if scale > 0 else mad(p.grad, ref)
            if scale > 1e-9 and rel > worst: worst, worst_name = rel, n
        if not (worst < 2e-3) and worst_name.endswith(('w_1.weight', 'w_1.bias')):
            # ONE hidden unit of a position-wise FFN carrying the whole error (every other unit at rounding level) is a ReLU whose
            # pre-activation sits within fp32 rounding of zero for one row: fp32 and fp64 take different sides of the kink, the
            # function is discontinuous there and no summation order is "right" (campaign of round 6: cases 336 and 390, unit 7 /
            # unit 88, all other units <= 1e-6 of the scale; the CPU fp32 oracle happens to fall on the fp64 side).  Counted apart.
            g, r_ = dict(m.named_parameters())[worst_name].grad.detach().double().cpu(), sd64[worst_name].grad
            per_unit = (g - r_).abs().reshape(g.shape[0], -1).max(1).values / r_.abs().max().item()
            if torch.sort(per_unit, descending=True).values[1].item() < 1e-5:
                flips += 1; print('RELU FLIP', i, c, worst, worst_name, 'unit', int(per_unit.argmax()), 'logits', mad(lg, rl))
                continue
        if not (worst < 2e-3):
            bad_t += 1; print('TRAIN MISMATCH', i, c, worst, worst_name, 'logits', mad(lg, rl))
            for n, p in m.named_parameters():   # where the gradient departs: per parameter, relative to its own maximum
                if p.grad is not None and sd64[n].grad is not None:
                    sc_ = sd64[n].grad.abs().max().item()
                    if sc_ > 1e-9 and mad(p.grad, sd64[n].grad) / sc_ > 2e-4: print('     ', n, mad(p.grad, sd64[n].grad) / sc_)
    except Exception as e:
        bad_t += 1; print('TRAIN ERROR', i, c, repr(e)); traceback.print_exc()
print('train cases', n_train, 'bad', bad_t, 'relu flips (single hidden unit, see above)', flips)
