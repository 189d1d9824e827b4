#!/usr/bin/env python3
"""Device time of the clipped AdamW step: lamp_grad_norm + lamp_optim_step_ext against clip_grad_norm_ + torch's fused AdamW and
against the plain lamp_optim_step, on the same tensors, and inside the training step.

    python tools/bench_optim_ext.py [--out profiles/optim_ext_bench.json] [--runs 11] [--skip-step]

1. The optimizer step alone, at two parameter lists: the reuters-shaped model's (d_model 512, 2 + 2 layers, 4 heads, 90 labels,
   2000 words: its trainable parameters as the model holds them) and ONE 16 M-element tensor.  Candidates, alternating window
   by window in one process on tensors allocated once:
     lamp_ext     lamp_amd.optim.AdamW(weight_decay=0.01, max_grad_norm=1.0).step(): one norm (two launches) + one update
     torch_fused  torch.nn.utils.clip_grad_norm_(params, 1.0) + torch.optim.AdamW(fused=True).step()
     lamp_plain   lamp_amd.optim.Adam().step(): the one launch without any option (no clipping, no decay)
   HIP events around a window of `reps` back-to-back steps (a window lasts about 20 ms), the median of the runs; all runs kept.
   The figures hold each route's host work too: a step whose kernels are shorter than its host side (the model's 75-tensor
   list: the table is rebuilt from the live pointers on every step) is issued at the host's rate.
2. The reuters-shaped batch-32 training step through lamp_amd.train.train_batch, same weights: lamp Adam without options,
   lamp AdamW with weight decay 0.01, clipping at 1.0 and skip_nonfinite, and torch's fused AdamW behind clip_grad_norm_;
   alternating round by round, every round's ratio kept.
No speed is promised; the ratios go into README.md and DESIGN.md section 8.11 whichever way they fall.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

WINDOW_MS = 20.0
MAX_REPS = 2000
BETAS = (0.9, 0.98)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns, runs):
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = [max(1, min(MAX_REPS, int(WINDOW_MS / max(window(fn, 10), 1e-4)) + 1)) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            times[i].append(window(fn, reps[i]))
    return reps, times


def reuters_model(dev, seed=0):
    from lamp_amd import synthetic
    from lamp_amd.Models import LAMP
    V, L, T_len, d, h = 2000, 90, 302, 512, 4
    sd = synthetic.make_state_dict(V, L, T_len + 1, d, 1024, h, 2, 2, seed=seed)
    adj = synthetic.make_adjacency(L, 0.2, 0)
    m = LAMP(V, L, T_len + 1, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d,
             d_inner_hid=1024, d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', label_adj_matrix=adj.clone(),
             label_mask='prior', dec_dropout2=False)
    m.load_state_dict(sd)
    return m.to(dev).train(), (V, L, T_len, d)


def bench_list(name, shapes, dev, runs):
    """Three optimizers over three copies of the same parameters and the same (constant) gradients."""
    from lamp_amd import optim as O
    g = torch.Generator(device=dev).manual_seed(len(shapes))
    base = [torch.randn(s, generator=g, device=dev) * 0.05 for s in shapes]
    grads = [torch.randn(s, generator=g, device=dev) * 0.5 for s in shapes]

    def copy():
        ps = [torch.nn.Parameter(b.clone()) for b in base]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        return ps

    pa, pb, pc = copy(), copy(), copy()
    ext = O.AdamW(pa, betas=BETAS, lr=1e-5, weight_decay=0.01, max_grad_norm=1.0)
    fused = torch.optim.AdamW(pb, betas=BETAS, lr=1e-5, weight_decay=0.01, fused=True)
    plain = O.Adam(pc, betas=BETAS, lr=1e-5)

    def torch_step():
        torch.nn.utils.clip_grad_norm_(pb, 1.0)
        fused.step()
        for p, gr in zip(pb, grads):      # clip_grad_norm_ rewrote the gradients: the next step clips the same ones again
            p.grad.copy_(gr)

    def torch_step_only():
        torch.nn.utils.clip_grad_norm_(pb, 1.0)
        fused.step()

    fns = [ext.step, torch_step_only, plain.step]
    # the first two compute the same update (one step from the same state): agreement before anything is timed
    ext.step()
    torch_step()
    torch.cuda.synchronize()
    agree = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(pa, pb))
    reps, times = alternate(fns, runs)
    med = statistics.median
    names = ('lamp_ext', 'torch_fused', 'lamp_plain')
    out = {'list': name, 'tensors': len(shapes), 'elements': int(sum(b.numel() for b in base)),
           'max_abs_difference_lamp_ext_vs_torch_after_one_step': agree,
           'note_torch_fused': 'clip_grad_norm_ rescales .grad in place, so after its first call the torch route holds a gradient '
                               'of norm 1 and multiplies by 1; its launches and bytes do not depend on the values'}
    for n, r, ts, fn in zip(names, reps, times, fns):
        out['%s_ms_median' % n] = med(ts)
        out['%s_reps_per_window' % n] = r
        out['%s_ms_all' % n] = ts
    out['lamp_ext_over_torch_fused'] = out['lamp_ext_ms_median'] / out['torch_fused_ms_median']
    out['lamp_ext_over_lamp_plain'] = out['lamp_ext_ms_median'] / out['lamp_plain_ms_median']
    return out


def step_rows(dev, B=32, rounds=10):
    from lamp_amd import optim as O
    from lamp_amd import synthetic
    from lamp_amd import train as T
    from lamp_amd.run_train import decay_param_groups
    seq = pos = tgt = None
    steps = []
    for which in ('lamp_plain', 'lamp_ext', 'torch_fused'):
        m, (V, L, T_len, d) = reuters_model(dev)
        if seq is None:
            seq, pos = synthetic.make_batch(B, V, T_len, seed=0)
            seq, pos = seq.to(dev), pos.to(dev)
            tgt = (torch.rand(B, L, device=dev) < 0.05).float()
        if which == 'lamp_plain':
            optim = O.Adam(list(m.get_trainable_parameters()), betas=BETAS, lr=1e-5)
        elif which == 'lamp_ext':
            optim = O.AdamW(decay_param_groups(m, 0.01), betas=BETAS, lr=1e-5, max_grad_norm=1.0, skip_nonfinite=True)
        else:
            groups = decay_param_groups(m, 0.01)
            optim = torch.optim.AdamW(groups, betas=BETAS, lr=1e-5, fused=True)
            clipped = [p for g in groups for p in g['params']]

            def clip_first(*_, clipped=clipped):
                torch.nn.utils.clip_grad_norm_(clipped, 1.0)
            optim.register_step_pre_hook(clip_first)
        opt = argparse.Namespace(tgt_vocab_size=L, binary_relevance=True, int_preds=False, int_pred_weight=0.2, attns_loss=False,
                                 matching_mlp=False, decoder='graph', loss_options=None)
        probs, rows = torch.empty(B, L, device=dev), torch.empty(1, B, device=dev)

        def f(m=m, optim=optim, opt=opt, probs=probs, rows=rows):
            T.train_batch(m, optim, opt, (seq, pos), None, tgt, probs, rows)
        steps.append(f)
    for fn in steps:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in steps]
    for _ in range(rounds):
        for i, fn in enumerate(steps):
            times[i].append(window(fn, 20))
    t_plain, t_ext, t_torch = times
    r_plain = sorted(a / b for a, b in zip(t_ext, t_plain))
    r_torch = sorted(a / b for a, b in zip(t_ext, t_torch))
    med = statistics.median
    return {'batch': B, 'iters_per_round': 20, 'rounds': rounds,
            'lamp_plain_step_ms_median': med(t_plain), 'lamp_ext_step_ms_median': med(t_ext), 'torch_fused_clip_step_ms_median': med(t_torch),
            'lamp_ext_over_lamp_plain_per_round': {'median': med(r_plain), 'min': r_plain[0], 'max': r_plain[-1]},
            'lamp_ext_over_torch_fused_clip_per_round': {'median': med(r_torch), 'min': r_torch[0], 'max': r_torch[-1]},
            'lamp_plain_step_ms_all': t_plain, 'lamp_ext_step_ms_all': t_ext, 'torch_fused_clip_step_ms_all': t_torch}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_ext_bench.json'))
    ap.add_argument('--runs', type=int, default=11)
    ap.add_argument('--skip-step', action='store_true', help='part 1 alone')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_optim_ext.py needs an MI355X: no HIP device visible')
    dev = torch.device('cuda:0')
    result = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'runs': args.runs,
              'timing': 'HIP events around a window of back-to-back steps, per-step ms (host work included), candidates '
                        'alternating; one run of this tool on one MI355X, not a distribution over runs',
              'optimizer_step': []}
    model, _ = reuters_model(dev)
    shapes = [tuple(p.shape) for p in model.get_trainable_parameters()]
    del model
    for name, sh in (('reuters-shaped model', shapes), ('one 16 M-element tensor', [(16 * 1024 * 1024,)])):
        entry = bench_list(name, sh, dev, args.runs)
        result['optimizer_step'].append(entry)
        print(json.dumps({k: v for k, v in entry.items() if not k.endswith('_all')}), flush=True)
    if not args.skip_step:
        result['training_step'] = step_rows(dev)
        print(json.dumps({k: v for k, v in result['training_step'].items() if not k.endswith('_all')}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
