#!/usr/bin/env python3
"""Device time of weight averaging: lamp_weight_average against torch._foreach_lerp_, lamp_weight_swap against three _foreach
copies through a scratch list, on the same tensors, and the training step with and without an EMA.

    python tools/bench_weight_avg.py [--out profiles/weight_avg_bench.json] [--runs 11] [--skip-step]

(a) lamp_weight_average (through lamp_amd._native.weight_average with the ctypes table kept between calls, as
    WeightAverage.update() keeps it while no parameter moves) against torch._foreach_lerp_(avgs, params, w) -- what
    torch.optim.swa_utils' multi_avg_fn calls -- on the reuters-shaped model's trainable parameters (d_model 512, 2 + 2 layers,
    4 heads, 90 labels, 2000 words);
(b) the same two on ONE 16 M-element tensor: a pure stream of 12 bytes per element (read p, read a, write a);
(c) lamp_weight_swap against _foreach_copy_(tmp, p); _foreach_copy_(p, a); _foreach_copy_(a, tmp) on the model's list.
    HIP events around a window of `reps` back-to-back calls (a window lasts about 20 ms), candidates alternating window by
    window on tensors allocated once, the median of the runs; all runs kept.  The figures hold each route's host work too.
    Beside (a) and (b): achieved bytes/s = 12 bytes per element over the per-call time, next to the 6.29 TB/s a float4 copy
    has been measured to reach on this part (8.0 TB/s is the HBM3E specification).  (a) also records whether the call is bound
    by the rate at which the host issues it: the host's wall time per call over 200 calls issued without a wait, against the
    back-to-back per-call time on the device, and the time a pure stream of its bytes would take.
(d) the reuters-shaped batch-32 training step through lamp_amd.train.train_batch with lamp_amd.optim.Adam, with and without
    opt.weight_average = WeightAverage(kind='ema'), alternating over 10 rounds, every round's ratio kept.
No speed is promised; the figures go into README.md and DESIGN.md section 8.14 whichever way they fall.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_optim_ext import BETAS, alternate, reuters_model, window  # noqa: E402

HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0
W = 1.0 - 0.999


def bench_average(name, shapes, dev, runs):
    from lamp_amd import _native as N
    g = torch.Generator(device=dev).manual_seed(len(shapes))
    params = [torch.randn(s, generator=g, device=dev) for s in shapes]
    a_lamp = [torch.randn(s, generator=g, device=dev) for s in shapes]
    a_torch = [a.clone() for a in a_lamp]
    entries = list(zip(params, a_lamp))
    table = N.average_table('bench', entries)

    def lamp():
        N.weight_average(entries, W, table)

    def torch_lerp():
        torch._foreach_lerp_(a_torch, params, W)

    lamp()
    torch_lerp()
    torch.cuda.synchronize()
    agree = max(float((x - y).abs().max()) for x, y in zip(a_lamp, a_torch))
    reps, times = alternate([lamp, torch_lerp], runs)
    med = statistics.median
    elements = int(sum(p.numel() for p in params))
    out = {'list': name, 'tensors': len(shapes), 'elements': elements, 'bytes_per_call': 12 * elements, 'weight': W,
           'max_abs_difference_lamp_vs_torch_after_one_update': agree,
           'hbm_float4_copy_measured_TBps': HBM_MEASURED_TBS, 'hbm_spec_TBps': HBM_SPEC_TBS}
    for n, r, ts in zip(('lamp', 'torch_foreach_lerp'), reps, times):
        out['%s_ms_median' % n] = med(ts)
        out['%s_reps_per_window' % n] = r
        out['%s_ms_all' % n] = ts
        out['%s_achieved_TBps' % n] = 12 * elements / (med(ts) * 1e-3) / 1e12
    out['lamp_over_torch_foreach_lerp'] = out['lamp_ms_median'] / out['torch_foreach_lerp_ms_median']
    # is the call bound by the launch rate?  host time of one call (no device wait inside), and the stream time of its bytes
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        lamp()
    host_ms = (time.perf_counter() - t0) / 200 * 1e3
    torch.cuda.synchronize()
    out['lamp_host_issue_ms_per_call'] = host_ms
    out['stream_ms_of_its_bytes_at_measured_hbm'] = 12 * elements / (HBM_MEASURED_TBS * 1e12) * 1e3
    out['launch_rate_bound'] = bool(host_ms >= 0.8 * out['lamp_ms_median'])
    out['note_launch_rate_bound'] = ('true when the host needs at least 0.8 of the back-to-back per-call time to issue one call: '
                                     'the device then waits for the host, and the figure is the issue rate, not the kernel')
    return out


def bench_swap(shapes, dev, runs):
    from lamp_amd import _native as N
    g = torch.Generator(device=dev).manual_seed(7)
    p1 = [torch.randn(s, generator=g, device=dev) for s in shapes]
    a1 = [torch.randn(s, generator=g, device=dev) for s in shapes]
    p2, a2 = [p.clone() for p in p1], [a.clone() for a in a1]
    tmp = [torch.empty_like(p) for p in p2]
    entries = list(zip(p1, a1))
    table = N.average_table('bench', entries)

    def lamp():
        N.weight_swap(entries, table)

    def torch_copies():
        torch._foreach_copy_(tmp, p2)
        torch._foreach_copy_(p2, a2)
        torch._foreach_copy_(a2, tmp)

    lamp()
    torch_copies()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(p1 + a1, p2 + a2))
    reps, times = alternate([lamp, torch_copies], runs)
    med = statistics.median
    elements = int(sum(p.numel() for p in p1))
    out = {'list': 'reuters-shaped model', 'tensors': len(shapes), 'elements': elements, 'same_bits_after_one_swap': same,
           'lamp_bytes_per_call': 16 * elements, 'torch_bytes_per_call': 24 * elements}
    for n, r, ts in zip(('lamp', 'torch_three_foreach_copies'), reps, times):
        out['%s_ms_median' % n] = med(ts)
        out['%s_reps_per_window' % n] = r
        out['%s_ms_all' % n] = ts
    out['lamp_over_torch_three_foreach_copies'] = out['lamp_ms_median'] / out['torch_three_foreach_copies_ms_median']
    return out


def step_rows(dev, B=32, rounds=10):
    from lamp_amd import optim as O
    from lamp_amd import synthetic
    from lamp_amd import train as T
    seq = pos = tgt = None
    steps = []
    for which in ('plain', 'ema'):
        m, (V, L, T_len, d) = reuters_model(dev)
        if seq is None:
            seq, pos = synthetic.make_batch(B, V, T_len, seed=0)
            seq, pos = seq.to(dev), pos.to(dev)
            tgt = (torch.rand(B, L, device=dev) < 0.05).float()
        params = list(m.get_trainable_parameters())
        optim = O.Adam(params, betas=BETAS, lr=1e-5)
        opt = argparse.Namespace(tgt_vocab_size=L, binary_relevance=True, int_preds=False, int_pred_weight=0.2, attns_loss=False,
                                 matching_mlp=False, decoder='graph', loss_options=None)
        if which == 'ema':
            opt.weight_average = O.WeightAverage(params, kind='ema', decay=0.999)
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
    t_plain, t_ema = times
    ratio = sorted(a / b for a, b in zip(t_ema, t_plain))
    med = statistics.median
    return {'batch': B, 'iters_per_round': 20, 'rounds': rounds, 'optimizer': 'lamp_amd.optim.Adam',
            'plain_step_ms_median': med(t_plain), 'ema_step_ms_median': med(t_ema),
            'ema_over_plain_per_round': {'median': med(ratio), 'min': ratio[0], 'max': ratio[-1]},
            'plain_step_ms_all': t_plain, 'ema_step_ms_all': t_ema}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'weight_avg_bench.json'))
    ap.add_argument('--runs', type=int, default=11)
    ap.add_argument('--skip-step', action='store_true', help='(a), (b) and (c) alone')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_weight_avg.py needs an MI355X: no HIP device visible')
    dev = torch.device('cuda:0')
    result = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'runs': args.runs,
              'timing': 'HIP events around a window of back-to-back calls, per-call ms (host work included), candidates '
                        'alternating; one run of this tool on one MI355X, not a distribution over runs',
              'weight_average': []}
    model, _ = reuters_model(dev)
    shapes = [tuple(p.shape) for p in model.get_trainable_parameters()]
    del model
    for name, sh in (('reuters-shaped model', shapes), ('one 16 M-element tensor', [(16 * 1024 * 1024,)])):
        entry = bench_average(name, sh, dev, args.runs)
        result['weight_average'].append(entry)
        print(json.dumps({k: v for k, v in entry.items() if not k.endswith('_all')}), flush=True)
    result['weight_swap'] = bench_swap(shapes, dev, args.runs)
    print(json.dumps({k: v for k, v in result['weight_swap'].items() if not k.endswith('_all')}), flush=True)
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
