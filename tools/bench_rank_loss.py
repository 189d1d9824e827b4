#!/usr/bin/env python3
"""Device time of lamp_rank_loss_train (LSEP, pairwise hinge, pairwise logistic) against lamp_bce_logits_train on the same
matrices, against the same losses written in ATen ops, and inside the training step.

    python tools/bench_rank_loss.py [--out profiles/rank_loss_bench.json] [--runs 11] [--skip-step]

1. The launch.  Shapes (rows x labels): 32 x 90, 32 x 983, 32 x 4096 and 4096 x 919, each with 1 and with 4 matrices, logits
   4 randn, 3 % positives (the train splits' density); plus 32 x 4096 with 50 % positives, the pairwise worst case (2048 x
   2048 pairs per row).  Candidates: lamp_bce_logits_train, and lamp_rank_loss_train with LSEP, HINGE (margin 1) and LOGISTIC,
   each with bce_weight 1 (the BCE share costs what it costs); all write probabilities, every gradient and every row loss
   into buffers allocated once.
   * HIP events on the current stream around a window of `reps` back-to-back calls, after warm-up of every candidate; reps is
     chosen per shape and candidate so that a window lasts about 20 ms (at most 2000 calls);
   * the candidates alternate window by window in one process; the median of the runs is reported, all runs are kept;
   * at the small shapes a kernel is shorter than the host takes to enqueue the next one: the figure is then the rate at
     which launches can be issued, an upper bound of the kernel's time, and equal for all candidates.  It says so
     (`launch_bound`: the BCE figure is within 10 % of the smallest shape's).
   The same losses in ATen ops with autograd's backward are timed in the same alternation with one matrix: LSEP through
   logsumexp, the pairwise logistic loss through its (rows, L, L) difference tensor wherever that tensor stays under 1 GiB.
2. The step.  The reuters-shaped training step (batch 32, 90 labels, d_model 512, 2 + 2 layers, 302 tokens): lamp_amd.train's
   train_batch with LSEP + 1 x BCE against the same model and weights with plain BCE, alternating round by round -- every
   round's ratio is kept, the report gives their median and range.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = tuple((B, L, n, 0.03) for B, L in ((32, 90), (32, 983), (32, 4096), (4096, 919)) for n in (1, 4)) + ((32, 4096, 1, 0.5),)
KINDS = (('lsep', 1, 0.0), ('hinge', 2, 1.0), ('logistic', 3, 0.0))
BCE_WEIGHT = 1.0
ATEN_PAIR_LIMIT = 1 << 30      # bytes of one (rows, L, L) fp32 intermediate
WINDOW_MS = 20.0
MAX_REPS = 2000


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns, runs):
    """-> ([reps per window] per candidate, [per-call ms of every run] per candidate), the candidates alternating window by
    window; every candidate's window is sized from a trial window of its own."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = [max(1, min(MAX_REPS, int(WINDOW_MS / max(window(fn, 5), 1e-4)) + 1)) for fn in fns]
    times = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            times[i].append(window(fn, reps[i]))
    return reps, times


def aten_rows(x, t, kind):
    """R_r + mean BCE of the row, in ATen ops: LSEP by logsumexp over the masked row, LOGISTIC through (rows, L, L)."""
    pos = t > 0.5
    bce = F.binary_cross_entropy_with_logits(x, t, reduction='none').mean(1)
    both = pos.any(1) & (~pos).any(1)
    if kind == 'lsep':
        # (a finite fill: the logsumexp of an empty class stays finite, and so does its gradient under the where)
        z = torch.logsumexp(x.masked_fill(pos, -1e30), 1) + torch.logsumexp((-x).masked_fill(~pos, -1e30), 1)
        return torch.where(both, F.softplus(torch.where(both, z, torch.zeros_like(z)), threshold=1e9), torch.zeros_like(z)) + bce
    d = x.unsqueeze(1) - x.unsqueeze(2)                           # [r, p, n] = x_n - x_p
    pair = pos.unsqueeze(2) & (~pos).unsqueeze(1)
    total = (F.softplus(d, threshold=1e9) * pair).sum((1, 2))
    return total / pair.sum((1, 2)).clamp(min=1) + bce


def bench_shape(B, L, n_mats, density, dev, runs):
    from lamp_amd import _native as N
    lib = N.lib()
    g = torch.Generator(device=dev).manual_seed(B + L + n_mats)
    xs = [torch.randn(B, L, generator=g, device=dev) * 4.0 for _ in range(n_mats)]
    t = (torch.rand(B, L, generator=g, device=dev) < density).float()
    weights = [1.0] + [0.2] * (n_mats - 1)
    probs = torch.empty(B, L, device=dev)
    grads = [torch.empty(B, L, device=dev) for _ in xs]
    rows = torch.empty(n_mats, B, device=dev)
    xp = (ctypes.c_void_p * n_mats)(*[x.data_ptr() for x in xs])
    gp = (ctypes.c_void_p * n_mats)(*[x.data_ptr() for x in grads])
    wp = (ctypes.c_float * n_mats)(*weights)
    stream = N.stream()
    common = (xp, wp, gp, n_mats, t.data_ptr(), B, L, probs.data_ptr(), L, rows.data_ptr(), B)

    def bce():
        N.check(lib.lamp_bce_logits_train(*common, stream), 'lamp_bce_logits_train')

    def rank(code, margin):
        opts = N.RankLossOptions(code, margin, BCE_WEIGHT, 0)

        def call():
            N.check(lib.lamp_rank_loss_train(*common, ctypes.byref(opts), stream), 'lamp_rank_loss_train')
        return call

    fns, names = [bce] + [rank(code, m) for _, code, m in KINDS], ['bce'] + [k for k, _, _ in KINDS]
    agree = {}
    if n_mats == 1:
        leaf = xs[0].clone().requires_grad_(True)
        for kind, code, m in KINDS:
            if kind == 'hinge' or (kind == 'logistic' and B * L * L * 4 > ATEN_PAIR_LIMIT):
                continue

            def aten(kind=kind):
                leaf.grad = None
                aten_rows(leaf, t, kind).mean().backward()
            # the candidates compute what they say: the library's gradient against autograd's
            rank(code, m)()
            aten()
            torch.cuda.synchronize()
            agree['aten_' + kind] = float((grads[0] - leaf.grad).abs().max())
            fns.append(aten)
            names.append('aten_' + kind)
    reps, times = alternate(fns, runs)
    med = statistics.median
    out = {'rows': B, 'labels': L, 'matrices': n_mats, 'positive_density': density, 'positives_per_row_mean': float(t.sum(1).mean()),
           'bce_weight': BCE_WEIGHT, 'bce_ms_median': med(times[0]), 'bce_ms_all': times[0],
           'reps_per_window': dict(zip(names, reps)), 'max_abs_gradient_difference_library_vs_aten': agree}
    for name, ts in list(zip(names, times))[1:]:
        out['%s_ms_median' % name] = med(ts)
        out['%s_over_bce' % name] = med(ts) / med(times[0])
        out['%s_ms_all' % name] = ts
    for kind, _, _ in KINDS:
        if 'aten_' + kind in names:
            out['aten_%s_over_library' % kind] = out['aten_%s_ms_median' % kind] / out['%s_ms_median' % kind]
    return out


def time_ms_rounds(fns, iters, warm, rounds):
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            times[i].append(window(fn, iters))
    return times


def step_rows(dev, B=32, rounds=10):
    """The reuters-shaped training step through lamp_amd.train.train_batch: LSEP + 1 x BCE against BCE."""
    from lamp_amd import synthetic
    from lamp_amd import train as T
    from lamp_amd.Models import LAMP
    V, L, T_len, d, h = 2000, 90, 302, 512, 4
    sd = synthetic.make_state_dict(V, L, T_len + 1, d, 1024, h, 2, 2, seed=0)
    adj = synthetic.make_adjacency(L, 0.2, 0)
    seq, pos = synthetic.make_batch(B, V, T_len, seed=0)
    seq, pos = seq.to(dev), pos.to(dev)
    tgt = (torch.rand(B, L, device=dev) < 0.03).float()
    steps = []
    for rl in (None, T.RankLossOptions('lsep', bce_weight=1.0)):
        m = LAMP(V, L, T_len + 1, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d,
                 d_inner_hid=1024, d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', label_adj_matrix=adj.clone(),
                 label_mask='prior', dec_dropout2=False)
        m.load_state_dict(sd)
        m = m.to(dev).train()
        optim = torch.optim.Adam(list(m.get_trainable_parameters()), lr=1e-5, fused=True)
        opt = argparse.Namespace(tgt_vocab_size=L, binary_relevance=True, int_preds=False, int_pred_weight=0.2, attns_loss=False,
                                 matching_mlp=False, decoder='graph', loss_options=None, rank_loss=rl)
        probs, rows = torch.empty(B, L, device=dev), torch.empty(1, B, device=dev)

        def f(m=m, optim=optim, opt=opt, probs=probs, rows=rows):
            T.train_batch(m, optim, opt, (seq, pos), None, tgt, probs, rows)
        steps.append(f)
    t_bce, t_rank = time_ms_rounds(steps, iters=20, warm=5, rounds=rounds)
    r = sorted(a / b for a, b in zip(t_rank, t_bce))
    return {'batch': B, 'labels': L, 'd_model': d, 'tokens': T_len, 'iters_per_round': 20, 'rounds': rounds,
            'bce_step_ms_median': statistics.median(t_bce), 'lsep_bce_step_ms_median': statistics.median(t_rank),
            'lsep_over_bce_per_round': {'median': statistics.median(r), 'min': r[0], 'max': r[-1]},
            'bce_step_ms_all': t_bce, 'lsep_bce_step_ms_all': t_rank}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rank_loss_bench.json'))
    ap.add_argument('--runs', type=int, default=11)
    ap.add_argument('--skip-step', action='store_true', help='part 1 alone')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_rank_loss.py needs an MI355X: no HIP device visible')
    dev = torch.device('cuda:0')
    result = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'runs': args.runs,
              'inputs': 'logits 4 randn, Bernoulli targets at the stated density, bce_weight 1, hinge margin 1',
              'timing': 'HIP events around a window of back-to-back calls, per-call ms, candidates alternating; one run of this '
                        'tool, not a distribution over runs',
              'launch': []}
    for B, L, n_mats, density in SHAPES:
        entry = bench_shape(B, L, n_mats, density, dev, args.runs)
        result['launch'].append(entry)
        entry['launch_bound'] = entry['bce_ms_median'] < 1.1 * result['launch'][0]['bce_ms_median']
        print(json.dumps({key: v for key, v in entry.items() if not key.endswith('_all')}), flush=True)
    if not args.skip_step:
        result['training_step'] = step_rows(dev)
        print(json.dumps({key: v for key, v in result['training_step'].items() if not key.endswith('_all')}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
