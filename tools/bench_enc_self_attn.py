"""What the live encoder self-attention (LAMP(enc_self_attn=True)) costs: forward samples/s and one training
step, live against dead, at the reuters shape (batch 32, d_model 512, 4 heads, 2+2 layers, 90 labels).

    python tools/bench_enc_self_attn.py [--rounds 7] [--iters 20] [--out profiles/enc_self_attn_bench.json]

One process, the product build, HIP events after a warm-up, live and dead alternating round by round, the median over the
rounds.  The dead figure is the yardstick.  `live` is the padded route, `live_packed` the packed route
(LAMP.use_packed_live_encoder, csrc/attention_ragged.hip): their ratio on the ragged workload is the A/B that decides the
default.

The kernel-only time of the encoder self-attention launch comes from a run of its own under the profiler, no counters:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o enc -- python tools/bench_enc_self_attn.py --encoder-only 30
    python tools/bench_enc_self_attn.py --kernel-stats DIR/.../enc_kernel_stats.csv [--out profiles/enc_self_attn_bench.json]

--encoder-only runs nothing but the live encoder (module route) on the ragged workload, so the one attention kernel in the
trace is the encoder's; --kernel-stats reports its mean time against 2 sum_b H plen_b^2 (d_k + d_v) FLOP as a fraction of the
157.3 TFLOP/s fp32-MFMA figure and merges that into the JSON."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lamp_amd import synthetic  # noqa: E402
from lamp_amd.Models import LAMP  # noqa: E402

V, L, T, D, DFF, H, B = 23000, 90, 302, 512, 1024, 4, 32


def model(live, dev, dropout=0.0):
    sd = synthetic.make_state_dict(V, L, T, D, DFF, H, 2, 2, seed=0)
    adj = synthetic.make_adjacency(L, 0.1, seed=0)
    m = LAMP(V, L, T, L, n_layers_enc=2, n_layers_dec=2, n_head=H, n_head2=H, d_word_vec=D, d_model=D, d_inner_hid=DFF,
             d_k=D // H, d_v=D // H, encoder='graph', decoder='graph', dropout=dropout, dec_dropout=dropout, dec_dropout2=False,
             label_adj_matrix=adj, label_mask='prior', enc_self_attn=live)
    m.load_state_dict(sd)
    return m.to(dev)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters   # ms


def alternate(fns, rounds, iters, warmup=5):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, iters))
    return {k: statistics.median(v) for k, v in ms.items()}, ms


PEAK_FP32_MFMA = 157.3e12


def ragged_lengths(g):
    lengths = torch.randint(20, T + 1, (B,), generator=g).tolist()
    lengths[0] = T
    return lengths


def attention_flop(lengths):
    return 2.0 * sum(H * n * n * (2 * D // H) for n in lengths)


def encoder_only(n):
    dev = torch.device('cuda', torch.cuda.current_device())
    m = model(True, dev).eval()
    seq, pos = synthetic.make_batch(B, V, T, lengths=ragged_lengths(torch.Generator().manual_seed(0)), seed=1)
    seq, pos = seq.to(dev), pos.to(dev)
    with torch.no_grad():
        for _ in range(n):
            m.encoder(seq, None, pos)
    torch.cuda.synchronize()


def kernel_stats(path, out_path):
    import csv
    with open(path) as f:
        rows = list(csv.DictReader(f))
    att = [r for r in rows if 'attn' in r['Name']]
    if len(att) != 1:
        raise SystemExit('expected one attention kernel in %s, found %s' % (path, [r['Name'][:60] for r in att]))
    r = att[0]
    calls, total_ns = int(r['Calls']), float(r['TotalDurationNs'])
    mean_s = total_ns / calls * 1e-9
    flop = attention_flop(ragged_lengths(torch.Generator().manual_seed(0)))
    res = {'kernel': r['Name'], 'calls': calls, 'mean_us': mean_s * 1e6, 'flop_live_pairs': flop,
           'tflops': flop / mean_s / 1e12, 'fraction_of_157.3_tflops': flop / mean_s / PEAK_FP32_MFMA,
           'workload': 'ragged_U20_302, batch %d, both encoder layers' % B}
    out = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            out = json.load(f)
    out['kernel_only_rocprofv3'] = res
    with open(out_path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default='profiles/enc_self_attn_bench.json')
    ap.add_argument('--encoder-only', type=int, default=0, help='run only the live encoder this many times (for rocprofv3)')
    ap.add_argument('--kernel-stats', default=None, help="rocprofv3's *_kernel_stats.csv of an --encoder-only run")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out)
    if a.encoder_only:
        return encoder_only(a.encoder_only)
    dev = torch.device('cuda', torch.cuda.current_device())
    g = torch.Generator().manual_seed(0)
    workloads = {'T302_fixed': [T] * B, 'ragged_U20_302': ragged_lengths(g)}
    out = {'device': torch.cuda.get_device_name(dev), 'batch': B, 'shape': dict(V=V, L=L, T=T, d=D, dff=DFF, h=H),
           'rounds': a.rounds, 'iters': a.iters, 'forward': {}, 'packed_vs_padded': "forward[*]['packed_over_padded_time'] (live_packed / live)",
           'kernel_only_rocprofv3': 'not measured (see --kernel-stats)'}
    models = {'live': model(True, dev).eval(), 'dead': model(False, dev).eval(), 'live_packed': model(True, dev).eval()}
    models['live'].use_packed_live_encoder = False      # the A/B: padded against packed on the same tree, whatever the default
    models['live_packed'].use_packed_live_encoder = True
    for name, lengths in workloads.items():
        seq, pos = synthetic.make_batch(B, V, T, lengths=lengths, seed=1)
        src = (seq.to(dev), pos.to(dev))

        def fwd(m):
            def run():
                with torch.no_grad():
                    m(src, None, None, None)
            return run
        med, raw = alternate({k: fwd(m) for k, m in models.items()}, a.rounds, a.iters)
        out['forward'][name] = {k: {'ms_median': med[k], 'samples_per_s': B / med[k] * 1e3, 'ms_rounds': raw[k]} for k in med}
        out['forward'][name]['live_over_dead_time'] = med['live'] / med['dead']
        out['forward'][name]['packed_over_padded_time'] = med['live_packed'] / med['live']
    seq, pos = synthetic.make_batch(B, V, T, lengths=workloads['ragged_U20_302'], seed=1)
    src = (seq.to(dev), pos.to(dev))
    tgt = (torch.rand(B, L, generator=g) < 0.05).float().to(dev)
    steps = {}
    for k in ('live', 'dead'):
        m = model(k == 'live', dev, dropout=0.1).train()
        opt = torch.optim.Adam(list(m.get_trainable_parameters()), betas=(0.9, 0.98), lr=2e-4, fused=True)

        def step(m=m, opt=opt):
            opt.zero_grad()
            logits = m(src, None, None, tgt)[0]
            torch.nn.functional.binary_cross_entropy_with_logits(logits, tgt).backward()
            opt.step()
        steps[k] = step
    med, raw = alternate(steps, a.rounds, max(a.iters // 2, 1))
    out['train_step'] = {k: {'ms_median': med[k], 'ms_rounds': raw[k]} for k in med}
    out['train_step']['live_over_dead_time'] = med['live'] / med['dead']
    os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k not in ('forward', 'train_step')}))
    for name, r in out['forward'].items():
        print('%s: live %.0f samples/s, dead %.0f samples/s, live/dead time x%.2f; live packed %.0f samples/s, packed/padded time '
              'x%.2f' % (name, r['live']['samples_per_s'], r['dead']['samples_per_s'], r['live_over_dead_time'],
                         r['live_packed']['samples_per_s'], r['packed_over_padded_time']))
    print('train step: live %.2f ms, dead %.2f ms' % (out['train_step']['live']['ms_median'], out['train_step']['dead']['ms_median']))


if __name__ == '__main__':
    main()
