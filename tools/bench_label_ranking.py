#!/usr/bin/env python3
"""Device time of lamp_label_ranking (lamp_amd.metrics: LRAP, coverage error, ranking loss, one-error, per-sample AUC) against
lamp_topk_labels(k = 5) + lamp_rank_at_k on the same resident matrices, and against sklearn's three calls on the host.

    python tools/bench_label_ranking.py [--out profiles/label_ranking_bench.json] [--runs 11] [--no-cpu]

Shapes (n x L, share of gold labels): 3019 x 90, 3019 x 983, 8000 x 919, 1024 x 4096 and 455 024 x 919 at 3 %; the dense worst
cases 32 x 4096 and 32 x 32768 at 50 % (work per row is n_pos L compares: lamp_amd/csrc/rank_at_k.hip).  Standard-normal scores.
  * events: HIP events on the current stream around one call (workspace and output allocations inside the interval: that is
    what a caller waits for, short of the copy back), after warm-up, the two candidates alternating in one process; the median
    of the runs is reported.  The two candidates do different work: the top-k pair ranks the head of every row, the label
    ranking every gold label among all L;
  * cpu: label_ranking_average_precision_score, coverage_error and label_ranking_loss of sklearn on THIS host, one process,
    over at most 20 000 rows, scaled up to n (the subset is recorded); skipped with a note where sklearn is absent.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = ((3019, 90, 0.03), (3019, 983, 0.03), (8000, 919, 0.03), (1024, 4096, 0.03), (455024, 919, 0.03),
          (32, 4096, 0.5), (32, 32768, 0.5))
CPU_ROWS = 20000


def make(n, L, density, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    s = torch.randn(n, L, generator=g, device=dev)
    t = (torch.rand(n, L, generator=g, device=dev) < density).float()
    return s, t


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def cpu_seconds(s, t):
    try:
        from sklearn.metrics import coverage_error, label_ranking_average_precision_score, label_ranking_loss
    except ImportError:
        return None
    rows = min(CPU_ROWS, s.size(0))
    sn, tn = s[:rows].double().cpu().numpy(), t[:rows].cpu().numpy()
    out = {'rows_timed': rows}
    for name, fn in (('label_ranking_average_precision_score', label_ranking_average_precision_score),
                     ('coverage_error', coverage_error), ('label_ranking_loss', label_ranking_loss)):
        t0 = time.perf_counter()
        value = float(fn(tn, sn))
        out[name] = {'seconds_timed': time.perf_counter() - t0, 'value_on_the_subset': value}
    out['seconds_timed'] = sum(out[k]['seconds_timed'] for k in list(out) if k != 'rows_timed')
    out['seconds_scaled_to_n'] = out['seconds_timed'] * s.size(0) / rows
    return out


def bench_shape(n, L, density, dev, runs, with_cpu):
    from lamp_amd import metrics as M
    s, t = make(n, L, density, dev)
    ours = lambda: M._label_ranking_buffer(s, t)             # noqa: E731
    rows = lambda: M._label_ranking_buffer(s, t, rows=True)  # noqa: E731
    head = lambda: M._rank_at_k_buffer(s, t, 5)              # noqa: E731  (lamp_topk_labels(k = 5) + lamp_rank_at_k)
    for _ in range(3):
        ours(), rows(), head()
    torch.cuda.synchronize()
    a, b, c = [], [], []
    for _ in range(runs):
        a.append(timed(ours))
        b.append(timed(head))
        c.append(timed(rows))
    figures = M.label_ranking(s, t)
    ma, mb = statistics.median(a), statistics.median(b)
    entry = {'n': n, 'L': L, 'gold_share': density, 'label_ranking_ms_median': ma, 'topk5_rank_at_k_ms_median': mb,
             'label_ranking_over_topk5_rank_at_k': ma / mb, 'label_ranking_with_row_outputs_ms_median': statistics.median(c),
             'label_ranking_ms_per_row': ma / n, 'label_ranking_ms_all': a, 'topk5_rank_at_k_ms_all': b,
             'figures': {k: figures[k] for k in ('LRAP', 'coverage_error', 'ranking_loss', 'one_error', 'instance_AUC')}}
    if with_cpu:
        cpu = cpu_seconds(s, t)
        if cpu is None:
            entry['cpu'] = {'skipped': 'sklearn is not installed on this host'}
        else:
            cpu['sklearn_over_label_ranking'] = cpu['seconds_scaled_to_n'] / (ma * 1e-3)
            entry['cpu'] = cpu
    return entry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'label_ranking_bench.json'))
    ap.add_argument('--runs', type=int, default=11)
    ap.add_argument('--no-cpu', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_label_ranking.py needs an MI355X: no HIP device visible')
    dev = torch.device('cuda:0')
    result = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'runs': args.runs, 'scores': 'standard normal',
              'note': 'one process, one run of this tool; medians of `runs` event intervals per candidate', 'results': []}
    for n, L, density in SHAPES:
        entry = bench_shape(n, L, density, dev, args.runs, not args.no_cpu)
        result['results'].append(entry)
        print(json.dumps({key: v for key, v in entry.items() if not key.endswith('_all')}), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
