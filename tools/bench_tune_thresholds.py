#!/usr/bin/env python3
"""Device time of lamp_tune_thresholds against lamp_ranking_metrics on the same resident matrix, and of
lamp_threshold_counts_vec against lamp_threshold_counts.

    python tools/bench_tune_thresholds.py [--out profiles/tune_thresholds_bench.json] [--runs 11]

Shapes (n x L): 3019 x 90, 3019 x 983, 8000 x 919, 455 024 x 919; uniform scores in [0, 1), 2 % positives.  The two calls of a
pair share the key build and the sort of every label column and differ in the walk over the sorted column, so their times
should be close; tuning at much more than twice the ranking metrics would point at the walk.
  * HIP events on the current stream around a window of `reps` back-to-back calls, after warm-up of every shape and entry; reps
    is chosen per shape so that a window lasts about 20 ms or more (one call at the largest shape);
  * the candidates of a pair alternate window by window in one process; the median of the runs is reported, all runs are kept;
  * the workspace and the outputs are allocated once per shape, outside the windows: the intervals hold the library's own
    launches only;
  * before timing, the tuned result is checked for being identical between two calls.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = ((3019, 90), (3019, 983), (8000, 919), (455024, 919))
WINDOW_MS = 20.0
MAX_REPS = 200


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def pick_reps(fns):
    slowest = max(window(fn, 1) for fn in fns)
    return max(1, min(MAX_REPS, int(WINDOW_MS / max(slowest, 1e-3)) + 1))


def alternate(fns, runs):
    """-> (reps, [per-call ms of every run] per candidate), the candidates alternating window by window."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = pick_reps(fns)
    times = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            times[i].append(window(fn, reps))
    return reps, times


def bench_shape(n, L, dev, runs):
    from lamp_amd import _native as N
    from lamp_amd import metrics as M
    lib = N.lib()
    g = torch.Generator(device=dev).manual_seed(n + L)
    p = torch.rand(n, L, generator=g, device=dev)
    t = (torch.rand(n, L, generator=g, device=dev) < 0.02).float()
    nbytes = lib.lamp_tune_thresholds_workspace_bytes(n, L)
    assert nbytes and nbytes == lib.lamp_ranking_metrics_workspace_bytes(n, L)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tuned = torch.empty((6, L), dtype=torch.int32, device=dev)
    ranked = torch.empty((5, L), dtype=torch.float64, device=dev)
    counts = torch.empty(3 * L + 4 * n, dtype=torch.int32, device=dev)
    lab, ex = counts[:3 * L].view(3, L), counts[3 * L:].view(4, n)
    stream = N.stream()

    def tune(criterion):
        def call():
            N.check(lib.lamp_tune_thresholds(N.ptr(p), L, N.ptr(t), L, n, L, criterion, 0.5, *[N.ptr(tuned[i]) for i in range(6)],
                                             N.ptr(ws), nbytes, stream), 'lamp_tune_thresholds')
        return call

    def rank():
        N.check(lib.lamp_ranking_metrics(N.ptr(p), L, N.ptr(t), L, n, L, 0.5, N.ptr(ranked[0]), N.ptr(ranked[1]), N.ptr(ranked[2]),
                                         N.ptr(ranked[3]), N.ptr(ranked[4]), N.ptr(ws), nbytes, stream), 'lamp_ranking_metrics')

    tune(0)()
    first = tuned.clone()
    tune(0)()
    deterministic = bool(torch.equal(first, tuned))
    thr = first[0].view(torch.float32).clone()

    def scalar():
        N.check(lib.lamp_threshold_counts(N.ptr(p), L, N.ptr(t), L, n, L, 0.5, *[N.ptr(lab[i]) for i in range(3)],
                                          *[N.ptr(ex[i]) for i in range(4)], stream), 'lamp_threshold_counts')

    def vec():
        N.check(lib.lamp_threshold_counts_vec(N.ptr(p), L, N.ptr(t), L, n, L, N.ptr(thr), *[N.ptr(lab[i]) for i in range(3)],
                                              *[N.ptr(ex[i]) for i in range(4)], stream), 'lamp_threshold_counts_vec')

    reps, (a, b, c, d) = alternate([tune(0), rank, tune(1), tune(2)], runs)
    creps, (v, s) = alternate([vec, scalar], runs)
    med = statistics.median
    return {'n': n, 'L': L, 'reps_per_window': reps, 'tune_f1_ms_median': med(a), 'ranking_metrics_ms_median': med(b),
            'tune_youden_ms_median': med(c), 'tune_balance_ms_median': med(d), 'tune_f1_over_ranking_metrics': med(a) / med(b),
            'counts_reps_per_window': creps, 'counts_vec_ms_median': med(v), 'counts_scalar_ms_median': med(s),
            'counts_vec_over_scalar': med(v) / med(s), 'tuned_identical_between_two_calls': deterministic,
            'n_labels_tuned': int((first[5] != 0).sum()), 'workspace_bytes': int(nbytes),
            'tune_f1_ms_all': a, 'ranking_metrics_ms_all': b, 'counts_vec_ms_all': v, 'counts_scalar_ms_all': s}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tune_thresholds_bench.json'))
    ap.add_argument('--runs', type=int, default=11)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_tune_thresholds.py needs an MI355X: no HIP device visible')
    dev = torch.device('cuda:0')
    result = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'runs': args.runs,
              'scores': 'uniform [0, 1), 2 % positives', 'timing': 'HIP events around a window of back-to-back calls, per-call ms',
              'results': []}
    for n, L in SHAPES:
        entry = bench_shape(n, L, dev, args.runs)
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
