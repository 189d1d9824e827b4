#!/usr/bin/env python3
"""Device time of lamp_amd.metrics.compute_metrics against the reference's three sklearn calls per label.

    python tools/bench_ranking_metrics.py [--out profiles/ranking_metrics_bench.json] [--no-trace] [--shapes reuters,valid,test]

Shapes: reuters (3019 x 90), DeepSEA valid (8000 x 919), DeepSEA test (455 024 x 919); synthetic scores, about 2 % positives.
  * device: compute_metrics on device-resident inputs, HIP events on the current stream, after warm-up, median of several runs
    (the two result copies and the host aggregation are inside the interval: that is what a caller waits for);
  * cpu: roc_auc_score + precision_recall_curve / auc + precision_recall_curve per label, as utils/evals.py:208-298 calls
    them, one thread, on THIS host; over a subset of the labels at the large shapes, scaled up (the subset is recorded).
    sklearn is used here only; skipped with a note where it is absent;
  * trace: ONE `rocprofv3 --kernel-trace --stats` child run of the largest shape: per-kernel time, each sort pass's achieved
    GB/s against the 8 TB/s HBM figure, the shares of key build / sort / walk.
"""
import argparse
import csv
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = {'reuters': (3019, 90), 'valid': (8000, 919), 'test': (455024, 919)}
HBM_GBS = 8000.0
TRACE_RUNS = 3


def make(n, L, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    t = (torch.rand(n, L, generator=g, device=dev) < 0.02).float()
    p = torch.sigmoid(torch.randn(n, L, generator=g, device=dev) * 1.5 + (t - 0.5) * 1.5 - 3.0)
    return p, t


def device_ms(p, t, runs):
    from lamp_amd import metrics as M
    M.compute_metrics(p, t, 0.0)      # warm-up (allocator, LDS attribute, page faults of the workspace)
    M.compute_metrics(p, t, 0.0)
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m = M.compute_metrics(p, t, 0.0)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms, m


def cpu_seconds(p, t, labels):
    try:
        from sklearn import metrics as skm
    except ImportError:
        return None
    pn, tn = p[:, :labels].cpu().numpy(), t[:, :labels].cpu().numpy()
    t0 = time.perf_counter()
    for l in range(labels):
        if tn[:, l].min() == tn[:, l].max():
            continue
        skm.roc_auc_score(tn[:, l], pn[:, l])
        prec, rec, _ = skm.precision_recall_curve(tn[:, l], pn[:, l], pos_label=1)
        skm.auc(rec, prec)
        skm.precision_recall_curve(tn[:, l], pn[:, l], pos_label=1)
    return time.perf_counter() - t0


def trace_child(name):
    from lamp_amd import metrics as M
    dev = torch.device('cuda:0')
    n, L = SHAPES[name]
    p, t = make(n, L, dev)
    for _ in range(TRACE_RUNS):
        M.compute_metrics(p, t, 0.0)
    torch.cuda.synchronize()


def trace(name):
    exe = shutil.which('rocprofv3') or ('/opt/rocm/bin/rocprofv3' if os.path.exists('/opt/rocm/bin/rocprofv3') else None)
    if exe is None:
        return {'skipped': 'rocprofv3 not found'}
    n, L = SHAPES[name]
    with tempfile.TemporaryDirectory() as out:
        cmd = [exe, '--kernel-trace', '--stats', '-d', out, '-o', 'p', '-f', 'csv', '--', sys.executable,
               os.path.abspath(__file__), '--trace-child', name]
        try:
            r = subprocess.run(cmd, capture_output=True, timeout=420)
        except subprocess.TimeoutExpired:
            return {'skipped': 'rocprofv3 sub-run exceeded 420 s'}
        path = None
        for dirpath, _, files in os.walk(out):
            if 'p_kernel_stats.csv' in files:
                path = os.path.join(dirpath, 'p_kernel_stats.csv')
        if r.returncode != 0 or path is None:
            return {'skipped': 'rocprofv3 sub-run failed (exit %d)' % r.returncode}
        rows = list(csv.DictReader(open(path)))
    keys_bytes = 4.0 * n * L
    # bytes a launch has to move at least: (reads, writes) in units of the key matrix; the key build reads two fp32 matrices
    traffic = {'metric_keys_kernel': 3.0, 'radix_hist_kernel': 1.0, 'radix_scatter_kernel': 2.0, 'curve_walk_kernel': 1.0,
               'sort_lds_kernel': 2.0, 'threshold_counts_kernel': 2.0}
    kernels, total = {}, 0.0
    for row in rows:
        short = row['Name'].replace('(anonymous namespace)::', '').split('(')[0].replace('void ', '').replace('lamp::', '')
        if short not in traffic and short != 'radix_scan_kernel':
            continue
        calls, avg_us = int(row['Calls']), float(row['AverageNs']) / 1e3
        per_call = calls / TRACE_RUNS
        entry = {'launches_per_call': per_call, 'avg_us': avg_us, 'us_per_call': avg_us * per_call}
        if short in traffic:
            entry['min_bytes'] = traffic[short] * keys_bytes
            entry['achieved_gbs'] = traffic[short] * keys_bytes / (avg_us * 1e-6) / 1e9
            entry['frac_of_hbm_peak'] = entry['achieved_gbs'] / HBM_GBS
        kernels[short] = entry
        total += entry['us_per_call']
    share = lambda names: sum(kernels[k]['us_per_call'] for k in names if k in kernels) / total if total else None  # noqa: E731
    return {'command': 'rocprofv3 --kernel-trace --stats -- python tools/bench_ranking_metrics.py --trace-child %s' % name,
            'shape': [n, L], 'runs_traced': TRACE_RUNS, 'kernels': kernels, 'kernel_us_per_call': total,
            'share': {'key_build': share(['metric_keys_kernel']),
                      'sort': share(['radix_hist_kernel', 'radix_scan_kernel', 'radix_scatter_kernel', 'sort_lds_kernel']),
                      'walk': share(['curve_walk_kernel']), 'threshold_counts': share(['threshold_counts_kernel'])},
            'note': 'one sort pass = radix_hist + radix_scan + radix_scatter; achieved GB/s = the least bytes the launch must '
                    'move (key matrix reads + writes) over its mean duration, against %.0f GB/s' % HBM_GBS}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ranking_metrics_bench.json'))
    ap.add_argument('--shapes', default='reuters,valid,test')
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--trace-child', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_ranking_metrics.py needs an MI355X: no HIP device visible')
    if args.trace_child:
        trace_child(args.trace_child)
        return
    dev = torch.device('cuda:0')
    result = {'device': torch.cuda.get_device_name(0), 'positives': 0.02, 'shapes': {}}
    names = [s for s in args.shapes.split(',') if s]
    for name in names:
        n, L = SHAPES[name]
        p, t = make(n, L, dev)
        ms, m = device_ms(p, t, args.runs if n < 100000 else max(3, args.runs // 2))
        labels = L if n * L <= 3019 * 90 else (64 if n <= 8000 else 8)
        cpu = cpu_seconds(p, t, labels)
        entry = {'n': n, 'L': L, 'device_ms_median': statistics.median(ms), 'device_ms_all': ms,
                 'meanAUC': m['meanAUC'], 'meanAUPR': m['meanAUPR'], 'meanFDR': m['meanFDR']}
        if cpu is None:
            entry['cpu'] = {'skipped': 'sklearn is not installed on this host'}
        else:
            entry['cpu'] = {'labels_timed': labels, 'seconds_timed': cpu, 'seconds_scaled_to_L': cpu * L / labels,
                            'threads': 1, 'calls': 'roc_auc_score, precision_recall_curve + auc, precision_recall_curve'}
            entry['speedup_vs_cpu_scaled'] = cpu * L / labels / (statistics.median(ms) * 1e-3)
        result['shapes'][name] = entry
        print(name, json.dumps(entry), flush=True)
        del p, t
        torch.cuda.empty_cache()
    if not args.no_trace and names:
        result['trace'] = trace(max(names, key=lambda s: SHAPES[s][0] * SHAPES[s][1]))
        print('trace', json.dumps(result['trace']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
