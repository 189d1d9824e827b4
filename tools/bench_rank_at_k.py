#!/usr/bin/env python3
"""Device time of lamp_amd.metrics.topk_labels (lamp_topk_labels) against torch.topk on the same resident tensor.

    python tools/bench_rank_at_k.py [--out profiles/rank_at_k_bench.json] [--no-trace] [--runs 11]

Shapes (n x L): 3019 x 90, 3019 x 983, 8000 x 919, 1024 x 4096, 455 024 x 919; k = 5 and k = 64; standard-normal scores.
  * events: HIP events on the current stream around one call, after warm-up, the two candidates alternating in one process;
    the median of the runs is reported (launch overhead and the output allocations are inside the interval: that is what a
    caller waits for).  torch.topk(sorted=True) returns int64 indices in an unspecified tie order; lamp_topk_labels int32
    indices in the order include/lamp_hip.h defines.  rank_at_k (top-k + the figures at every rank) is timed the same way;
  * trace: ONE `rocprofv3 --kernel-trace --stats` child run over every shape: the kernel-only time of lamp_topk_labels per
    (shape, k), read from the dispatch records in launch order, its bytes (n L 4 + the outputs) and their share of the
    8 TB/s HBM figure.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = ((3019, 90), (3019, 983), (8000, 919), (1024, 4096), (455024, 919))
KS = (5, 64)
HBM_GBS = 8000.0
TRACE_RUNS = 5


def make(n, L, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(n, L, generator=g, device=dev)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def bench_shape(n, L, k, dev, runs):
    from lamp_amd import metrics as M
    s = make(n, L, dev)
    t = (torch.rand(n, L, device=dev) < 0.02).float()
    ours = lambda: M.topk_labels(s, k)                       # noqa: E731
    theirs = lambda: torch.topk(s, k, dim=1, sorted=True)    # noqa: E731
    at_k = lambda: M._rank_at_k_buffer(s, t, k)              # noqa: E731
    for _ in range(3):
        ours(), theirs(), at_k()
    torch.cuda.synchronize()
    a, b, c = [], [], []
    for _ in range(runs):
        a.append(timed(ours))
        b.append(timed(theirs))
        c.append(timed(at_k))
    idx, val = ours()
    tv, ti = theirs()
    same_values = bool(torch.equal(val, tv))                 # tie-free normal scores: the values agree; the indices where no tie
    nbytes = n * L * 4 + n * k * 8
    ma, mb = statistics.median(a), statistics.median(b)
    return {'n': n, 'L': L, 'k': k, 'lamp_topk_ms_median': ma, 'torch_topk_ms_median': mb, 'torch_over_lamp': mb / ma,
            'faster': 'lamp_topk_labels' if ma < mb else 'torch.topk', 'rank_at_k_ms_median': statistics.median(c),
            'lamp_topk_ms_all': a, 'torch_topk_ms_all': b, 'bytes': nbytes,
            'event_gbs': nbytes / (ma * 1e-3) / 1e9, 'values_equal_torch': same_values,
            'indices_equal_torch': bool(torch.equal(idx.long(), ti))}


def trace_child():
    from lamp_amd import metrics as M
    dev = torch.device('cuda:0')
    for n, L in SHAPES:
        s = make(n, L, dev)
        for k in KS:
            for _ in range(TRACE_RUNS):
                M.topk_labels(s, k)
        torch.cuda.synchronize()
        del s


def trace():
    exe = shutil.which('rocprofv3') or ('/opt/rocm/bin/rocprofv3' if os.path.exists('/opt/rocm/bin/rocprofv3') else None)
    if exe is None:
        return {'skipped': 'rocprofv3 not found'}
    with tempfile.TemporaryDirectory() as out:
        cmd = [exe, '--kernel-trace', '--stats', '-d', out, '-o', 'p', '-f', 'csv', '--', sys.executable,
               os.path.abspath(__file__), '--trace-child']
        try:
            r = subprocess.run(cmd, capture_output=True, timeout=420)
        except subprocess.TimeoutExpired:
            return {'skipped': 'rocprofv3 sub-run exceeded 420 s'}
        path = None
        for dirpath, _, files in os.walk(out):
            if 'p_kernel_trace.csv' in files:
                path = os.path.join(dirpath, 'p_kernel_trace.csv')
        if r.returncode != 0 or path is None:
            return {'skipped': 'rocprofv3 sub-run failed (exit %d)' % r.returncode}
        rows = [row for row in csv.DictReader(open(path)) if 'topk_labels_kernel' in row.get('Kernel_Name', '')]
    rows.sort(key=lambda row: int(row['Start_Timestamp']))
    if len(rows) != len(SHAPES) * len(KS) * TRACE_RUNS:
        return {'skipped': 'expected %d lamp_topk_labels dispatches, the trace holds %d'
                           % (len(SHAPES) * len(KS) * TRACE_RUNS, len(rows))}
    entries, i = [], 0
    for n, L in SHAPES:
        for k in KS:
            mine = rows[i:i + TRACE_RUNS]
            i += TRACE_RUNS
            us = [(int(row['End_Timestamp']) - int(row['Start_Timestamp'])) / 1e3 for row in mine]
            med = statistics.median(us)
            nbytes = n * L * 4 + n * k * 8
            gbs = nbytes / (med * 1e-6) / 1e9
            name = mine[0]['Kernel_Name'].replace('(anonymous namespace)::', '').split('(')[0].replace('void ', '')
            entries.append({'n': n, 'L': L, 'k': k, 'kernel': name,
                            'kernel_us_median': med, 'kernel_us_all': us, 'bytes': nbytes, 'achieved_gbs': gbs,
                            'frac_of_hbm_peak': gbs / HBM_GBS})
    return {'command': 'rocprofv3 --kernel-trace --stats -- python tools/bench_rank_at_k.py --trace-child',
            'runs_traced': TRACE_RUNS, 'entries': entries,
            'note': 'bytes = n L 4 + the idx and val outputs; achieved GB/s over the median kernel duration, against %.0f GB/s'
                    % HBM_GBS}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rank_at_k_bench.json'))
    ap.add_argument('--runs', type=int, default=11)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--trace-child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_rank_at_k.py needs an MI355X: no HIP device visible')
    if args.trace_child:
        trace_child()
        return
    dev = torch.device('cuda:0')
    result = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'runs': args.runs, 'scores': 'standard normal',
              'results': []}
    for n, L in SHAPES:
        for k in KS:
            entry = bench_shape(n, L, k, dev, args.runs)
            result['results'].append(entry)
            print(json.dumps({key: v for key, v in entry.items() if not key.endswith('_all')}), flush=True)
        torch.cuda.empty_cache()
    if not args.no_trace:
        result['trace'] = trace()
        print('trace', json.dumps(result['trace']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
