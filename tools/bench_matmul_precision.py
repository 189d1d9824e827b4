#!/usr/bin/env python3
"""matmul_precision 'highest' against 'high' (bf16x3) and 'bf16x6', same process and box (GPU only).

    python tools/bench_matmul_precision.py [--out profiles/matmul_precision_bench.json] [--rounds 5]

Product build, HIP events, after warm-up; the three precisions alternate inside every round and the medians over the rounds are
reported.  (1) Launch time of lamp_linear_prec_fwd at every GEMM shape of the reuters, bibtex and delicious forwards at batch
32, with its ratio to the fp32 launch (< 1: the split launch is faster).  A multi-segment launch of the forward (K/V of both
decoder layers: 4 segments; Q/K/V: 3) is timed as ONE launch with the segments' weight rows stacked, N = nseg x d: the same
tiles, the same bytes.  (2) The whole forward, samples/s: reuters at fixed T = 302, ragged reuters, bibtex, delicious.
"""
import argparse
import json
import os
import socket
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (WORKLOADS / RAGGED / build: the shapes bench.py measures)
from lamp_amd import _native as N  # noqa: E402

MODES = ('highest', 'high', 'bf16x6')


def event_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def alternate(fns, rounds, iters, warm):
    """fns: {mode: callable}.  Warm every mode, then `rounds` rounds of one timed burst per mode -> {mode: median us}."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    samples = {m: [] for m in fns}
    for _ in range(rounds):
        for m, fn in fns.items():
            samples[m].append(event_us(fn, iters))
    return {m: statistics.median(v) for m, v in samples.items()}


def gemm_shapes(name, B=32):
    """(label, M, N, K, bias, relu, residual) of the linear() launches of one fused eval forward (2 + 2 layers)."""
    w = bench.WORKLOADS[name]
    d, dff, L, T = w['d'], w['dff'], w['L'], w['T']
    tok, lab = B * T, B * L
    rows = [('encoder W1 (layer 1; layer 0 is folded into the tables)', tok, dff, d, True, True, False),
            ('encoder W2 + residual (both layers)', tok, d, dff, True, False, True),
            ('K/V of both decoder layers, 4 segments as N = 4 d', tok, 4 * d, d, False, False, False),
            ('decoder layer 1 query', lab, d, d, False, False, False),
            ('label self-attention Q/K/V, 3 segments as N = 3 d', lab, 3 * d, d, False, False, False)]
    if lab > 12288:   # past the chain launch's reach the row-local tail is separate launches
        rows += [('decoder fc + residual', lab, d, d, False, False, True), ('decoder W1', lab, dff, d, True, True, False),
                 ('decoder W2 + residual', lab, d, dff, True, False, True)]
    return rows


def launches(dev, rounds):
    out = []
    lib = N.lib()
    for name in ('reuters', 'bibtex', 'delicious'):
        for label, M, Nn, K, use_b, relu, use_r in gemm_shapes(name):
            A = torch.randn(M, K, device=dev)
            W = torch.randn(Nn, K, device=dev) / K ** 0.5
            b = torch.randn(Nn, device=dev) if use_b else None
            r = torch.randn(M, Nn, device=dev) if use_r else None
            Cc = torch.empty(M, Nn, device=dev)

            def call(prec):
                def fn():
                    N.check(lib.lamp_linear_prec_fwd(N.ptr(A), M, K, K, N.ptr(W), Nn, K, N.ptr(b), N.ptr(r), Nn if use_r else 0,
                                                     int(relu), N.ptr(Cc), Nn, prec, N.stream()), 'lamp_linear_prec_fwd')
                return fn
            t = alternate({m: call(N.MATMUL_PRECISIONS[m][0]) for m in MODES}, rounds, 30, 5)
            row = dict(workload=name, launch=label, M=M, N=Nn, K=K, fp32_us=round(t['highest'], 2), bf16x3_us=round(t['high'], 2),
                       bf16x6_us=round(t['bf16x6'], 2), x3_over_fp32=round(t['high'] / t['highest'], 3),
                       x6_over_fp32=round(t['bf16x6'] / t['highest'], 3))
            out.append(row)
            print(row, flush=True)
            del A, W, b, r, Cc
    return out


def forwards(dev, rounds, B=32):
    out = []
    for label, name, ragged in (('reuters T=302', 'reuters', False), ('reuters ragged', 'reuters', True), ('bibtex', 'bibtex', False),
                                ('delicious', 'delicious', False)):
        args = argparse.Namespace(ragged=ragged, workload=name, batch=B)
        w, lengths = bench.batch_of_rank(args, bench.WORKLOADS[name], 0)
        model, _, _, seq, pos = bench.build(w, B, dev, seed=0, lengths=lengths, n_max=bench.RAGGED[name][1] if ragged else None)
        src = (seq.to(dev), pos.to(dev))

        def run(mode):
            def fn():
                model.matmul_precision = mode
                with torch.no_grad():
                    return model(src, None, None, None)
            return fn
        fns = {m: run(m) for m in MODES}
        ref = fns['highest']()[0]
        gaps = {m: float((fns[m]()[0] - ref).abs().max()) for m in ('high', 'bf16x6')}
        t = alternate(fns, rounds, 20 if name != 'delicious' else 5, 5)
        row = dict(workload=label, batch=B, T=w['T'], highest_us=round(t['highest'], 1), high_us=round(t['high'], 1),
                   bf16x6_us=round(t['bf16x6'], 1), highest_samples_per_s=round(B / t['highest'] * 1e6, 1),
                   high_samples_per_s=round(B / t['high'] * 1e6, 1), bf16x6_samples_per_s=round(B / t['bf16x6'] * 1e6, 1),
                   high_over_highest_time=round(t['high'] / t['highest'], 3), bf16x6_over_highest_time=round(t['bf16x6'] / t['highest'], 3),
                   max_logit_gap_to_highest=gaps)
        out.append(row)
        print(row, flush=True)
        del model
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'matmul_precision_bench.json'))
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(box=socket.gethostname(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               method='HIP events, product build; fp32 / bf16x3 / bf16x6 alternate inside each of %d rounds, medians' % a.rounds,
               launches=launches(dev, a.rounds), forwards=forwards(dev, a.rounds))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
