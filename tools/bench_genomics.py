#!/usr/bin/env python3
"""The one-hot genomics encoder on a DeepSEA-shaped synthetic workload: V 9, T 1000, 919 labels, d 512,
d_ff 1024, 4 heads, 2+2 layers, batch 32, label mask 'none' (the prior graph of synthetic.make_adjacency is passed and
unused, as the reference does with label_mask='none').

    python tools/bench_genomics.py [--steps 20] [--warmup 5]

Prints one JSON line:
  forward_samples_per_s   LAMP(onehot=True).forward in eval mode, synchronised, after warm-up
  conv2_kernel_us         conv_window_kernel's average duration from a separate `rocprofv3 --kernel-trace --stats` run of
                          this script (--inner-conv2), and its fraction of the 157.3 TFLOP/s fp32-MFMA roof
  train_step_ms           one forward + backward in train() mode (dropout 0.1)
  conv2_ab                same-box, alternating A/B of conv2 + its epilogue: the new implicit-GEMM kernel (lamp_conv_window_fwd)
                          against the existing-code composition -- lamp_gemm over the overlapping window view of the padded input,
                          then a pointwise epilogue (b2, ReLU, the position rows)
"""
import argparse
import csv
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from lamp_amd import _native as N, synthetic  # noqa: E402
from lamp_amd.Models import LAMP  # noqa: E402

V, T, L, D, DFF, H, B = 9, 1000, 919, 512, 1024, 4, 32
ROOF_TFLOPS = 157.3
T2 = T // 2
CONV2_FLOP = 2.0 * B * T2 * D * 16 * D


def build(dropout=0.0):
    torch.manual_seed(0)
    adj = synthetic.make_adjacency(L, 0.05, seed=0)
    m = LAMP(V, L, T, L, n_layers_enc=2, n_layers_dec=2, n_head=H, n_head2=H, d_word_vec=D, d_model=D, d_inner_hid=DFF,
             d_k=D // H, d_v=D // H, encoder='graph', decoder='graph', dropout=dropout, dec_dropout=dropout,
             dec_dropout2=False, onehot=True, label_mask='none', label_adj_matrix=adj)
    m.load_state_dict(synthetic.make_onehot_state_dict(L, T, D, DFF, H, 2, 2, seed=0))
    seq, pos = synthetic.make_batch(B, V, T, seed=0)
    return m.cuda(), seq.cuda(), pos.cuda()


def conv2_operands(m, seq, pos):
    enc = m.encoder
    with torch.no_grad():
        t1 = N.onehot_tap_table(enc.src_word_emb.weight, enc.conv1.weight)
        w2 = N.f32c(enc.conv2.weight)
        fe = N.onehot_frontend(t1, enc.conv1.bias, w2, enc.conv2.bias)
        xpad = N.onehot_front_fwd(seq, fe, D)
    return dict(xpad=xpad, pack=N.conv_pack(w2), b2=enc.conv2.bias.detach(), pos_w=enc.position_enc.weight.detach(), pos=pos,
                keep=(t1, w2, fe))


def conv2_new(o):
    return N.conv_window(o['xpad'], B, T2, T2 + 16, o['pack'], o['b2'], True, o['pos_w'], o['pos'])


def conv2_composed(o, y_all):
    """lamp_gemm (strided descriptor) over the overlapping window view: row r of A = the 16 d floats from padded row r
    (row stride d), all B (T2 + 16) rows; then a pointwise epilogue: + b2, ReLU, keep the output rows, + the position rows.
    (The tile GEMM behind lamp_linear_fwd refuses lda < K, so it cannot read the overlapping view.)"""
    Tp = T2 + 16
    win = o['xpad'].as_strided((B * Tp, 16 * D), (D, 1))
    N.matmul_nt(win, o['pack'].view(D, 16 * D), out=y_all)
    y = torch.relu(y_all.view(B, Tp, D)[:, :T2] + o['b2'])
    return y + torch.nn.functional.embedding(o['pos'][:, :T2], o['pos_w'])


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def kernel_trace():
    exe = shutil.which('rocprofv3') or ('/opt/rocm/bin/rocprofv3' if os.path.exists('/opt/rocm/bin/rocprofv3') else None)
    if exe is None:
        return {'skipped': 'rocprofv3 not found'}
    out = tempfile.mkdtemp(prefix='lamp_genomics_trace_')
    try:
        r = subprocess.run([exe, '--kernel-trace', '--stats', '-d', out, '-o', 'p', '-f', 'csv', '--', sys.executable,
                            os.path.abspath(__file__), '--inner-conv2'], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                           timeout=300, cwd='/tmp')
        path = os.path.join(out, 'p_kernel_stats.csv')
        if r.returncode != 0 or not os.path.exists(path):
            return {'skipped': 'rocprofv3 sub-run failed (exit %d)' % r.returncode}
        with open(path) as f:
            rows = [x for x in csv.DictReader(f) if 'conv_window_kernel' in x['Name']]
    finally:
        shutil.rmtree(out, ignore_errors=True)
    if not rows:
        return {'skipped': 'no conv_window_kernel in the trace'}
    us = float(rows[0]['AverageNs']) / 1e3
    return {'conv2_kernel_us': us, 'calls': int(rows[0]['Calls']), 'conv2_tflops': CONV2_FLOP / us / 1e6,
            'conv2_frac_of_fp32_mfma_roof': CONV2_FLOP / us / 1e6 / ROOF_TFLOPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--ab-rounds', type=int, default=8)
    ap.add_argument('--inner-conv2', action='store_true', help='(the profiled sub-run) conv2 alone, 30 launches')
    args = ap.parse_args()
    m, seq, pos = build()
    o = conv2_operands(m, seq, pos)
    if args.inner_conv2:
        for _ in range(30):
            conv2_new(o)
        torch.cuda.synchronize()
        return
    res = {'workload': 'deepsea-shaped onehot: V 9, T 1000, L 919, d 512, dff 1024, 4 heads, 2+2 layers, batch 32',
           'conv2_gflop_per_forward': CONV2_FLOP / 1e9}

    # conv2 A/B, alternating rounds; both routes' results compared first
    y_all = torch.empty(B * (T2 + 16), D, device='cuda')
    a, b = conv2_new(o).view(B, T2, D), conv2_composed(o, y_all)
    res['conv2_ab_max_abs_diff'] = float((a - b).abs().max())
    for _ in range(3):
        conv2_new(o)
        conv2_composed(o, y_all)
    new_ms, old_ms = [], []
    for _ in range(args.ab_rounds):
        new_ms.append(timed(lambda: conv2_new(o), 5))
        old_ms.append(timed(lambda: conv2_composed(o, y_all), 5))
    new_ms.sort()
    old_ms.sort()
    res['conv2_ab'] = {'new_kernel_ms_median': new_ms[len(new_ms) // 2], 'composed_ms_median': old_ms[len(old_ms) // 2],
                       'new_kernel_ms': new_ms, 'composed_ms': old_ms,
                       'speedup_new_over_composed': old_ms[len(old_ms) // 2] / new_ms[len(new_ms) // 2]}
    del y_all

    # eval forward
    m.eval()
    with torch.no_grad():
        for _ in range(args.warmup):
            m((seq, pos), None, None, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m((seq, pos), None, None, None)
        torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    res['forward_ms'] = dt * 1e3
    res['forward_samples_per_s'] = B / dt

    # one training step (forward + backward), dropout 0.1
    mt, _, _ = build(dropout=0.1)
    mt.train()
    w = torch.randn(B, L, device='cuda')
    for _ in range(2):
        (mt((seq, pos), None, None, None)[0] * w).sum().backward()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_train = 5
    for _ in range(n_train):
        (mt((seq, pos), None, None, None)[0] * w).sum().backward()
    torch.cuda.synchronize()
    res['train_step_ms'] = (time.perf_counter() - t0) / n_train * 1e3
    del mt, m, o
    torch.cuda.empty_cache()

    res['kernel_trace'] = kernel_trace()
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
