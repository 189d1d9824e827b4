#!/usr/bin/env python3
"""Sigmoid against softmax attention, same process and box (GPU only).

    python tools/bench_sigmoid_attn.py [--out profiles/sigmoid_attn_bench.json]

Launch time of lamp_sdpa_act_fwd at the (sample, head) shapes of the three datasets, batch 32, no maps, head-fused layout; then
the reuters-sized batch-32 forward (samples/s) and one training step (ms) with LAMP(dec_attn_type=None | 'sigmoid').
"""
import argparse
import ctypes as C
import json
import os
import socket
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lamp_amd import _native as N  # noqa: E402
from lamp_amd import synthetic  # noqa: E402

SHAPES = [('reuters self', 90, 90, 4, 128), ('reuters enc-dec', 90, 302, 4, 128), ('bibtex self', 159, 159, 4, 128),
          ('bibtex enc-dec', 159, 100, 4, 128), ('delicious self', 983, 983, 8, 128), ('delicious enc-dec', 983, 40, 8, 128)]


def time_us(fn, iters=50, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters * 1e3)
    return best


def launches(dev, B=32):
    rows = []
    for name, lq, lk, H, d in SHAPES:
        q = torch.randn(B, lq, H * d, device=dev)
        k = torch.randn(B, lk, H * d, device=dev)
        v = torch.randn(B, lk, H * d, device=dev)
        o = torch.empty(B, lq, H * d, device=dev)
        lay = N.AttnLayout(lq * H * d, d, H * d, lk * H * d, d, H * d, lk * H * d, d, H * d, lq * H * d, d, H * d)
        t = {}
        for act, label in ((N.LAMP_ATTN_SOFTMAX, 'softmax_us'), (N.LAMP_ATTN_SIGMOID, 'sigmoid_us')):
            def fn():
                N.check(N.lib().lamp_sdpa_act_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), None, B, H, lq, lk, d, d,
                                                  1.0 / d ** 0.5, act, None, C.byref(lay), N.stream()), 'lamp_sdpa_act_fwd')
            t[label] = round(time_us(fn), 2)
        t.update(shape=name, lq=lq, lk=lk, heads=H, d=d, batch=B, sigmoid_over_softmax=round(t['sigmoid_us'] / t['softmax_us'], 3))
        rows.append(t)
        print(t, flush=True)
    return rows


def model_rows(dev, B=32):
    from lamp_amd.Models import LAMP
    V, L, T, d, h = 2000, 90, 302, 512, 4
    sd = synthetic.make_state_dict(V, L, T + 1, d, 1024, h, 2, 2, seed=0)
    adj = synthetic.make_adjacency(L, 0.2, 0)
    seq, pos = synthetic.make_batch(B, V, T, seed=0)
    seq, pos = seq.to(dev), pos.to(dev)
    tgt = (torch.rand(B, L, device=dev) < 0.05).float()
    out = {}
    for label, kw in (('softmax', {}), ('sigmoid', dict(dec_attn_type='sigmoid'))):
        m = LAMP(V, L, T + 1, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=1024,
                 d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', label_adj_matrix=adj.clone(), label_mask='prior',
                 dec_dropout2=False, **kw)
        m.load_state_dict(sd)
        m = m.to(dev).eval()

        def fwd():
            with torch.no_grad():
                m((seq, pos), None, None, None)
        f_us = time_us(fwd, iters=30)
        m.train()
        opt = torch.optim.Adam(list(m.get_trainable_parameters()), lr=1e-4)

        def step():
            opt.zero_grad(set_to_none=True)
            logits = m((seq, pos), None, None, tgt)[0]
            F.binary_cross_entropy_with_logits(logits, tgt).backward()
            opt.step()
        s_us = time_us(step, iters=10, warm=3)
        out[label] = dict(forward_samples_per_s=round(B / f_us * 1e6, 1), train_step_ms=round(s_us / 1e3, 3))
        print(label, out[label], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sigmoid_attn_bench.json'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(box=socket.gethostname(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               launches=launches(dev), reuters_batch32=model_rows(dev))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
