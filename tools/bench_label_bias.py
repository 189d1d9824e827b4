#!/usr/bin/env python3
"""The weighted label graph (LAMP(label_bias=...)) against today's routes, same process and device (GPU only).

    python tools/bench_label_bias.py [--out profiles/label_bias_bench.json] [--skip-4096] [--only-learn]

1. The label self-attention launch (lamp_sdpa_fwd, no maps, head-fused layout, batch 32, d_k = d_v = 128, 4 heads) with the
   graph as a LAMP_MASK_BIAS_F32 bias (csrc/attention_bias.hip) against the descriptor GraphDecoder hands the library today for
   the same graph -- bit-packed rows with its tile list / sparse-rows flag ('none': no mask at all) -- at L = 90, 159, 983 and
   4096, for 'none' and 'prior' graphs.  At 4096 the prior is the Bernoulli(0.05) graph whose route today is the pair kernel.
   The two are timed alternately, best of the rounds.
2. The reuters-shaped batch-32 forward (samples/s) and one training step (ms) with and without a bias.
3. The learnable bias (LAMP(learn_label_bias=True)): lamp_attn_bias_bwd against lamp_colsum on the same dS [H B = 128, L, L] at
   L = 90, 159 and 983, alternating; and the reuters-shaped training step with a constant bias (the flag off) against the same
   model with the flag on, alternating round by round -- every round's ratio is kept, the report gives their median and range.
   --only-learn runs this part alone and merges it into an existing result file.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lamp_amd import _native as N  # noqa: E402
from lamp_amd import synthetic  # noqa: E402
from lamp_amd.Decoders import GraphDecoder  # noqa: E402

SIZES = [(90, 0.2), (159, 0.2), (983, 0.2), (4096, 0.05)]   # (labels, density of the prior graph)


def time_us_alternating(fns, iters, warm=5, rounds=4):
    """Best time per call of each function, the functions taking turns round by round."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    best = [float('inf')] * len(fns)
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            best[i] = min(best[i], e0.elapsed_time(e1) / iters * 1e3)
    return best


def time_us_rounds(fns, iters, warm=5, rounds=8):
    """Every round's time per call of each function ([fn][round]), the functions taking turns round by round."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[i].append(e0.elapsed_time(e1) / iters * 1e3)
    return times


def ratio_summary(num, den):
    """Median, minimum and maximum of the per-round ratios num[r] / den[r]."""
    r = sorted(a / b for a, b in zip(num, den))
    mid = r[len(r) // 2] if len(r) % 2 else 0.5 * (r[len(r) // 2 - 1] + r[len(r) // 2])
    return dict(median=round(mid, 4), min=round(r[0], 4), max=round(r[-1], 4), rounds=len(r))


def bias_bwd_rows(dev, n_slices=128):
    """lamp_attn_bias_bwd (with the -inf select of a 20 % prior) against lamp_colsum on the same dS."""
    rows = []
    lib = N.lib()
    for L in (90, 159, 983):
        dS = torch.randn(n_slices, L, L, device=dev) * 0.01
        adj = synthetic.make_adjacency(L, 0.2, 0)
        folded = N.pad_bias_rows(torch.zeros(L, L).masked_fill(adj == 0, float('-inf'))).to(dev)
        out = torch.empty(L, L, device=dev)
        nb = lib.lamp_attn_bias_bwd_workspace_bytes(n_slices, L, L)
        assert nb == lib.lamp_colsum_workspace_bytes(n_slices, L * L)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)

        def bwd():
            N.check(lib.lamp_attn_bias_bwd(dS.data_ptr(), n_slices, L, L, 8.0, folded.data_ptr(), folded.size(1), out.data_ptr(), L,
                                           ws.data_ptr(), nb, N.stream()), 'lamp_attn_bias_bwd')

        def colsum():
            N.check(lib.lamp_colsum(dS.data_ptr(), n_slices, L * L, L * L, out.data_ptr(), ws.data_ptr(), nb, N.stream()),
                    'lamp_colsum')
        t_bwd, t_col = time_us_rounds([bwd, colsum], iters=100 if L < 983 else 20)
        row = dict(labels=L, n_slices=n_slices, bytes_read=4 * n_slices * L * L, attn_bias_bwd_us=round(min(t_bwd), 2),
                   colsum_us=round(min(t_col), 2), bwd_over_colsum=ratio_summary(t_bwd, t_col))
        rows.append(row)
        print(row, flush=True)
    return rows


def learn_step_rows(dev, B=32):
    """The reuters-shaped training step: a constant bias (the flag off) against the learnable bias, same weights."""
    from lamp_amd.Models import LAMP
    V, L, T, d, h = 2000, 90, 302, 512, 4
    sd = synthetic.make_state_dict(V, L, T + 1, d, 1024, h, 2, 2, seed=0)
    adj = synthetic.make_adjacency(L, 0.2, 0)
    seq, pos = synthetic.make_batch(B, V, T, seed=0)
    seq, pos = seq.to(dev), pos.to(dev)
    tgt = (torch.rand(B, L, device=dev) < 0.05).float()
    bias = torch.randn(L, L, generator=torch.Generator().manual_seed(0))
    steps = []
    for learn in (False, True):
        m = LAMP(V, L, T + 1, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=1024,
                 d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', label_adj_matrix=adj.clone(), label_mask='prior',
                 dec_dropout2=False, label_bias=bias, learn_label_bias=learn)
        m.load_state_dict(sd)
        m = m.to(dev).train()
        opt = torch.optim.Adam(list(m.get_trainable_parameters()), lr=1e-4, fused=True)

        def f(m=m, opt=opt):
            opt.zero_grad(set_to_none=True)
            logits = m((seq, pos), None, None, tgt)[0]
            F.binary_cross_entropy_with_logits(logits, tgt).backward()
            opt.step()
        steps.append(f)
    t_const, t_learn = time_us_rounds(steps, iters=20, warm=5, rounds=10)
    out = dict(batch=B, constant_bias_step_ms=round(min(t_const) / 1e3, 3), learnable_bias_step_ms=round(min(t_learn) / 1e3, 3),
               learnable_over_constant=ratio_summary(t_learn, t_const))
    print(out, flush=True)
    return out


def descriptors(L, graph, density, dev):
    """-> (today's descriptor or None, the bias descriptor, objects to keep alive) of one graph."""
    adj = synthetic.make_adjacency(L, density, 0) if graph == 'prior' else None
    kw = dict(n_layers=0, n_head=4, n_head2=4, d_k=128, d_v=128, d_word_vec=512, d_model=512, label_mask=graph)
    today = GraphDecoder(L, L, label_adj_matrix=adj.clone() if adj is not None else None, **kw).to(dev)
    biased = GraphDecoder(L, L, label_adj_matrix=adj.clone() if adj is not None else None, label_bias=torch.zeros(L, L), **kw).to(dev)
    return today.label_mask_struct(), biased.label_mask_struct(), (today, biased)


def launches(dev, sizes, B=32, H=4, d=128):
    rows = []
    for L, density in sizes:
        q, k, v = (torch.randn(B, L, H * d, device=dev) for _ in range(3))
        o = torch.empty(B, L, H * d, device=dev)
        lay = N.AttnLayout(*([L * H * d, d, H * d] * 4))
        for graph in ('none', 'prior'):
            m_today, m_bias, keep = descriptors(L, graph, density, dev)

            def call(ms):
                def fn():
                    N.check(N.lib().lamp_sdpa_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), None, B, H, L, L, d, d,
                                                  1.0 / d ** 0.5, C.byref(ms) if ms is not None else None, C.byref(lay), N.stream()),
                            'lamp_sdpa_fwd')
                return fn
            t_today, t_bias = time_us_alternating([call(m_today), call(m_bias)], iters=50 if L < 4096 else 5)
            row = dict(labels=L, graph=graph, density=density if graph == 'prior' else 1.0, batch=B, heads=H, d=d,
                       today_kind=int(m_today.kind) if m_today is not None else 0,
                       today_flags=int(m_today.flags) if m_today is not None else 0,
                       today_tiles=bool(m_today is not None and m_today.tile_list), today_us=round(t_today, 2),
                       bias_us=round(t_bias, 2), bias_over_today=round(t_bias / t_today, 3))
            rows.append(row)
            print(row, flush=True)
            del keep
    return rows


def model_rows(dev, B=32):
    from lamp_amd.Models import LAMP
    V, L, T, d, h = 2000, 90, 302, 512, 4
    sd = synthetic.make_state_dict(V, L, T + 1, d, 1024, h, 2, 2, seed=0)
    adj = synthetic.make_adjacency(L, 0.2, 0)
    seq, pos = synthetic.make_batch(B, V, T, seed=0)
    seq, pos = seq.to(dev), pos.to(dev)
    tgt = (torch.rand(B, L, device=dev) < 0.05).float()
    bias = torch.randn(L, L, generator=torch.Generator().manual_seed(0))
    models, fwd, step = {}, [], []
    for label, kw in (('mask', {}), ('bias', dict(label_bias=bias))):
        m = LAMP(V, L, T + 1, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=1024,
                 d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', label_adj_matrix=adj.clone(), label_mask='prior',
                 dec_dropout2=False, **kw)
        m.load_state_dict(sd)
        models[label] = m.to(dev)

    def make_fwd(m):
        def f():
            with torch.no_grad():
                m((seq, pos), None, None, None)
        return f

    def make_step(m):
        opt = torch.optim.Adam(list(m.get_trainable_parameters()), lr=1e-4)

        def f():
            opt.zero_grad(set_to_none=True)
            logits = m((seq, pos), None, None, tgt)[0]
            F.binary_cross_entropy_with_logits(logits, tgt).backward()
            opt.step()
        return f
    for m in models.values():
        m.eval()
    f_us = time_us_alternating([make_fwd(m) for m in models.values()], iters=30)
    for m in models.values():
        m.train()
    s_us = time_us_alternating([make_step(m) for m in models.values()], iters=10, warm=3)
    out = {label: dict(forward_samples_per_s=round(B / f * 1e6, 1), train_step_ms=round(s / 1e3, 3))
           for label, f, s in zip(models, f_us, s_us)}
    out['bias_over_mask_forward_time'] = round(f_us[1] / f_us[0], 3)
    out['bias_over_mask_train_step_time'] = round(s_us[1] / s_us[0], 3)
    print(out, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'label_bias_bench.json'))
    ap.add_argument('--skip-4096', action='store_true')
    ap.add_argument('--only-learn', action='store_true', help='part 3 alone, merged into the result file if it exists')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    learn = dict(attn_bias_bwd=bias_bwd_rows(dev), reuters_batch32_train_step=learn_step_rows(dev))
    if a.only_learn:
        res = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        res.update(device=torch.cuda.get_device_name(0), torch=torch.__version__, learn_label_bias=learn)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
        print(json.dumps(res))
        return
    sizes = [s for s in SIZES if not (a.skip_4096 and s[0] == 4096)]
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, launches=launches(dev, sizes),
               reuters_batch32=model_rows(dev), learn_label_bias=learn)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
