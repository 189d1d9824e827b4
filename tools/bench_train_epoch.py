#!/usr/bin/env python3
"""Training-epoch throughput: the reference's loop body on the pieces that existed before lamp_amd/train.py (route A) against
train_epoch (route B), alternating in one process on a reuters-shaped split (3019 ragged documents, batch 32, dropout 0.1).

    python tools/bench_train_epoch.py [--rounds 5] [--docs 3019] [--batch 32] [--out profiles/train_epoch_bench.json]

  A  per batch: pad + get_gold_binary on the host, one upload, model.train() forward, F.sigmoid +
     F.binary_cross_entropy_with_logits, `.item()`, loss.backward(), torch.optim.Adam (main.py:99's call), predictions to the
     host -- train.py:28-73 as tools/bench_train.py composes its step.
  B  lamp_amd.train.train_epoch with lamp_amd.optim.Adam (and, as B_torch_fused, with torch.optim.Adam(fused=True)).
Also: optimizer.step() alone -- lamp_amd.optim.Adam against torch.optim.Adam foreach and fused=True on the model's own
gradients --, the loss kernel against the ATen sequence it replaces, and the issuing thread's share of a step
(host_issue_ms_per_step: the epoch's issue time / batches, before the final synchronize).  Medians over the rounds; the routes
are interleaved round by round (same box, same process, warm-up first).  One JSON document on stdout and in --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def make_split(n_docs, vocab, n_labels, t_max, seed=0):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(20, t_max - 1, (n_docs,), generator=g).tolist()
    src = [[2] + torch.randint(4, vocab, (n,), generator=g).tolist() + [3] for n in lens]
    tgt = []
    for _ in range(n_docs):
        k = int(torch.randint(1, 5, (1,), generator=g))
        tgt.append([2] + sorted(set((4 + torch.randint(0, n_labels, (k,), generator=g)).tolist())) + [3])
    return src, tgt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--docs', type=int, default=3019)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--dropout', type=float, default=0.1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from lamp_amd import _native as N
    from lamp_amd import hostcpu, optim
    from lamp_amd.data import get_gold_binary
    from lamp_amd.train import TrainBatcher, train_epoch
    hostcpu.fit_intra_op_threads()
    dev = torch.device('cuda:0')
    w = bench.WORKLOADS['reuters']
    L = w['L']
    src, tgt = make_split(a.docs, w['V'], L, w['T'])
    opt_ns = argparse.Namespace(tgt_vocab_size=L, binary_relevance=True, int_preds=False, int_pred_weight=0.2, attns_loss=False,
                                matching_mlp=False, decoder='graph')

    def fresh():
        model = bench.build(w, a.batch, dev)[0]
        for mod in model.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = a.dropout
        return model.train()

    def adam(model, kind):
        params = list(model.get_trainable_parameters())
        if kind == 'lamp':
            return optim.Adam(params, lr=2e-4, betas=(0.9, 0.98))
        return torch.optim.Adam(params, lr=2e-4, betas=(0.9, 0.98), **({'fused': True} if kind == 'fused' else {'foreach': True}))

    def route_a(model, opt, data):
        n = data.n_insts
        preds, targets = torch.zeros(n, L), torch.zeros(n, L)
        total, bi = 0.0, 0
        t0 = time.perf_counter()
        for (seq, pos), adj, t in data:
            gold = get_gold_binary(t[:, 1:], L).to(dev)
            opt.zero_grad()
            pred, _, *_ = model((seq.to(dev), pos.to(dev)), adj, None, gold)
            norm = torch.sigmoid(pred)
            loss = F.binary_cross_entropy_with_logits(pred, gold, reduction='mean')
            total += loss.item()
            loss.backward()
            opt.step()
            lo = bi * a.batch
            preds[lo:lo + seq.size(0)] = norm.detach().cpu()
            targets[lo:lo + seq.size(0)] = gold.cpu()
            bi += 1
        issued = time.perf_counter() - t0
        torch.cuda.synchronize()
        return time.perf_counter() - t0, issued, bi

    def route_b(model, opt, data):
        tl = {}
        t0 = time.perf_counter()
        train_epoch(model, data, opt, opt_ns, device=dev, timeline=tl)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, tl['issued'], len(data)

    routes = {'A': (route_a, 'foreach'), 'B': (route_b, 'lamp'), 'B_torch_fused': (route_b, 'fused')}
    state = {}
    for name, (fn, kind) in routes.items():
        torch.manual_seed(0)
        model = fresh()
        state[name] = (fn, model, adam(model, kind), TrainBatcher(src, tgt, a.batch, shuffle=True, drop_last=True))
    times = {k: [] for k in routes}
    issue = {k: [] for k in routes}
    for r in range(a.rounds + 1):          # round 0 warms every route up
        for name, (fn, model, opt, data) in state.items():
            dt, issued, nb = fn(model, opt, data)
            if r:
                times[name].append(dt)
                issue[name].append(issued / nb * 1e3)
    n_seen = len(state['A'][3]) * a.batch
    out = {'workload': 'reuters-shaped: %d ragged documents, batch %d, dropout %.2f, %d batches per epoch (drop_last)' %
                       (a.docs, a.batch, a.dropout, len(state['A'][3])), 'rounds': a.rounds, 'routes': {}}
    for name in routes:
        med = statistics.median(times[name])
        out['routes'][name] = {'epoch_s_median': med, 'epoch_s_all': times[name], 'samples_per_s': n_seen / med,
                               'spread': (max(times[name]) - min(times[name])) / med,
                               'host_issue_ms_per_step': statistics.median(issue[name])}
    out['B_over_A_epoch_time'] = out['routes']['B']['epoch_s_median'] / out['routes']['A']['epoch_s_median']

    # optimizer.step() alone, on the model's own gradient set
    def time_calls(fn, n=50, warm=5):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        host = (time.perf_counter() - t0) / n
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, host * 1e3

    steps = {k: [] for k in ('lamp', 'foreach', 'fused')}
    model = state['B'][1]
    grads = {p: torch.randn_like(p) * 1e-3 for p in model.get_trainable_parameters()}
    opts = {k: adam(model, k) for k in steps}
    for p, g in grads.items():
        p.grad = g
    for r in range(a.rounds):
        for k in steps:
            steps[k].append(time_calls(opts[k].step))
    out['optimizer_step_ms'] = {k: {'wall': statistics.median(s[0] for s in v), 'host_issue': statistics.median(s[1] for s in v)}
                                for k, v in steps.items()}
    out['lamp_optim_beats_torch_fused'] = out['optimizer_step_ms']['lamp']['wall'] < out['optimizer_step_ms']['fused']['wall']

    # the loss kernel against the ATen sequence (forward and backward to the logits)
    x = torch.randn(a.batch, L, device=dev, requires_grad=True)
    t = (torch.rand(a.batch, L, device=dev) < 0.05).float()

    def aten():
        torch.sigmoid(x)
        loss = F.binary_cross_entropy_with_logits(x, t, reduction='mean')
        torch.autograd.grad(loss, x)

    def kernel():
        N.bce_logits_train([x], [1.0], t)

    loss_ms = {'aten': [], 'lamp': []}
    for r in range(a.rounds):
        loss_ms['aten'].append(time_calls(aten)[0])
        loss_ms['lamp'].append(time_calls(kernel)[0])
    out['loss_ms'] = {k: statistics.median(v) for k, v in loss_ms.items()}
    # the embedding gradient: the atomic scatter-add against the ordered one train_epoch uses, on one batch's token stream
    (seq, _), _, _ = state['B'][3].batch(0)
    seq_d = seq.to(dev)
    dout = torch.randn(seq.numel(), w['d'], device=dev)
    emb_ms = {'atomic': [], 'ordered': []}
    for r in range(a.rounds):
        emb_ms['atomic'].append(time_calls(lambda: N.embed_bwd(seq_d, dout, w['V'], pad_idx=0))[0])
        emb_ms['ordered'].append(time_calls(lambda: N.embed_bwd(seq_d, dout, w['V'], pad_idx=0, ordered=True))[0])
    out['embed_bwd_ms'] = dict({k: statistics.median(v) for k, v in emb_ms.items()}, tokens=int(seq.numel()),
                               note='each call includes zero-filling the [V, d] gradient table')
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
