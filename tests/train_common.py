"""Shared pieces of the training-epoch tests: the recorded fixture (tests/golden/train_epoch.npz, made by
tests/golden/make_golden_train.py from the reference's own train_epoch), a synthetic dataset in the reference's on-disk format,
and fp64 restatements of the loss and of the optimizer updates."""
import argparse
import os
import random

import numpy as np
import torch

from conftest import GOLDEN

ADAM_BETAS = (0.9, 0.98)   # main.py:99


def unflatten(flat, off):
    return [[int(v) for v in flat[off[i]:off[i + 1]]] for i in range(len(off) - 1)]


def load_fixture():
    z = np.load(os.path.join(GOLDEN, 'train_epoch.npz'), allow_pickle=False)
    fx = {k: z[k] for k in z.files}
    fx['src'] = unflatten(fx['train_src_flat'], fx['train_src_off'])
    fx['tgt'] = unflatten(fx['train_tgt_flat'], fx['train_tgt_off'])
    fx['sd'] = {k[4:]: torch.from_numpy(fx[k]) for k in z.files if k.startswith('sd__')}
    fx['final32'] = {k[9:]: torch.from_numpy(fx[k]) for k in z.files if k.startswith('final32__')}
    fx['final64'] = {k[9:]: torch.from_numpy(fx[k]) for k in z.files if k.startswith('final64__')}
    return fx


def fixture_tolerance(fx, name):
    """The project's G13 rule: max(1e-4, 3 x the reference's own recorded fp32-vs-fp64 gap)."""
    return max(1e-4, 3.0 * float(fx['gap_' + name]))


def train_opt(n_labels, int_preds=False, int_pred_weight=0.2, attns_loss=False, decoder='graph'):
    return argparse.Namespace(tgt_vocab_size=n_labels, binary_relevance=decoder in ('graph', 'mlp', 'sa_b'), int_preds=int_preds,
                              int_pred_weight=int_pred_weight, attns_loss=attns_loss, matching_mlp=False, decoder=decoder)


def fixture_model(fx, int_preds=False, dropout=0.0):
    from lamp_amd.Models import LAMP
    d, h, L = int(fx['d_model']), int(fx['n_head']), int(fx['tgt_vocab_size'])
    m = LAMP(int(fx['src_vocab_size']), L, int(fx['max_token_seq_len_e']), L, n_layers_enc=2, n_layers_dec=2, n_head=h,
             n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=2 * d, d_k=d // h, d_v=d // h, encoder='graph', decoder='graph',
             dropout=dropout, dec_dropout=dropout, dec_dropout2=False, label_adj_matrix=torch.from_numpy(fx['label_adj_matrix']).clone(),
             label_mask='prior', int_preds=int_preds)
    m.load_state_dict(fx['sd'], strict=not int_preds)
    return m


def synthetic_dataset(n_train=96, n_valid=24, n_test=40, n_words=60, n_labels=11, max_len=14, seed=3):
    """A dataset dict in the reference's on-disk format (utils/preprocess.py:218-232): learnable -- a label is on iff one of
    its two marker words occurs in the document."""
    rng = random.Random(seed)
    src_dict = {'<blank>': 0, '<unk>': 1, '<s>': 2, '</s>': 3}
    src_dict.update({'w%d' % i: 4 + i for i in range(n_words)})
    tgt_dict = {'<blank>': 0, '<unk>': 1, '<s>': 2, '</s>': 3}
    tgt_dict.update({'l%d' % i: 4 + i for i in range(n_labels)})

    def sample(i):
        n = rng.randint(2, max_len)
        words = [rng.randint(0, n_words - 1) for _ in range(n)]
        words[0] = 2 * (i % n_labels)      # every label occurs
        labels = sorted({w // 2 for w in words if w // 2 < n_labels})
        return [2] + [4 + w for w in words] + [3], [2] + [4 + l for l in labels] + [3]

    data = {'settings': argparse.Namespace(max_seq_len=max_len + 2), 'dict': {'src': src_dict, 'tgt': tgt_dict}}
    k = 0
    for name, n in (('train', n_train), ('valid', n_valid), ('test', n_test)):
        items = [sample(k + i) for i in range(n)]
        k += n
        data[name] = {'src': [s for s, _ in items], 'tgt': [t for _, t in items]}
    return data


def bce_reference(logits, weights, targets, dtype=torch.float64):
    """-> (probs of matrix 0, [dlogits_k], row_loss (n_mats, B)) by torch on the CPU in `dtype`, from the SAME fp32 logits:
    sigmoid, the stable loss max(x,0) - x t + log1p(exp(-|x|)) summed per row, and w_k (sigmoid(x) - t) / (B L)."""
    t = targets.cpu().to(dtype)
    B, L = t.shape
    probs, grads, rows = None, [], []
    for k, (x, w) in enumerate(zip(logits, weights)):
        x = x.detach().cpu().to(dtype)
        s = torch.sigmoid(x)
        if k == 0:
            probs = s
        grads.append((s - t) * (torch.tensor(w, dtype=dtype) / (B * L)))
        rows.append((torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).sum(1))
    return probs, grads, torch.stack(rows)


def adam_reference(p, grads, lrs, betas=ADAM_BETAS, eps=1e-8, m=None, v=None, step0=0):
    """fp64 evaluation of torch.optim.Adam's formula (no weight decay, no amsgrad) over a sequence of gradients / learning rates."""
    p = p.detach().cpu().double().clone()
    m = torch.zeros_like(p) if m is None else m.detach().cpu().double().clone()
    v = torch.zeros_like(p) if v is None else v.detach().cpu().double().clone()
    b1, b2 = betas
    for i, (g, lr) in enumerate(zip(grads, lrs)):
        g = g.detach().cpu().double()
        step = step0 + i + 1
        m = m + (g - m) * (1 - b1)
        v = v * b2 + (1 - b2) * g * g
        denom = v.sqrt() / (1 - b2 ** step) ** 0.5 + eps
        p = p - lr / (1 - b1 ** step) * m / denom
    return p, m, v


def ulp32(x):
    """One fp32 unit in the last place at |x| (elementwise, float64 tensor)."""
    a = x.detach().cpu().double().abs().clamp(min=2.0 ** -126).float()
    return (torch.nextafter(a, torch.full_like(a, float('inf'))) - a).double()


def within(got, want64, gap, what):
    """|got - want| <= max(1 fp32 ulp at the value, 4 x gap) elementwise (the issue's rule for the two kernels); NaNs must
    coincide.  -> the largest violation ratio, asserted <= 1."""
    got, want64 = got.detach().cpu().double(), want64.detach().cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(want64)), what
    ok = ~torch.isnan(want64)
    err = (got - want64).abs()[ok]
    tol = torch.maximum(ulp32(want64)[ok], torch.full_like(err, 4.0 * gap))
    worst = float((err / tol).max()) if err.numel() else 0.0
    print('%s: max |err| %.3e, 4 x torch fp32 gap %.3e, worst err / tol %.3f' % (what, float(err.max()) if err.numel() else 0.0,
                                                                                 4.0 * gap, worst))
    assert worst <= 1.0, (what, worst)
    return worst


# ---- the cases of the kernel tests and their yardstick: torch's own fp32 CPU result against fp64 on the same fp32 inputs ----
BCE_CASES = [(32, 90, 1), (32, 159, 2), (32, 983, 5), (1, 90, 2), (7, 37, 1), (5, 1, 2)]


def gap(a32, a64):
    return float((a32.double() - a64).abs().max())


def bce_case(B, L, n_mats, seed):
    g = torch.Generator().manual_seed(seed)
    logits = [torch.randn(B, L, generator=g) * 4.0 for _ in range(n_mats)]
    logits[0][0, 0] = 30.0          # saturated either way, and next to t = 1
    logits[0][0, L - 1] = -30.0
    targets = (torch.rand(B, L, generator=g) < 0.1).float()
    targets[0, 0] = 1.0
    weights = [1.0] + [0.2, 0.5, 0.2, 1.5][:n_mats - 1]
    return logits, weights, targets


SIZES = (1, 3, 4095, 3 * 4096 + 5)


def optim_case(seed, n_steps):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g) for n in SIZES] + [torch.randn(1001, generator=g)]
    grads = []
    for _ in range(n_steps):
        step = []
        for p in params:
            gr = torch.randn(p.shape, generator=g) * 0.1
            gr[::7] *= 1e-7          # gradients near eps: where Adam's division amplifies rounding
            gr[::11] = 0.0
            step.append(gr)
        grads.append(step)
    return params, grads


def torch_adam_fp32(params, grads, lrs):
    """torch's own fp32 Adam (foreach) on the CPU over the case's gradients -> (parameters, optimizer)."""
    cpu = [torch.nn.Parameter(p.clone()) for p in params]
    ref = torch.optim.Adam(cpu, betas=ADAM_BETAS, lr=lrs[0], foreach=True)
    for i in range(len(lrs)):
        ref.param_groups[0]['lr'] = lrs[i]
        for p, gr in zip(cpu, grads[i]):
            p.grad = gr.clone()
        ref.step()
    return cpu, ref
