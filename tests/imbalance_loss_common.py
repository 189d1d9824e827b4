"""Shared pieces of the imbalanced-label loss tests (lamp_multilabel_loss_train): the loss family
restated in torch on the CPU -- fp64 with gradients from torch.autograd is the reference, the same function in fp32 is the
yardstick of tests/train_common.py's tolerance rule -- its closed-form gradients, and the cases of the kernel tests."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def f32(v):
    """The value the kernel receives for a parameter: rounded to fp32 (0.05 is not an fp32 number)."""
    return float(np.float32(v))


# name -> (gamma_pos, gamma_neg, clip, has pos_weight)
PARAM_SETS = {
    'pos_weight': (0.0, 0.0, 0.0, True),
    'focal_2': (2.0, 2.0, 0.0, False),
    'gamma_1': (1.0, 1.0, 0.0, False),            # the lower edge of the exponents
    'asl': (0.0, 4.0, f32(0.05), False),          # the published asymmetric setting
    'asl_pos_1': (1.0, 4.0, f32(0.05), False),
    'margin_only': (0.0, 0.0, f32(0.2), False),
    'asl_pos_weight': (0.0, 4.0, f32(0.05), True),
}
# (B, L, n_mats): one lane, the edges of one and of two lane passes, the matrix limit, a long row
SHAPES = [(1, 1, 1), (3, 63, 1), (5, 64, 2), (4, 65, 3), (7, 130, 8), (2, 983, 2)]
PLANTED = (0.0, 30.0, -30.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4)


def loss_elements(x, t, gamma_pos=0.0, gamma_neg=0.0, clip=0.0, pos_weight=None):
    """The family, elementwise, in x's dtype:  t w l+ + (1 - t) l-,  l+ = -ns^g+ log s,  l- = -p^g- log(1 - p),
    p = max(s - m, 0).  log s and log ns are logsigmoid(+-x); without a margin l- is taken from log ns (log1p(-s) loses
    8e-9 of the gradient in fp64); x^0 = 1, 0^0 included (torch.pow's rule)."""
    s, ns = torch.sigmoid(x), torch.sigmoid(-x)
    l_pos = -torch.pow(ns, gamma_pos) * F.logsigmoid(x)
    if clip == 0.0:
        l_neg = -torch.pow(s, gamma_neg) * F.logsigmoid(-x)
    else:
        p = torch.clamp(s - clip, min=0.0)
        l_neg = -torch.pow(p, gamma_neg) * torch.log1p(-p)
    w = 1.0 if pos_weight is None else pos_weight.to(x.dtype)
    return t * w * l_pos + (1.0 - t) * l_neg


def closed_form_gradient(x, t, gamma_pos=0.0, gamma_neg=0.0, clip=0.0, pos_weight=None):
    """d loss_elements / dx as the header writes it (no autograd)."""
    s, ns = torch.sigmoid(x), torch.sigmoid(-x)
    d_pos = -torch.pow(ns, gamma_pos) * (ns - gamma_pos * s * F.logsigmoid(x))
    if clip == 0.0:
        p, omp, log_omp = s, ns, F.logsigmoid(-x)
    else:
        p = torch.clamp(s - clip, min=0.0)
        omp, log_omp = ns + clip, torch.log1p(-p)
    pow_m1 = torch.pow(p, gamma_neg - 1.0) if gamma_neg != 0.0 else torch.zeros_like(p)
    d_neg = s * ns * (torch.pow(p, gamma_neg) / omp - gamma_neg * pow_m1 * log_omp)
    d_neg = torch.where(s > clip, d_neg, torch.zeros_like(d_neg))
    w = 1.0 if pos_weight is None else pos_weight.to(x.dtype)
    return t * w * d_pos + (1.0 - t) * d_neg


def loss_reference(logits, weights, targets, gamma_pos=0.0, gamma_neg=0.0, clip=0.0, pos_weight=None, dtype=torch.float64):
    """-> (probs of matrix 0, [dlogits_k], row_loss (n_mats, B)) by torch on the CPU in `dtype` from the SAME fp32 logits:
    dlogits_k = d( weights[k] * mean(loss_k) ) / d logits[k] by torch.autograd."""
    t = targets.cpu().to(dtype)
    w = None if pos_weight is None else pos_weight.cpu().to(dtype)
    B, L = t.shape
    probs, grads, rows = None, [], []
    for k, (x, wk) in enumerate(zip(logits, weights)):
        x = x.detach().cpu().to(dtype).requires_grad_(True)
        el = loss_elements(x, t, gamma_pos, gamma_neg, clip, w)
        (el.sum() * (torch.tensor(wk, dtype=dtype) / (B * L))).backward()
        if k == 0:
            probs = torch.sigmoid(x.detach())
        grads.append(x.grad)
        rows.append(el.detach().sum(1))
    return probs, grads, torch.stack(rows)


def loss_case(B, L, n_mats, seed, clip=0.0):
    """-> (logits [n_mats x (B, L)], loss weights, targets, pos_weight (L,)): logits 6 randn with 0, +-30, +-88, +-104 and
    +-1e4 planted (spread over every matrix; with room also side by side in the all-zero and in the all-one target row);
    about 10 % positives, row 0 without a positive and row B - 1 with nothing else (B >= 2).  With a margin, a logit within
    1e-3 of logit(clip) is moved away from it: at gamma_neg = 0 the gradient jumps there and the two precisions may
    legitimately stand on different sides, so nothing has to be left out of the comparison."""
    g = torch.Generator().manual_seed(seed)
    logits = [torch.randn(B, L, generator=g) * 6.0 for _ in range(n_mats)]
    targets = (torch.rand(B, L, generator=g) < 0.1).float()
    if B >= 2:
        targets[0] = 0.0
        targets[B - 1] = 1.0
    numel = B * L
    stride = max(1, numel // len(PLANTED))
    for k, x in enumerate(logits):
        flat = x.view(-1)
        for i, v in enumerate(PLANTED):
            flat[(i * stride + k) % numel] = v
        if B >= 2 and L >= len(PLANTED):
            x[0, :len(PLANTED)] = torch.tensor(PLANTED)
            x[B - 1, L - len(PLANTED):] = torch.tensor(PLANTED)
    if clip > 0.0:
        edge = math.log(clip / (1.0 - clip))
        for x in logits:
            near = (x - edge).abs() < 1e-3
            x[near] = edge + 2e-3
    weights = [1.0] + [0.2, 0.5, 0.2, 1.5, 0.2, 0.7, 0.2][:n_mats - 1]
    pos_weight = torch.exp(torch.randn(L, generator=g)) * 3.0          # log-normal about 3: between ~0.2 and ~60
    if L >= 2:
        pos_weight[1] = 100.0                                          # the cap of -pos_weight
    return logits, weights, targets, pos_weight


def count_labels(train_tgt, n_labels):
    """c_j = train samples carrying label j (numpy; targets are [BOS, ids + 4 ..., EOS]; a repeated label counts once)."""
    c = np.zeros(n_labels, dtype=np.int64)
    for sample in train_tgt:
        for j in set(int(v) - 4 for v in sample[1:-1]):
            c[j] += 1
    return c
