"""Shared pieces of the ranking-loss tests (lamp_rank_loss_train): LSEP and the pairwise hinge and
logistic losses restated in torch on the CPU -- fp64 with gradients from torch.autograd is the reference, the same function in
fp32 is the yardstick of tests/train_common.py's tolerance rule -- a brute-force double loop over the pairs for the
reference's own check, and the cases of the kernel tests."""
import functools
import math

import torch
import torch.nn.functional as F

from imbalance_loss_common import PLANTED

KINDS = ('lsep', 'hinge', 'logistic')
# (rows, L, n_mats): one column, one pair, the edges of one and of two lane passes, several matrices, the reuters and delicious
# widths, the widest row the pair kinds serve
SHAPES = [(1, 1, 1), (3, 2, 1), (4, 63, 1), (5, 64, 2), (7, 65, 3), (32, 90, 1), (9, 983, 2), (5, 4096, 1)]
GRID = 2.0 ** -10                       # the HINGE cases' logits are multiples of it
HINGE_MARGIN = 1.0 + 2.0 ** -11         # ... and their margin lies half a step off it: |a_pn| >= 2^-11 for every pair
DENSITY = 0.03


def softplus(d):
    """max(d, 0) + log1p(exp(-|d|)), the stable form in d's dtype, as -logsigmoid(-d): torch evaluates logsigmoid as
    min(x, 0) - log1p(exp(-|x|)) and gives it its closed-form derivative.  (Written out with clamp and abs, autograd returns a
    subgradient at d = 0 exactly -- 0 or 1 where the derivative is 1/2 -- and the cases plant equal logits; F.softplus
    switches to the identity above 20.)"""
    return -F.logsigmoid(-d)


def bce_elements(x, t):
    """max(x, 0) - x t + log1p(exp(-|x|)) as -(t log s + (1 - t) log(1 - s)) from logsigmoid(+-x), for the same reason."""
    return -(t * F.logsigmoid(x) + (1.0 - t) * F.logsigmoid(-x))


def rank_row(x, pos, kind, margin):
    """The ranking term R of ONE row, in x's dtype: x (L,), pos (L,) bool.  An empty class gives 0 (on the graph)."""
    xp, xn = x[pos], x[~pos]
    if xp.numel() == 0 or xn.numel() == 0:
        return x.sum() * 0.0
    if kind == 'lsep':
        return softplus(torch.logsumexp(xn, 0) + torch.logsumexp(-xp, 0))
    d = xn.unsqueeze(0) - xp.unsqueeze(1)                     # (n_p, n_n): x_n - x_p, the difference first
    if kind == 'hinge':
        return torch.relu(torch.tensor(margin, dtype=x.dtype) + d).mean()      # (relu's gradient at 0 is 0: active iff > 0)
    if kind == 'logistic':
        return softplus(d).mean()
    raise ValueError(kind)


def rank_reference(logits, weights, targets, kind, margin=0.0, bce_weight=0.0, dtype=torch.float64):
    """-> (probs of matrix 0, [dlogits_k], row_loss (n_mats, B)) by torch on the CPU in `dtype` from the SAME fp32 logits:
    row_loss = R_r + bce_weight * bce_row_r / L, dlogits_k = d( weights[k] * mean_r row_loss ) / d logits[k] by autograd."""
    t = targets.cpu().to(dtype)
    pos = targets.cpu() > 0.5
    B, L = t.shape
    probs, grads, rows = None, [], []
    for k, (x, wk) in enumerate(zip(logits, weights)):
        x = x.detach().cpu().to(dtype).requires_grad_(True)
        row = torch.stack([rank_row(x[r], pos[r], kind, margin) for r in range(B)])
        if bce_weight != 0.0:
            row = row + torch.tensor(bce_weight, dtype=dtype) * bce_elements(x, t).sum(1) / L
        (row.sum() * (torch.tensor(wk, dtype=dtype) / B)).backward()
        if k == 0:
            probs = torch.sigmoid(x.detach())
        grads.append(x.grad)
        rows.append(row.detach())
    return probs, grads, torch.stack(rows)


def closed_form_row(x, pos, kind, margin):
    """(R, dR/dx) of one row from the formulas include/lamp_hip.h states, vectorised, no autograd: x (L,) fp64, pos (L,) bool."""
    g = torch.zeros_like(x)
    xp, xn = x[pos], x[~pos]
    if xp.numel() == 0 or xn.numel() == 0:
        return x.new_zeros(()), g
    if kind == 'lsep':
        lse_n, lse_p = torch.logsumexp(xn, 0), torch.logsumexp(-xp, 0)
        z = lse_n + lse_p
        g[~pos] = torch.sigmoid(z) * torch.exp(xn - lse_n)
        g[pos] = -torch.sigmoid(z) * torch.exp(-xp - lse_p)
        return -F.logsigmoid(-z), g
    d = xn.unsqueeze(0) - xp.unsqueeze(1)
    pairs = d.numel()
    if kind == 'hinge':
        a = margin + d
        w = (a > 0).to(x.dtype)                                # active iff a_pn > 0
        R = (a * w).sum() / pairs
    else:
        w = torch.sigmoid(d)
        R = (torch.clamp(d, min=0) + torch.log1p(torch.exp(-d.abs()))).sum() / pairs
    g[~pos] = w.sum(0) / pairs
    g[pos] = -w.sum(1) / pairs
    return R, g


def brute_force_row(x, pos, kind, margin):
    """R and dR/dx of one row by a double loop over the pairs in Python floats (fp64), straight from the definitions; LSEP
    as the naive log1p(sum sum exp) -- for moderate logits only."""
    L = len(x)
    P = [i for i in range(L) if pos[i]]
    Nn = [i for i in range(L) if not pos[i]]
    g = [0.0] * L
    if not P or not Nn:
        return 0.0, g
    total = 0.0
    for p in P:
        for n in Nn:
            d = x[n] - x[p]
            if kind == 'lsep':
                e = math.exp(d)
                total += e
                g[n] += e
                g[p] -= e
            elif kind == 'hinge':
                a = margin + d
                if a > 0.0:
                    total += a
                    g[n] += 1.0
                    g[p] -= 1.0
            else:
                total += max(d, 0.0) + math.log1p(math.exp(-abs(d)))
                s = 1.0 / (1.0 + math.exp(-d))
                g[n] += s
                g[p] -= s
    if kind == 'lsep':
        return math.log1p(total), [v / (1.0 + total) for v in g]
    pairs = len(P) * len(Nn)
    return total / pairs, [v / pairs for v in g]


def rank_targets(B, L, g, density=DENSITY):
    """Bernoulli(density) with the planted rows, as many as B has room for: row 0 without a positive, row B - 1 with nothing
    else, row 1 with column 0 as its only positive, row 2 with column L - 1, and at L = 4096 row 3 half positive (every
    other column: the largest pair count a row can have)."""
    t = (torch.rand(B, L, generator=g) < density).float()
    t[0] = 0.0
    if B >= 3:
        t[1] = 0.0
        t[1, 0] = 1.0
    if B >= 4:
        t[2] = 0.0
        t[2, L - 1] = 1.0
    if B >= 5 and L == 4096:
        t[3] = 0.0
        t[3, ::2] = 1.0
    if B >= 2:
        t[B - 1] = 1.0
    return t


def rank_case(B, L, n_mats, kind, seed):
    """-> (logits [n_mats x (B, L)], loss weights, targets, margin).  Logits 6 randn with 0, +-30, +-88, +-104 and +-1e4
    planted: spread over every matrix and, with room, side by side in the rows that have BOTH classes (the single-positive
    rows and the half-positive row; the all-zero and all-one rows have no pairs).  HINGE: every logit rounded to a multiple of
    2^-10 and the margin 1 + 2^-11, so that x_n - x_p is exact in fp32 and no a_pn lies within 2^-11 of the kink
    (assert_hinge_inputs): the two precisions cannot stand on different sides of it."""
    g = torch.Generator().manual_seed(seed)
    logits = [torch.randn(B, L, generator=g) * 6.0 for _ in range(n_mats)]
    targets = rank_targets(B, L, g)
    numel = B * L
    stride = max(1, numel // len(PLANTED))
    planted = torch.tensor(PLANTED)
    for k, x in enumerate(logits):
        flat = x.view(-1)
        for i, v in enumerate(PLANTED):
            flat[(i * stride + k) % numel] = v
        if L >= 2 * len(PLANTED):
            for r in range(1, min(B - 1, 4)):
                x[r, :len(PLANTED)] = planted
                x[r, L - len(PLANTED):] = planted.flip(0)
    margin = 0.0
    if kind == 'hinge':
        logits = [torch.round(x / GRID) * GRID for x in logits]
        margin = HINGE_MARGIN
        assert_hinge_inputs(logits, targets, margin)
    weights = [1.0] + [0.2, 0.5, 0.2, 1.5, 0.2, 0.7, 0.2][:n_mats - 1]
    return logits, weights, targets, margin


def assert_hinge_inputs(logits, targets, margin):
    """The property the HINGE cases rest on, checked in fp64: |x| <= 1e4 on the 2^-10 grid, every x_n - x_p exact in fp32,
    and |margin + (x_n - x_p)| >= 2^-11 for every pair of every row."""
    pos = targets > 0.5
    for x in logits:
        x64 = x.double()
        assert float(x64.abs().max()) <= 1e4 and bool((x64 / GRID == torch.round(x64 / GRID)).all())
        for r in range(x.size(0)):
            xp, xn = x[r][pos[r]], x[r][~pos[r]]
            if xp.numel() == 0 or xn.numel() == 0:
                continue
            d32 = xn.unsqueeze(0) - xp.unsqueeze(1)
            d64 = xn.double().unsqueeze(0) - xp.double().unsqueeze(1)
            assert torch.equal(d32.double(), d64)
            assert float((margin + d64).abs().min()) >= 2.0 ** -11


@functools.lru_cache(maxsize=None)
def reference_case(kind, B, L, n_mats, bce_weight):
    """One kernel case with its fp64 reference and fp32 yardstick, computed once and left unchanged by every test."""
    logits, weights, targets, margin = rank_case(B, L, n_mats, kind, seed=B * 1000 + L)
    ref64 = rank_reference(logits, weights, targets, kind, margin, bce_weight, torch.float64)
    ref32 = rank_reference(logits, weights, targets, kind, margin, bce_weight, torch.float32)
    return logits, weights, targets, margin, ref64, ref32
