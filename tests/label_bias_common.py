"""Shared pieces of the weighted-label-graph tests (LAMP(label_bias=...), lamp_mask kind LAMP_MASK_BIAS_F32): an fp64-capable
torch restatement of the definition

    S[b, h, q, k] = <Q[b, h, q, :], K[b, h, k, :]> / temperature + bias[q, k];   P = softmax_k(S);   O = P V

with ``-inf`` in the bias = blocked, exactly as ``masked_fill + softmax`` blocks.  Model-level expectations substitute it for
``oracle.lamp_ref.sdpa`` around the existing oracle composition (``mha`` looks ``sdpa`` up at call time): the wrapper adds the
bias only to a square L x L call, i.e. to the decoder's label self-attention -- the test shapes keep L != T."""
import random

import numpy as np
import torch

ULP = 2.0 ** -23   # one fp32 ulp of a value in [1, 2): the floor of every relative bound here


def bias_sdpa(q, k, v, bias=None, blocked=None, temperature=None):
    """q, k, v: (N, l, d); bias: broadcastable to (N, lq, lk), -inf = blocked; blocked: (N, lq, lk) bool or None."""
    if temperature is None:
        temperature = np.power(q.size(-1), 0.5)
    s = torch.bmm(q, k.transpose(1, 2)) / temperature
    if blocked is not None:
        s = s.masked_fill(blocked.bool(), float('-inf'))
    if bias is not None:
        s = s + bias.to(s.dtype)
    p = torch.softmax(s, dim=2)
    return torch.bmm(p, v), p


def sdpa_with_label_bias(bias, L):
    """A stand-in for oracle.lamp_ref.sdpa that adds `bias` (L, L) to the label self-attention (lq == lk == L) only."""
    def sdpa(q, k, v, blocked=None, temperature=None):
        square = q.size(1) == L and k.size(1) == L
        return bias_sdpa(q, k, v, bias if square else None, blocked, temperature)
    return sdpa


def random_bias(lq, lk, g, B=None, full_row=None):
    """N(0, 2) with about 30 % -inf; row 0 (when there are two rows) keeps a single allowed key; a few entries of +-30 so that
    the maximum subtraction matters; no fully blocked row unless `full_row` names one (then exactly that row, in sample 0)."""
    shape = (lq, lk) if B is None else (B, lq, lk)
    bias = 2.0 * torch.randn(shape, generator=g)
    drop = torch.rand(shape, generator=g) < 0.3
    keep_one = torch.randint(0, lk, shape[:-1], generator=g)
    drop.scatter_(-1, keep_one.unsqueeze(-1), False)          # every row keeps at least one key
    bias[drop] = float('-inf')
    b2 = bias.view(-1, lq, lk)
    for m in b2:
        if lq > 1 and lk > 1:
            only = int(keep_one.view(-1, lq)[0, 0])
            m[0, :] = float('-inf')
            m[0, only] = 0.7
        for i in range(min(4, lq)):
            qi, ki = (7 * i + 1) % lq, (5 * i + 2) % lk
            if qi != 0 or lq == 1 or lk == 1:
                m[qi, ki] = 30.0 if i % 2 == 0 else -30.0
    if full_row is not None:
        b2[0, full_row, :] = float('-inf')
    return bias


def flat(t):
    """[B, H, l, d] -> [H * B, l, d] (index h * B + b, the library's map order)."""
    B, H = t.shape[:2]
    return t.permute(1, 0, 2, 3).reshape(H * B, t.size(2), t.size(3))


def row_rel(o, o64, p64, v64):
    """max over rows and columns of |O - O64| / sum_k p_k |v_k| over the rows that are not NaN in the reference."""
    ok = ~torch.isnan(o64).any(dim=2)
    scale = torch.bmm(torch.nan_to_num(p64), v64.abs())
    err = (o.double() - o64).abs()
    return (err[ok] / scale[ok].clamp_min(1e-30)).max().item() if ok.any() else 0.0


def toy_split(seed=5, n=40, L=11):
    """About 40 target rows [BOS, labels + 4 ..., EOS] over 11 labels: one sample repeats a label, one is empty, and label
    L - 1 never occurs.  -> (rows, n_tgt_dict)."""
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        labels = [l for l in range(L - 1) if rng.random() < 0.25]
        rows.append([2] + [4 + l for l in labels] + [3])
    rows[3] = [2, 4 + 1, 4 + 5, 4 + 1, 3]     # a duplicated label
    rows[7] = [2, 3]                          # an empty sample
    return rows, L + 4


def brute_counts(rows, L):
    C = torch.zeros(L, L)
    for r in rows:
        labels = sorted({v - 4 for v in r[1:-1]})
        for a in labels:
            for b in labels:
                C[a, b] += 1
    return C
