"""Shared pieces of the sigmoid attention tests: an fp64-capable torch restatement of the reference's
``ScaledDotProductAttention(attn_type='sigmoid')`` (lamp/SubLayers.py:17-25,27-43), pinned against the reference's own modules
by tests/golden/sigmoid_attn.npz (tests/test_sigmoid_attn_cpu.py).  Model-level expectations substitute it for
``oracle.lamp_ref.sdpa`` around the existing oracle composition (``mha`` looks ``sdpa`` up at call time)."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MASKS = ('none', 'keypad', 'shared', 'fullrow')


def sigmoid_sdpa(q, k, v, blocked=None, temperature=None):
    """q, k, v: (N, l, d); blocked: (N, lq, lk) bool.  P = sigmoid(q k^T / t), blocked entries sigmoid(-inf) = 0; O = P v."""
    if temperature is None:
        temperature = np.power(q.size(-1), 0.5)
    attn = torch.bmm(q, k.transpose(1, 2)) / temperature
    if blocked is not None:
        attn = attn.masked_fill(blocked.bool(), float('-inf'))
    attn = torch.sigmoid(attn)
    return torch.bmm(attn, v), attn


def load_fixture():
    with np.load(os.path.join(HERE, 'golden', 'sigmoid_attn.npz')) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def mha_state(fx, h):
    pre = 'mha%d_sd__' % h
    return {k[len(pre):]: v for k, v in fx.items() if k.startswith(pre)}
