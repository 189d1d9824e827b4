#!/usr/bin/env python3
"""Generate tests/golden/sigmoid_attn.npz by running the *reference's* sigmoid attention modules on the CPU.

Runs ONLY where the reference checkout exists (LAMP_REFERENCE, default /root/reference).  It imports the reference's own
``lamp`` package (never this repo's), applies the semantics-preserving shims of make_golden.py (uint8 mask -> bool for
``masked_fill``), drives ``ScaledDotProductAttention(attn_type='sigmoid')`` and ``MultiHeadAttention(attn_type='sigmoid')``
(lamp/SubLayers.py:17-25,39,65-75) in eval mode with seeded inputs and stores inputs, weights, masks and outputs.

    python tests/golden/make_golden_sigmoid.py

The fixture is data only.  No reference source text is copied anywhere.
"""
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get('LAMP_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path = [REF] + [p for p in sys.path if os.path.abspath(p or '.') not in
                    (os.path.abspath(os.path.join(HERE, '..', '..')),
                     os.path.abspath(os.path.join(HERE, '..', '..', 'dropin')))]

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
_mf = torch.Tensor.masked_fill
torch.Tensor.masked_fill = lambda self, m, v: _mf(self, m.bool() if m.dtype == torch.uint8 else m, v)

from lamp.SubLayers import MultiHeadAttention, ScaledDotProductAttention  # noqa: E402

assert os.path.abspath(sys.modules['lamp'].__file__).startswith(os.path.abspath(REF))


def npy(t):
    return t.detach().cpu().numpy()


def masks_for(N, lq, lk, g):
    """none / key padding / one shared label mask / the shared mask with one fully blocked row."""
    kp = torch.zeros(N, lq, lk, dtype=torch.bool)
    for n in range(N):
        kp[n, :, lk - (n % 4):] = True
    shared = (torch.rand(lq, lk, generator=g) < 0.5)
    shared[:, 0] = False
    shared = shared.unsqueeze(0).expand(N, lq, lk).clone()
    full = shared.clone()
    full[min(2, N - 1), 3, :] = True
    return {'none': None, 'keypad': kp, 'shared': shared, 'fullrow': full}


def main():
    out = {}
    g = torch.Generator().manual_seed(311)
    N, lq, lk, dk = 6, 7, 9, 16
    q = torch.randn(N, lq, dk, generator=g)
    k = torch.randn(N, lk, dk, generator=g)
    v = torch.randn(N, lk, dk, generator=g)
    mod = ScaledDotProductAttention(temperature=np.power(dk, 0.5), attn_type='sigmoid').eval()
    out.update(sdpa_q=npy(q), sdpa_k=npy(k), sdpa_v=npy(v))
    for name, m in masks_for(N, lq, lk, g).items():
        o, a = mod(q, k, v, attn_mask=m)
        if m is not None:
            out['sdpa_mask_' + name] = npy(m)
        out['sdpa_out_' + name] = npy(o)
        out['sdpa_attn_' + name] = npy(a)
    for h in (1, 4):
        g = torch.Generator().manual_seed(320 + h)
        d, B, lq, lk = 64, 3, 10, 13
        torch.manual_seed(400 + h)
        mod = MultiHeadAttention(h, d, d // h, d // h, attn_type='sigmoid').eval()
        for n_, p in mod.named_parameters():
            if 'layer_norm' in n_:
                p.data.add_(torch.randn(p.shape, generator=g) * 0.05)
        xq = torch.randn(B, lq, d, generator=g)
        xkv = torch.randn(B, lk, d, generator=g)
        pre = 'mha%d_' % h
        for k_, v_ in mod.state_dict().items():
            out[pre + 'sd__' + k_] = npy(v_)
        out[pre + 'xq'], out[pre + 'xkv'] = npy(xq), npy(xkv)
        for name, m in masks_for(B, lq, lk, g).items():
            o, a = mod(xq, xkv, xkv, attn_mask=m)
            if m is not None:
                out[pre + 'mask_' + name] = npy(m)
            out[pre + 'out_' + name] = npy(o)
            out[pre + 'attn_' + name] = npy(a)
    path = os.path.join(HERE, 'sigmoid_attn.npz')
    np.savez_compressed(path, **out)
    print('%-40s %7.1f KB' % ('sigmoid_attn', os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
