#!/usr/bin/env python3
"""Generate tests/golden/geometry.npz by running the *reference's* LAMP on the CPU at head geometries away from
d_k = d_v = d_model / n_head and n_head2 = n_head (every fixture of make_golden.py sits on that diagonal):

    G1   d_model 64, d_inner 96, n_head 3, n_head2 2, d_k 24, d_v 40, prior label graph
    G2   d_model 64, d_inner 96, n_head 1, n_head2 2, d_k 48, d_v 64 (enc-attention without fc), fully connected labels

Runs ONLY where the reference checkout exists (LAMP_REFERENCE, default /root/reference).  It imports the reference's own
``lamp`` package (never this repo's), applies the semantics-preserving shims of make_golden.py, drives the model in eval mode
with seeded inputs and stores the state dict, the inputs, logits, enc_output, every attention map and the intermediate
predictions, every key prefixed with the geometry's name.  One encoder and two decoder layers; the weights are rounded to
the fp16 grid BEFORE the reference runs and stored as float16 (exactly, half the bytes -- the arithmetic is fp32 throughout),
which keeps the file small.

    python tests/golden/make_golden_geometry.py

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

from lamp.Models import LAMP  # noqa: E402

assert os.path.abspath(sys.modules['lamp'].__file__).startswith(os.path.abspath(REF))

GEOMS = {
    'G1': dict(d=64, dff=96, h=3, h2=2, dk=24, dv=40, mask='prior'),
    'G2': dict(d=64, dff=96, h=1, h2=2, dk=48, dv=64, mask='none'),
}
V, L, T, LENGTHS = 30, 24, 20, [20, 9, 1]


def npy(t):
    return t.detach().cpu().numpy()


def main():
    out = {}
    for case, (name, g) in enumerate(sorted(GEOMS.items())):
        gen = torch.Generator().manual_seed(4100 + case)
        adj = None
        if g['mask'] == 'prior':
            adj = (torch.rand(L, L, generator=gen) < 0.25).float()
            adj = ((adj + adj.t()) > 0).float()
            adj.fill_diagonal_(1.0)
        torch.manual_seed(4200 + case)
        m = LAMP(V, L, T, L, proj_share_weight=True, embs_share_weight=True, d_k=g['dk'], d_v=g['dv'], d_model=g['d'],
                 d_word_vec=g['d'], d_inner_hid=g['dff'], n_layers_enc=1, n_layers_dec=2, n_head=g['h'], n_head2=g['h2'],
                 dropout=0.1, dec_dropout=0.1, dec_dropout2=False, encoder='graph', decoder='graph', enc_transform='',
                 onehot=False, no_enc_pos_embedding=False, no_dec_self_att=False, loss='ce',
                 label_adj_matrix=adj.clone() if adj is not None else None, attn_type='softmax', label_mask=g['mask'],
                 matching_mlp=False, graph_conv=False, int_preds=False).eval()
        for n_, p in m.named_parameters():   # LayerNorm affine parameters away from their trivial 1 / 0 defaults
            if 'layer_norm' in n_:
                p.data.add_(torch.randn(p.shape, generator=gen) * 0.05)
            if 'position_enc' not in n_:         # every trained-class weight on the fp16 grid: stored in half the bytes, exactly
                p.data.copy_(p.data.half().float())
        seq = torch.zeros(len(LENGTHS), T, dtype=torch.int64)
        pos = torch.zeros(len(LENGTHS), T, dtype=torch.int64)
        for b, n in enumerate(LENGTHS):
            seq[b, :n] = torch.randint(4, V, (n,), generator=gen)
            pos[b, :n] = torch.arange(1, n + 1)
        with torch.no_grad():
            logits, enc, _ = m((seq, pos), None, None, None)
            lg2, _, enc_attns, dec2 = m((seq, pos), None, None, None, return_attns=True)
            lg3, _, ips = m((seq, pos), None, None, None, int_preds=True)
        assert torch.equal(logits, lg2) and torch.equal(logits, lg3)
        pre = name + '__'
        for k_, v_ in m.state_dict().items():
            exact16 = torch.equal(v_.half().float(), v_)
            out[pre + 'sd__' + k_] = npy(v_.half() if exact16 else v_)
        out.update({pre + 'src_seq': npy(seq), pre + 'src_pos': npy(pos), pre + 'logits': npy(logits),
                    pre + 'enc_output': npy(enc), pre + 'label_mask': np.array(g['mask'])})
        for key in ('d', 'dff', 'h', 'h2', 'dk', 'dv'):
            out[pre + key] = np.int64(g[key])
        if adj is not None:
            out[pre + 'label_adj_matrix'] = npy(adj)
        if m.decoder.label_mask is not None:
            out[pre + 'ref_label_mask'] = npy(m.decoder.label_mask)
        for i, a in enumerate(enc_attns[0]):
            out[pre + 'attn_enc_%d' % i] = npy(a)
        for i, a in enumerate(dec2[0]):
            out[pre + 'attn_dec_slf_%d' % i] = npy(a)
        for i, a in enumerate(dec2[1]):
            out[pre + 'attn_dec_enc_%d' % i] = npy(a)
        for i, p in enumerate(ips):
            out[pre + 'int_pred_%d' % i] = npy(p)
    path = os.path.join(HERE, 'geometry.npz')
    np.savez_compressed(path, **out)
    print('%-40s %7.1f KB' % ('geometry', os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
