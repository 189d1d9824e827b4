#!/usr/bin/env python3
"""Golden vectors of the reference's LAMP.forward at the BASELINE.json sizes (tests/test_oracle_vs_reference.py).

    LAMP_REFERENCE=<checkout of the reference> python tests/golden/make_golden_reference_sizes.py

Imports the reference's own `lamp` package (never this repo's), loads the seeded synthetic weights of
lamp_amd/synthetic.make_state_dict into it, and runs it on the seeded batches of lamp_amd/synthetic.make_batch -- so the
test can regenerate weights and inputs without the reference and compare the oracle with what the reference returned.
Recorded per case: the logits in full; of enc_output (too large to keep whole) the values at ENC_SAMPLES positions drawn
with seed 0 and, at every (sample, position), the sum over d_model in float64.  Data only; no reference source is copied.
"""
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ['LAMP_REFERENCE']
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
# the name `lamp` must resolve to the reference; this repo is importable after it for lamp_amd.synthetic only
sys.path = [REF] + [p for p in sys.path if os.path.abspath(p or '.') not in (ROOT, os.path.join(ROOT, 'dropin'), HERE)] + [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
_mf = torch.Tensor.masked_fill
torch.Tensor.masked_fill = lambda self, m, v: _mf(self, m.bool() if m.dtype == torch.uint8 else m, v)

from lamp.Models import LAMP  # noqa: E402
from lamp_amd import synthetic as S  # noqa: E402

assert os.path.abspath(sys.modules['lamp'].__file__).startswith(os.path.abspath(REF))

ENC_SAMPLES = 16384
CASES = {
    'reuters_fixed': dict(V=23666, L=90, T=302, d=512, dff=512, h=4, mask='prior', pos_emb=True, B=8, p=0.10),
    'reuters_ragged': dict(V=23666, L=90, T=302, d=512, dff=512, h=4, mask='prior', pos_emb=True, B=6, p=0.10,
                           lengths=[302, 20, 150, 77, 201, 33]),
    'bibtex': dict(V=1840, L=159, T=100, d=512, dff=1024, h=4, mask='prior', pos_emb=False, B=4, p=0.05),
    'delicious': dict(V=504, L=983, T=40, d=1024, dff=2048, h=8, mask='none', pos_emb=False, B=2, p=0.0),
    'inveye_h1': dict(V=300, L=50, T=30, d=128, dff=256, h=1, mask='inveye', pos_emb=True, B=3, p=0.0),
}


def enc_sample_index(numel):
    return torch.randint(numel, (ENC_SAMPLES,), generator=torch.Generator().manual_seed(0)).sort().values


def run(V, L, T, d, dff, h, mask, pos_emb, B, p, lengths=None):
    adj = S.make_adjacency(L, p, seed=0) if mask == 'prior' else None
    m = LAMP(V, L, T, L, proj_share_weight=True, embs_share_weight=True, d_k=d // h, d_v=d // h,
             d_model=d, d_word_vec=d, d_inner_hid=dff, n_layers_enc=2, n_layers_dec=2, n_head=h,
             n_head2=h, dropout=0.1, dec_dropout=0.1, dec_dropout2=False, encoder='graph',
             decoder='graph', enc_transform='', onehot=False, no_enc_pos_embedding=not pos_emb,
             no_dec_self_att=False, loss='ce',
             label_adj_matrix=adj.clone() if adj is not None else None, attn_type='softmax',
             label_mask=mask, matching_mlp=False, graph_conv=False, int_preds=False)
    m.load_state_dict(S.make_state_dict(V, L, T, d, dff, h, 2, 2, pos_emb=pos_emb, seed=0))
    m.eval()
    seq, pos = S.make_batch(B, V, T, lengths=lengths, seed=0)
    with torch.no_grad():
        lg, enc, _ = m((seq, pos), None, None, None)
    idx = enc_sample_index(enc.numel())
    return {'logits': lg.numpy(), 'enc_idx': idx.numpy(), 'enc_val': enc.reshape(-1)[idx].numpy(),
            'enc_rowsum': enc.double().sum(-1).numpy()}


def main():
    arrays = {}
    for name, kw in CASES.items():
        for k, a in run(**kw).items():
            arrays['%s__%s' % (name, k)] = a
    path = os.path.join(HERE, 'reference_sizes.npz')
    np.savez_compressed(path, **arrays)
    print('%-40s %7.1f KB' % ('reference_sizes', os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
