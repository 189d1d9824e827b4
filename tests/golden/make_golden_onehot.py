#!/usr/bin/env python3
"""Golden vectors of the reference's one-hot genomics model (GraphEncoder(onehot=True), lamp/Encoders.py:46-51,68-73):
tests/test_onehot_cpu.py / tests/test_onehot_gpu.py.

    LAMP_REFERENCE=<checkout of the reference> python tests/golden/make_golden_onehot.py

Imports the reference's own `lamp` package (never this repo's), loads the seeded weights of
lamp_amd/synthetic.make_onehot_state_dict into its LAMP(onehot=True) and runs it on the seeded DNA batches of
lamp_amd/synthetic.make_batch (tokens 4..8), once in float32 and once cast to float64.  Recorded per case: the state_dict
names and shapes, the logits and enc_output, and for the maps case the intermediate predictions and every attention map.
Data only; no reference source is copied.
"""
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ['LAMP_REFERENCE']
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path = [REF] + [p for p in sys.path if os.path.abspath(p or '.') not in (ROOT, os.path.join(ROOT, 'dropin'), HERE)] + [ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
_mf = torch.Tensor.masked_fill
torch.Tensor.masked_fill = lambda self, m, v: _mf(self, m.bool() if m.dtype == torch.uint8 else m, v)

from lamp.Models import LAMP  # noqa: E402
from lamp_amd import synthetic as S  # noqa: E402

assert os.path.abspath(sys.modules['lamp'].__file__).startswith(os.path.abspath(REF))

D, H, DFF, L, T_MAX = 64, 4, 128, 23, 64
CASES = {
    'even_none': dict(T=40, lengths=None, B=2, mask='none', maps=False),
    'odd_prior': dict(T=41, lengths=None, B=2, mask='prior', maps=False),
    'ragged_prior': dict(T=48, lengths=[48, 30, 9], B=3, mask='prior', maps=False),
    'maps_none': dict(T=32, lengths=[32, 19], B=2, mask='none', maps=True),
}


def run(T, lengths, B, mask, maps, seed=0):
    adj = S.make_adjacency(L, 0.2, seed=0) if mask == 'prior' else None
    m = LAMP(9, L, T_MAX, L, proj_share_weight=True, embs_share_weight=True, d_k=D // H, d_v=D // H, d_model=D,
             d_word_vec=D, d_inner_hid=DFF, n_layers_enc=2, n_layers_dec=2, n_head=H, n_head2=H, dropout=0.1,
             dec_dropout=0.1, dec_dropout2=False, encoder='graph', decoder='graph', enc_transform='', onehot=True,
             no_enc_pos_embedding=False, no_dec_self_att=False, loss='ce',
             label_adj_matrix=adj.clone() if adj is not None else None, attn_type='softmax', label_mask=mask,
             matching_mlp=False, graph_conv=False, int_preds=False)
    sd = S.make_onehot_state_dict(L, T_MAX, D, DFF, H, 2, 2, seed=seed)
    m.load_state_dict(sd)
    m.eval()
    seq, pos = S.make_batch(B, 9, T, lengths=lengths, seed=seed)
    ref_sd = m.state_dict()
    out = {'seq': seq.numpy(), 'pos': pos.numpy(), 'sd_names': np.array(sorted(ref_sd)),
           'sd_shapes': np.array([list(ref_sd[k].shape) + [0] * (3 - ref_sd[k].dim()) for k in sorted(ref_sd)])}
    for tag, dt in (('', torch.float32), ('_fp64', torch.float64)):
        mm = m.to(dt)
        with torch.no_grad():
            lg, enc, _ = mm((seq, pos), None, None, None)
            out['logits' + tag], out['enc' + tag] = lg.numpy(), enc.numpy()
            if maps:
                _, _, ip = mm((seq, pos), None, None, None, int_preds=True)
                for i, a in enumerate(ip):
                    out['int_pred%d%s' % (i, tag)] = a.numpy()
                _, _, enc_attns, dec2 = mm((seq, pos), None, None, None, return_attns=True)
                for i, a in enumerate(enc_attns[0]):
                    out['enc_attn%d%s' % (i, tag)] = a.numpy()
                for j, group in enumerate(dec2):
                    for i, a in enumerate(group):
                        out['dec_attn%d_%d%s' % (j, i, tag)] = a.numpy()
    return out


def main():
    for name, kw in CASES.items():
        path = os.path.join(HERE, 'onehot_%s.npz' % name)
        np.savez_compressed(path, **run(**kw))
        print('%-40s %7.1f KB' % ('onehot_' + name, os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
