"""The oracle against the reference at the BASELINE.json sizes.

tests/golden/reference_sizes.npz holds what the reference's own LAMP.forward returned (made by
tests/golden/make_golden_reference_sizes.py) for the seeded synthetic weights and batches below, which the oracle
regenerates: the logits in full, enc_output as a seeded sample of its elements plus its sum over d_model at every
(sample, position).
"""
import os

import numpy as np
import torch

from conftest import GOLDEN
from oracle import lamp_ref as R

CASES = {
    'reuters_fixed': dict(V=23666, L=90, T=302, d=512, dff=512, h=4, mask='prior', pos_emb=True, B=8, p=0.10),
    'reuters_ragged': dict(V=23666, L=90, T=302, d=512, dff=512, h=4, mask='prior', pos_emb=True, B=6, p=0.10,
                           lengths=[302, 20, 150, 77, 201, 33]),
    'bibtex': dict(V=1840, L=159, T=100, d=512, dff=1024, h=4, mask='prior', pos_emb=False, B=4, p=0.05),
    'delicious': dict(V=504, L=983, T=40, d=1024, dff=2048, h=8, mask='none', pos_emb=False, B=2, p=0.0),
    'inveye_h1': dict(V=300, L=50, T=30, d=128, dff=256, h=1, mask='inveye', pos_emb=True, B=3, p=0.0),
}
TOL = 1e-5


def test_oracle_matches_live_reference_at_baseline_sizes():
    z = np.load(os.path.join(GOLDEN, 'reference_sizes.npz'))
    for case, c in CASES.items():
        ref = {k: z['%s__%s' % (case, k)] for k in ('logits', 'enc_idx', 'enc_val', 'enc_rowsum')}
        adj = R.make_adjacency(c['L'], c['p'], seed=0) if c['mask'] == 'prior' else None
        sd = R.make_state_dict(c['V'], c['L'], c['T'], c['d'], c['dff'], c['h'], 2, 2, pos_emb=c['pos_emb'], seed=0)
        seq, pos = R.make_batch(c['B'], c['V'], c['T'], lengths=c.get('lengths'), seed=0)
        blocked = R.label_block_mask(adj, c['mask'], c['L'])
        for aw in (False, True):
            with torch.no_grad():
                lg, enc, _ = R.forward(sd, seq, pos, c['h'], blocked, as_written=aw)
            assert lg.shape == ref['logits'].shape and enc.shape[:2] == ref['enc_rowsum'].shape, case
            err = {'logits': np.abs(lg.numpy() - ref['logits']).max(),
                   'enc': np.abs(enc.reshape(-1)[torch.from_numpy(ref['enc_idx'])].numpy() - ref['enc_val']).max(),
                   # |sum of d errors| <= d * TOL wherever every element is within TOL
                   'enc_rowsum': np.abs(enc.double().sum(-1).numpy() - ref['enc_rowsum']).max() / c['d']}
            for k, v in err.items():
                assert v <= TOL, (case, aw, k, v)
