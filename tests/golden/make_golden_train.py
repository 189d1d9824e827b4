#!/usr/bin/env python3
"""Golden vectors for the training epoch (lamp_amd/train.py against the reference's train.py:15-76).

Runs ONLY in the build container: imports the reference's own `train.train_epoch`, `utils.data_loader.DataLoader` /
`process_data` and `lamp.Models.LAMP` (with the oracle shims of SURVEY.md 8c) and drives them on the CPU:
  * the synthetic dataset of make_golden_harness.py; the first 20 training instances in a fixed order (shuffle=False),
    batch size 8: three batches, the last one short (4 rows);
  * a tiny graph model (d = 32, 2 heads, 2 + 2 layers, prior label mask), dropout 0, main.py:99's Adam
    (betas (0.9, 0.98), lr 0.0002, torch's default eps);
  * once in fp32 and once in fp64 from the same initial state_dict.
Recorded: the instances, the label adjacency, the initial weights, every batch's mean BCE, sigmoid predictions and targets of
both runs, the final weights of both runs, and the maximum fp32-vs-fp64 gap of each quantity (the tolerance of tests/test_train_gpu.py is
derived from these gaps: Adam divides by sqrt(v) + eps, so elements whose gradients are near eps amplify rounding).
Data only; no reference source is copied.
"""
import argparse
import os
import random
import sys

sys.dont_write_bytecode = True
REF = os.environ.get('LAMP_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path = [REF] + [p for p in sys.path if os.path.abspath(p or '.') not in
                    (os.path.abspath(os.path.join(HERE, '..', '..')),
                     os.path.abspath(os.path.join(HERE, '..', '..', 'dropin')), HERE,
                     os.path.abspath(os.path.join(HERE, '..')))]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
_mf = torch.Tensor.masked_fill
torch.Tensor.masked_fill = lambda self, m, v: _mf(self, m.bool() if m.dtype == torch.uint8 else m, v)

from utils.data_loader import DataLoader, process_data  # noqa: E402
import train as ref_train  # noqa: E402  (the reference's train.py)
from lamp.Models import LAMP  # noqa: E402

assert os.path.abspath(ref_train.__file__).startswith(os.path.abspath(REF))

N_TRAIN, BATCH, LR = 20, 8, 0.0002


def flatten(lists):
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.int64)
    flat = np.array([v for x in lists for v in x], dtype=np.int64)
    return flat, off


class Recorder(object):
    """Stands in for `F` inside the reference's train.py: the same functions, with every batch's loss and sigmoid kept in the
    run's own precision (the reference stores them through a float32 matrix and a python float sum)."""

    def __init__(self):
        self.bce, self.probs = [], []

    def sigmoid(self, x):
        p = torch.sigmoid(x)
        self.probs.append(p.detach().clone())
        return p

    def binary_cross_entropy_with_logits(self, pred, target, reduction='mean'):
        loss = TF.binary_cross_entropy_with_logits(pred, target.to(pred.dtype), reduction=reduction)
        self.bce.append(loss.detach().clone())
        return loss

    def __getattr__(self, name):
        return getattr(TF, name)


def dataset():
    rng = random.Random(7)
    n_words, n_labels, max_len = 60, 11, 14
    src_dict = {'<blank>': 0, '<unk>': 1, '<s>': 2, '</s>': 3}
    src_dict.update({'w%d' % i: 4 + i for i in range(n_words)})
    tgt_dict = {'<blank>': 0, '<unk>': 1, '<s>': 2, '</s>': 3}
    tgt_dict.update({'l%d' % i: 4 + i for i in range(n_labels)})

    def sample(force_label=None):
        n = rng.randint(1, max_len)
        src = [2] + [rng.randint(4, 4 + n_words - 1) for _ in range(n)] + [3]
        k = rng.randint(1, 4)
        labels = sorted(rng.sample(range(4, 4 + n_labels), k))
        if force_label is not None and force_label not in labels:
            labels = sorted(labels + [force_label])
        return src, [2] + labels + [3]

    splits = {}
    for name, n in (('train', 40), ('valid', 9), ('test', 19)):
        items = [sample(4 + (i % n_labels) if name == 'train' else None) for i in range(n)]
        splits[name] = {'src': [s for s, _ in items], 'tgt': [t for _, t in items]}
    settings = argparse.Namespace(max_seq_len=max_len + 2)
    return {'settings': settings, 'dict': {'src': src_dict, 'tgt': tgt_dict}, **splits}


def run(model, data, opt, dtype):
    model = model.to(dtype)
    loader = DataLoader(data['dict']['src'], data['dict']['tgt'], src_insts=data['train']['src'][:N_TRAIN],
                        tgt_insts=data['train']['tgt'][:N_TRAIN], batch_size=BATCH, binary_relevance=True, cuda=False,
                        shuffle=False, drop_last=False)
    optimizer = torch.optim.Adam(model.get_trainable_parameters(), betas=(0.9, 0.98), lr=LR)   # main.py:99
    rec = Recorder()
    ref_train.F = rec
    ref_train.tqdm = lambda it, **k: it
    try:
        preds, targets, bce_total = ref_train.train_epoch(model, loader, None, optimizer, None, 1, data['dict'], opt)
    finally:
        ref_train.F = TF
    return {'bce': torch.stack(rec.bce).double().numpy(), 'probs': torch.cat(rec.probs).double().numpy(),
            'all_predictions': preds.numpy(), 'all_targets': targets.numpy(), 'bce_total': float(bce_total),
            'sd': {k: v.detach().double().numpy().copy() for k, v in model.state_dict().items()}}


def main():
    data = dataset()
    opt = argparse.Namespace(adj_matrix_lambda=0.0, label_mask='prior', dataset='synthetic', summarize_data=False,
                             batch_size=BATCH, test_batch_size=BATCH, binary_relevance=True, cuda=False, max_ar_length=30,
                             multi_gpu=True, int_preds=False, matching_mlp=False, attns_loss=False, thresh1=10,
                             int_pred_weight=0.2)
    random.seed(0)
    _, _, _, adj, opt = process_data(data, opt)
    d, h = 32, 2

    def fresh():
        torch.manual_seed(5)
        return LAMP(opt.src_vocab_size, opt.tgt_vocab_size, opt.max_token_seq_len_e, opt.max_token_seq_len_d,
                    proj_share_weight=True, embs_share_weight=True, d_k=d // h, d_v=d // h, d_model=d, d_word_vec=d,
                    d_inner_hid=2 * d, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, dropout=0.0, dec_dropout=0.0,
                    dec_dropout2=False, encoder='graph', decoder='graph', enc_transform='', onehot=False,
                    no_enc_pos_embedding=False, no_dec_self_att=False, loss='ce', label_adj_matrix=adj.clone(),
                    attn_type='softmax', label_mask='prior', matching_mlp=False, graph_conv=False, int_preds=False)

    init = {k: v.detach().clone() for k, v in fresh().state_dict().items()}
    r32 = run(fresh(), data, opt, torch.float32)
    r64 = run(fresh(), data, opt, torch.float64)
    out = {}
    for part in ('src', 'tgt'):
        flat, off = flatten(data['train'][part][:N_TRAIN])
        out['train_%s_flat' % part], out['train_%s_off' % part] = flat, off
    out.update(n_src_dict=np.int64(len(data['dict']['src'])), n_tgt_dict=np.int64(len(data['dict']['tgt'])),
               max_seq_len=np.int64(data['settings'].max_seq_len), batch_size=np.int64(BATCH), lr=np.float64(LR),
               n_head=np.int64(h), d_model=np.int64(d), label_adj_matrix=adj.numpy(),
               src_vocab_size=np.int64(opt.src_vocab_size), tgt_vocab_size=np.int64(opt.tgt_vocab_size),
               max_token_seq_len_e=np.int64(opt.max_token_seq_len_e))
    for k, v in init.items():
        out['sd__' + k] = v.numpy()
    out['bce32'], out['bce64'] = r32['bce'], r64['bce']
    out['probs32'], out['probs64'] = r32['probs'].astype(np.float32), r64['probs']
    out['all_predictions'], out['all_targets'] = r32['all_predictions'], r32['all_targets']
    out['bce_total32'], out['bce_total64'] = np.float64(r32['bce_total']), np.float64(r64['bce_total'])
    assert np.array_equal(r32['all_targets'], r64['all_targets'])
    gap_w = 0.0
    for k in init:
        out['final32__' + k] = r32['sd'][k].astype(np.float32)
        out['final64__' + k] = r64['sd'][k]
        gap_w = max(gap_w, float(np.abs(r32['sd'][k] - r64['sd'][k]).max()))
    out['gap_bce'] = np.float64(np.abs(r32['bce'] - r64['bce']).max())
    out['gap_probs'] = np.float64(np.abs(r32['probs'] - r64['probs']).max())
    out['gap_weights'] = np.float64(gap_w)
    moved = max(float(np.abs(r64['sd'][k] - init[k].double().numpy()).max()) for k in init)
    out['max_weight_step'] = np.float64(moved)
    # what the tolerance of tests/test_train_gpu.py (max(1e-4, 3 x gap), the G13 rule) has to tell apart: an epoch that trained
    # from one that did not.  The largest weight step must stand well clear of it, and so must the change of the loss the
    # updates cause (batch 1 and 2 of a run WITHOUT updates against the recorded ones).
    for name in ('gap_bce', 'gap_probs', 'gap_weights'):
        print('%-12s %.3e  -> tolerance %.3e' % (name, float(out[name]), max(1e-4, 3 * float(out[name]))))
    assert moved > 5 * max(1e-4, 3 * float(out['gap_weights'])), moved
    frozen = fresh().double().train()
    loader = DataLoader(data['dict']['src'], data['dict']['tgt'], src_insts=data['train']['src'][:N_TRAIN],
                        tgt_insts=data['train']['tgt'][:N_TRAIN], batch_size=BATCH, binary_relevance=True, cuda=False,
                        shuffle=False, drop_last=False)
    import utils.utils as ref_utils
    with torch.no_grad():
        untrained = [float(TF.binary_cross_entropy_with_logits(
            frozen(b[0], b[1], None, None)[0], ref_utils.get_gold_binary(b[2][:, 1:], opt.tgt_vocab_size).double()))
            for b in loader]
    effect = max(abs(u - t) for u, t in zip(untrained[1:], r64['bce'][1:]))
    out['bce_untrained64'] = np.array(untrained)
    print('the updates move the later batches\' BCE by up to %.3e' % effect)
    assert abs(untrained[0] - r64['bce'][0]) < 1e-12 and effect > 5 * max(1e-4, 3 * float(out['gap_bce'])), effect
    print('per-batch BCE fp64: %s; largest weight step %.3e' % (r64['bce'], moved))
    path = os.path.join(HERE, 'train_epoch.npz')
    np.savez_compressed(path, **out)
    print('train_epoch.npz %.1f KB' % (os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
