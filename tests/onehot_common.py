"""Shared pieces of the one-hot genomics encoder tests: a small model and a test-local fp64 restatement of
lamp/Encoders.py:68-73 composed with the oracle's FFN, decoder and read-out."""
import torch
import torch.nn.functional as F

from oracle import lamp_ref as R


def build_model(d=64, h=4, L=23, T_max=64, dff=None, mask='none', adj=None, dropout=0.0, int_preds=False, seed=0):
    from lamp_amd.Models import LAMP
    torch.manual_seed(seed)
    m = LAMP(9, L, T_max, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d,
             d_inner_hid=dff or 2 * d, d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', dropout=dropout,
             dec_dropout=dropout, dec_dropout2=dropout, onehot=True, label_mask=mask,
             label_adj_matrix=adj, int_preds=int_preds)
    return m


def make_dna(B, T, lengths=None, seed=0):
    """Tokens in 1..8 (UNK, BOS, EOS, five bases as the reference's vocabulary lays them out), PAD tails."""
    g = torch.Generator().manual_seed(seed)
    seq = torch.randint(1, 9, (B, T), generator=g)
    pos = torch.arange(1, T + 1).repeat(B, 1)
    for b, n in enumerate(lengths or [T] * B):
        seq[b, n:] = 0
        pos[b, n:] = 0
    return seq, pos


def onehot_encoder_ref(sd, seq, pos):
    """lamp/Encoders.py:66-73 then the encoder layers (FFN only, lamp/Layers.py:16-18); dtype of sd."""
    x = F.embedding(seq, sd['encoder.src_word_emb.weight'], padding_idx=0).transpose(1, 2)   # nn.Embedding(padding_idx=PAD)
    y = F.relu(F.conv1d(x, sd['encoder.conv1.weight'], sd['encoder.conv1.bias'], padding=8))[:, :, :-1]
    y = F.max_pool1d(y, 2, 2)
    y = F.relu(F.conv1d(y, sd['encoder.conv2.weight'], sd['encoder.conv2.bias'], padding=8).transpose(1, 2))[:, :-1, :]
    T2 = y.size(1)
    y = y + F.embedding(pos[:, :T2], sd['encoder.position_enc.weight'])
    for i in range(R.count_layers(sd, 'encoder')):
        y = R.ffn(y, *R._ffn_params(sd, 'encoder.layer_stack.%d.pos_ffn.' % i))
    return y, seq[:, :T2]


def onehot_forward_ref(sd, seq, pos, n_head, label_blocked=None, int_preds=False):
    enc, seq2 = onehot_encoder_ref(sd, seq, pos)
    y, slf, encdec, int_outs = R.decoder_forward(sd, seq2, enc, label_blocked, n_head)
    w = sd['tgt_word_proj.linear.weight']
    logits = R.readout(y, w)
    if int_preds:
        return logits, enc, [R.readout(o, w) for o in int_outs[:-1]]
    return logits, enc, (slf, encdec)


def fp64_state(model):
    return {k: v.detach().cpu().double() for k, v in model.state_dict().items()}


# the golden fixtures' model (tests/golden/make_golden_onehot.py)
GOLDEN_DIMS = dict(d=64, h=4, dff=128, L=23, T_max=64)


def golden_case(name):
    """-> (fixture arrays, fp32 state_dict of lamp_amd.synthetic.make_onehot_state_dict, label adjacency or None)."""
    from conftest import GOLDEN
    import os
    import numpy as np
    from lamp_amd import synthetic
    g = GOLDEN_DIMS
    z = dict(np.load(os.path.join(GOLDEN, 'onehot_%s.npz' % name), allow_pickle=False))
    sd = synthetic.make_onehot_state_dict(g['L'], g['T_max'], g['d'], g['dff'], g['h'], 2, 2, seed=0)
    adj = synthetic.make_adjacency(g['L'], 0.2, seed=0) if 'prior' in name else None
    return z, sd, adj


def golden_model(name):
    z, sd, adj = golden_case(name)
    g = GOLDEN_DIMS
    m = build_model(d=g['d'], h=g['h'], L=g['L'], T_max=g['T_max'], dff=g['dff'], mask='prior' if adj is not None else 'none',
                    adj=adj.clone() if adj is not None else None)
    m.load_state_dict(sd)
    return m, z, sd, adj
