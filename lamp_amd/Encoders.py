"""Encoders of LaMP (reference: lamp/Encoders.py).

GraphEncoder (lamp/Encoders.py:31-110) is the hot path: token (+ sinusoid position) embeddings and a stack of
EncoderLayers on the HIP kernels.  ``enc_transform`` pooling (:96-105) is a cheap reduction of its output, done in
PyTorch on the device.  MLPEncoder (:16-27) and RNNEncoder (:112-137) are the reference's baseline models (SURVEY.md
8f n4): plain PyTorch modules with the reference's parameter names and shapes, so every ``main.py -encoder`` choice
constructs and reference checkpoints load; they run wherever their tensors live.  Per-sample input graphs (``adj``,
:81-85) only shape the encoder's attention maps -- its attention OUTPUT is dead compute -- and are served as a generic
uint8 mask on the module-by-module route when maps are requested (logits identical either way).  With
``enc_self_attn=True`` the attention output is LIVE (Layers.EncoderLayer: the paper's feature->feature step, which the
reference's code never trains): every layer attends under the key-padding mask, or under ``adj`` when it is given, and
the graphs then reach the predictions.  The genomics
one-hot branch (onehot=True, :46-51,68-73: conv1 -> ReLU(dropout) -> max-pool -> conv2 -> ReLU + positions) runs on
csrc/conv.hip; it serves the reference's 9-symbol DNA vocabulary with position rows and no enc_transform.
"""
import torch
import torch.nn as nn

from . import Constants, utils
from . import _native as N
from .Layers import EncoderLayer


class GraphEncoder(nn.Module):
    def __init__(self, n_src_vocab, n_max_seq, n_layers=6, n_head=8, d_k=64, d_v=64, d_word_vec=512,
                 d_model=512, d_inner_hid=1024, onehot=False, enc_transform='', dropout=0.1,
                 no_enc_pos_embedding=False, enc_self_attn=False):
        super().__init__()
        self.enc_self_attn = bool(enc_self_attn)
        if onehot:
            if n_src_vocab != ONEHOT_VOCAB:
                # conv1 has 9 input channels: the reference fails at its first forward for any other vocabulary
                raise NotImplementedError('the one-hot encoder takes the %d-symbol DNA vocabulary, not %d'
                                          % (ONEHOT_VOCAB, n_src_vocab))
            if no_enc_pos_embedding:
                raise NotImplementedError('onehot without position embedding is an AttributeError in the reference')
            if enc_transform != '':
                raise NotImplementedError('onehot with enc_transform=%r is not served' % (enc_transform,))
        if enc_transform not in ('', 'sum', 'mean', 'flatten', 'max'):
            raise NotImplementedError('enc_transform=%r' % (enc_transform,))
        self.n_max_seq = n_max_seq
        self.d_model = d_model
        self.onehot = onehot
        self.enc_transform = enc_transform
        self.dropout = nn.Dropout(dropout)
        if onehot:
            # lamp/Encoders.py:46-51: a frozen-by-convention identity table over the bases, then the two convolutions
            self.src_word_emb = nn.Embedding(n_src_vocab, n_src_vocab, padding_idx=Constants.PAD)
            self.src_word_emb.weight.data.fill_(0)
            self.src_word_emb.weight.data[1:, 1:] = torch.eye(n_src_vocab - 1)
            self.conv1 = nn.Conv1d(ONEHOT_VOCAB, d_model, 16, stride=1, padding=8)
            self.conv2 = nn.Conv1d(d_model, d_model, 16, stride=1, padding=8)
        else:
            self.src_word_emb = nn.Embedding(n_src_vocab, d_word_vec, padding_idx=Constants.PAD)
        if no_enc_pos_embedding is False:
            n_position = n_max_seq + 1
            self.position_enc = nn.Embedding(n_position, d_word_vec, padding_idx=Constants.PAD)
            self.position_enc.weight.data = utils.position_encoding_init(n_position, d_word_vec)
        self.layer_stack = nn.ModuleList(
            EncoderLayer(d_model, d_inner_hid, n_head, d_k, d_v, dropout=dropout, live_attn=self.enc_self_attn)
            for _ in range(n_layers))

    def forward(self, src_seq, adj, src_pos, return_attns=False):
        pos_table = self.position_enc.weight if hasattr(self, 'position_enc') else None
        if self.onehot:
            if adj:
                raise NotImplementedError('per-sample input graphs (adj) are not served with the one-hot encoder')
            x = onehot_input(self, src_seq, src_pos)
            src_seq = src_seq[:, :x.size(1)].contiguous()   # lamp/Encoders.py:73
        elif self.training:
            # module-by-module training (graph encoder + enc_transform feeding another decoder): the embedding records
            # autograd here, the layers below dispatch to lamp_amd/training.py by themselves
            from . import training
            N.require_device(src_seq)
            x = training._EmbedFn.apply(src_seq.long().contiguous(), src_pos.long().contiguous(),
                                        self.src_word_emb.weight, pos_table)
        else:
            x = N.embed(src_seq, src_pos, self.src_word_emb.weight, pos_table)
        attns = []
        live = self.enc_self_attn
        pad_mask, keep = (N.key_token_mask(src_seq, src_seq.size(1)) if return_attns or live else (None, None))
        if adj and (return_attns or live):
            # per-sample input graphs (lamp/Encoders.py:81-85): inside each sample's n x n corner the self-attention mask
            # is the complement of its adjacency instead of the key-padding pattern.  In the dead mode the encoder's
            # self-attention OUTPUT is discarded (lamp/Layers.py:16-18), so this only ever shows in the returned maps.
            pad_mask, keep = adj_attn_mask(src_seq, adj), None
        if live:
            # the live attention's kernel is chosen from the sample, not from the padded length (LAMP_MASK_SELF_RAGGED)
            if not isinstance(pad_mask, N.Mask):
                pad_mask, keep = N.make_mask(pad_mask, src_seq.size(0), src_seq.size(1), src_seq.size(1))
            pad_mask.flags |= N.LAMP_MASK_SELF_RAGGED
        for layer in self.layer_stack:
            x, a = layer(x, slf_attn_mask=pad_mask, need_attn=return_attns)
            if return_attns:
                attns.append(a)
        del keep
        x = pool_encoder_output(x, src_seq, self.enc_transform)
        return (x, attns) if return_attns else (x, None)


ONEHOT_VOCAB = 9   # PAD, UNK, BOS, EOS and five bases


def adj_attn_mask(src_seq, adj):
    """lamp/Encoders.py:82,85-89: the encoder self-attention's uint8 mask [B, T, T] (nonzero = blocked) -- the key-padding
    pattern, with the complement of sample i's adjacency in its n x n corner."""
    m = utils.get_attn_padding_mask(src_seq, src_seq).to(torch.uint8).contiguous()
    for i, a in enumerate(adj):
        n = a.size(0)
        m[i, :n, :n] = utils.swap_0_1(a.to(m.device), 1, 0).to(torch.uint8)
    return m


def onehot_input(enc, src_seq, src_pos):
    """lamp/Encoders.py:68-72: the one-hot encoder's input rows [B, T // 2, d] (module-by-module route)."""
    N.require_device(src_seq)
    seq, pos = src_seq.long().contiguous(), src_pos.long().contiguous()
    if enc.training:
        from . import training
        return training.onehot_train(enc, seq, pos, training._Seeds())
    with torch.no_grad():
        t1 = N.onehot_tap_table(enc.src_word_emb.weight, enc.conv1.weight)
        w2 = N.f32c(enc.conv2.weight)
        fe = N.onehot_frontend(t1, N.f32c(enc.conv1.bias), w2, N.f32c(enc.conv2.bias))
        return N.onehot_encoder_input(seq, pos, fe, N.conv_pack(w2), N.f32c(enc.conv2.bias), N.f32c(enc.position_enc.weight),
                                      enc.d_model)


def pool_encoder_output(enc_output, src_seq, enc_transform):
    """lamp/Encoders.py:96-105: collapse the token states to ONE vector per sample, (B, 1, .).  'mean' divides the
    sum over ALL positions by the number of non-PAD tokens, exactly as the reference does; 'max' is a NameError in the
    reference (an undefined `x`, :98) and is rejected here."""
    if enc_transform == '':
        return enc_output
    B = enc_output.size(0)
    if enc_transform == 'sum':
        out = enc_output.sum(1)
    elif enc_transform == 'mean':
        out = enc_output.sum(1) / ((src_seq > 0).sum(dim=1).float().view(-1, 1))
    elif enc_transform == 'flatten':
        out = enc_output.reshape(B, -1).float()
    else:
        raise NotImplementedError("enc_transform='max' raises NameError in the reference (lamp/Encoders.py:98)")
    return out.view(B, 1, -1)


class MLPEncoder(nn.Module):
    """Bag-of-features baseline (lamp/Encoders.py:16-27): one Linear over the (B, n_src_vocab) FLOAT feature rows the
    caller passes as ``src_seq``; returns ((B, 1, d_model), None)."""

    def __init__(self, n_src_vocab, n_max_seq, n_layers=6, n_head=8, d_k=64, d_v=64, d_word_vec=512, d_model=512,
                 d_inner_hid=1024, onehot=False, dropout=0.1):
        super().__init__()
        self.n_max_seq, self.d_model = n_max_seq, d_model
        self.linear1 = nn.Linear(n_src_vocab, d_model)

    def forward(self, src_seq, adj, src_pos, return_attns=False):
        # one "token" per sample: the projected feature row
        return self.linear1(src_seq).unsqueeze(1), None


class RNNEncoder(nn.Module):
    """Bidirectional-GRU baseline (lamp/Encoders.py:112-137): embedding -> n_layers BiGRU -> Linear(2d, d)."""

    def __init__(self, n_src_vocab, n_max_seq, n_layers=6, n_head=8, d_k=64, d_v=64, d_word_vec=512, d_model=512,
                 d_inner_hid=1024, onehot=False, dropout=0.1):
        super().__init__()
        if onehot:
            raise NotImplementedError('the one-hot / Conv1d genomics encoder is outside the label-graph hot path')
        self.onehot = onehot
        self.src_word_emb = nn.Embedding(n_src_vocab, d_word_vec, padding_idx=Constants.PAD)
        self.brnn = nn.GRU(d_word_vec, d_model, n_layers, batch_first=True, bidirectional=True, dropout=dropout)
        self.U = nn.Linear(d_model * 2, d_model)

    def forward(self, src_seq, adj, src_pos, return_attns=False):
        both_directions = self.brnn(self.src_word_emb(src_seq))[0]   # (B, T, 2 d_model)
        return self.U(both_directions), None
