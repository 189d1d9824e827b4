"""Shared pieces of the live encoder self-attention tests (LAMP(enc_self_attn=True)): the issue's shapes and the oracle
composition -- per encoder layer ``oracle.lamp_ref.mha(x, x, blocked, ...)`` then ``oracle.lamp_ref.ffn(...)``, followed by
``decoder_forward`` and ``readout``, all functions the golden fixtures pin against the reference's own modules."""
import torch
import torch.nn.functional as F

from oracle import lamp_ref as R

PAD_EXTRA = 37   # the re-padding of the bit-identity tests

# the smallest shapes that reach every route: A small everything; B crosses the 256-query and 64-key boundaries of the attention
# kernels; C has 128-wide heads at d_model 512
SHAPES = {
    'A': dict(V=50, L=24, d=128, h=2, dff=256, T=40, lengths=[40, 17, 1]),
    'B': dict(V=50, L=24, d=128, h=2, dff=256, T=300, lengths=[300, 257, 64, 20]),
    'C': dict(V=50, L=24, d=512, h=4, dff=512, T=48, lengths=[48, 33]),
    # d_model 512 with >= 512 encoder rows: the live layer's row-local tail runs as one chain launch
    'D': dict(V=50, L=24, d=512, h=4, dff=512, T=300, lengths=[300, 281]),
}


def build(shape, mask='prior', pos=True, live=True, dropout=0.0, int_preds=False, seed=0, **kw):
    """-> (LAMP on the CPU, state_dict, label block mask, src_seq, src_pos, n_head)."""
    from lamp_amd.Models import LAMP
    s = SHAPES[shape] if isinstance(shape, str) else shape
    V, L, d, h, dff, T = s['V'], s['L'], s['d'], s['h'], s['dff'], s['T']
    n_max = T + PAD_EXTRA
    sd = R.make_state_dict(V, L, n_max, d, dff, h, 2, 2, pos_emb=pos, seed=seed)
    adj = R.make_adjacency(L, 0.2, seed) if mask == 'prior' else None
    seq, spos = R.make_batch(len(s['lengths']), V, T, lengths=s['lengths'], seed=seed)
    if seq.size(1) < T:
        seq, spos = F.pad(seq, (0, T - seq.size(1))), F.pad(spos, (0, T - spos.size(1)))
    extra = dict(enc_self_attn=True) if live else {}
    extra.update(kw)
    m = LAMP(V, L, n_max, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=dff,
             d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', dropout=dropout, dec_dropout=dropout,
             no_enc_pos_embedding=not pos, label_adj_matrix=adj.clone() if adj is not None else None, label_mask=mask,
             dec_dropout2=False, int_preds=int_preds, **extra)
    m.load_state_dict(sd, strict=not int_preds)
    return m, sd, R.label_block_mask(adj, mask, L), seq, spos, h


def enc_blocked_mask(seq, adj=None):
    """lamp/Encoders.py:82 (key padding), with the complement of each sample's adjacency in its n x n corner (:85-89)."""
    B, T = seq.shape
    blocked = seq.eq(R.PAD).unsqueeze(1).expand(B, T, T).clone()
    for i, a in enumerate(adj or []):
        n = a.size(0)
        blocked[i, :n, :n] = a == 0
    return blocked


def live_encoder_ref(sd, seq, pos, n_head, adj=None):
    x = F.embedding(seq, sd['encoder.src_word_emb.weight'])
    if 'encoder.position_enc.weight' in sd:
        x = x + F.embedding(pos, sd['encoder.position_enc.weight'])
    blocked = enc_blocked_mask(seq, adj)
    attns = []
    for i in range(R.count_layers(sd, 'encoder')):
        p = 'encoder.layer_stack.%d.' % i
        x, a = R.mha(x, x, blocked, *R._mha_params(sd, p + 'slf_attn.'), n_head=n_head)
        x = R.ffn(x, *R._ffn_params(sd, p + 'pos_ffn.'))
        attns.append(a)
    return x, attns


def live_forward_ref(sd, seq, pos, n_head, label_blocked, adj=None, n_head2=None):
    """-> (logits, enc_output, encoder maps, (decoder self maps, enc-dec maps), intermediate predictions).  n_head2: heads of
    the label self-attention (default n_head)."""
    enc, enc_attns = live_encoder_ref(sd, seq, pos, n_head, adj)
    y, slf, encdec, int_outs = R.decoder_forward(sd, seq, enc, label_blocked, n_head, n_head2)
    w = sd['tgt_word_proj.linear.weight']
    return R.readout(y, w), enc, enc_attns, (slf, encdec), [R.readout(o, w) for o in int_outs[:-1]]


def random_graphs(lengths, seed=0):
    """Per-sample symmetric 0/1 input graphs WITH self-loops (no row is fully blocked)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in lengths:
        a = (torch.rand(n, n, generator=g) < 0.3).float()
        a = ((a + a.t()) > 0).float()
        a.fill_diagonal_(1.0)
        out.append(a)
    return out
