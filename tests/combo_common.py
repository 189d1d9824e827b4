"""Shared pieces of the option-combination tests (tests/test_combo_cpu.py, tests/test_combo_gpu.py): the model's options are flags
on ONE pass of lamp_amd/csrc/api.hip::forward (one workspace layout, one micro-batch loop, one `packed` decision, one label-mask
slot) and of lamp_amd/training.py::forward_train, and every other test turns them on one at a time.

* ``combo_forward_ref``: one composable restatement in the dtype of the state dict, assembled from the pieces the golden fixtures
  already pin -- oracle.lamp_ref's embedding, ``mha``, ``ffn``, ``decoder_forward`` and ``readout``, onehot_common's convolution
  front end, enc_live_common's encoder mask, sigmoid_common's and label_bias_common's attention.  The attention function is chosen
  PER BLOCK (the self-attention is the call whose key source IS its query source), so L == T would be no ambiguity.
* ``CASES``: the committed table.  ``python tests/combo_common.py`` printed it once (a greedy pairwise cover over AXES minus
  EXCLUDED) together with each case's seed: the first of 0..7 for which the fp32 CPU run of ``combo_oracle_run`` stays inside the
  gradient bars against the fp64 run (the ReLU-kink caveat of tests/fuzz_parity.py).  tests/test_combo_cpu.py recomputes the pair
  coverage from CASES and EXCLUDED and re-asserts the seeds.
* ``MUTANTS``: one-line interplay mistakes of the restatement; the CPU test shows that some committed case sees each of them.

Importable without a GPU."""
import collections
import itertools
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:     # run as a script (under pytest, conftest.py has done this)
    sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import enc_live_common as EC  # noqa: E402
import head_geometry_common as HG  # noqa: E402
import onehot_common as OC  # noqa: E402
from conftest import max_abs_diff  # noqa: E402
from label_bias_common import bias_sdpa  # noqa: E402
from oracle import lamp_ref as R  # noqa: E402
from sigmoid_common import sigmoid_sdpa  # noqa: E402

# the project's bars (tests/test_gpu_parity.py, test_enc_self_attn_gpu.py, test_matmul_precision_gpu.py); each is used as
# max(bar, 4 x the fp32 CPU restatement's own gap to fp64 on the case) -- the rule of tests/fuzz_parity.py
TOL_LOGIT, TOL_ENC, TOL_ENC_LIVE, TOL_MAP, TOL_MAP_LIVE, TOL_INT = 1e-4, 5e-5, 1e-4, 1e-5, 1e-4, 1e-4
INT_PRED_WEIGHT = 0.2     # lamp_amd/train.py: the weight of every intermediate prediction's loss term

# ------------------------------------------------------------------ the axes
AXES = collections.OrderedDict([
    ('front', ('tokpos', 'tok', 'onehot')),                      # tokens + positions, tokens alone, the one-hot front end
    ('enc', ('dead', 'live', 'packed', 'adj')),                  # dead self-attention; live: padded, packed switch, with graphs
    ('score', ('prior', 'none', 'inveye', 'sigmoid', 'bias', 'lbias')),   # label masks; sigmoid, constant / learned bias on 'prior'
    ('geom', ('std', 'gen', 'one')),
    ('slf', ('on', 'off')),                                      # the label self-attention, no_dec_self_att
    ('layers', ('1x1', '2x2', '3x2')),                           # encoder x decoder
    ('out', ('plain', 'attns', 'ints')),
    ('batch', ('whole', 'micro')),
    ('prec', ('highest', 'high')),                               # 'high': eval only
])
GEOMETRY = {
    'std': dict(d=64, h=4, h2=4, dk=16, dv=16),                  # d_k = d_v = d / h
    'gen': dict(d=64, h=3, h2=2, dk=24, dv=40),                  # head_geometry_common.GEOMS['G1']
    'one': dict(d=64, h=1, h2=2, dk=48, dv=64),                  # ... ['G2']: one head, no fc (d_v = d)
}
DFF, VOCAB = 96, 50
# shape of a case: (L, T of the token front end, lengths); the one-hot front end always reads T_in = 64 bases -> 32 encoder rows
SHAPES = {
    'S': dict(L=23, T=40, lengths=[40, 24, 16, 3, 1]),
    'S37': dict(L=37, T=40, lengths=[40, 24, 16, 3, 1]),         # crosses the 32-key mask word
    'T300': dict(L=23, T=300, lengths=[300, 257, 64, 20]),       # enc_live_common.SHAPES['B']: the 256-query / 64-key routes
    'L260': dict(L=260, T=40, lengths=[40, 24, 16, 3, 1]),       # head_geometry_common.GEOMS['G6']'s label count
}
ONEHOT_T_IN, ONEHOT_LENGTHS = 64, [64, 38, 26, 3, 1]
MASK_SCORES = ('prior', 'none', 'inveye')

# Pairs no case may hold, each with what the code does about it.  (Two refusals live INSIDE one axis and so are no pairs of
# this table: sigmoid attention with a label bias -- GraphDecoder.__init__ raises NotImplementedError, check_forward returns
# LAMP_E_UNSUPPORTED for LAMP_FWD_DEC_SIGMOID | LAMP_FWD_LABEL_BIAS -- and the one-hot front end without position rows --
# GraphEncoder.__init__ raises NotImplementedError, onehot_check returns LAMP_E_NULL.  test_combo_gpu.py asserts all of them.)
EXCLUDED = [
    (('front', 'onehot'), ('enc', 'adj'),
     'LAMP.forward and GraphEncoder.forward raise NotImplementedError: per-sample graphs are not served with the one-hot encoder'),
    (('score', 'bias'), ('slf', 'off'),
     'GraphDecoder.__init__ raises ValueError: without the label self-attention nothing would read the bias'),
    (('score', 'lbias'), ('slf', 'off'),
     'GraphDecoder.__init__ raises ValueError: without the label self-attention nothing would read the bias'),
]
# 'high' is an eval-forward matter (LAMP.matmul_precision: model.train() stays fp32): its cases have no training test


def excluded(a, b):
    return any({a, b} == {x, y} for x, y, _ in EXCLUDED)


def allowed_pairs():
    """Every pair of values from two different axes that no EXCLUDED entry names."""
    out = set()
    for (ax, vals), (bx, wals) in itertools.combinations(AXES.items(), 2):
        for v in vals:
            for w in wals:
                if not excluded((ax, v), (bx, w)):
                    out.add(((ax, v), (bx, w)))
    return out


def case_pairs(cfg):
    return {((ax, cfg[ax]), (bx, cfg[bx])) for ax, bx in itertools.combinations(AXES, 2)}


def n_int_preds(cfg):
    n_dec = int(cfg['layers'][2])
    return n_dec * (2 if cfg['slf'] == 'on' else 1) - 1


def valid(cfg):
    """No excluded pair, and an 'ints' case has an intermediate prediction to compare (1x1 without the label self-attention has none)."""
    if any(excluded(a, b) for a, b in case_pairs(cfg)):
        return False
    return cfg['out'] != 'ints' or n_int_preds(cfg) >= 1


# ------------------------------------------------------------------ the committed table (printed by __main__, pasted in)
def _c(name, front, enc, score, geom, slf, layers, out, batch, prec, shape='S', seed=0):
    return dict(name=name, front=front, enc=enc, score=score, geom=geom, slf=slf, layers=layers, out=out, batch=batch, prec=prec,
                shape=shape, seed=seed)


CASES = []     # filled below by _TABLE


def case(name):
    return next(c for c in CASES if c['name'] == name)


def training_cases():
    return [c for c in CASES if c['prec'] == 'highest']


# ------------------------------------------------------------------ building a case
Built = collections.namedtuple('Built', 'model sd blocked seq pos tgt adj bias g')


def make_bias(L, blocked, seed):
    """N(0, 2) with about 20 % -inf; every row keeps the first key its mask allows (tests/test_label_bias_gpu.py's model bias)."""
    gen = torch.Generator().manual_seed(31 + seed)
    bias = 2.0 * torch.randn(L, L, generator=gen)
    drop = torch.rand(L, L, generator=gen) < 0.2
    allowed = ~blocked if blocked is not None else torch.ones(L, L, dtype=torch.bool)
    drop[torch.arange(L), allowed.float().argmax(dim=1)] = False
    return bias.masked_fill(drop, float('-inf'))


def case_geometry(cfg):
    s = SHAPES[cfg['shape']]
    onehot = cfg['front'] == 'onehot'
    g = dict(GEOMETRY[cfg['geom']], dff=DFF, V=9 if onehot else VOCAB, L=s['L'], T=ONEHOT_T_IN if onehot else s['T'],
             lengths=list(ONEHOT_LENGTHS if onehot else s['lengths']), n_enc=int(cfg['layers'][0]), n_dec=int(cfg['layers'][2]),
             mask=cfg['score'] if cfg['score'] in MASK_SCORES else 'prior', pos=cfg['front'] != 'tok',
             no_dec_self_att=cfg['slf'] == 'off')
    return g


def combo_build(cfg, seed=None, learn=None):
    """-> Built(LAMP on the CPU, state dict, label block mask, src_seq, src_pos, targets, adj list or None, bias or None,
    geometry dict).  ``learn``: override of learn_label_bias (the constant-bias twin of an 'lbias' case)."""
    from lamp_amd import synthetic
    seed = cfg['seed'] if seed is None else seed
    g = case_geometry(cfg)
    onehot = cfg['front'] == 'onehot'
    L, T, lengths = g['L'], g['T'], g['lengths']
    sd = HG.make_state_dict(g['V'], L, T, g['d'], g['dff'], g['h'], g['h2'], g['dk'], g['dv'], g['n_enc'], g['n_dec'],
                            pos_emb=g['pos'], seed=seed, no_dec_self_att=g['no_dec_self_att'])
    if onehot:     # the identity table and the two convolutions as lamp_amd.synthetic draws them
        extra = synthetic.make_onehot_state_dict(L, T, g['d'], g['dff'], 4, 1, 1, seed=seed)
        for k in ('encoder.src_word_emb.weight', 'encoder.conv1.weight', 'encoder.conv1.bias', 'encoder.conv2.weight',
                  'encoder.conv2.bias'):
            sd[k] = extra[k]
        seq, pos = OC.make_dna(len(lengths), T, lengths=lengths, seed=seed)
    else:
        seq, pos = R.make_batch(len(lengths), g['V'], T, lengths=lengths, seed=seed)
    label_adj = R.make_adjacency(L, 0.2, seed) if g['mask'] == 'prior' else None
    blocked = R.label_block_mask(label_adj, g['mask'], L)
    bias = make_bias(L, blocked, seed) if cfg['score'] in ('bias', 'lbias') else None
    kw = {}
    if onehot:
        kw['onehot'] = True
    if cfg['enc'] != 'dead':
        kw['enc_self_attn'] = True
    if cfg['score'] == 'sigmoid':
        kw['dec_attn_type'] = 'sigmoid'
    if bias is not None:
        kw['label_bias'] = bias
        kw['learn_label_bias'] = (cfg['score'] == 'lbias') if learn is None else learn
    m = HG.build_model(g, sd, label_adj, n_max_seq=T, **kw)
    adj = EC.random_graphs(lengths, seed=3 + seed) if cfg['enc'] == 'adj' else None
    tgt = (torch.rand(len(lengths), L, generator=torch.Generator().manual_seed(seed + 1)) < 0.2).float()
    return Built(m, sd, blocked, seq, pos, tgt, adj, bias, g)


def micro_batch(cfg):
    """Samples per pass of a micro-batched case: 1 <= mb < B and B no multiple of mb."""
    B = len(case_geometry(cfg)['lengths'])
    return 2 if B % 2 else 3


# ------------------------------------------------------------------ the composable restatement
MUTANTS = collections.OrderedDict([
    # name: (the mistake, which cases hold the pair in question)
    ('bias_in_encdec', ('mutant: the bias (its finite entries) is also added in the enc-dec block, at columns k mod L',
                        lambda c: c['score'] in ('bias', 'lbias'))),
    ('bias_replaces_mask', ('mutant: the bias goes into the label-mask slot before the mask is folded into it, not on top of it',
                            lambda c: c['score'] in ('bias', 'lbias'))),
    ('sigmoid_one_block', ('mutant: sigmoid in the label self-attention only, the enc-dec block stays softmax',
                           lambda c: c['score'] == 'sigmoid')),
    # (geometry 'one': its widths divide by either head count; at 'gen' the swap does not even reshape)
    ('heads_swapped', ('mutant: n_head and n_head2 swapped in the decoder', lambda c: c['geom'] == 'one' and c['slf'] == 'on')),
    ('adj_ignored', ('mutant: the per-sample graphs are ignored', lambda c: c['enc'] == 'adj')),
    ('onehot_mask_strided', ('mutant: the one-hot key-padding mask read from seq[:, :T_in] with stride 2 instead of seq[:, :T2]',
                             lambda c: c['front'] == 'onehot')),
    ('onehot_pos_T_in', ('mutant: the one-hot position rows indexed for T_in (stride 2) instead of the first T2',
                         lambda c: c['front'] == 'onehot')),
    ('micro_sample0', ("mutant: a micro-batch's adj and encoder mask taken from sample 0 on instead of from b0 on",
                       lambda c: c['batch'] == 'micro' and c['enc'] != 'dead')),
])


def _without_encoder_layers(sd):
    return {k: v for k, v in sd.items() if not k.startswith('encoder.layer_stack.')}


def _decoder(sd, seq2, enc, label_blocked, n_head, n_head2, fn_enc, fn_slf):
    """oracle.lamp_ref.decoder_forward with the attention function chosen per block: the label self-attention is the ``mha`` call
    whose key source is its query source."""
    real_mha, real_sdpa = R.mha, R.sdpa

    def mha(xq, xkv, blocked, *a, **kw):
        R.sdpa = (fn_slf if xkv is xq else fn_enc) or real_sdpa
        try:
            return real_mha(xq, xkv, blocked, *a, **kw)
        finally:
            R.sdpa = real_sdpa
    R.mha = mha
    try:
        return R.decoder_forward(sd, seq2, enc, label_blocked, n_head, n_head2)
    finally:
        R.mha = real_mha


def combo_forward_ref(sd, seq, pos, cfg, blocked=None, adj=None, bias=None, mutant=None):
    """-> (logits, enc, encoder maps, (label self maps, enc-dec maps), intermediate predictions), in the dtype of ``sd``.
    ``blocked``: the (L, L) label block mask or None; ``adj``: the per-sample graphs of an 'adj' case; ``bias``: the (L, L) score
    bias of a 'bias' / 'lbias' case (a leaf that requires grad for the learned one); ``mutant``: a key of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    g = GEOMETRY[cfg['geom']]
    h, h2 = g['h'], g['h2']
    live = cfg['enc'] != 'dead'
    # front end
    if cfg['front'] == 'onehot':     # onehot_common.onehot_encoder_ref without the layers: convolutions + position rows
        p_in = pos[:, ::2] if mutant == 'onehot_pos_T_in' else pos
        x, seq2 = OC.onehot_encoder_ref(_without_encoder_layers(sd), seq, p_in)
        if mutant == 'onehot_mask_strided':
            seq2 = seq[:, ::2][:, :x.size(1)]
    else:                            # oracle.lamp_ref.encoder_forward without the layers: token (+ position) embedding
        x, _ = R.encoder_forward(_without_encoder_layers(sd), seq, pos, h)
        seq2 = seq
    # encoder layers: the loop of enc_live_common.live_encoder_ref (the dead mode discards the attention output, keeps its map)
    graphs = None if mutant == 'adj_ignored' else adj
    enc_blocked = EC.enc_blocked_mask(seq2, graphs)
    if mutant == 'micro_sample0':
        mb = micro_batch(cfg)
        sizes = [min(mb, seq2.size(0) - b0) for b0 in range(0, seq2.size(0), mb)]
        parts = [EC.enc_blocked_mask(seq2[:nb], graphs[:nb] if graphs else None) for nb in sizes]
        enc_blocked = torch.cat(parts)
    enc_maps = []
    for i in range(R.count_layers(sd, 'encoder')):
        p = 'encoder.layer_stack.%d.' % i
        o, a = R.mha(x, x, enc_blocked, *R._mha_params(sd, p + 'slf_attn.'), n_head=h)
        x = R.ffn(o if live else x, *R._ffn_params(sd, p + 'pos_ffn.'))
        enc_maps.append(a)
    # decoder: the attention function per block
    fn_enc = fn_slf = None
    if cfg['score'] == 'sigmoid':
        fn_slf = sigmoid_sdpa
        fn_enc = None if mutant == 'sigmoid_one_block' else sigmoid_sdpa
    label_blocked = blocked
    if bias is not None:
        def fn_slf(q, k, v, blocked=None, temperature=None):
            return bias_sdpa(q, k, v, bias, blocked, temperature)
        if mutant == 'bias_in_encdec':
            def fn_enc(q, k, v, blocked=None, temperature=None):
                wrong = torch.nan_to_num(bias, neginf=0.0)[:, torch.arange(k.size(1)) % bias.size(1)]     # (finite: no NaN rows)
                return bias_sdpa(q, k, v, wrong, blocked, temperature)
        if mutant == 'bias_replaces_mask':
            label_blocked = None
    if mutant == 'heads_swapped':
        h, h2 = h2, h
    y, slf, encdec, int_outs = _decoder(sd, seq2, x, label_blocked, h, h2, fn_enc, fn_slf)
    w = sd['tgt_word_proj.linear.weight']
    # lamp/Models.py:129-132: the intermediate predictions read out through a detached copy of the projection
    return R.readout(y, w), x, enc_maps, (slf, encdec), [R.readout(o, w.detach()) for o in int_outs[:-1]]


def combo_loss(cfg, logits, ips, tgt):
    """BCE on the logits, plus INT_PRED_WEIGHT x BCE on every intermediate prediction of an 'ints' case."""
    loss = F.binary_cross_entropy_with_logits(logits, tgt)
    if cfg['out'] == 'ints':
        for p in ips:
            loss = loss + INT_PRED_WEIGHT * F.binary_cross_entropy_with_logits(p, tgt)
    return loss


def combo_oracle_run(cfg, b, dtype=torch.float64):
    """The restatement's forward, combo_loss and autograd in ``dtype`` on Built ``b`` -> (logits, enc, loss, {parameter name:
    gradient or None}); the learned bias' gradient under 'decoder.label_bias'."""
    sdx = {k: v.detach().clone().to(dtype).requires_grad_(True) if v.is_floating_point() else v for k, v in b.sd.items()}
    bias = b.bias
    if bias is not None:
        bias = bias.detach().clone().to(dtype).requires_grad_(cfg['score'] == 'lbias')
    logits, enc, _, _, ips = combo_forward_ref(sdx, b.seq, b.pos, cfg, b.blocked, b.adj, bias)
    loss = combo_loss(cfg, logits, ips, b.tgt.to(dtype))
    loss.backward()
    grads = {k: (v.grad if v.is_floating_point() else None) for k, v in sdx.items()}
    if cfg['score'] == 'lbias':
        grads['decoder.label_bias'] = bias.grad
    return logits.detach(), enc.detach(), loss.item(), grads


def fp32_oracle_is_inside(cfg, seed):
    """head_geometry_common.fp32_oracle_is_inside for a case of this table -> (bool, worst gradient error / its bar)."""
    b = combo_build(cfg, seed)
    l64, _, _, g64 = combo_oracle_run(cfg, b, torch.float64)
    l32, _, _, g32 = combo_oracle_run(cfg, b, torch.float32)
    ok = max_abs_diff(l32, l64) < TOL_LOGIT
    worst = 0.0
    for pname in g64:
        if g64[pname] is None:
            continue
        ref = HG.reference_gradient(g64, pname)
        bar = HG.GRAD_RTOL * ref.abs().max().item() + HG.GRAD_ATOL
        worst = max(worst, max_abs_diff(HG.reference_gradient(g32, pname), ref) / bar)
    return ok and worst <= 1.0, worst


# ------------------------------------------------------------------ the table
# name front enc score geom slf layers out batch prec shape seed.  c00 .. c31: the generator's output as printed.  c32 and c33 are
# added by hand: pairwise cover alone never put the packed switch on a model that really takes the packed route (token front end,
# d_k = d_v, more than one head -- everywhere else the switch falls back to the padded route, and the test asserts that).
_TABLE = """
c00 tokpos dead lbias gen on 2x2 attns whole highest L260 0
c01 onehot live sigmoid std on 1x1 ints micro highest L260 0
c02 tok packed inveye one off 1x1 plain whole highest S 0
c03 tok adj prior gen off 3x2 ints micro highest T300 0
c04 tokpos live none one off 2x2 attns micro highest S 0
c05 tokpos adj bias std on 3x2 plain whole highest S 0
c06 onehot packed prior std off 2x2 attns whole highest S37 0
c07 onehot dead inveye one on 3x2 ints micro highest S 0
c08 onehot packed none gen on 3x2 plain micro highest S 0
c09 tok dead sigmoid std off 2x2 plain whole highest S37 0
c10 tok live bias gen on 1x1 attns whole highest S 0
c11 tokpos adj prior one on 1x1 ints whole highest S 0
c12 onehot live lbias one on 3x2 plain micro highest S37 0
c13 tokpos packed bias one on 2x2 ints micro highest S 0
c14 tokpos adj sigmoid one on 3x2 attns micro highest S 0
c15 tok adj none std on 2x2 ints whole highest S37 0
c16 tok dead lbias std on 1x1 ints whole highest S 0
c17 tokpos live inveye std off 2x2 attns micro highest S 0
c18 onehot packed sigmoid gen off 3x2 ints whole highest S37 0
c19 tokpos adj inveye gen off 3x2 ints micro highest S 0
c20 onehot dead none gen on 1x1 ints whole highest S 0
c21 onehot dead prior one on 1x1 plain micro highest S37 0
c22 onehot dead bias std on 3x2 ints micro highest S 0
c23 onehot live prior std on 3x2 plain micro highest S 0
c24 onehot packed lbias std on 1x1 ints whole highest S37 0
c25 tok adj lbias gen on 2x2 ints whole highest S 0
c26 onehot packed prior one on 3x2 attns micro high S 0
c27 tok live none gen off 2x2 plain whole high S37 0
c28 tokpos dead inveye std on 1x1 ints micro high S 0
c29 tok adj lbias one on 2x2 ints micro high S 0
c30 tokpos dead sigmoid gen off 2x2 ints micro high S37 0
c31 tok dead bias one on 2x2 attns micro high S 0
c32 tokpos packed prior std on 2x2 plain micro highest T300 0
c33 tok packed lbias std on 3x2 ints whole highest S37 0
"""


def _parse(table):
    out = []
    for line in table.strip().splitlines():
        f = line.split()
        out.append(_c(f[0], *f[1:10], shape=f[10], seed=int(f[11])))
    return out


CASES.extend(_parse(_TABLE))


# ------------------------------------------------------------------ the generator (run once; its output is _TABLE)
def _greedy_cover():
    """Cases until every allowed pair is held.  First 'highest' cases until every pair of the other axes is held -- those run the
    backward too -- then 'high' cases until every value has met 'high'.  Each step takes, axis by axis over a few axis orders,
    the value that covers the most pairs still open, and keeps the best candidate."""
    import random
    rng = random.Random(0)
    names = list(AXES)
    cases = []
    for prec in AXES['prec']:
        todo = {p for p in allowed_pairs() if (p[1] == ('prec', 'high') if prec == 'high' else p[1][0] != 'prec')}
        while todo:
            best, best_gain = None, -1
            for _ in range(60):
                order = [n for n in names if n != 'prec']
                rng.shuffle(order)
                cfg = {'prec': prec}
                for ax in order:
                    def gain(v):
                        trial = dict(cfg, **{ax: v})
                        return sum(1 for bx in trial if bx != ax and
                                   (tuple(sorted([(ax, v), (bx, trial[bx])], key=lambda t: names.index(t[0]))) in todo))
                    ok = [v for v in AXES[ax] if not any(excluded((ax, v), (bx, cfg[bx])) for bx in cfg)]
                    rng.shuffle(ok)
                    cfg[ax] = max(ok, key=gain)
                if not valid(cfg):
                    continue
                g = len(case_pairs(cfg) & todo)
                if g > best_gain:
                    best, best_gain = cfg, g
            assert best is not None and best_gain > 0
            cases.append(best)
            todo -= case_pairs(best)
    return cases


def _shape_for(i, cfg, used):
    """No more than four larger shapes, all in cases that train: T = 300 for a live encoder on the really packed route and for one
    with graphs, L = 260 for one bias and one sigmoid case; L = 37 for every third of the rest."""
    if cfg['prec'] == 'highest' and cfg['front'] != 'onehot':
        if cfg['enc'] == 'packed' and cfg['geom'] == 'std' and not used['T300p']:
            used['T300p'] = 1
            return 'T300'
        if cfg['enc'] == 'adj' and not used['T300a']:
            used['T300a'] = 1
            return 'T300'
    if cfg['prec'] == 'highest' and cfg['slf'] == 'on':
        for kind, scores in (('L260b', ('bias', 'lbias')), ('L260s', ('sigmoid',))):
            if cfg['score'] in scores and not used[kind]:
                used[kind] = 1
                return 'L260'
    return 'S37' if i % 3 == 0 else 'S'


if __name__ == '__main__':
    if CASES:      # the seed choice of the committed table, re-run
        for c in CASES:
            if c['prec'] != 'highest':
                continue
            for s in range(8):
                inside, frac = fp32_oracle_is_inside(c, s)
                print('%-6s seed %d: fp32 CPU restatement %s (worst gradient error %.3f of its bar)%s' % (
                    c['name'], s, 'inside' if inside else 'OUTSIDE', frac, '  <- recorded' if s == c['seed'] else ''))
                if inside:
                    break
    else:          # the table itself
        used = collections.defaultdict(int)
        for i, cfg in enumerate(_greedy_cover()):
            cfg = dict(cfg, name='c%02d' % i, shape='S', seed=0)
            cfg['shape'] = _shape_for(i, cfg, used)
            seed = next((s for s in range(8) if cfg['prec'] != 'highest' or fp32_oracle_is_inside(cfg, s)[0]), None)
            assert seed is not None, cfg
            print(' '.join([cfg['name']] + [cfg[ax] for ax in AXES] + [cfg['shape'], str(seed)]))
