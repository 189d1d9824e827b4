"""No GPU: the option-combination table and its restatement (tests/combo_common.py) are checked for themselves -- the table
covers every allowed pair, the restatement IS every single-option reference of the suite when one option is on, each interplay
mutant moves some committed case, and the fp32 CPU run of every training case stays inside the gradient bars."""
import itertools

import pytest
import torch

import combo_common as CC
import enc_live_common as EC
import head_geometry_common as HG
import onehot_common as OC
from conftest import max_abs_diff
from oracle import lamp_ref as R


# ------------------------------------------------------------------ 1. the table
def test_table_is_well_formed():
    names = [c['name'] for c in CC.CASES]
    assert len(names) == len(set(names)) and 30 <= len(names) <= 45
    for c in CC.CASES:
        assert all(c[ax] in vals for ax, vals in CC.AXES.items()), c
        assert CC.valid(c) and c['shape'] in CC.SHAPES and 0 <= c['seed'] <= 7, c
        B = len(CC.case_geometry(c)['lengths'])
        assert 1 <= CC.micro_batch(c) < B and B % CC.micro_batch(c)
    large = [c['name'] for c in CC.CASES if c['shape'] in ('T300', 'L260')]
    assert len(large) <= 4 and sum(c['shape'] == 'S37' for c in CC.CASES) >= 4
    # the L = 260 shapes sit on a bias and on a sigmoid combination, T = 300 on live encoders, one of them really packed
    assert {('bias' if c['score'] in ('bias', 'lbias') else c['score']) for c in CC.CASES if c['shape'] == 'L260'} <= {'bias', 'sigmoid'}
    assert all(c['enc'] != 'dead' and c['front'] != 'onehot' for c in CC.CASES if c['shape'] == 'T300')
    assert any(c['enc'] == 'packed' and c['geom'] == 'std' and c['front'] != 'onehot' for c in CC.CASES)
    assert sum(c['out'] == 'ints' for c in CC.training_cases()) >= 3 and sum(c['out'] == 'attns' for c in CC.training_cases()) >= 2


def test_every_allowed_pair_is_in_a_case_and_in_a_training_case():
    allowed = CC.allowed_pairs()
    n_all = sum(len(a) * len(b) for a, b in itertools.combinations(CC.AXES.values(), 2))
    assert len(allowed) == n_all - len(CC.EXCLUDED)
    held = set().union(*(CC.case_pairs(c) for c in CC.CASES))
    assert not held - allowed, 'a case holds an excluded pair: %s' % sorted(held - allowed)
    assert not allowed - held, 'pairs no case holds: %s' % sorted(allowed - held)
    # ... and forward AND backward: every pair that does not involve the precision is in a case that trains
    trained = set().union(*(CC.case_pairs(c) for c in CC.training_cases()))
    need = {p for p in allowed if p[1][0] != 'prec'}
    assert not need - trained, 'pairs no training case holds: %s' % sorted(need - trained)


# ------------------------------------------------------------------ 2. anchoring: one option on = the suite's own reference
def _equal(got, want):
    """Tensors and nested lists / tuples of them (None included), torch.equal leaf by leaf."""
    if isinstance(want, (list, tuple)):
        assert len(got) == len(want)
        return all(_equal(a, b) for a, b in zip(got, want))
    if want is None:
        return got is None
    return torch.equal(got, want)


def _cfg(**kw):
    base = dict(name='anchor', front='tokpos', enc='dead', score='prior', geom='gen', slf='on', layers='2x2', out='plain',
                batch='whole', prec='highest', shape='S', seed=0)
    base.update(kw)
    return base


def _built64(cfg):
    b = CC.combo_build(cfg)
    return b, R.to_dtype(b.sd, torch.float64)


@pytest.mark.parametrize('kw', [dict(), dict(score='none', geom='std'), dict(score='inveye', front='tok', geom='one'),
                                dict(slf='off', layers='3x2')], ids=['prior_gen', 'none_std', 'inveye_tok_one', 'no_dec_self_att'])
def test_no_option_is_the_oracle(kw):
    cfg = _cfg(**kw)
    b, sd64 = _built64(cfg)
    g = b.g
    with torch.no_grad():
        got = CC.combo_forward_ref(sd64, b.seq, b.pos, cfg, b.blocked)
        logits, enc, enc_attns, (slf, encdec) = R.forward(sd64, b.seq, b.pos, g['h'], b.blocked, n_head2=g['h2'], return_attns=True)
        ips = R.forward(sd64, b.seq, b.pos, g['h'], b.blocked, n_head2=g['h2'], int_preds=True)[2]
    assert _equal(got, (logits, enc, enc_attns[0], (slf, encdec), ips))
    assert len(ips) == CC.n_int_preds(cfg)


@pytest.mark.parametrize('enc', ['live', 'adj'])
def test_live_encoder_is_the_live_reference(enc):
    cfg = _cfg(enc=enc)
    b, sd64 = _built64(cfg)
    assert (b.adj is not None) == (enc == 'adj')
    with torch.no_grad():
        got = CC.combo_forward_ref(sd64, b.seq, b.pos, cfg, b.blocked, adj=b.adj)
        want = HG.live_forward_ref(sd64, b.seq, b.pos, b.g, b.blocked, adj=b.adj)
    assert _equal(got, want)


def test_sigmoid_is_the_sigmoid_reference():
    cfg = _cfg(score='sigmoid')
    b, sd64 = _built64(cfg)
    with torch.no_grad():
        got = CC.combo_forward_ref(sd64, b.seq, b.pos, cfg, b.blocked)
        want = HG.sigmoid_forward_ref(sd64, b.seq, b.pos, b.g, b.blocked)
    assert _equal(got, want)


@pytest.mark.parametrize('score', ['bias', 'lbias'])
def test_label_bias_is_the_label_bias_reference(score):
    cfg = _cfg(score=score)
    b, sd64 = _built64(cfg)
    assert torch.isinf(b.bias).any() and torch.isfinite(b.bias[b.blocked]).any()
    with torch.no_grad():
        got = CC.combo_forward_ref(sd64, b.seq, b.pos, cfg, b.blocked, bias=b.bias.double())
        want = HG.label_bias_forward_ref(sd64, b.seq, b.pos, b.g, b.blocked, b.bias.double())
    assert _equal(got, want)


@pytest.mark.parametrize('score', ['none', 'prior'])
def test_onehot_is_the_onehot_reference(score):
    cfg = _cfg(front='onehot', geom='std', score=score)
    b, sd64 = _built64(cfg)
    with torch.no_grad():
        got = CC.combo_forward_ref(sd64, b.seq, b.pos, cfg, b.blocked)
        logits, enc, maps = OC.onehot_forward_ref(sd64, b.seq, b.pos, b.g['h'], b.blocked)
        ips = OC.onehot_forward_ref(sd64, b.seq, b.pos, b.g['h'], b.blocked, int_preds=True)[2]
    assert enc.size(1) == CC.ONEHOT_T_IN // 2
    assert _equal((got[0], got[1], got[3], got[4]), (logits, enc, maps, ips))


def test_onehot_live_is_the_composition_of_the_live_encoder_test():
    from test_enc_self_attn_gpu import _onehot_live_ref
    cfg = _cfg(front='onehot', enc='live', geom='std', score='none')
    b, sd64 = _built64(cfg)
    with torch.no_grad():
        got = CC.combo_forward_ref(sd64, b.seq, b.pos, cfg, b.blocked)
        want = _onehot_live_ref(sd64, b.seq, b.pos, b.g['h'])
    assert _equal((got[0], got[1]), want)


def test_the_model_is_built_as_the_case_says():
    """combo_build's LAMP carries the options of its case (checked on the CPU module: nothing runs)."""
    for c in CC.CASES:
        m, g = CC.combo_build(c).model, CC.case_geometry(c)
        assert m.onehot == (c['front'] == 'onehot') and m.enc_self_attn == (c['enc'] != 'dead')
        assert hasattr(m.encoder, 'position_enc') == (c['front'] != 'tok')
        assert (m.dec_attn_type == 'sigmoid') == (c['score'] == 'sigmoid')
        assert (m.decoder.label_bias_f32 is not None) == (c['score'] in ('bias', 'lbias'))
        assert (m.decoder.label_bias is not None) == (c['score'] == 'lbias')
        assert all(hasattr(l, 'slf_attn') == (c['slf'] == 'on') for l in m.decoder.layer_stack)
        assert (len(m.encoder.layer_stack), len(m.decoder.layer_stack)) == (g['n_enc'], g['n_dec'])
        assert (m.decoder.label_mask is None) == (c['score'] == 'none')
        if c['score'] in ('bias', 'lbias'):     # the row stride of the bias buffer differs from L wherever L is no multiple of 4
            assert m.decoder.label_bias_f32.size(1) == (g['L'] + 3) & ~3


# ------------------------------------------------------------------ 3. sensitivity: every mutant is seen by a committed case
_MOVED = {}


def _moved(c, mutant):
    key = (c['name'], mutant)
    if key not in _MOVED:
        b, sd64 = _built64(c)
        bias = b.bias.double() if b.bias is not None else None
        with torch.no_grad():
            ref = CC.combo_forward_ref(sd64, b.seq, b.pos, c, b.blocked, b.adj, bias)[0]
            mut = CC.combo_forward_ref(sd64, b.seq, b.pos, c, b.blocked, b.adj, bias, mutant=mutant)[0]
        _MOVED[key] = max_abs_diff(mut, ref)     # (a NaN the mutant makes counts as inf)
    return _MOVED[key]


@pytest.mark.parametrize('mutant', list(CC.MUTANTS))
def test_a_committed_case_sees_the_mutant(mutant):
    doc, applies = CC.MUTANTS[mutant]
    assert doc.startswith('mutant:')
    cases = [c for c in CC.CASES if applies(c)]
    assert cases, 'no case holds the pair this mutant is about'
    moved = {c['name']: _moved(c, mutant) for c in cases}
    print('%s: fp64 logits move by %s' % (mutant, ', '.join('%s %.2e' % kv for kv in sorted(moved.items()))))
    assert max(moved.values()) >= 10 * CC.TOL_LOGIT


# ------------------------------------------------------------------ 4. ReLU kinks: the recorded seeds
@pytest.mark.parametrize('name', [c['name'] for c in CC.training_cases()])
def test_fp32_restatement_is_inside_the_gradient_bars(name):
    c = CC.case(name)
    inside, worst = CC.fp32_oracle_is_inside(c, c['seed'])
    print('%s seed %d: worst fp32 gradient error %.3f of its bar' % (name, c['seed'], worst))
    assert inside
