"""-m gpu: the eval path's cached tables across a model's life cycle (tests/lifecycle_common.py).

The invariant: after every supported operation on a model, its next eval forward is BIT-EQUAL to the forward of a second model of
the same construction that has just loaded the first one's state_dict (load_state_dict invalidates wholesale, so the twin never
depends on the keys under test), and both stay inside the project's bars against the fp64 restatement of the current state dict
(max(bar, 4 x the fp32 CPU restatement's own gap to fp64): the rule of tests/fuzz_parity.py).  No test here flips train() / eval()
between a change and the forward that must see it, unless the flip is what it is about.

a. every parameter, one at a time, in place -- and which of them moved the output;
b. the control: ONE table put back stale under the fresh key must be seen, or the shape does not read that table;
c. whole-model mutators: optimizers, load_state_dict, copy_, .data =, device and dtype round trips, a training step, the route
   switches, evaluate.test_epoch, and the documented exception (an in-place write through .data);
d. replacing a Parameter, a submodule, tying two weights;
e. copy.deepcopy, torch.save / torch.load, AveragedModel: nothing shared with the original.

Every test prints its fp64 errors as fractions of their bars ("LIFECYCLE ..." lines)."""
import collections
import copy
import io
import zlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import lifecycle_common as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from lamp_amd import _native as N
    N.lib()  # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


class Life:
    """A family's model on the device after its first forward, its twin, and the checks."""

    def __init__(self, family, dev, model=None):
        self.case, self.dev, self.twin = LC.make(family), dev, None
        self.m = self.case.model.to(dev).eval() if model is None else model
        if model is None:
            self.check('start')

    def run(self, m=None):
        return LC.run(self.case, self.m if m is None else m, self.dev)

    def truth(self, m=None):
        """The freshly loaded twin's forward."""
        self.twin = LC.fresh(self.case, self.m if m is None else m, self.dev, into=self.twin)
        return self.run(self.twin)

    def check(self, what, m=None, fp64=True):
        """m's forward == its twin's, bit for bit; and inside the fp64 bars -> the forward."""
        m = self.m if m is None else m
        assert not m.training
        out = self.run(m)
        assert LC.same(out, self.truth(m)), '%s %s: not the freshly loaded model\'s bits' % (self.case.family, what)
        assert torch.isfinite(out[0]).all()
        if fp64:
            frac = LC.fp64_fractions(self.case, m, out)
            print('LIFECYCLE %s %s: %s' % (self.case.family, what, ' '.join('%s %.3f' % kv for kv in sorted(frac.items()))))
            assert max(frac.values()) <= 1.0, (what, frac)
        return out

    def perturb_all(self, m=None):
        for name, p in (self.m if m is None else m).named_parameters():
            LC.perturb(name, p)


def _assign_grads(m, nan_in=None):
    """p.grad = a fixed randn per parameter name; exactly 0 where a learned label bias is -inf (as its backward gives it)."""
    for name, p in m.named_parameters():
        if not p.requires_grad:
            continue
        gen = torch.Generator().manual_seed(zlib.crc32(('grad:' + name).encode()))
        g = (0.1 * torch.randn(p.shape, generator=gen)).to(p.device)
        if name == 'decoder.label_bias':
            g = g.masked_fill(torch.isinf(p.detach()), 0.0)
        if name == nan_in:
            g.view(-1)[0] = float('nan')
        p.grad = g


def _groups(m, **decay):
    """The trainable parameters; a learned label bias in a group of its own without decay (its -inf entries times a decay are NaN
    in any optimizer)."""
    rest = [p for n, p in m.named_parameters() if p.requires_grad and n != 'decoder.label_bias']
    groups = [dict(params=rest, **decay)]
    if getattr(m.decoder, 'label_bias', None) is not None:
        groups.append(dict(params=[m.decoder.label_bias], weight_decay=0.0))
    return groups


# ------------------------------------------------------------------ a. every parameter, one at a time
@pytest.mark.parametrize('family', LC.FAMILIES)
def test_every_parameter_in_place(dev, family):
    """In eval mode, with no train() / eval() in between: perturb one parameter in place, forward, compare with the reloaded twin.
    The parameters that moved the twin's output must include every tensor of the code's own table lists (_chain_weights,
    _enc_chain_weights, _gemm_pack_weights, _fold_weights, _onehot_weights, the two hoist operands, decoder.label_bias) -- none of
    them is invisible at these inputs -- and be everything but the dead encoder's self-attention, which must move nothing."""
    life = Life(family, dev)
    m = life.m
    prev, moved, names = life.run(), set(), []
    for name, p in m.named_parameters():
        names.append(name)
        LC.perturb(name, p)
        out, want = life.run(), life.truth()
        assert LC.same(out, want), 'stale after an in-place change of %s' % name
        if not LC.same(want, prev):
            moved.add(name)
        prev = want
    feeding = LC.feeding_names(m, family)
    assert (family == 'bias') == (not feeding)
    assert feeding <= moved, sorted(feeding - moved)
    dead = set() if life.case.live else {n for n in names if n.startswith('encoder.layer_stack.') and '.slf_attn.' in n}
    assert len(dead) == (0 if life.case.live else 6 * len(m.encoder.layer_stack))     # w_qs, w_ks, w_vs, fc, the LayerNorm pair
    assert moved == set(names) - dead, (sorted(set(names) - dead - moved), sorted(moved & dead))
    life.check('after the sweep')


# ------------------------------------------------------------------ b. the control
CONTROL = [(f, t) for f in LC.FAMILIES for t in LC.TABLES[f] if t != 'lbias']


@pytest.mark.parametrize('family,table', CONTROL)
def test_a_stale_table_is_seen(dev, family, table):
    """Perturb only the table's weights, forward, then put the OLD table back under the fresh key (through the test: no product
    switch does this): the forward must now differ from the twin's and leave the fp64 bar.  If it did not, the table would not
    be read at this shape and every other test here would prove nothing about it.  No table is exempt: hoisted query, decoder
    chain packs, GEMM packs, K / V packs and both folded tables at 'tokpos', the token-only fold at 'tok', the encoder's and the
    decoder's chain packs at 'live', the one-hot tables at 'onehot' (the folded bias buffer: the next test)."""
    life = Life(family, dev)
    m = life.m
    old_key, old_built = m._native_cache
    names = {id(p): n for n, p in m.named_parameters()}
    for w in LC.table_weights(m, table):
        LC.perturb(names[id(w)], w)
    want = life.check('fresh %s' % table)
    key, built = m._native_cache
    assert key != old_key and built is not old_built
    m._native_cache = (key, LC.stale_built(built, old_built, table))
    stale = life.run()
    assert m._native_cache[0] == key, 'the stale table was rebuilt: the control did not run'
    frac = LC.fp64_fractions(life.case, m, stale)
    print('LIFECYCLE %s stale %s: %s' % (family, table, ' '.join('%s %.3f' % kv for kv in sorted(frac.items()))))
    assert not LC.same(stale, want), 'a stale %s table changes nothing: it is not read at this shape' % table
    assert max(frac.values()) > 1.0, frac
    m._native_cache = (key, built)
    assert LC.same(life.run(), want)


def test_a_stale_bias_buffer_is_seen(dev):
    """The folded label-bias buffer (GraphDecoder.current_label_bias keeps its own key): the old contents under the new key."""
    life = Life('lbias', dev)
    m = life.m
    buf = m.decoder.label_bias_f32
    old = buf.clone()
    LC.perturb('decoder.label_bias', m.decoder.label_bias)
    want = life.check('fresh lbias')
    assert not torch.equal(torch.nan_to_num(buf, neginf=0.0), torch.nan_to_num(old, neginf=0.0))
    key = m.decoder._label_bias_key
    buf.copy_(old)
    stale = life.run()
    assert m.decoder._label_bias_key == key
    frac = LC.fp64_fractions(life.case, m, stale)
    print('LIFECYCLE lbias stale buffer: %s' % ' '.join('%s %.3f' % kv for kv in sorted(frac.items())))
    assert not torch.equal(stale[0], want[0]) and frac['logits'] > 1.0, frac
    m.invalidate_native_cache()
    assert LC.same(life.run(), want)


# ------------------------------------------------------------------ c. whole-model mutators
TORCH_OPTIMS = collections.OrderedDict([
    ('SGD', lambda g, **kw: torch.optim.SGD(g, lr=0.05, momentum=0.9, **kw)),
    ('Adam', lambda g, **kw: torch.optim.Adam(g, lr=0.01, **kw)),
    ('AdamW', lambda g, **kw: torch.optim.AdamW(g, lr=0.01, weight_decay=0.01, **kw)),
])
MODES = collections.OrderedDict([('single', dict(foreach=False)), ('foreach', dict(foreach=True)), ('fused', dict(fused=True))])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('opt', TORCH_OPTIMS)
@pytest.mark.parametrize('family', ['tokpos', 'onehot', 'lbias'])
def test_torch_optimizer_steps_in_eval_mode(dev, family, opt, mode):
    """Gradients assigned directly, two steps in eval mode: only the version counters protect the tables."""
    life = Life(family, dev)
    try:
        optimizer = TORCH_OPTIMS[opt](_groups(life.m), **MODES[mode])
    except (RuntimeError, ValueError, TypeError) as e:      # this torch build refuses the implementation
        pytest.skip('torch.optim.%s(%s): %s' % (opt, mode, e))
    before = life.run()
    for step in (1, 2):
        _assign_grads(life.m)
        optimizer.step()
        out = life.check('%s %s step %d' % (opt, mode, step))
        assert not torch.equal(out[0], before[0])
        before = out


def _lamp_optims():
    from lamp_amd import optim as O
    return collections.OrderedDict([
        ('Adam', lambda g: O.Adam(g, lr=0.01)),
        ('AdamW', lambda g: O.AdamW(g, lr=0.01)),
        ('SGD', lambda g: O.SGD(g, lr=0.05)),
        ('Adam clip decay', lambda g: O.Adam(g, lr=0.01, weight_decay=0.01, max_grad_norm=1.0)),
        ('AdamW clip', lambda g: O.AdamW(g, lr=0.01, weight_decay=0.05, max_grad_norm=0.5)),
        ('SGD momentum clip decay', lambda g: O.SGD(g, lr=0.05, momentum=0.9, weight_decay=0.01, max_grad_norm=1.0)),
    ])


@pytest.mark.parametrize('family', LC.FAMILIES)
def test_lamp_optimizer_steps_in_eval_mode(dev, family):
    """lamp_amd.optim, plain and extended, the same way; and a skip_nonfinite step on a NaN gradient, which writes nothing: the
    output is the output of before, bit for bit."""
    from lamp_amd import optim as O
    life = Life(family, dev)
    before = life.run()
    for name, make in _lamp_optims().items():
        optimizer = make(_groups(life.m))
        for step in (1, 2):
            _assign_grads(life.m)
            optimizer.step()
            out = life.check('lamp %s step %d' % (name, step), fp64=step == 2)
            assert not torch.equal(out[0], before[0])
            before = out
    for make in (lambda g: O.Adam(g, lr=0.01, skip_nonfinite=True), lambda g: O.SGD(g, lr=0.05, momentum=0.9, skip_nonfinite=True)):
        optimizer = make(_groups(life.m))
        _assign_grads(life.m, nan_in='decoder.layer_stack.0.pos_ffn1.w_1.weight')
        optimizer.step()
        out = life.check('skipped step')
        assert LC.same(out, before) and int(optimizer.skipped_steps.item()) == 1


def _noisy_state_dict(m, prefix='', salt='sd:'):
    out = collections.OrderedDict()
    for k, v in m.state_dict().items():
        out[prefix + k] = v.detach().cpu() + LC.noise_for(salt + k, v.detach().cpu()) if v.is_floating_point() else v.detach().cpu()
    return out


def _mut_load_state_dict(life):
    life.m.load_state_dict(_noisy_state_dict(life.m))


def _mut_load_module_prefixed(life):
    life.m.load_state_dict(_noisy_state_dict(life.m, prefix='module.', salt='dp:'))


def _mut_copy_(life):
    with torch.no_grad():
        for name, p in life.m.named_parameters():
            p.copy_(p.detach().cpu() + LC.noise_for('copy:' + name, p.detach().cpu()))


def _mut_data_assign(life):
    for name, p in life.m.named_parameters():
        p.data = p.data + LC.noise_for('data:' + name, p)


def _mut_cpu_round_trip(life):
    life.m.to('cpu')
    life.perturb_all()
    life.m.to(life.dev)


def _mut_double_float(life):
    life.m.double()
    life.perturb_all()
    life.m.float()


def _mut_training_step(life):
    from lamp_amd import optim as O
    m, case = life.m, life.case
    m.train()
    optimizer = O.Adam(_groups(m), lr=0.01)
    tgt = (torch.rand(case.seq.size(0), m.n_labels, generator=torch.Generator().manual_seed(5)) < 0.2).float().to(life.dev)
    logits = m((case.seq.to(life.dev), case.pos.to(life.dev)), None, None, tgt)[0]
    F.binary_cross_entropy_with_logits(logits, tgt).backward()
    optimizer.step()
    m.zero_grad(set_to_none=True)
    m.eval()


MUTATORS = [_mut_load_state_dict, _mut_load_module_prefixed, _mut_copy_, _mut_data_assign, _mut_cpu_round_trip, _mut_double_float,
            _mut_training_step]


@pytest.mark.parametrize('mutator', MUTATORS, ids=lambda f: f.__name__[5:])
@pytest.mark.parametrize('family', LC.FAMILIES)
def test_other_ways_weights_change(dev, family, mutator):
    life = Life(family, dev)
    before = life.run()
    mutator(life)
    out = life.check(mutator.__name__[5:])
    assert not torch.equal(out[0], before[0])
    life.perturb_all()          # ... and the version keys hold on what the mutator left behind
    life.check(mutator.__name__[5:] + ', then in place')


SWITCHES = ('cache_layer0_query', 'use_chain_packs', 'use_gemm_packs', 'use_kv_gemm_packs', 'fold_embedding')


@pytest.mark.parametrize('family', LC.FAMILIES)
def test_route_switches_off_and_on_with_a_weight_change_in_between(dev, family):
    life = Life(family, dev)
    for switch in SWITCHES:
        setattr(life.m, switch, False)
        life.check(switch + ' off', fp64=False)
        life.perturb_all()
        life.check(switch + ' off, changed', fp64=False)
        delattr(life.m, switch)
        life.check(switch + ' on again')
        life.perturb_all()
        life.check(switch + ' on again, changed', fp64=False)


@pytest.mark.parametrize('family', LC.FAMILIES)
def test_matmul_precision_there_and_back_with_a_weight_change_in_between(dev, family):
    """'highest' -> 'high' -> 'highest' (a model of its own: the bf16x3 products' error grows with the weights, and the test above
    has changed them twenty times by its end)."""
    life = Life(family, dev)
    highest = life.run()
    life.m.matmul_precision = 'high'
    life.perturb_all()
    high = life.check('high, changed')
    life.m.matmul_precision = 'highest'
    back = life.check('highest again')
    assert not torch.equal(high[0], back[0]) and not torch.equal(back[0], highest[0])
    life.perturb_all()
    life.check('highest again, changed')


@pytest.mark.parametrize('family', ['tokpos', 'lbias'])
def test_eval_epochs_around_an_in_place_change(dev, family):
    """evaluate.test_epoch(streams=2), an in-place change, test_epoch again: the second epoch is the twin's epoch."""
    from lamp_amd import data as D
    from lamp_amd.evaluate import test_epoch
    life = Life(family, dev)
    case, L = life.case, life.m.n_labels
    src = [[t for t in row.tolist() if t != 0] for row in case.seq]
    tgt = [[2, 4 + (3 * i) % L, 4 + (5 * i + 1) % L, 3] for i in range(len(src))]

    def epoch(m):
        return test_epoch(m, D.EvalBatcher(src, tgt, 3), L, 3, dev, streams=2)
    first = epoch(life.m)
    life.perturb_all()
    second = epoch(life.m)
    want = epoch(LC.fresh(case, life.m, dev))
    assert torch.equal(second[0], want[0]) and torch.equal(second[1], want[1]) and second[2] == want[2]
    assert not torch.equal(second[0], first[0])
    life.check('after the epochs')


@pytest.mark.parametrize('family', LC.FAMILIES)
def test_in_place_writes_through_dot_data_need_invalidate_native_cache(dev, family):
    """The documented exception stays what it is: `.data` writes move no version counter, so the forward keeps the hoisted query
    of before until invalidate_native_cache() is called."""
    life = Life(family, dev)
    before = life.run()
    w = life.m.decoder.layer_stack[0].enc_attn.w_qs.weight
    w.data.add_(LC.noise_for('dot data', w))
    stale, want = life.run(), life.truth()
    assert LC.same(stale, before) and not LC.same(stale, want)
    life.m.invalidate_native_cache()
    assert LC.same(life.check('after invalidate_native_cache'), want)


# ------------------------------------------------------------------ d. replacement
@pytest.mark.parametrize('family', ['tokpos', 'tok', 'lbias'])
def test_replaced_parameters_and_submodules_are_seen(dev, family):
    life = Life(family, dev)
    m = life.m
    seen = [life.run()]

    def moved(what):
        seen.append(life.check(what))
        assert not torch.equal(seen[-1][0], seen[-2][0]), what

    def noisy(name, p):
        return (p.detach() + LC.noise_for(name, p)).clone()
    lin = m.decoder.layer_stack[1].pos_ffn2.w_2                      # a chain-pack weight
    lin.weight = nn.Parameter(noisy('replaced w_2', lin.weight))
    moved('a Parameter replaced')
    ln = m.decoder.layer_stack[0].pos_ffn1.layer_norm                # read live, through its address
    ln.bias = nn.Parameter(noisy('replaced ln', ln.bias))
    moved('a LayerNorm bias replaced')
    m.encoder.src_word_emb = nn.Embedding.from_pretrained(noisy('replaced emb', m.encoder.src_word_emb.weight), freeze=False)
    moved('the token table replaced')                                # folded into W1
    m.decoder.tgt_word_emb = nn.Embedding.from_pretrained(noisy('replaced labels', m.decoder.tgt_word_emb.weight), freeze=False)
    m.tgt_word_proj.weight = m.decoder.tgt_word_emb.weight           # the constructor's second key of the same Parameter
    moved('the label table replaced')                                # feeds the hoisted query
    m.decoder.layer_stack[0].enc_attn.w_ks.weight = m.decoder.layer_stack[1].enc_attn.w_ks.weight
    moved('two weights tied')
    LC.perturb('tied', m.decoder.layer_stack[1].enc_attn.w_ks.weight)
    moved('the tied weight changed in place')
    m.decoder.layer_stack[1] = copy.deepcopy(m.decoder.layer_stack[0])
    moved('a decoder layer replaced')


# ------------------------------------------------------------------ e. copies
def _deepcopy(m):
    return copy.deepcopy(m)


def _save_load(m):
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def _averaged(m):
    return torch.optim.swa_utils.AveragedModel(m).module


@pytest.mark.parametrize('how', [_deepcopy, _save_load, _averaged], ids=lambda f: f.__name__.strip('_'))
@pytest.mark.parametrize('family', ['tokpos', 'onehot', 'lbias'])
def test_copies_after_a_forward_share_nothing(dev, family, how):
    life = Life(family, dev)
    m = life.m
    mine = life.run()
    c = how(m)
    assert c._native_cache is None and m._native_cache is not None
    assert LC.same(life.run(c), mine)
    other = Life(family, dev, model=c)      # (with a twin of its own)
    other.perturb_all()
    theirs = other.check('the copy, changed')
    assert not torch.equal(theirs[0], mine[0])
    assert LC.same(life.run(), mine)        # the original did not move
    life.perturb_all()
    life.perturb_all()                      # (twice: once would be the very change the copy went through)
    assert not torch.equal(life.check('the original, changed')[0], mine[0])
    assert LC.same(other.run(), theirs)     # nor does the copy


def test_deepcopy_between_forward_and_backward(dev):
    """The reference's training loop deep-copies the model between forward and backward: the backward and the step of the
    original still work, with the gradients of a run without the copy."""
    from lamp_amd import optim as O
    case = LC.make('tokpos')
    tgt = (torch.rand(case.seq.size(0), case.model.n_labels, generator=torch.Generator().manual_seed(5)) < 0.2).float().to(dev)
    src = (case.seq.to(dev), case.pos.to(dev))
    grads = []
    for with_copy in (False, True):
        m = LC.make('tokpos').model.to(dev).train()
        logits = m(src, None, None, tgt)[0]
        c = copy.deepcopy(m) if with_copy else None
        F.binary_cross_entropy_with_logits(logits, tgt).backward()
        grads.append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 40
    for n in grads[0]:
        if n == 'encoder.src_word_emb.weight':     # scatter-add of repeated tokens through atomics: order not fixed
            assert (grads[0][n] - grads[1][n]).abs().max().item() <= 1e-6 * grads[0][n].abs().max().item()
        else:
            assert torch.equal(grads[0][n], grads[1][n]), n
    assert c.training and all(p.grad is None for p in c.parameters())
    before = LC.run(case, c.eval(), dev)
    O.Adam(_groups(m), lr=0.01).step()
    life = Life('tokpos', dev, model=m.eval())
    assert not torch.equal(life.check('after the step')[0], before[0])
    assert LC.same(LC.run(case, c, dev), before)
