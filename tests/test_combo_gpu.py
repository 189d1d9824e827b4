"""-m gpu: every case of tests/combo_common.py's table -- pairs of model options that meet on ONE pass of api.hip::forward and of
training.forward_train -- against the fp64 restatement combo_forward_ref / combo_oracle_run, forward and backward, plus the bit
rules README and DESIGN promise (micro-batch split, a sample alone at its own length, run to run, output modes on the softmax
mask routes, the packed switch's fallback, a learned bias and its constant twin, 'high' against 'highest') and the refusals.

Bars: the project's own (combo_common.TOL_*), each as max(bar, 4 x the fp32 CPU restatement's gap to fp64 on the case) -- the
rule of tests/fuzz_parity.py.  Every test prints its errors as fractions of their bars ("COMBO ..." lines)."""
import pytest
import torch

import combo_common as CC
import head_geometry_common as HG
from conftest import max_abs_diff
from oracle import lamp_ref as R

pytestmark = pytest.mark.gpu

OUT_KW = {'plain': {}, 'attns': dict(return_attns=True), 'ints': dict(int_preds=True)}
ALL = [c['name'] for c in CC.CASES]
TRAIN = [c['name'] for c in CC.training_cases()]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from lamp_amd import _native as N
    N.lib()  # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def _N():
    from lamp_amd import _native as N
    return N


def _model(c, b, dev, train=False, **over):
    m = (CC.combo_build(c, **over).model if over else b.model).to(dev)
    m = m.train() if train else m.eval()
    if c['enc'] == 'packed':
        m.use_packed_live_encoder = True
    if c['prec'] == 'high':
        m.matmul_precision = 'high'
    return m


def _named(out, c, mode):
    """A forward's return tuple (reference or model) as a dict of lists of tensors, in the mode's own layout."""
    if mode == 'ref':
        logits, enc, enc_maps, (slf, encdec), ips = out
        return dict(logits=[logits], enc=[enc], enc_maps=list(enc_maps), dec_maps=[a for a in slf if a is not None] + list(encdec),
                    ips=list(ips))
    d = dict(logits=[out[0]], enc=[out[1]], enc_maps=[], dec_maps=[], ips=[])
    if mode == 'attns':
        d['enc_maps'] = list(out[2][0])
        d['dec_maps'] = [a for a in out[3][0] if a is not None] + list(out[3][1])
    elif mode == 'ints':
        d['ips'] = list(out[2])
    else:
        assert out[2] is None
    return d


def _run(m, b, dev, mode, rows=None, trim=None):
    seq, pos, adj = b.seq, b.pos, b.adj
    if rows is not None:
        seq, pos = seq[rows, :trim], pos[rows, :trim]
        adj = adj[rows] if adj is not None else None
    with torch.no_grad():
        return m((seq.to(dev), pos.to(dev)), adj, None, None, **OUT_KW[mode])


def _counted(fn):
    """fn() with the library's launch counters on -> (result, launches of every kernel class)."""
    N = _N()
    N.prof_enable(True)
    try:
        N.prof_reset()
        out = fn()
        torch.cuda.synchronize()
        prof = N.prof_read()
    finally:
        N.prof_enable(False)
    return out, sum(int(v['launches']) for v in prof.values())


def _same(a, b):
    a, b = [t for k in sorted(a) for t in a[k]], [t for k in sorted(b) for t in b[k]]
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _bars(c, ref64, ref32):
    live, high = c['enc'] != 'dead', c['prec'] == 'high'
    base = dict(logits=CC.TOL_LOGIT, enc=CC.TOL_ENC_LIVE if live or high else CC.TOL_ENC, dec_maps=CC.TOL_MAP,
                enc_maps=CC.TOL_MAP_LIVE if live else CC.TOL_MAP, ips=CC.TOL_INT)
    gap = {k: max([max_abs_diff(x, y) for x, y in zip(ref32[k], ref64[k])] or [0.0]) for k in base}
    return {k: max(base[k], 4 * gap[k]) for k in base}


def _fractions(got, ref64, bars, what):
    """Each quantity the run returned against the fp64 restatement -> {quantity: error / bar}; maps exactly 0 where blocked."""
    frac = {}
    for k in ('logits', 'enc', 'enc_maps', 'dec_maps', 'ips'):
        if not got[k]:
            continue
        assert len(got[k]) == len(ref64[k]), (what, k)
        for g_, r_ in zip(got[k], ref64[k]):
            assert tuple(g_.shape) == tuple(r_.shape), (what, k)
        frac[k] = max(max_abs_diff(g_, r_) for g_, r_ in zip(got[k], ref64[k])) / bars[k]
        if k.endswith('maps'):
            for g_, r_ in zip(got[k], ref64[k]):
                gone = r_ == 0                     # softmax and sigmoid of -inf: exactly 0 in the restatement, nowhere else
                assert (g_.cpu()[gone] == 0).all(), (what, k)
    return frac


def _refs(c, b):
    bias = b.bias
    with torch.no_grad():
        r64 = CC.combo_forward_ref(R.to_dtype(b.sd, torch.float64), b.seq, b.pos, c, b.blocked, b.adj,
                                   bias.double() if bias is not None else None)
        r32 = CC.combo_forward_ref(b.sd, b.seq, b.pos, c, b.blocked, b.adj, bias)
    return _named(r64, c, 'ref'), _named(r32, c, 'ref')


def _micro_limit(m, b, dev, mode, monkeypatch):
    """The workspace_limit_bytes that makes combo_common.micro_batch(c) samples a pass.  The library sizes a split pass without
    the K/V-ahead buffers the whole-batch size function counts, so the limit is not computed but found: the samples a pass
    grow with the limit, a pass costs the same launches whatever it holds, and the largest limit that still takes
    ceil(B / mb) passes is the one with mb samples a pass (bisection between one sample a pass and what LAMP.forward asks
    N.workspace for at the whole batch).  -> (limit, launches: whole batch, at that limit, one sample a pass; whole-batch result)."""
    N = _N()
    seen, real = [], N.workspace

    def recording(nbytes, device):
        seen.append(int(nbytes))
        return real(nbytes, device)
    _run(m, b, dev, mode)          # (the first forward also builds the weights-only tables: not counted)
    monkeypatch.setattr(N, 'workspace', recording)
    whole, n_whole = _counted(lambda: _run(m, b, dev, mode))
    monkeypatch.setattr(N, 'workspace', real)
    B, mb = b.seq.size(0), mb_of(b)

    def launches(limit):
        m.workspace_limit_bytes = limit
        try:
            return _counted(lambda: _run(m, b, dev, mode))[1]
        finally:
            del m.workspace_limit_bytes
    n_one = launches(1)
    a_pass, want = n_one // B, -(-B // mb)
    assert n_one == a_pass * B and n_whole < 2 * a_pass
    lo, hi = 1, max(seen)          # lo: `want` passes or more; hi: fewer
    while hi - lo > 64:
        mid = (lo + hi) // 2
        if launches(mid) >= want * a_pass:
            lo = mid
        else:
            hi = mid
    return lo, n_whole, want * a_pass, n_one, whole


def mb_of(b):
    return 2 if b.seq.size(0) % 2 else 3


# ------------------------------------------------------------------ 1. eval: every case against fp64, and the bit rules
@pytest.mark.parametrize('name', ALL)
def test_eval_case(dev, name, monkeypatch):
    c = CC.case(name)
    b = CC.combo_build(c)
    mode, B = c['out'], b.seq.size(0)
    assert mb_of(b) == CC.micro_batch(c)
    ref64, ref32 = _refs(c, b)
    bars = _bars(c, ref64, ref32)
    m = _model(c, b, dev)

    # whole batch and micro-batched: both run, the case's own is held against fp64, and they are the same bits
    limit, n_whole, n_want, n_one, whole = _micro_limit(m, b, dev, mode, monkeypatch)
    m.workspace_limit_bytes = limit
    try:
        micro, n_micro = _counted(lambda: _run(m, b, dev, mode))
    finally:
        del m.workspace_limit_bytes
    assert n_whole < n_micro == n_want < n_one, 'the limit did not split the batch as meant: %d / %d (%d) / %d launches' % (
        n_whole, n_micro, n_want, n_one)
    whole, micro = _named(whole, c, mode), _named(micro, c, mode)
    got = micro if c['batch'] == 'micro' else whole
    frac = _fractions(got, ref64, bars, name)
    print('COMBO eval %s %s: %s' % (name, ' '.join(c[ax] for ax in CC.AXES) + ' ' + c['shape'],
                                     ' '.join('%s %.3f' % kv for kv in sorted(frac.items()))))
    assert torch.isfinite(got['logits'][0]).all()
    assert max(frac.values()) <= 1.0, frac
    assert _same(whole, micro)
    assert _same(_named(_run(m, b, dev, mode), c, mode), whole)                       # run to run

    plain = whole if mode == 'plain' else _named(_run(m, b, dev, 'plain'), c, 'plain')
    packed_for_real = c['enc'] == 'packed' and c['geom'] == 'std' and c['front'] != 'onehot'
    if c['enc'] == 'packed':
        m.use_packed_live_encoder = False
        padded = _named(_run(m, b, dev, 'plain'), c, 'plain')
        padded_mode = _named(_run(m, b, dev, mode), c, mode)
        m.use_packed_live_encoder = True
        if packed_for_real:       # another route: its own bits, and the maps come from the padded route whatever the switch says
            assert not torch.equal(padded['enc'][0], plain['enc'][0])
            if mode == 'attns':
                assert _same(padded_mode, whole)
        else:                     # d_k != d_v, one head or the one-hot front end: the switch falls back, the padded route's bits
            assert _same(padded, plain) and _same(padded_mode, whole)
    if mode != 'plain' and c['score'] in CC.MASK_SCORES and c['prec'] == 'highest' and not (packed_for_real and mode == 'attns'):
        # maps and intermediate predictions do not change the bits (the softmax mask routes: tests/test_head_geometry_gpu.py)
        assert torch.equal(plain['logits'][0], whole['logits'][0]) and torch.equal(plain['enc'][0], whole['enc'][0])
    if c['front'] != 'onehot':
        # a sample alone, trimmed to its own length: its rows of the batch
        for row in (1, B - 1):
            n = b.g['lengths'][row]
            alone = _run(m, b, dev, 'plain', rows=slice(row, row + 1), trim=n)
            assert torch.equal(alone[0][0], plain['logits'][0][row]) and torch.equal(alone[1][0], plain['enc'][0][row, :n]), row
    if c['score'] == 'lbias':     # the learned bias against a constant-bias model holding the same values
        twin = _model(c, b, dev, learn=False)
        assert twin.decoder.label_bias is None and m.decoder.label_bias is not None
        assert _same(_named(_run(twin, b, dev, mode), c, mode), whole)
    if c['prec'] == 'high':       # another kernel's bits, the same bar
        del m.matmul_precision
        highest = _named(_run(m, b, dev, mode), c, mode)
        assert not torch.equal(highest['logits'][0], whole['logits'][0])
        assert max_abs_diff(highest['logits'][0], ref64['logits'][0]) <= bars['logits']


# ------------------------------------------------------------------ 2. training: every gradient against fp64 autograd
def _train_step(m, c, b, dev, mode, defer=True, composite=True):
    from lamp_amd import training
    training.DEFER_WEIGHT_GRADS, training.COMPOSITE_CALLS = defer, composite
    try:
        m.zero_grad(set_to_none=True)
        tgt = b.tgt.to(dev)
        out = m((b.seq.to(dev), b.pos.to(dev)), b.adj, None, tgt, **OUT_KW[mode])
        CC.combo_loss(c, out[0], out[2] if mode == 'ints' else [], tgt).backward()
        assert training._weight_grads.pending() == 0
        return out, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    finally:
        training.DEFER_WEIGHT_GRADS = training.COMPOSITE_CALLS = True


@pytest.mark.parametrize('name', TRAIN)
def test_train_case(dev, name):
    c = CC.case(name)
    b = CC.combo_build(c)
    mode, L = c['out'], b.g['L']
    m = _model(c, b, dev, train=True)
    ref_logits, ref_enc, ref_loss, ref = CC.combo_oracle_run(c, b, torch.float64)
    l32 = CC.combo_oracle_run(c, b, torch.float32)[0]
    out, grads = _train_step(m, c, b, dev, mode)
    frac = {'logits': max_abs_diff(out[0], ref_logits) / max(CC.TOL_LOGIT, 4 * max_abs_diff(l32, ref_logits))}
    if mode == 'attns':           # the training forward's maps: the eval bars, exactly 0 where blocked
        ref64, ref32 = _refs(c, b)
        got = {k: [t.detach() for t in v] for k, v in _named(out, c, mode).items()}
        maps = _fractions(dict(got, logits=[], enc=[]), ref64, _bars(c, ref64, ref32), name)
        frac.update(maps)
    # every parameter
    checked, worst, worst_name = 0, 0.0, None
    for pname, p in m.named_parameters():
        if p.grad is None:        # the frozen tables, and a dead encoder self-attention (its output is discarded)
            assert (pname == 'encoder.position_enc.weight' or (c['front'] == 'onehot' and pname == 'encoder.src_word_emb.weight')
                    or (c['enc'] == 'dead' and 'encoder.layer_stack' in pname and 'slf_attn' in pname)), pname
            continue
        if pname == 'encoder.position_enc.weight':
            continue
        want = HG.reference_gradient(ref, pname)
        assert want is not None, pname
        bar = HG.GRAD_RTOL * want.abs().max().item() + HG.GRAD_ATOL
        err = max_abs_diff(p.grad, want) / bar
        if err > worst:
            worst, worst_name = err, pname
        checked += 1
    frac['grad'] = worst
    print('COMBO train %s %s: %s (%d gradients, worst %s)' % (name, ' '.join(c[ax] for ax in CC.AXES) + ' ' + c['shape'],
                                                              ' '.join('%s %.3f' % kv for kv in sorted(frac.items())), checked,
                                                              worst_name))
    assert checked >= 12 and max(frac.values()) <= 1.0, frac
    if c['score'] == 'lbias':     # exactly 0 at -inf entries and under the mask, and only there
        got = m.decoder.label_bias.grad
        gone = torch.isinf(m.decoder.label_bias_f32[:, :L])
        assert gone.any() and (got[gone] == 0).all() and got[~gone].abs().min() > 0
        assert (ref['decoder.label_bias'][gone.cpu()] == 0).all()
    # the routes of tests/test_gpu_training.py::test_deferred_weight_gradients_equal_the_autograd_route, by its rule: one library
    # call per sub-layer against the per-launch route bit for bit; the deferred weight gradients against the immediate ones up
    # to the K-split's summation order, and bit for bit for everything that never goes through the queue
    _, per_launch = _train_step(m, c, b, dev, mode, composite=False)
    assert per_launch.keys() == grads.keys()
    for n in grads:
        if n == 'encoder.src_word_emb.weight':     # scatter-add of repeated tokens through atomics: order not fixed
            assert max_abs_diff(per_launch[n], grads[n]) <= 1e-6 * grads[n].abs().max().item()
        else:
            assert torch.equal(per_launch[n], grads[n]), n
    _, now = _train_step(m, c, b, dev, mode, defer=False)
    assert now.keys() == grads.keys()
    for n in grads:
        scale = now[n].abs().max().item()
        assert max_abs_diff(now[n], grads[n]) <= 2e-5 * scale + 1e-9, n
        if (n.endswith('bias') or 'layer_norm' in n or 'tgt_word' in n) and not n.startswith('encoder.conv'):
            assert torch.equal(now[n], grads[n]), n


# ------------------------------------------------------------------ 3. what the library refuses is refused before any launch
def _refused(fn, exc, match=None):
    with pytest.raises(exc, match=match):
        _counted(fn)
    N = _N()
    torch.cuda.synchronize()
    prof = N.prof_read()         # (the counters still hold what ran since _counted's reset)
    assert sum(int(v['launches']) for v in prof.values()) == 0


def test_refusals(dev):
    N = _N()
    base = CC._c('r', 'tokpos', 'live', 'bias', 'gen', 'on', '2x2', 'plain', 'whole', 'highest')
    b = CC.combo_build(base)
    adj = R.make_adjacency(b.g['L'], 0.2, 0)
    # sigmoid attention with a label bias: at construction, and at the library for a caller that sets both flags
    for learn in (False, True):
        _refused(lambda: HG.build_model(b.g, b.sd, adj, n_max_seq=b.g['T'], dec_attn_type='sigmoid', label_bias=b.bias,
                                        learn_label_bias=learn), NotImplementedError, 'sigmoid')
    m = _model(base, b, dev)
    want = _run(m, b, dev, 'plain')[0]
    m.dec_attn_type = 'sigmoid'       # LAMP.forward now sets LAMP_FWD_DEC_SIGMOID beside LAMP_FWD_LABEL_BIAS: check_forward refuses
    _refused(lambda: _run(m, b, dev, 'plain'), N.LampError, 'not supported')
    m.dec_attn_type = None
    assert torch.equal(_run(m, b, dev, 'plain')[0], want)
    # a label bias without the label self-attention
    g_off = dict(b.g, no_dec_self_att=True)
    sd_off = {k: v for k, v in b.sd.items() if '.slf_attn.' not in k or k.startswith('encoder.')}
    for learn in (False, True):
        _refused(lambda: HG.build_model(g_off, sd_off, adj, n_max_seq=b.g['T'], label_bias=b.bias, learn_label_bias=learn),
                 ValueError, 'no_dec_self_att')
    # the one-hot front end: without position rows at construction; with per-sample graphs at the call, eval and training
    oh = CC._c('r', 'onehot', 'live', 'prior', 'std', 'on', '2x2', 'plain', 'whole', 'highest')
    bo = CC.combo_build(oh)
    _refused(lambda: HG.build_model(dict(bo.g, pos=False), bo.sd, R.make_adjacency(bo.g['L'], 0.2, 0), n_max_seq=bo.g['T'],
                                    onehot=True), NotImplementedError, 'position')
    mo = _model(oh, bo, dev)
    graphs = CC.EC.random_graphs(bo.g['lengths'], seed=3)
    src = (bo.seq.to(dev), bo.pos.to(dev))
    for train in (False, True):
        mo.train(train)
        for kw in OUT_KW.values():
            _refused(lambda: mo(src, graphs, None, None, **kw), NotImplementedError, 'one-hot')
    mo.eval()
    assert torch.isfinite(_run(mo, bo, dev, 'plain')[0]).all()
