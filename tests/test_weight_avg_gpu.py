"""-m gpu: weight averaging on the device (lamp_weight_average, lamp_weight_swap, lamp_amd.optim.WeightAverage, run_train
-weight_avg, run_eval -weights) against the fp64 restatement of tests/weight_avg_common.py.

The bar of one update is the project's: max(one fp32 ulp at the fp64 value, 4 x the gap of torch's own fp32 CPU lerp on the
same inputs); planted non-finite elements are compared exactly.  Every test prints the used fraction of its bar ("WAVG ..."
lines; run with -s)."""
import gc
import os
import tempfile

import pytest
import torch

import large_extent_common as LX
import lifecycle_common as LC
import redzone_common as RZ
import train_common as TC
import weight_avg_common as W

pytestmark = pytest.mark.gpu

NUMELS = (1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 3)
ALIGNMENTS = ((0, 0), (1, 0), (0, 1), (1, 1))          # (param, avg) offset in floats: only (0, 0) takes the 16-byte route
WEIGHTS = (1.0, 0.5, 0.25, 1e-3, 1.0 / 7.0, 0.0)
TABLE = 75                                             # crosses the 72-entry launch boundary


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def N():
    from lamp_amd import _native
    _native.lib()
    return _native


def ok(rc, what):
    assert rc == 0, '%s returned %d' % (what, rc)


# ------------------------------------------------------------------ the 75-entry table in a red-zoned arena
def table_specs():
    """[(numel, param offset, avg offset, seed)]: every numel at every alignment (32 entries, mixed in one table), two
    zero-numel entries (one in each launch), filled up to 75 with further numels at rotating alignments."""
    specs = [(n, po, ao) for n in NUMELS for po, ao in ALIGNMENTS]
    extra = (7, 255, 257, 1023, 1025, 4094, 4098, 2 * 4096, 2 * 4096 + 1, 6000)
    k = 0
    while len(specs) < TABLE - 2:
        specs.append((extra[k % len(extra)] + k // len(extra),) + ALIGNMENTS[k % 4])
        k += 1
    specs.insert(10, (0, 0, 0))
    specs.insert(73, (0, 0, 0))
    assert len(specs) == TABLE
    return [s + (100 + i,) for i, s in enumerate(specs)]


GUARD = 123.25      # the float in front of a buffer that starts one float late


class Carved(object):
    """One (param, avg) pair in an arena: the device views, the CPU originals and the guard views."""

    def __init__(self, ar, spec, tag, both_writable=False):
        self.n, po, ao, seed = spec
        self.p0, self.a0, self.hard = W.planted(self.n, seed)
        self.lead = []
        if self.n == 0:
            self.p = self.a = None
            return

        def carve(data, off, writable, name):
            full = torch.cat([torch.full((off,), GUARD), data])
            v = (ar.inout if writable else ar.inp)(full, name)
            if off:
                self.lead.append(v[:off])
            return v[off:]
        self.p = carve(self.p0, po, both_writable, 'p%s' % tag)
        self.a = carve(self.a0, ao, True, 'a%s' % tag)
        assert (self.p.data_ptr() % 16 == 0) == (po == 0) and (self.a.data_ptr() % 16 == 0) == (ao == 0)

    def guards_intact(self):
        return all(float(g[0]) == GUARD for g in self.lead)


def carve_table(dev, specs, both_writable=False, fill=RZ.FILL_NAN):
    ar = RZ.Arena(dev, fill, capacity=48 << 20)
    return ar, [Carved(ar, s, str(i), both_writable) for i, s in enumerate(specs)]


def entry_array(N, items):
    arr = (N.OptimEntry * len(items))()
    for i, c in enumerate(items):
        if c.n:
            arr[i].param, arr[i].exp_avg = c.p.data_ptr(), c.a.data_ptr()
        arr[i].numel = c.n
    return arr


def run_average(N, items, w):
    ok(N.lib().lamp_weight_average(entry_array(N, items), len(items), w, N.stream()), 'lamp_weight_average')


def run_swap(N, items):
    ok(N.lib().lamp_weight_swap(entry_array(N, items), len(items), N.stream()), 'lamp_weight_swap')


@pytest.fixture(scope='module')
def averaged_tables(dev, N):
    """weight -> the table's result bits (CPU int32 per entry) of the run every test below shares."""
    return {}


@pytest.mark.parametrize('w', WEIGHTS, ids=lambda w: 'w=%.6g' % w)
def test_one_update_against_fp64(dev, N, w, averaged_tables):
    specs = table_specs()
    ar, items = carve_table(dev, specs)
    run_average(N, items, w)
    ar.check()                       # red zones, the params (inputs) and the leading guards' buffers outside the avgs
    worst = 0.0
    bits = []
    for i, c in enumerate(items):
        if not c.n:
            bits.append(None)
            continue
        assert c.guards_intact(), 'entry %d: the float in front of a late-starting buffer changed' % i
        assert RZ.bit_equal(c.p.cpu(), c.p0), 'entry %d: the weight is read only' % i
        got = c.a.cpu()
        bits.append(RZ.bits(got).clone())
        if w == 1.0:
            assert RZ.bit_equal(got, c.p0), 'entry %d: weight 1 is a copy of the bits' % i
        elif w == 0.0:
            assert RZ.bit_equal(got, c.a0), 'entry %d: weight 0 leaves the average' % i
        worst = max(worst, W.compare(got, c.p0, c.a0, w, c.hard, 'entry %d (%d elements, offsets %s) w = %g' % (i, c.n, specs[i][1:3], w)))
    print('WAVG one update w = %g: worst used fraction of the bar %.3f' % (w, worst))
    averaged_tables[w] = bits


@pytest.mark.parametrize('w', (0.25, 1.0 / 7.0, 0.5), ids=lambda w: 'w=%.6g' % w)
def test_result_is_independent_of_the_table_and_repeatable(dev, N, w, averaged_tables):
    specs = table_specs()
    if w not in averaged_tables:
        ar, items = carve_table(dev, specs)
        run_average(N, items, w)
        averaged_tables[w] = [RZ.bits(c.a.cpu()).clone() if c.n else None for c in items]
    first = averaged_tables[w]
    ar, items = carve_table(dev, specs)                       # a second time, the whole table
    run_average(N, items, w)
    torch.cuda.synchronize()
    for i, c in enumerate(items):
        if c.n:
            assert torch.equal(RZ.bits(c.a.cpu()), first[i]), 'entry %d differs between two runs' % i
    # alone: the largest numel at each alignment, and entries of the second launch
    alone = [i for i, s in enumerate(specs) if s[0] == NUMELS[-1]] + [72, 74]
    for i in alone:
        ar1, one = carve_table(dev, [specs[i]])
        run_average(N, one, w)
        ar1.check()
        assert torch.equal(RZ.bits(one[0].a.cpu()), first[i]), 'entry %d alone differs from the entry in the table' % i


def test_swap(dev, N):
    specs = table_specs()
    ar, items = carve_table(dev, specs, both_writable=True)
    payload_p, payload_a = 0x7FC12345, -0x003FFFFF          # (0xFFC00001 as an int32): quiet NaNs with payloads
    for c in items:
        if c.n >= 64:
            RZ.bits(c.p0)[11] = payload_p
            c.p.view(torch.int32)[11] = payload_p
            RZ.bits(c.a0)[12] = payload_a
            c.a.view(torch.int32)[12] = payload_a
    for c in items:
        if c.n:
            c.p0, c.a0 = c.p.cpu(), c.a.cpu()
    ar._pristine.copy_(ar.mem)                               # (the planted words are the state before the call)
    run_swap(N, items)
    ar.check()
    for i, c in enumerate(items):
        if c.n:
            assert c.guards_intact()
            assert RZ.bit_equal(c.p.cpu(), c.a0) and RZ.bit_equal(c.a.cpu(), c.p0), 'entry %d after one swap' % i
    run_swap(N, items)
    ar.check()
    for i, c in enumerate(items):
        if c.n:
            assert c.guards_intact()
            assert RZ.bit_equal(c.p.cpu(), c.p0) and RZ.bit_equal(c.a.cpu(), c.a0), 'entry %d after two swaps' % i
    assert ar.untouched()                                    # twice is the identity on every byte of the arena


# ------------------------------------------------------------------ the recurrence, through WeightAverage
class _Three(torch.nn.Module):
    def __init__(self, sizes):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n)) for n in sizes])


def _torch_fp32_average(seq, kind, decay, warmup):
    """torch's own fp32 CPU AveragedModel over the sequence -> its parameters."""
    from torch.optim.swa_utils import AveragedModel, get_swa_multi_avg_fn
    net = _Three([p.numel() for p in seq[0]])

    def ema(avg_list, cur_list, num_averaged):
        torch._foreach_lerp_(avg_list, cur_list, W.schedule_weight('ema', decay, warmup, int(num_averaged)))
    ref = AveragedModel(net, multi_avg_fn=ema if kind == 'ema' else get_swa_multi_avg_fn())
    for ps in seq:
        with torch.no_grad():
            for p, v in zip(net.ps, ps):
                p.copy_(v)
        ref.update_parameters(net)
    return [p.detach() for p in ref.module.ps]


@pytest.mark.parametrize('kind,decay,warmup', [('ema', 0.9, False), ('ema', 0.999, True), ('swa', 0.0, False)])
def test_recurrence_of_50_updates(dev, N, kind, decay, warmup):
    from lamp_amd import optim as O
    sizes = (5, 4097, 1001)
    g = torch.Generator().manual_seed(17)
    params = [torch.nn.Parameter(torch.zeros(n, device=dev)) for n in sizes]
    avg = O.WeightAverage(params, kind=kind, decay=decay, warmup=warmup)
    ptrs = [b.data_ptr() for b in avg.buffers]
    seq, worst_step = [], 0.0
    for step in range(50):
        ps = [torch.randn(n, generator=g) for n in sizes]
        seq.append(ps)
        with torch.no_grad():
            for p, v in zip(params, ps):
                p.copy_(v)
        prev = [b.cpu() for b in avg.buffers]
        versions = [b._version for b in avg.buffers]
        avg.update()
        assert avg.last_weight == W.schedule_weight(kind, decay, warmup, step)
        assert all(b._version > v for b, v in zip(avg.buffers, versions))
        for k, (b, p, a) in enumerate(zip(avg.buffers, ps, prev)):
            worst_step = max(worst_step, W.compare(b.cpu(), p, a, avg.last_weight, torch.zeros(sizes[k], dtype=torch.bool),
                                                   '%s step %d tensor %d' % (kind, step, k)))
    assert (avg.n_averaged, avg.n_calls) == (50, 50) and [b.data_ptr() for b in avg.buffers] == ptrs
    want = W.recurrence64(seq, kind, decay, warmup)
    t32 = _torch_fp32_average(seq, kind, decay, warmup)
    worst_end = 0.0
    for k, b in enumerate(avg.buffers):
        gap = float((t32[k].double() - want[k]).abs().max())
        err = (b.cpu().double() - want[k]).abs()
        tol = torch.maximum(W.ulp32(want[k]), torch.full_like(err, 4.0 * gap))
        worst_end = max(worst_end, float((err / tol).max()))
    print('WAVG recurrence %s decay %g warmup %s: worst used fraction per step %.3f, at the end %.3f'
          % (kind, decay, warmup, worst_step, worst_end))
    assert worst_end <= 1.0


# ------------------------------------------------------------------ the life cycle: cached tables follow the swap
def _assign_grads(m):
    import zlib
    for name, p in m.named_parameters():
        if not p.requires_grad:
            continue
        gen = torch.Generator().manual_seed(zlib.crc32(('grad:' + name).encode()))
        g = (0.1 * torch.randn(p.shape, generator=gen)).to(p.device)
        if name == 'decoder.label_bias':
            g = g.masked_fill(torch.isinf(p.detach()), 0.0)
        p.grad = g


@pytest.mark.parametrize('family', ['tokpos', 'lbias'])
def test_life_cycle_cached_tables_follow_the_swap(dev, N, family):
    from lamp_amd import optim as O
    case = LC.make(family)
    m = case.model.to(dev).eval()
    start = LC.run(case, m, dev)                              # the caches are filled
    rest = [p for n, p in m.named_parameters() if p.requires_grad and n != 'decoder.label_bias']
    groups = [dict(params=rest)]
    bias = getattr(m.decoder, 'label_bias', None)
    if family == 'lbias':
        assert bias is not None and bool(torch.isinf(bias.detach()).any()), 'the family has no -inf bias entry'
        groups.append(dict(params=[bias], weight_decay=0.0))
    optimizer = O.Adam(groups, lr=0.01)
    avg = O.WeightAverage([p for g in optimizer.param_groups for p in g['params']], kind='ema', decay=0.5)
    for _ in range(3):
        _assign_grads(m)
        optimizer.step()
        avg.update()
    raw_sd = LC.cpu_state_dict(m)
    avg_sd = {k: v.detach().cpu().clone() for k, v in avg.averaged_state_dict(m).items()}
    assert any(not torch.equal(avg_sd[k], raw_sd[k]) for k in raw_sd)
    raw_out = LC.run(case, m, dev)
    assert not LC.same(raw_out, start)
    twin = LC.fresh(case, m, dev)
    assert LC.same(raw_out, LC.run(case, twin, dev))
    if family == 'lbias':
        where = torch.isinf(raw_sd['decoder.label_bias'])
        a = avg_sd['decoder.label_bias']
        assert not bool(torch.isnan(a).any()), 'an averaged -inf entry became NaN'
        assert torch.equal(torch.isinf(a), where) and bool((a[where] < 0).all())
    with avg.applied():
        inside = LC.run(case, m, dev)
        twin.load_state_dict(avg_sd)
        assert LC.same(inside, LC.run(case, twin, dev)), 'inside applied(): not the bits of a model that loaded the average'
        assert not LC.same(inside, raw_out), 'the average changes nothing: the test shows nothing'
        assert bool(torch.isfinite(inside[0]).all())
    after = LC.run(case, m, dev)
    twin.load_state_dict(raw_sd)
    assert LC.same(after, LC.run(case, twin, dev)) and LC.same(after, raw_out), 'after applied(): not the trained weights\' bits'
    now = LC.cpu_state_dict(m)
    assert all(RZ.bit_equal(now[k], raw_sd[k]) for k in raw_sd), 'the state dict did not come back bit for bit'
    with pytest.raises(RuntimeError):
        with avg.applied():
            avg.update()
    assert LC.same(LC.run(case, m, dev), raw_out)            # swapped back after the exception
    # copy_to is the out-of-place load: the model then IS the average, and the buffers keep it
    avg.copy_to(m)
    assert LC.same(LC.run(case, m, dev), inside)
    shipped = LC.cpu_state_dict(m)
    assert all(RZ.bit_equal(shipped[k], avg_sd[k]) for k in avg_sd)
    with pytest.raises(ValueError):
        avg.copy_to(twin)                                     # another module: load averaged_state_dict() into it instead


# ------------------------------------------------------------------ through the training loop
ARGS = ['-data', 'x.pt', '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '1', '-dropout', '0.0',
        '-label_mask', 'prior']


def _loop_setup(dev):
    from lamp_amd import optim as O
    from lamp_amd import run_train as RT
    from lamp_amd import train as T
    data = TC.synthetic_dataset(n_train=48)
    opt = RT.parse(ARGS)
    torch.manual_seed(5)
    model = RT.build_model(opt, data, dev).to(dev)
    batches = T.TrainBatcher(data['train']['src'], data['train']['tgt'], 16, shuffle=False, drop_last=False)
    params = list(model.get_trainable_parameters())
    optimizer = O.Adam(params, betas=TC.ADAM_BETAS, lr=1e-3)
    torch.manual_seed(3)
    return T, O, data, opt, model, batches, params, optimizer


def test_train_epoch_averages_without_touching_the_trained_weights(dev, N):
    from lamp_amd import data as D
    from lamp_amd import training
    # 1: the epoch as it has always been
    T, O, data, opt, model, batches, params, optimizer = _loop_setup(dev)
    T.train_epoch(model, batches, optimizer, opt, device=dev)
    plain = [p.detach().clone() for p in params]
    # 2: with opt.weight_average
    T, O, data, opt, model, batches, params, optimizer = _loop_setup(dev)
    avg = opt.weight_average = O.WeightAverage(params, kind='ema', decay=0.9)
    T.train_epoch(model, batches, optimizer, opt, device=dev)
    torch.cuda.synchronize()
    assert avg.n_averaged == len(batches) == 3
    for a, b in zip(plain, params):
        assert RZ.bit_equal(a, b.detach()), 'averaging changed the trained weights'
    # 3: the weight sequence, from a plain loop over train_batch
    T, O, data, opt, model, batches, params, optimizer = _loop_setup(dev)
    model.train()
    L, n_mats = opt.tgt_vocab_size, T.n_loss_matrices(model, opt)
    seq, before = [], training.ORDERED_EMBED_GRAD
    training.ORDERED_EMBED_GRAD = True
    try:
        for (src_seq, src_pos), adj, tgt in batches:
            gold = D.get_gold_binary(tgt[:, 1:], L).float().to(dev)
            real = gold.shape[0]
            T.train_batch(model, optimizer, opt, (src_seq.to(dev), src_pos.to(dev)), adj.to(dev) if torch.is_tensor(adj) else adj, gold,
                          torch.zeros(real, L, device=dev), torch.zeros(n_mats, real, device=dev))
            seq.append([p.detach().cpu().clone() for p in params])
    finally:
        training.ORDERED_EMBED_GRAD = before
    for a, b in zip(plain, seq[-1]):
        assert RZ.bit_equal(a.cpu(), b), 'the plain loop is not the epoch'
    want = W.recurrence64(seq, 'ema', 0.9)
    t32 = _torch_fp32_average(seq_flat(seq), 'ema', 0.9, False)
    worst = 0.0
    for k, b in enumerate(avg.buffers):
        w64 = want[k].reshape(-1)
        fin = torch.isfinite(w64)
        assert torch.equal(b.cpu().reshape(-1)[~fin].double(), w64[~fin])
        gap = float((t32[k].double() - w64).abs()[fin].max())
        err = (b.cpu().reshape(-1).double() - w64).abs()[fin]
        tol = torch.maximum(W.ulp32(w64)[fin], torch.full_like(err, 4.0 * gap))
        worst = max(worst, float((err / tol).max()))
    print('WAVG train_epoch: worst used fraction of the recurrence bar %.3f' % worst)
    assert worst <= 1.0


def seq_flat(seq):
    return [[p.reshape(-1) for p in ps] for ps in seq]


# ------------------------------------------------------------------ run_train / run_eval end to end
def test_run_train_and_run_eval_end_to_end(dev, N, monkeypatch):
    from lamp_amd import data as D
    from lamp_amd import evaluate, run_eval, run_train
    from lamp_amd import train as T
    with tempfile.TemporaryDirectory(prefix='lamp_wavg_') as root:
        assert 'test' not in root
        data_path = os.path.join(root, 'train_valid_data.pt')
        torch.save(TC.synthetic_dataset(n_train=64, n_valid=16, n_test=16), data_path)
        model_args = ['-data', data_path, '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '1', '-label_mask', 'prior',
                      '-batch_size', '16']
        run_args = ['-epoch', '2', '-lr', '0.003', '-dropout', '0.0', '-results_dir', os.path.join(root, 'res'), '-seed', '1',
                    '-optim_impl', 'lamp']
        base = run_train.main(model_args + run_args + ['-name', 'b'])
        hist = run_train.main(model_args + run_args + ['-name', 'b', '-weight_avg', 'ema', '-ema_decay', '0.5', '-avg_start_epoch', '2'])
        # epoch 1: averaging has not begun, every number is the plain run's
        assert hist[0]['valid_loss'] == base[0]['valid_loss'] and hist[0]['test_loss'] == base[0]['test_loss']
        assert hist[0]['train_loss'] == base[0]['train_loss'] and hist[1]['train_loss'] == base[1]['train_loss']
        assert hist[0]['weights'] == 'raw' and hist[1]['weights'] == 'avg' and 'weights' not in base[0]
        assert hist[1]['valid_loss'] != base[1]['valid_loss']
        assert '.wavg_ema_0.5_s2.b/' in hist[1]['checkpoint'] and '.wavg' not in base[1]['checkpoint']
        plain = torch.load(base[1]['checkpoint'], map_location='cpu', weights_only=False)
        assert sorted(plain) == ['epoch', 'model', 'settings']
        first = torch.load(hist[0]['checkpoint'], map_location='cpu', weights_only=False) if hist[0]['checkpoint'] != hist[1]['checkpoint'] else None
        assert first is None                                  # (-save_mode best rewrites one file)
        ckpt = torch.load(hist[1]['checkpoint'], map_location='cpu', weights_only=False)
        assert sorted(ckpt) == ['epoch', 'model', 'model_avg', 'settings', 'weight_avg']
        n_steps = len(T.TrainBatcher(D.load_dataset(data_path)['train']['src'], D.load_dataset(data_path)['train']['tgt'], 16,
                                     shuffle=True, drop_last=True))      # (the steps of epoch 2: averaging began with it)
        assert n_steps >= 3
        assert ckpt['weight_avg'] == dict(kind='ema', decay=0.5, warmup=False, update_every=1, n_averaged=n_steps, n_calls=n_steps)
        st = ckpt['settings']
        assert (st.weight_avg, st.ema_decay, st.ema_warmup, st.avg_every, st.avg_start_epoch) == ('ema', 0.5, False, 1, 2)
        assert not hasattr(plain['settings'], 'weight_avg') and not hasattr(plain['settings'], 'ema_decay')
        assert sorted(ckpt['model']) == sorted(ckpt['model_avg'])
        for k in ckpt['model']:                               # 'model' is what was trained: the plain run's bits
            assert RZ.bit_equal(ckpt['model'][k], plain['model'][k]), k
        assert any(not torch.equal(ckpt['model'][k], ckpt['model_avg'][k]) for k in ckpt['model'])

        captured = {}
        real = run_eval.test_epoch

        def spy(*a, **k):
            out = real(*a, **k)
            captured['preds'] = out[0].clone()
            return out
        monkeypatch.setattr(run_eval, 'test_epoch', spy)

        def mine(state):
            opt = run_train.parse(model_args)
            data = D.load_dataset(data_path)
            torch.manual_seed(0)
            m = run_train.build_model(opt, data, dev)
            m.load_state_dict(state)
            m = m.to(dev).eval()
            batches = D.EvalBatcher(data['test']['src'], data['test']['tgt'], 16)
            return evaluate.test_epoch(m, batches, opt.tgt_vocab_size, 16, dev)[0]
        eval_args = model_args + ['-checkpoint', hist[1]['checkpoint'], '-split', 'test', '-batch_size', '16']
        out = run_eval.main(eval_args)
        assert out['weights'] == 'avg' and out['bce_total'] / out['n_samples'] == hist[1]['test_loss']
        assert RZ.bit_equal(captured['preds'], mine(ckpt['model_avg']))
        out_avg = run_eval.main(eval_args + ['-weights', 'avg'])
        assert out_avg['weights'] == 'avg' and out_avg['bce_total'] == out['bce_total']
        out_raw = run_eval.main(eval_args + ['-weights', 'raw'])
        assert 'weights' not in out_raw and out_raw['bce_total'] / out_raw['n_samples'] == base[1]['test_loss']
        assert RZ.bit_equal(captured['preds'], mine(ckpt['model']))
        old = run_eval.main(model_args + ['-checkpoint', base[1]['checkpoint'], '-split', 'test', '-batch_size', '16'])
        assert 'weights' not in old and set(old) == set(out_raw)
        with pytest.raises(SystemExit, match='model_avg'):
            run_eval.main(model_args + ['-checkpoint', base[1]['checkpoint'], '-split', 'test', '-weights', 'avg'])


# ------------------------------------------------------------------ past 2^32 bytes
BIG = (1 << 30) + 4097


def _flat_fill(view, vals):
    P, n = vals.numel(), view.numel()
    LX.fill_periodic_rows(view[:n // P * P].view(-1, P), vals.view(1, P))
    view[n // P * P:].copy_(vals[:n - n // P * P])


def _big_body(ar, N):
    P, n = LX.PERIOD, BIG
    g = torch.Generator().manual_seed(23)
    pp, pa = torch.randn(P, generator=g), torch.randn(P, generator=g)
    pv, av = ar.view('p'), ar.view('a')
    _flat_fill(pv, pp)
    _flat_fill(av, pa)
    arr = (N.OptimEntry * 1)()
    arr[0].param, arr[0].exp_avg, arr[0].numel = ar.ptr('p'), ar.ptr('a'), n
    w = 1.0 / 7.0
    ok(N.lib().lamp_weight_average(arr, 1, w, N.stream()), 'lamp_weight_average')
    ar.check_zones()
    whole = n // P * P
    LX.assert_bit_periodic(av[:whole].view(-1, P), 1, 'a after the update')
    LX.assert_bit_periodic(pv[:whole].view(-1, P), 1, 'p after the update')
    wins = LX.windows(n, 4, LX.FLAT_WINDOW)
    assert any(a <= (1 << 29) < b for a, b in wins) and any(a <= (1 << 30) < b for a, b in wins)      # 2^31 and 2^32 bytes
    worst, avg_win = 0.0, {}
    for a, b in wins:
        idx = torch.arange(a, b) % P
        assert torch.equal(pv[a:b].cpu(), pp[idx]), 'the weight is read only'
        got = av[a:b].cpu()
        avg_win[(a, b)] = got
        worst = max(worst, W.compare(got, pp[idx], pa[idx], w, torch.zeros(b - a, dtype=torch.bool), 'elements [%d, %d)' % (a, b)))
    print('WAVG large extent: worst used fraction of the bar %.3f' % worst)
    ok(N.lib().lamp_weight_swap(arr, 1, N.stream()), 'lamp_weight_swap')
    ar.check_zones()
    LX.assert_bit_periodic(av[:whole].view(-1, P), 1, 'a after the swap')
    LX.assert_bit_periodic(pv[:whole].view(-1, P), 1, 'p after the swap')
    for a, b in wins:
        idx = torch.arange(a, b) % P
        assert torch.equal(av[a:b].cpu(), pp[idx]) and RZ.bit_equal(pv[a:b].cpu(), avg_win[(a, b)]), 'swap, elements [%d, %d)' % (a, b)


def test_an_entry_past_2_to_the_32_bytes(dev, N):
    assert LX.crossings(4 * BIG) == ['B31', 'B32']
    ops = [('a', 4 * BIG), ('p', 4 * BIG)]
    need = LX.need_bytes(ops)
    LX.require_memory(need)
    ar = None
    try:
        ar = LX.BigArena(dev, LX.FILL_NAN, ops)
        _big_body(ar, N)
        torch.cuda.synchronize()
    finally:
        if ar is not None:
            ar.free()
        del ar
        gc.collect()
        torch.cuda.empty_cache()
