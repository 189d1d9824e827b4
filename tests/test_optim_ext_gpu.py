"""lamp_grad_norm and lamp_optim_step_ext on the MI355X: the global gradient norm against an fp64 sum on the CPU (at most one
fp32 ulp), the clipped / decayed / momentum updates against fp64 evaluations of their formulas under the project's rule
(train_common.within: |err| <= max(1 fp32 ulp, 4 x the gap of torch's own fp32 CPU run of clip_grad_norm_ + torch.optim on the
same inputs), NaNs coincide), the non-finite skip, and the training loop with the options on.

The norm record is asserted bit-identical from run to run; it is NOT asserted under a permutation of the table (the partials
are added in table order: DESIGN.md section 8.11).

Measured (one run on one MI355X).  Norm, |err| / fp32 ulp: randn 0.31, 1e18 beside 1e-18 0.22, all 1e-18 0.19, one 3e38 0.00,
80 entries 0.25.  Updates, worst used fraction of the bar per configuration over 1 / 2 / 10 steps and the three clip settings
(none, binds, does not bind), parameters and moments: AdamW wd 0.01 0.70, AdamW wd 0.1 0.70, Adam with L2 decay 0.60, SGD
momentum 0.45, SGD momentum with decay 0.45.  After a skipped step: at most 0.47.
"""
import copy
import math
import os
import tempfile

import pytest
import torch

from lamp_amd import _native as N
from lamp_amd import optim as O
from lamp_amd import run_train as RT
from lamp_amd import train as T

import optim_ext_common as XC
import train_common as TC

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _misaligned(t):
    """A device copy that starts one float past a 16-byte boundary (4-byte aligned only)."""
    base = torch.empty(t.numel() + 1, device=DEV)
    base[1:] = t.to(DEV).reshape(-1)
    out = base[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out


def _to_dev(t):
    return _misaligned(t) if t.numel() == XC.MISALIGNED else t.to(DEV)


def _record(grads_dev, max_norm, skipped=None):
    rec = torch.full((4,), -7.0, device=DEV)
    N.grad_norm([(None, g, None, None) for g in grads_dev], max_norm, rec, skipped)
    torch.cuda.synchronize()
    return rec.cpu()


def _check_norm(grads, max_norm, what):
    dev = [_to_dev(g) for g in grads]
    rec = _record(dev, max_norm)
    want = XC.norm64(grads)
    got = float(rec[0].double())
    ulp = float(TC.ulp32(torch.tensor([want], dtype=torch.float64)))
    print('%s: norm %.9g, fp64 %.17g, |err| / ulp %.3f' % (what, got, want, abs(got - want) / ulp))
    assert abs(got - want) <= ulp, what
    assert torch.equal(rec[1], XC.scale32(rec[0], max_norm)), what
    assert float(rec[2]) == 1.0 and float(rec[3]) == 0.0
    assert torch.equal(_record(dev, max_norm), rec), what         # bit-identical from run to run
    return rec


# ------------------------------------------------------------------ the norm
def test_grad_norm_against_fp64():
    grads = XC.norm_case(0)
    want = XC.norm64(grads)
    rec = _check_norm(grads, None, 'randn')
    assert float(rec[1]) == 1.0
    rec = _check_norm(grads, 0.5 * want, 'randn, clip binds')
    assert 0.49 < float(rec[1]) < 0.51
    rec = _check_norm(grads, 1e6, 'randn, clip does not bind')
    assert float(rec[1]) == 1.0
    assert float(_check_norm(grads, 0.0, 'max_norm 0')[1]) == 0.0
    # 1e18 and 1e-18 side by side: fp32 squares would overflow / underflow
    big = [g.clone() for g in grads]
    big[3][7], big[3][8], big[5][-1] = 1e18, 1e-18, -1e18
    _check_norm(big, 1.0, '1e18 beside 1e-18')
    tiny = [torch.full_like(g, 1e-18) for g in grads]
    rec = _check_norm(tiny, None, 'all 1e-18')
    assert float(rec[0]) > 0.0
    _check_norm([torch.tensor([0.0, -3e38, 0.0]), torch.zeros(5)], 1.0, '3e38: its square leaves fp32, the norm does not')
    # the standalone diagnostic is the same launch
    ps = [torch.nn.Parameter(torch.zeros_like(g, device=DEV)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.to(DEV)
    n = O.grad_norm(ps)
    assert n.is_cuda and n.dim() == 0 and abs(float(n) - want) <= float(TC.ulp32(torch.tensor([want], dtype=torch.float64)))


def test_grad_norm_over_a_table_longer_than_one_launch():
    grads = XC.long_table_case()
    assert len(grads) == 80
    _check_norm(grads, 3.0, '80 entries')
    # global over the whole table: the first 72 entries alone give another norm
    assert XC.norm64(grads[:72]) < XC.norm64(grads) * (1 - 1e-3)


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
def test_a_planted_non_finite_gradient_is_seen(bad):
    for where in (0, 3, 5):
        grads = XC.norm_case(2)
        grads[where][-1] = bad
        skipped = torch.zeros((), dtype=torch.int32, device=DEV)
        rec = _record([_to_dev(g) for g in grads], 1.0, skipped)
        assert float(rec[2]) == 0.0 and not math.isfinite(float(rec[0]))
        assert int(skipped) == 1
        if bad != bad:
            assert rec[1] != rec[1]          # a NaN norm: a NaN scale, as clip_grad_norm_ gives
        else:
            assert float(rec[1]) == 0.0
    skipped = torch.zeros((), dtype=torch.int32, device=DEV)
    assert float(_record([g.to(DEV) for g in XC.norm_case(2)], 1.0, skipped)[2]) == 1.0 and int(skipped) == 0


def test_an_exact_workspace_is_enough_and_a_short_one_is_refused():
    grads = [g.to(DEV) for g in XC.norm_case(3)]
    arr = N._optim_table([(None, g, None, None) for g in grads])
    nbytes = N.lib().lamp_grad_norm_workspace_bytes(arr, len(grads))
    assert nbytes == 8 * sum((g.numel() + 4095) // 4096 for g in grads)
    ws = torch.full((nbytes // 8 + 2,), -1.0, dtype=torch.float64, device=DEV)     # one sentinel on either side
    rec = torch.zeros(4, device=DEV)
    N.check(N.lib().lamp_grad_norm(arr, len(grads), -1.0, ws[1:].data_ptr(), nbytes, rec.data_ptr(), None, N.stream()), 'norm')
    torch.cuda.synchronize()
    assert float(ws[0]) == -1.0 and float(ws[-1]) == -1.0 and bool((ws[1:-1] >= 0).all())
    assert abs(float(rec[0]) - XC.norm64(grads)) <= float(TC.ulp32(torch.tensor([XC.norm64(grads)], dtype=torch.float64)))
    assert N.lib().lamp_grad_norm(arr, len(grads), -1.0, ws[1:].data_ptr(), nbytes - 8, rec.data_ptr(), None, N.stream()) == -3


# ------------------------------------------------------------------ the updates
def _make(kind, dev_params, lr, wd, decoupled, momentum, max_norm, skip=False):
    extra = dict(max_grad_norm=max_norm, skip_nonfinite=skip)
    if kind == 'adam':
        return O.Adam(dev_params, betas=TC.ADAM_BETAS, lr=lr, weight_decay=wd, decoupled_weight_decay=decoupled, **extra)
    return O.SGD(dev_params, lr=lr, momentum=momentum, weight_decay=wd, **extra)


def _run_device(kind, params, grads, lr_seq, wd, decoupled, momentum, max_norm, skip=False):
    dev = [torch.nn.Parameter(_to_dev(p)) for p in params]
    opt = _make(kind, dev, lr_seq[0], wd, decoupled, momentum, max_norm, skip)
    for i, lr in enumerate(lr_seq):
        for g in opt.param_groups:
            g['lr'] = lr
        kept = []
        for p, gr in zip(dev, grads[i]):
            p.grad = _to_dev(gr)
            kept.append(p.grad.clone())
        opt.step()
        for p, k in zip(dev, kept):
            assert torch.equal(p.grad.view(torch.int32), k.view(torch.int32))     # the gradient buffer keeps its bits, clipped or not
    torch.cuda.synchronize()
    return dev, opt


def _state(opt, p, kind):
    st = opt.state[p]
    return (st['exp_avg'], st['exp_avg_sq']) if kind == 'adam' else (st.get('momentum_buffer'), None)


@pytest.mark.parametrize('n_steps', [1, 2, 10])
@pytest.mark.parametrize('config', sorted(XC.CONFIGS))
def test_updates_against_fp64(config, n_steps):
    kind, wd, decoupled, momentum = XC.CONFIGS[config]
    params, grads = XC.ext_case(3, n_steps)
    lr_seq = XC.lrs(kind, n_steps)
    worst = 0.0
    for clip in XC.CLIPS:
        max_norm = XC.max_norm_of(clip, grads)
        want = XC.reference64(kind, params, grads, lr_seq, wd, decoupled, momentum, max_norm)
        cpu, ref = XC.torch_fp32(kind, params, grads, lr_seq, wd, decoupled, momentum, max_norm)
        dev, opt = _run_device(kind, params, grads, lr_seq, wd, decoupled, momentum, max_norm)
        if clip == 'binds':
            assert float(opt.grad_state[1]) < 1.0
        elif clip == 'loose':
            assert float(opt.grad_state[1]) == 1.0
        else:
            assert opt.grad_state is None
        for k, p in enumerate(dev):
            if p.numel() == 0:
                continue
            what = '%s, clip %s, %d elements, %d steps' % (config, clip, p.numel(), n_steps)
            worst = max(worst, TC.within(p.detach(), want[k][0], TC.gap(cpu[k].detach(), want[k][0]), 'param ' + what))
            tm, tv = XC.torch_state(ref, cpu[k], kind)
            m, v = _state(opt, p, kind)
            worst = max(worst, TC.within(m, want[k][1], TC.gap(tm, want[k][1]), 'first moment / buffer ' + what))
            if v is not None:
                worst = max(worst, TC.within(v, want[k][2], TC.gap(tv, want[k][2]), 'exp_avg_sq ' + what))
    print('%s, %d steps: worst used fraction of the bar %.3f' % (config, n_steps, worst))


def test_mixed_groups_give_the_bits_of_two_single_group_optimizers():
    params, grads = XC.ext_case(5, 2)
    half = len(params) // 2
    for cls, kw in ((O.AdamW, dict(betas=TC.ADAM_BETAS, lr=2e-3)), (O.Adam, dict(betas=TC.ADAM_BETAS, lr=2e-3)),
                    (O.SGD, dict(lr=0.05, momentum=0.9))):
        a = [torch.nn.Parameter(_to_dev(p)) for p in params]
        b = [torch.nn.Parameter(_to_dev(p)) for p in params]
        one = cls([dict(params=a[:half], weight_decay=0.1), dict(params=a[half:], weight_decay=0.0)], **kw)
        two = [cls(b[:half], weight_decay=0.1, **kw), cls(b[half:], weight_decay=0.0, **kw)]
        for i in range(2):
            for p, q, gr in zip(a, b, grads[i]):
                p.grad, q.grad = _to_dev(gr), _to_dev(gr)
            one.step()
            for o in two:
                o.step()
        torch.cuda.synchronize()
        for p, q in zip(a, b):
            assert torch.equal(p.detach(), q.detach()), cls.__name__
        assert not torch.equal(a[0].detach(), params[0].to(DEV))


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_with_every_option_at_its_default_the_extended_step_is_the_old_one(kind):
    params, grads = TC.optim_case(7, 1)
    K = N.LAMP_OPTIM_ADAM if kind == 'adam' else N.LAMP_OPTIM_SGD

    def table():
        ps = [_to_dev(p) for p in params]
        return [(p, _to_dev(g), torch.zeros_like(p) if kind == 'adam' else None, torch.zeros_like(p) if kind == 'adam' else None)
                for p, g in zip(ps, grads[0])]

    old, new, unit = table(), table(), table()
    N.optim_step(old, K, 1, 2e-3, 0.9, 0.98, 1e-8)
    N.optim_step_ext(new, K, 1, 2e-3, 0.9, 0.98, 1e-8)
    # ... and through the extended kernel itself: a record whose scale is 1, decay 0 everywhere
    rec = torch.zeros(4, device=DEV)
    N.grad_norm(unit, None, rec)
    N.optim_step_ext(unit, K, 1, 2e-3, 0.9, 0.98, 1e-8, weight_decay=[0.0] * len(unit), grad_state=rec)
    torch.cuda.synchronize()
    assert float(rec[1]) == 1.0
    for o, n, u in zip(old, new, unit):
        for a, b, c in zip(o, n, u):
            if a is not None:
                assert torch.equal(a, b) and torch.equal(a, c)


def test_minus_infinity_in_a_zero_decay_group_stays_and_the_rest_stays_finite():
    g = torch.Generator().manual_seed(9)
    bias = torch.randn(37, 37, generator=g)
    bias[torch.rand(37, 37, generator=g) < 0.3] = float('-inf')
    blocked = torch.isinf(bias)
    w = torch.randn(50, 20, generator=g)
    for cls, kw in ((O.AdamW, dict(betas=TC.ADAM_BETAS, lr=1e-2)), (O.Adam, dict(betas=TC.ADAM_BETAS, lr=1e-2)),
                    (O.SGD, dict(lr=1e-2, momentum=0.9))):
        pb, pw = torch.nn.Parameter(bias.to(DEV)), torch.nn.Parameter(w.to(DEV))
        opt = cls([dict(params=[pw], weight_decay=0.1), dict(params=[pb], weight_decay=0.0)], max_grad_norm=0.5, **kw)
        for _ in range(3):
            gb = torch.randn(37, 37, generator=g)
            gb[blocked] = 0.0                     # a blocked edge has no gradient
            pb.grad, pw.grad = gb.to(DEV), torch.randn(50, 20, generator=g).to(DEV)
            opt.step()
        torch.cuda.synchronize()
        out = pb.detach().cpu()
        assert torch.equal(torch.isinf(out) & (out < 0), blocked), cls.__name__
        assert bool(torch.isfinite(out[~blocked]).all()) and bool(torch.isfinite(pw.detach()).all())
        assert not torch.equal(out[~blocked], bias[~blocked])


def test_state_round_trips_to_the_torch_optimizers_on_the_device():
    params, grads = TC.optim_case(11, 2)
    lr_seq = [2e-3, 2e-3]
    for config, theirs_cls in (('adamw_0.1', torch.optim.AdamW), ('adam_l2', torch.optim.Adam), ('sgd_momentum_decay', torch.optim.SGD)):
        kind, wd, decoupled, momentum = XC.CONFIGS[config]
        dev, opt = _run_device(kind, params, grads, lr_seq, wd, decoupled, momentum, None)
        there = theirs_cls(dev, lr=1.0)
        there.load_state_dict(opt.state_dict())
        grp = there.param_groups[0]
        assert grp['weight_decay'] == wd and grp['lr'] == 2e-3
        key = 'exp_avg' if kind == 'adam' else 'momentum_buffer'
        assert all(torch.equal(there.state[p][key], opt.state[p][key]) for p in dev)
        if kind == 'sgd':
            assert grp['momentum'] == momentum
        # and back: the state torch hands over drives the next step here to the same bits as staying here
        back = _make(kind, dev, 1.0, 0.0, False, 0.0, None)
        back.load_state_dict(there.state_dict())
        assert back.param_groups[0]['weight_decay'] == wd
        twin = [torch.nn.Parameter(p.detach().clone()) for p in dev]
        stay = _make(kind, twin, 1.0, 0.0, False, 0.0, None)
        stay.load_state_dict(copy.deepcopy(opt.state_dict()))      # (load_state_dict keeps the tensors it is given)
        for p, q in zip(dev, twin):
            p.grad = torch.ones_like(p)
            q.grad = torch.ones_like(q)
        back.step()
        stay.step()
        torch.cuda.synchronize()
        assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(dev, twin))


# ------------------------------------------------------------------ the skip
@pytest.mark.parametrize('config', ['adamw_0.01', 'sgd_momentum_decay'])
def test_a_non_finite_step_is_skipped_on_the_device(config):
    kind, wd, decoupled, momentum = XC.CONFIGS[config]
    params, grads = XC.ext_case(13, 3)
    grads[1][3][5] = float('nan')                     # one element, step 2 of 3
    lr_seq = XC.lrs(kind, 3)
    max_norm = 0.5 * XC.norm64(grads[0])
    dev = [torch.nn.Parameter(_to_dev(p)) for p in params]
    opt = _make(kind, dev, lr_seq[0], wd, decoupled, momentum, max_norm, skip=True)
    snaps = []
    for i, lr in enumerate(lr_seq):
        opt.param_groups[0]['lr'] = lr
        for p, gr in zip(dev, grads[i]):
            p.grad = _to_dev(gr)
        opt.step()
        snaps.append([[t.detach().clone() for t in (p,) + tuple(x for x in _state(opt, p, kind) if x is not None)] for p in dev])
    torch.cuda.synchronize()
    assert int(opt.skipped_steps) == 1 and float(opt.grad_state[2]) == 1.0
    for a, b in zip(snaps[0], snaps[1]):               # step 2 wrote nothing
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    if kind == 'adam':
        assert float(opt.state[dev[0]]['step']) == 3   # the host-side count advanced all the same
    want = XC.reference64(kind, params, grads, lr_seq, wd, decoupled, momentum, max_norm, skip_nonfinite=True)
    # torch's fp32 yardstick: the same sequence without the bad step, Adam's bias correction aside (a gap, not a reference)
    cpu, _ = XC.torch_fp32(kind, params, [grads[0], grads[2]], [lr_seq[0], lr_seq[2]], wd, decoupled, momentum, max_norm)
    clean = XC.reference64(kind, params, [grads[0], grads[2]], [lr_seq[0], lr_seq[2]], wd, decoupled, momentum, max_norm)
    for k, p in enumerate(dev):
        if p.numel():
            TC.within(p.detach(), want[k][0], TC.gap(cpu[k].detach(), clean[k][0]), '%s after a skipped step, %d elements' % (config, p.numel()))
    # without the flag the NaN spreads exactly as the formula says
    dev2, opt2 = _run_device(kind, params, grads, lr_seq, wd, decoupled, momentum, None)
    spread = XC.reference64(kind, params, grads, lr_seq, wd, decoupled, momentum, None)
    for k, p in enumerate(dev2):
        assert torch.equal(torch.isnan(p.detach().cpu()), torch.isnan(spread[k][0])), k
    assert int(torch.isnan(dev2[3].detach()).sum()) == 1
    dev3, _ = _run_device(kind, params, grads, lr_seq, wd, decoupled, momentum, max_norm)       # clipped: the NaN scale reaches all
    spread = XC.reference64(kind, params, grads, lr_seq, wd, decoupled, momentum, max_norm)
    for k, p in enumerate(dev3):
        assert torch.equal(torch.isnan(p.detach().cpu()), torch.isnan(spread[k][0])), k
        assert bool(torch.isnan(p.detach()).all())


# ------------------------------------------------------------------ through the loop
ARGS = ['-data', 'x.pt', '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '1', '-dropout', '0.1',
        '-learn_label_bias', '-label_mask', 'prior']


def _epochs(make_optimizer, n_epochs=2):
    data = TC.synthetic_dataset(n_train=48)
    opt = RT.parse(ARGS)
    torch.manual_seed(5)
    model = RT.build_model(opt, data, DEV).to(DEV)
    batches = T.TrainBatcher(data['train']['src'], data['train']['tgt'], 16, shuffle=False, drop_last=False)
    optimizer = make_optimizer(model)
    torch.manual_seed(3)
    for _ in range(n_epochs):
        _, _, loss = T.train_epoch(model, batches, optimizer, opt, device=DEV)
    torch.cuda.synchronize()
    assert loss == loss
    return {k: v.detach().clone() for k, v in model.state_dict().items()}, optimizer


def test_training_epochs_with_the_options_are_reproducible_and_defaults_are_todays_epoch():
    def adamw(model):
        return O.AdamW(RT.decay_param_groups(model, 0.05), betas=TC.ADAM_BETAS, lr=1e-3, max_grad_norm=0.05, skip_nonfinite=True)

    a, opt_a = _epochs(adamw)
    b, _ = _epochs(adamw)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert int(opt_a.skipped_steps) == 0 and float(opt_a.grad_state[2]) == 1.0 and 0.0 < float(opt_a.grad_state[1]) <= 1.0
    bias = a['decoder.label_bias']
    assert not bool(torch.isnan(bias).any())
    # a clip too large to bind and decay 0: bit for bit the epoch of today's Adam
    loose, _ = _epochs(lambda m: O.AdamW(RT.decay_param_groups(m, 0.0), betas=TC.ADAM_BETAS, lr=1e-3, max_grad_norm=1e9,
                                         skip_nonfinite=True))
    plain, _ = _epochs(lambda m: O.Adam(list(m.get_trainable_parameters()), betas=TC.ADAM_BETAS, lr=1e-3))
    assert all(torch.equal(loose[k], plain[k]) for k in plain)
    assert not all(torch.equal(a[k], plain[k]) for k in plain)


def test_run_train_with_the_flags_on_both_optimizer_routes():
    """run_train -optim adamw -weight_decay -max_grad_norm -skip_nonfinite end to end (two short epochs): steps_skipped in
    every epoch's record, the flags in the results name and the checkpoint's settings, a learnable label bias that never
    decays; and the torch route (clip_grad_norm_ + torch.optim.SGD(momentum=)) from the same flags."""
    with tempfile.TemporaryDirectory(prefix='lamp_optx_') as root:
        assert 'test' not in root
        data_path = os.path.join(root, 'train_valid_data.pt')
        torch.save(TC.synthetic_dataset(n_train=64, n_valid=16, n_test=16), data_path)
        args = ['-data', data_path, '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '1', '-label_mask', 'prior',
                '-learn_label_bias', '-batch_size', '16', '-lr', '0.003', '-dropout', '0.0', '-results_dir', os.path.join(root, 'res'),
                '-seed', '1']
        hist = RT.main(args + ['-epoch', '2', '-name', 'ext', '-optim', 'adamw', '-weight_decay', '0.05', '-max_grad_norm', '0.5',
                               '-skip_nonfinite', '-optim_impl', 'lamp'])
        assert [h['steps_skipped'] for h in hist] == [0, 0] and hist[1]['train_loss'] < hist[0]['train_loss']
        assert '.adamw.' in hist[1]['checkpoint'] and '.clip_0.5.wd_0.05.skipnf.ext/' in hist[1]['checkpoint']
        ckpt = torch.load(hist[1]['checkpoint'], map_location='cpu', weights_only=False)
        st = ckpt['settings']
        assert (st.optim, st.weight_decay, st.max_grad_norm, st.skip_nonfinite) == ('adamw', 0.05, 0.5, True)
        assert not hasattr(st, 'momentum')
        assert all(bool(torch.isfinite(v).all()) for k, v in ckpt['model'].items() if v.is_floating_point() and 'label_bias' not in k)
        more = RT.main(args + ['-epoch', '1', '-name', 'sgdm', '-optim', 'sgd', '-momentum', '0.9', '-weight_decay', '0.01',
                               '-max_grad_norm', '0.5', '-optim_impl', 'torch'])
        assert 'steps_skipped' not in more[0] and more[0]['train_loss'] == more[0]['train_loss']
        assert '.sgd.' in more[0]['checkpoint'] and '.clip_0.5.wd_0.01.mom_0.9.sgdm/' in more[0]['checkpoint']
