"""CPU-side checks of gradient clipping, weight decay and momentum in the one-launch optimizer step: the ABI bookkeeping of the
three new entry points, what the optimizers' constructors accept and refuse, torch's param-group keys and state layout, which
native calls step() makes (defaults: exactly the old one), run_train's flags, and lamp_grad_norm's workspace contract.  Nothing
here needs a GPU."""
import copy
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from lamp_amd import _native as N
from lamp_amd import optim as O
from lamp_amd import run_train as RT

import optim_ext_common as XC
import train_common as TC

NEW_SYMBOLS = ('lamp_grad_norm_workspace_bytes', 'lamp_grad_norm', 'lamp_optim_step_ext')


def test_header_ctypes_and_library_carry_the_new_entry_points():
    text = open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in N.PROTOTYPES and name in N.LATE_ENTRY_POINTS and hasattr(lib, name)
    assert N.lib().lamp_version() == N.ABI_VERSION == 5        # additive: no struct changed
    assert ctypes.sizeof(N.OptimEntry) == 40 and ctypes.sizeof(N.OptimExt) == 32
    assert 'NaN spreads' in text and 'LAMP_OPTIM_SKIP_NONFINITE' in code and 'LAMP_OPTIM_DECOUPLED_DECAY' in code
    from lamp_amd import build as B
    res = B.kernel_resources('train_step.hip')
    for want in ('grad_norm_partial_kernel', 'grad_norm_final_kernel', 'optim_step_ext_kernel', 'optim_step_kernel'):
        assert any(want in k for k in res), want
    for name, r in res.items():
        assert r.get('scratch', 0) == 0 and r.get('agpr', 0) == 0, (name, r)


def _params():
    return [torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(5))]


def test_constructors_accept_the_new_keywords_and_refuse_the_unserved():
    a = O.Adam(_params(), weight_decay=0.01)           # (a TypeError before the feature)
    assert a.param_groups[0]['weight_decay'] == 0.01 and a.param_groups[0]['decoupled_weight_decay'] is False
    a = O.Adam(_params(), weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0, skip_nonfinite=True)
    assert a.param_groups[0]['decoupled_weight_decay'] is True and a.max_grad_norm == 1.0 and a.skip_nonfinite is True
    w = O.AdamW(_params())
    assert w.param_groups[0]['weight_decay'] == 1e-2 and w.param_groups[0]['decoupled_weight_decay'] is True
    s = O.SGD(_params(), momentum=0.9, weight_decay=0.1, max_grad_norm=2.0, skip_nonfinite=True)
    assert s.param_groups[0]['momentum'] == 0.9 and s.param_groups[0]['weight_decay'] == 0.1 and s.max_grad_norm == 2.0
    for cls, kw in ((O.Adam, dict(amsgrad=True)), (O.Adam, dict(maximize=True)), (O.AdamW, dict(amsgrad=True)),
                    (O.Adam, dict(weight_decay=-0.1)), (O.Adam, dict(max_grad_norm=-1.0)), (O.Adam, dict(max_grad_norm=float('nan'))),
                    (O.SGD, dict(nesterov=True, momentum=0.9)), (O.SGD, dict(dampening=0.1, momentum=0.9)),
                    (O.SGD, dict(momentum=1.0)), (O.SGD, dict(momentum=-0.1)), (O.SGD, dict(weight_decay=-1.0)),
                    (O.SGD, dict(maximize=True))):
        with pytest.raises(ValueError):
            cls(_params(), **kw)
    # defaults: the optimizers they have always been
    assert O.Adam(_params()).max_grad_norm is None and not O.Adam(_params())._extended()
    assert not O.SGD(_params())._extended()


def test_param_groups_carry_torchs_keys_and_adamw_state_round_trips():
    ps = _params()
    assert set(O.AdamW(ps).state_dict()['param_groups'][0]) == set(torch.optim.AdamW(ps).state_dict()['param_groups'][0])
    assert set(O.Adam(ps, weight_decay=0.1).state_dict()['param_groups'][0]) == \
        set(torch.optim.Adam(ps, weight_decay=0.1).state_dict()['param_groups'][0])
    assert set(O.SGD(ps, momentum=0.9).state_dict()['param_groups'][0]) == \
        set(torch.optim.SGD(ps, momentum=0.9).state_dict()['param_groups'][0])
    theirs = torch.optim.AdamW(ps, betas=TC.ADAM_BETAS, lr=2e-4, weight_decay=0.05)
    g = torch.Generator().manual_seed(0)
    for _ in range(3):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        theirs.step()
    ours = O.AdamW(ps, lr=1.0)
    ours.load_state_dict(copy.deepcopy(theirs.state_dict()))
    grp = ours.param_groups[0]
    assert (grp['weight_decay'], grp['lr'], grp['betas'], grp['decoupled_weight_decay']) == (0.05, 2e-4, TC.ADAM_BETAS, True)
    back = ours.state_dict()
    again = torch.optim.AdamW(ps, lr=1.0)
    again.load_state_dict(copy.deepcopy(back))
    assert again.param_groups[0]['weight_decay'] == 0.05
    for p in ps:
        for k in ('step', 'exp_avg', 'exp_avg_sq'):
            assert torch.equal(again.state[p][k], theirs.state[p][k]), k
    # SGD's momentum_buffer, both ways
    sgd = torch.optim.SGD(ps, lr=0.1, momentum=0.9)
    sgd.step()
    mine = O.SGD(ps, lr=1.0, momentum=0.5)
    mine.load_state_dict(copy.deepcopy(sgd.state_dict()))
    assert mine.param_groups[0]['momentum'] == 0.9
    assert all(torch.equal(mine.state[p]['momentum_buffer'], sgd.state[p]['momentum_buffer']) for p in ps)
    torch.optim.SGD(ps, lr=1.0, momentum=0.9).load_state_dict(mine.state_dict())


@pytest.fixture
def calls(monkeypatch):
    seen = []
    monkeypatch.setattr(N, 'optim_step', lambda *a, **k: seen.append(('optim_step', a, k)))
    monkeypatch.setattr(N, 'optim_step_ext', lambda *a, **k: seen.append(('optim_step_ext', a, k)))
    monkeypatch.setattr(N, 'grad_norm', lambda *a, **k: seen.append(('grad_norm', a, k)))
    monkeypatch.setattr(O, '_check', lambda p: p.grad)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: None)
    return seen


def _with_grads(ps):
    for p in ps:
        p.grad = torch.ones_like(p)
    return ps


def test_defaults_make_exactly_the_old_call(calls):
    ps = _with_grads(_params())
    O.Adam(ps, betas=TC.ADAM_BETAS, lr=0.5).step()
    assert [c[0] for c in calls] == ['optim_step']
    name, args, kwargs = calls[0]
    assert kwargs == {} and len(args) == 7           # N.optim_step(entries, KIND, step, lr, b1, b2, eps), positional
    assert args[1:] == (N.LAMP_OPTIM_ADAM, 1, 0.5, 0.9, 0.98, 1e-8) and len(args[0]) == 2
    del calls[:]
    O.SGD(ps, lr=0.25).step()
    assert [c[0] for c in calls] == ['optim_step'] and calls[0][1][1:] == (N.LAMP_OPTIM_SGD, 0, 0.25, 0.0, 0.0, 0.0)


def test_clipping_is_one_norm_launch_and_one_step_for_groups_that_differ_in_decay(calls):
    a, b = _with_grads(_params())
    opt = O.AdamW([dict(params=[a], weight_decay=0.1), dict(params=[b], weight_decay=0.0)], betas=TC.ADAM_BETAS, lr=0.5,
                  max_grad_norm=1.0)
    opt.step()
    assert [c[0] for c in calls] == ['grad_norm', 'optim_step_ext']
    _, nargs, nkw = calls[0]
    assert len(nargs[0]) == 2 and nargs[1] == 1.0 and nargs[2] is opt.grad_state and nargs[3] is None
    assert tuple(opt.grad_state.shape) == (4,) and opt.grad_state.dtype == torch.float32
    assert opt.skipped_steps.dtype == torch.int32 and opt.skipped_steps.numel() == 1
    _, sargs, skw = calls[1]
    assert sargs[1:] == (N.LAMP_OPTIM_ADAM, 1, 0.5, 0.9, 0.98, 1e-8)
    assert [e[0] for e in sargs[0]] == [a, b]
    assert skw == dict(weight_decay=[0.1, 0.0], decoupled=True, momentum=0.0, grad_state=opt.grad_state, skip_nonfinite=False)
    # groups that differ in lr launch separately, under ONE norm; the skip counter travels with skip_nonfinite
    del calls[:]
    opt = O.SGD([dict(params=[a], lr=0.1), dict(params=[b], weight_decay=0.3)], lr=0.5, momentum=0.9, skip_nonfinite=True)
    opt.step()
    assert [c[0] for c in calls] == ['grad_norm', 'optim_step_ext', 'optim_step_ext']
    assert calls[0][1][1] is None and calls[0][1][3] is opt.skipped_steps
    assert [c[2]['weight_decay'] for c in calls[1:]] == [[0.0], [0.3]] and all(c[2]['momentum'] == 0.9 for c in calls[1:])
    assert all(c[2]['skip_nonfinite'] is True for c in calls[1:])
    assert set(opt.state[a]) == {'momentum_buffer'}
    # weight decay alone: no norm launch
    del calls[:]
    O.Adam([a, b], weight_decay=0.1).step()
    assert [c[0] for c in calls] == ['optim_step_ext'] and calls[0][2]['grad_state'] is None and calls[0][2]['decoupled'] is False


# ------------------------------------------------------------------ run_train
BASE = ['-data', 'x.pt', '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-name', 'n1']


def test_run_train_name_and_settings_unchanged_without_the_flags_and_extended_with_them():
    opt = RT.parse(BASE)
    plain = opt.model_name
    assert not any(t in plain for t in ('.clip_', '.wd_', '.mom_', '.skipnf')) and plain.endswith('.adam.lr_0002.drop_10_10.nonemask.n1')
    st = RT.checkpoint_settings(opt)
    assert not any(hasattr(st, k) for k in RT.OPTIM_CONTROL_FLAGS)
    opt = RT.parse(BASE + ['-max_grad_norm', '1', '-weight_decay', '0.05', '-optim', 'adamw', '-skip_nonfinite', '-optim_impl', 'lamp'])
    assert opt.model_name == plain.replace('.adam.', '.adamw.')[:-len('.n1')] + '.clip_1.0.wd_0.05.skipnf.n1'
    st = RT.checkpoint_settings(opt)
    assert (st.max_grad_norm, st.weight_decay, st.skip_nonfinite, st.optim) == (1.0, 0.05, True, 'adamw')
    assert not hasattr(st, 'momentum')
    opt = RT.parse(BASE + ['-optim', 'sgd', '-momentum', '0.9'])
    assert opt.model_name == plain.replace('.adam.', '.sgd.')[:-len('.n1')] + '.mom_0.9.n1'
    st = RT.checkpoint_settings(opt)
    assert st.momentum == 0.9 and not any(hasattr(st, k) for k in ('max_grad_norm', 'weight_decay', 'skip_nonfinite'))


@pytest.mark.parametrize('argv', [['-skip_nonfinite', '-optim_impl', 'torch'], ['-momentum', '0.9'], ['-optim', 'sgd', '-momentum', '1.0'],
                                  ['-max_grad_norm', '-1'], ['-weight_decay', 'inf'], ['-optim', 'adamw', '-momentum', '0.5']])
def test_run_train_refuses_what_is_not_served(argv):
    with pytest.raises(ValueError):
        RT.parse(BASE + argv)


def test_label_bias_and_one_dimensional_parameters_never_decay():
    data = TC.synthetic_dataset(n_train=40)
    opt = RT.parse(BASE + ['-n_layers_enc', '1', '-learn_label_bias', '-weight_decay', '0.1', '-optim_impl', 'lamp'])
    model = RT.build_model(opt, data, 'cpu')
    decay, rest = RT.decay_param_groups(model, 0.1)
    assert (decay['weight_decay'], rest['weight_decay']) == (0.1, 0.0)
    names = {id(p): n for n, p in model.named_parameters()}
    assert any(names[id(p)].endswith('decoder.label_bias') for p in rest['params'])
    assert all(p.ndim >= 2 and not names[id(p)].endswith('label_bias') for p in decay['params']) and decay['params']
    assert all(p.ndim < 2 or names[id(p)].endswith('label_bias') for p in rest['params'])
    trainable = list(model.get_trainable_parameters())
    assert sorted(id(p) for g in (decay, rest) for p in g['params']) == sorted({id(p) for p in trainable})
    ours = RT.build_optimizer(model, opt)
    assert isinstance(ours, O.Adam) and [g['weight_decay'] for g in ours.param_groups] == [0.1, 0.0]
    # the torch route builds torch's optimizers over the same two groups
    opt_t = RT.parse(BASE + ['-n_layers_enc', '1', '-learn_label_bias', '-optim', 'adamw'])
    opt_t.optim_impl = 'torch'
    theirs = RT.build_optimizer(model, opt_t)
    assert isinstance(theirs, torch.optim.AdamW) and [g['weight_decay'] for g in theirs.param_groups] == [1e-2, 0.0]
    opt_t = RT.parse(BASE + ['-n_layers_enc', '1', '-optim', 'sgd', '-momentum', '0.9', '-max_grad_norm', '0.5'])
    opt_t.optim_impl = 'torch'
    theirs = RT.build_optimizer(model, opt_t)
    assert isinstance(theirs, torch.optim.SGD) and theirs.param_groups[0]['momentum'] == 0.9
    for p in model.get_trainable_parameters():
        p.grad = torch.ones_like(p)
    theirs.step()                                # clip_grad_norm_ runs in front of the step
    total = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.get_trainable_parameters()))
    assert abs(float(total) - 0.5) < 1e-4
    # without the flags: one flat group, as always
    flat = RT.parse(BASE + ['-n_layers_enc', '1', '-optim_impl', 'lamp'])
    assert len(RT.build_optimizer(RT.build_model(flat, data, 'cpu'), flat).param_groups) == 1


# ------------------------------------------------------------------ lamp_grad_norm's workspace contract
def _fake_table(sizes):
    """A table of fake (never dereferenced) 16-byte aligned device addresses: every check below fails before any launch."""
    arr = (N.OptimEntry * len(sizes))()
    for i, n in enumerate(sizes):
        arr[i].grad, arr[i].numel = 0x10000 * (i + 1), n
    return arr


def test_workspace_query_is_eight_bytes_per_chunk_and_a_short_workspace_is_refused():
    table = XC.hand_counted_table()
    arr = _fake_table([n for n, _ in table])
    chunks = sum(c for _, c in table)
    assert chunks == 18
    lib = N.lib()
    assert lib.lamp_grad_norm_workspace_bytes(arr, len(table)) == 8 * chunks
    assert lib.lamp_grad_norm_workspace_bytes(arr, 0) == 0
    # one byte short: refused before any launch (no device is touched: the addresses are fake)
    assert lib.lamp_grad_norm(arr, len(table), 1.0, 0x100000, 8 * chunks - 1, 0x200000, None, None) == -3      # LAMP_E_WORKSPACE
    assert lib.lamp_grad_norm(arr, len(table), 1.0, 0x100000, 8 * chunks, None, None, None) == -5              # no grad_state
    assert lib.lamp_grad_norm(arr, len(table), float('nan'), 0x100000, 8 * chunks, 0x200000, None, None) == -4
    bad = _fake_table([5, -1])
    assert lib.lamp_grad_norm(bad, 2, 1.0, 0x100000, 64, 0x200000, None, None) == -1


def test_optim_step_ext_refuses_before_any_launch():
    arr = _fake_table([8])
    arr[0].param, arr[0].exp_avg, arr[0].exp_avg_sq = 0x300000, 0x400000, 0x500000
    lib = N.lib()

    def call(kind, ext, step=1):
        return lib.lamp_optim_step_ext(arr, 1, kind, step, 1e-3, 0.9, 0.98, 1e-8, ctypes.byref(ext), None)

    wd = (ctypes.c_float * 1)(0.1)
    neg = (ctypes.c_float * 1)(-0.1)
    U = -4
    assert call(N.LAMP_OPTIM_ADAM, N.OptimExt(wd, None, 0.0, 4, 0)) == U                    # an unknown flag bit
    assert call(N.LAMP_OPTIM_ADAM, N.OptimExt(wd, None, 0.0, 0, 1)) == U                    # reserved
    assert call(N.LAMP_OPTIM_ADAM, N.OptimExt(neg, None, 0.0, 0, 0)) == U                   # negative decay
    assert call(N.LAMP_OPTIM_SGD, N.OptimExt(None, None, 1.0, 0, 0)) == U                   # momentum outside [0, 1)
    assert call(N.LAMP_OPTIM_SGD, N.OptimExt(None, None, -0.5, 0, 0)) == U
    assert call(N.LAMP_OPTIM_ADAM, N.OptimExt(None, None, 0.9, 0, 0)) == U                  # momentum with Adam
    assert call(N.LAMP_OPTIM_ADAM, N.OptimExt(wd, None, 0.0, N.LAMP_OPTIM_SKIP_NONFINITE, 0)) == U   # a skip without grad_state
    assert call(N.LAMP_OPTIM_SGD, N.OptimExt(wd, None, 0.0, N.LAMP_OPTIM_DECOUPLED_DECAY, 0)) == U   # SGD has the L2 form only
    assert call(7, N.OptimExt(wd, None, 0.0, 0, 0)) == U
    assert call(N.LAMP_OPTIM_ADAM, N.OptimExt(wd, None, 0.0, 0, 0), step=0) == -1
    arr[0].exp_avg = None
    assert call(N.LAMP_OPTIM_SGD, N.OptimExt(None, None, 0.9, 0, 0)) == -5                  # momentum needs its buffer
