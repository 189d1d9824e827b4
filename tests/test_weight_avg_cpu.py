"""Weight averaging (lamp_amd.optim.WeightAverage, lamp_weight_average, lamp_weight_swap) where no
device is needed: the fp64 restatement of tests/weight_avg_common.py against torch.optim.swa_utils.AveragedModel, the host
schedule, every refusal of the two C entries (fake addresses that are never dereferenced: no call here reaches a launch),
the Python-side refusals, and what run_train / run_eval make of the new flags."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import weight_avg_common as W  # noqa: E402
from lamp_amd import _native as N  # noqa: E402
from lamp_amd import optim, run_eval, run_train  # noqa: E402

OK, E_DIMS, E_ALIGN, E_UNSUPPORTED, E_NULL = 0, -1, -2, -4, -5


# ------------------------------------------------------------------ the restatement against torch's AveragedModel, in fp64
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.zeros(37, 5, dtype=torch.float64))
        self.b = torch.nn.Parameter(torch.zeros(11, dtype=torch.float64))


@pytest.mark.parametrize('kind,decay', [('ema', 0.9), ('ema', 0.999), ('ema', 0.3), ('swa', 0.0)])
def test_restatement_equals_averaged_model_fp64(kind, decay):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn, get_swa_multi_avg_fn
    g = torch.Generator().manual_seed(11)
    net = _Net()
    fn = get_ema_multi_avg_fn(decay) if kind == 'ema' else get_swa_multi_avg_fn()
    ref = AveragedModel(net, multi_avg_fn=fn)
    seq = []
    for _ in range(12):
        with torch.no_grad():
            for p in net.parameters():
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64))      # (no equal, no infinite elements)
        ref.update_parameters(net)
        seq.append([p.detach().clone() for p in net.parameters()])
    want = [p.detach() for p in ref.module.parameters()]
    # torch's ema function hands lerp the Python double 1 - decay; its swa function takes 1 / (num_averaged + 1) from an
    # integer TENSOR, which makes the weight an fp32 number: the same rounding the kernel's host entry applies
    got = W.recurrence64(seq, kind, decay, round_weight=kind == 'swa')
    for x, y in zip(got, want):
        rel = float(((x - y).abs() / y.abs().clamp(min=1e-300)).max())
        print(kind, decay, 'max relative difference %.3e' % rel)
        assert rel <= 1e-15


# ------------------------------------------------------------------ the schedule
SCHEDULES = [('ema', d, wu, k) for d in (0.0, 0.9, 0.999) for wu in (False, True) for k in (1, 3)] + \
            [('swa', 0.0, False, 1), ('swa', 0.0, False, 3)]


@pytest.mark.parametrize('kind,decay,warmup,every', SCHEDULES)
def test_schedule(kind, decay, warmup, every):
    avg = optim.WeightAverage([], kind=kind, decay=decay, warmup=warmup, update_every=every)      # (no parameter: no launch)
    assert (avg.n_averaged, avg.n_calls) == (0, 0)
    for w, n_avg, n_calls in W.schedule(kind, decay, warmup, every, 40):
        avg.update()
        assert avg.last_weight == w
        assert (avg.n_averaged, avg.n_calls) == (n_avg, n_calls)
    assert avg.n_averaged == 40 // every
    sd = avg.state_dict()
    assert sd == dict(kind=kind, decay=float(decay), warmup=warmup, update_every=every, n_averaged=40 // every, n_calls=40,
                      buffers=[])
    twin = optim.WeightAverage([], kind='swa')
    twin.load_state_dict(sd)
    assert twin.state_dict() == sd and twin.next_weight() == avg.next_weight()


def test_schedule_values():
    assert W.schedule_weight('ema', 0.999, False, 0) == 1.0
    assert W.schedule_weight('ema', 0.999, False, 5) == 1.0 - 0.999
    assert W.schedule_weight('ema', 0.999, True, 5) == 1.0 - 6.0 / 15.0
    assert W.schedule_weight('ema', 0.9, True, 500) == 1.0 - 0.9
    assert W.schedule_weight('swa', 0.0, False, 3) == 0.25


# ------------------------------------------------------------------ the C entries' refusals
def fake(i):
    return 0x100000 * (i + 1)


def table(change=None, sizes=(8, 0, 4097)):
    arr = (N.OptimEntry * len(sizes))()
    for i, n in enumerate(sizes):
        arr[i].param, arr[i].exp_avg, arr[i].numel = fake(2 * i), fake(2 * i + 1), n
    for (i, field), v in (change or {}).items():
        setattr(arr[i], field, v)
    return arr


def call(entry, arr, n, weight=0.5):
    lib = N.lib()
    if entry == 'average':
        return lib.lamp_weight_average(arr, n, weight, None)
    return lib.lamp_weight_swap(arr, n, None)


REFUSALS = [
    ('n_negative', lambda: (table(), -1), E_DIMS),
    ('numel_negative', lambda: (table({(1, 'numel'): -1}), 3), E_DIMS),
    ('null_entries', lambda: (None, 3), E_NULL),
    ('null_param', lambda: (table({(0, 'param'): None}), 3), E_NULL),
    ('null_avg', lambda: (table({(2, 'exp_avg'): None}), 3), E_NULL),
    ('misaligned_param', lambda: (table({(2, 'param'): fake(4) + 2}), 3), E_ALIGN),
    ('misaligned_avg', lambda: (table({(0, 'exp_avg'): fake(1) + 1}), 3), E_ALIGN),
    ('chunks_2p31', lambda: (table({(0, 'numel'): 4096 << 31, (0, 'exp_avg'): fake(0) + (4096 << 33)}), 3), E_UNSUPPORTED),
    ('overlap_above', lambda: (table({(2, 'exp_avg'): fake(4) + 4 * 4096}), 3), E_UNSUPPORTED),
    ('overlap_below', lambda: (table({(2, 'param'): fake(5) + 4}), 3), E_UNSUPPORTED),
]


@pytest.mark.parametrize('entry', ['average', 'swap'])
@pytest.mark.parametrize('name,make,status', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_refuses(entry, name, make, status):
    arr, n = make()
    assert call(entry, arr, n) == status


@pytest.mark.parametrize('weight', [-1e-9, 1.0 + 1e-9, 2.0, float('nan'), float('inf'), -float('inf')])
def test_average_refuses_weight(weight):
    assert call('average', table(), 3, weight) == E_UNSUPPORTED


@pytest.mark.parametrize('entry', ['average', 'swap'])
def test_entry_without_launch(entry):
    """What succeeds without a launch: n == 0 (entries NULL or not), a table of empty tensors (NULL pointers allowed there),
    a table of entries whose two pointers are identical (no-ops), and lamp_weight_average with weight 0."""
    assert call(entry, None, 0) == OK
    assert call(entry, table(), 0) == OK
    assert call(entry, table({(0, 'param'): None, (1, 'exp_avg'): None}, sizes=(0, 0)), 2) == OK
    assert call(entry, table({(0, 'exp_avg'): fake(0)}, sizes=(8, 0)), 2) == OK
    if entry == 'average':
        assert call(entry, table(), 3, 0.0) == OK
        assert call(entry, table(), 3, 1e-60) == OK        # (rounds to an fp32 zero)


def test_weight_checked_before_entries_and_n_first():
    assert call('average', None, 3, 2.0) == E_UNSUPPORTED
    assert call('average', None, -1, 2.0) == E_DIMS


def test_abi_version_unchanged():
    assert N.lib().lamp_version() == 5


# ------------------------------------------------------------------ WeightAverage's own refusals
@pytest.mark.parametrize('kw', [dict(decay=1.0), dict(decay=-0.1), dict(decay=float('nan')), dict(kind='mean'), dict(update_every=0),
                                dict(update_every=-2), dict(update_every=1.5)])
def test_constructor_value_errors(kw):
    with pytest.raises(ValueError):
        optim.WeightAverage([], **kw)


def test_constructor_refuses_unserved_parameters():
    with pytest.raises(RuntimeError, match='There is no CPU path'):
        optim.WeightAverage([torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(RuntimeError, match='There is no CPU path'):
        optim.WeightAverage([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])


def test_applied_does_not_nest_and_update_while_swapped_raises():
    avg = optim.WeightAverage([])
    avg.update()
    with avg.applied():
        with pytest.raises(RuntimeError, match='nest'):
            with avg.applied():
                pass
        with pytest.raises(RuntimeError, match='swapped'):
            avg.update()
        with pytest.raises(RuntimeError, match='swapped'):
            avg.state_dict()
    assert (avg.n_averaged, avg.n_calls) == (1, 1)
    with pytest.raises(KeyError):          # swapped back on an exception too
        with avg.applied():
            raise KeyError('x')
    avg.update()
    assert (avg.n_averaged, avg.n_calls) == (2, 2)


def test_native_wrappers_refuse_cpu_tensors():
    p, a = torch.zeros(4), torch.zeros(4)
    with pytest.raises(RuntimeError):
        N.weight_average([(p, a)], 0.5)
    with pytest.raises(RuntimeError):
        N.weight_swap([(p, a)])
    with pytest.raises(RuntimeError):
        N.weight_average([(p, a.double())], 0.5)


# ------------------------------------------------------------------ run_train: parsing, naming, settings
BASE = ['-data', 'x.pt', '-dataset', 'reuters', '-d_model', '64', '-n_head', '4', '-n_layers_enc', '2', '-label_mask', 'prior',
        '-results_dir', 'r/']
NEW_KEYS = set(run_train.WEIGHT_AVG_FLAGS)


def test_without_the_flag_nothing_changes():
    opt = run_train.parse(BASE)
    with_flag = run_train.parse(BASE + ['-weight_avg', 'ema'])
    assert '.wavg' not in opt.model_name
    assert with_flag.model_name == opt.model_name + '.wavg_ema_0.999'
    s0, s1 = vars(run_train.checkpoint_settings(opt)), vars(run_train.checkpoint_settings(with_flag))
    assert not (NEW_KEYS | {'weight_average'}) & set(s0)
    assert {k: v for k, v in s1.items() if k not in NEW_KEYS | {'model_name'}} == {k: v for k, v in s0.items() if k != 'model_name'}
    assert {k: s1[k] for k in NEW_KEYS} == dict(weight_avg='ema', ema_decay=0.999, ema_warmup=False, avg_every=1, avg_start_epoch=1)
    # the other new flags alone change nothing either: they travel with -weight_avg only
    lone = run_train.parse(BASE + ['-ema_decay', '0.5', '-ema_warmup', '-avg_every', '4', '-avg_start_epoch', '3'])
    assert lone.model_name == opt.model_name
    assert vars(run_train.checkpoint_settings(lone)) == s0
    opt.weight_average = None          # (what main() leaves on opt is no setting)
    assert vars(run_train.checkpoint_settings(opt)) == s0


@pytest.mark.parametrize('argv,suffix', [
    (['-weight_avg', 'ema'], '.wavg_ema_0.999'),
    (['-weight_avg', 'ema', '-ema_decay', '0.99', '-ema_warmup'], '.wavg_ema_0.99_w'),
    (['-weight_avg', 'ema', '-avg_every', '4'], '.wavg_ema_0.999_e4'),
    (['-weight_avg', 'swa', '-avg_start_epoch', '38'], '.wavg_swa_swa_s38'),
    (['-weight_avg', 'swa', '-ema_warmup', '-avg_every', '2', '-avg_start_epoch', '3'], '.wavg_swa_swa_e2_s3'),
    (['-weight_avg', 'ema', '-ema_decay', '0.9', '-ema_warmup', '-avg_every', '2', '-avg_start_epoch', '3'], '.wavg_ema_0.9_w_e2_s3'),
])
def test_results_name(argv, suffix):
    base = run_train.parse(BASE).model_name
    opt = run_train.parse(BASE + argv + ['-name', 'run1'])
    assert opt.model_name == base + suffix + '.run1'
    assert opt.model_name.count('.wavg_') == 1       # (each flag once: the suffix above is all of it)


@pytest.mark.parametrize('argv', [['-avg_start_epoch', '0'], ['-ema_decay', '1'], ['-ema_decay', '-0.5'], ['-avg_every', '0']])
def test_run_train_refuses(argv):
    with pytest.raises((ValueError, SystemExit)):
        run_train.parse(BASE + ['-weight_avg', 'ema'] + argv)


def test_weight_avg_choices():
    with pytest.raises(SystemExit):
        run_train.parse(BASE + ['-weight_avg', 'mean'])


# ------------------------------------------------------------------ run_eval -weights
def test_run_eval_weights_choice():
    raw, avg = {'w': torch.zeros(2)}, {'w': torch.ones(2)}
    old = {'model': raw, 'settings': None, 'epoch': 3}
    new = dict(old, model_avg=avg, weight_avg={'kind': 'ema'})
    for ckpt, which, state, averaged in ((old, 'auto', raw, False), (old, 'raw', raw, False), (new, 'auto', avg, True),
                                         (new, 'avg', avg, True), (new, 'raw', raw, False),
                                         (raw, 'auto', raw, False), (raw, 'raw', raw, False)):      # (raw: a bare state dict)
        got, flag = run_eval.checkpoint_weights(ckpt, which)
        assert got is state and flag is averaged
    for ckpt in (old, raw, None):
        with pytest.raises(ValueError, match='model_avg'):
            run_eval.checkpoint_weights(ckpt, 'avg')
    assert run_eval.checkpoint_settings(new)[0] is raw                    # (the existing reader still sees what was trained)


def test_run_eval_parses_weights():
    base = ['-data', 'x.pt']
    assert run_eval.parse(base).weights == 'auto'
    assert run_eval.parse(base + ['-weights', 'avg']).weights == 'avg'
    with pytest.raises(SystemExit):
        run_eval.parse(base + ['-weights', 'ema'])
