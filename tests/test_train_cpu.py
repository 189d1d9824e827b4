"""CPU-side checks of the training layer: ABI bookkeeping of the two new entry points, run_train's flags against the
reference's config_args.py, the training batcher against the reference's DataLoader, the checkpoint format, optimizer state
exchange with torch.optim.Adam, StepLR, and the scope guards.  Nothing here needs a GPU."""
import argparse
import copy
import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

from lamp_amd import _native as N
from lamp_amd import optim as O
from lamp_amd import run_train as RT
from lamp_amd.train import TrainBatcher, train_epoch

import train_common as TC

REF = '/root/reference'


def test_header_ctypes_and_library_carry_the_training_entry_points():
    text = open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ('lamp_bce_logits_train', 'lamp_optim_step', 'lamp_embed_bwd_ordered'):
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in N.PROTOTYPES and hasattr(lib, name)
    assert N.lib().lamp_version() == N.ABI_VERSION == 5     # the ABI grew by addition only
    assert ctypes.sizeof(N.OptimEntry) == 40
    from lamp_amd import build as B
    assert 'train_step.hip' in B.SOURCES
    for name, r in B.kernel_resources('train_step.hip').items():
        assert r.get('scratch', 0) == 0 and r.get('agpr', 0) == 0, (name, r)
    assert any('optim_step_kernel' in k for k in B.kernel_resources('train_step.hip'))


LISTED = ('epoch', 'batch_size', 'lr', 'lr_step_size', 'lr_decay', 'optim', 'dropout', 'dec_dropout', 'int_preds',
          'int_pred_weight', 'label_mask', 'save_mode', 'load_pretrained', 'name', 'results_dir',
          # derived on the way
          'n_layers_dec', 'test_batch_size', 'd_k', 'd_v', 'd_inner_hid', 'n_head2', 'no_enc_pos_embedding', 'onehot',
          'binary_relevance', 'proj_share_weight', 'dec_dropout2', 'd_word_vec', 'model_name')


def _is_reference_module(name):
    return name.split('.')[0] in ('utils', 'lamp', 'config_args')


@pytest.fixture
def reference_imports(monkeypatch, has_reference):
    """The reference checkout first on sys.path for one test; its modules (and whatever they shadowed) are put back after."""
    if not has_reference:
        pytest.skip('the reference checkout is not on this machine')
    saved = {k: v for k, v in sys.modules.items() if _is_reference_module(k)}
    for k in saved:
        del sys.modules[k]
    monkeypatch.syspath_prepend(REF)
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self, raising=False)
    yield
    for k in [k for k in sys.modules if _is_reference_module(k)]:
        del sys.modules[k]
    sys.modules.update(saved)


def _reference_opt(argv, monkeypatch):
    import config_args as CA
    monkeypatch.setattr(sys, 'argv', ['main.py'] + argv)
    return CA.config_args(CA.get_args(argparse.ArgumentParser()))


@pytest.mark.parametrize('argv', [
    [],
    ['-dataset', 'bibtext', '-batch_size', '32', '-d_model', '256', '-n_head', '4', '-n_layers_enc', '2', '-label_mask', 'prior',
     '-int_preds', '-lr', '0.0005', '-lr_decay', '0.9', '-lr_step_size', '10', '-dropout', '0.2', '-name', 'x1', '-epoch', '3'],
    ['-dataset', 'gm12878', '-dec_dropout', '0.3', '-n_head2', '2', '-save_mode', 'all', '-int_pred_weight', '0.5',
     '-no_dec_self_att', '-results_dir', 'out/'],
])
def test_run_train_flags_and_derived_defaults_equal_config_args(argv, monkeypatch, reference_imports):
    ref = _reference_opt(argv + ['-decoder', 'graph'], monkeypatch)
    ours = RT.parse(['-data', 'unused.pt'] + argv)
    for key in LISTED:
        assert getattr(ours, key) == getattr(ref, key), key
    if not argv:   # the bare defaults, flag by flag
        assert (ours.epoch, ours.batch_size, ours.lr, ours.optim, ours.save_mode) == (50, 64, 0.0002, 'adam', 'best')


def test_scope_guards_name_their_reasons():
    with pytest.raises(NotImplementedError, match='rnn_m'):
        RT.parse(['-data', 'x.pt', '-decoder', 'rnn_m'])
    with pytest.raises(NotImplementedError, match='collective'):
        RT.parse(['-data', 'x.pt', '-gpus', '2'])
    with pytest.raises(NotImplementedError, match='rnn_m'):
        train_epoch(None, None, None, TC.train_opt(5, decoder='rnn_m'))


def _reference_loader(src, tgt, batch_size, shuffle, drop_last):
    from utils.data_loader import DataLoader
    d = {'<blank>': 0}
    return DataLoader(d, d, src_insts=list(src), tgt_insts=list(tgt), batch_size=batch_size, binary_relevance=True, cuda=False,
                      shuffle=shuffle, drop_last=drop_last)


@pytest.mark.parametrize('n,batch_size,drop_last', [(40, 8, True), (37, 8, True), (20, 8, False), (37, 8, False)])
def test_batcher_order_and_last_batch_equal_the_reference_loader(n, batch_size, drop_last, reference_imports):
    """The reference's training loader (process_data: shuffle=True, drop_last=True) shuffles at construction and after every
    pass and takes one batch off the count -- a FULL one when n is a multiple of the batch size.  Its permutation comes from
    Python's `random`; ours from a torch.Generator, so the reference's order is read back and set explicitly: every batch's
    tokens, positions and targets must then be equal, pass after pass."""
    data = TC.synthetic_dataset(n_train=n)
    src, tgt = data['train']['src'], data['train']['tgt']
    random.seed(11)
    ref = _reference_loader(src, tgt, batch_size, True, drop_last)
    ours = TrainBatcher(src, tgt, batch_size, shuffle=True, drop_last=drop_last)
    assert len(ours) == len(ref) == (n + batch_size - 1) // batch_size - (1 if drop_last else 0)
    assert ours.n_insts == len(ref._src_insts) == n
    index = {id(s): i for i, s in enumerate(src)}
    for _ in range(2):
        order = [index[id(s)] for s in ref._src_insts]
        assert sorted(order) == list(range(n)) and order != list(range(n))
        ours.set_order(order)
        ref_batches, our_batches = list(ref), list(ours)     # (both reshuffle at the end of the pass)
        assert len(ref_batches) == len(our_batches) == len(ref)
        for ((rs, rp), radj, rt), ((s, p), adj, t) in zip(ref_batches, our_batches):
            assert radj is None and adj is None
            assert torch.equal(rs, s) and torch.equal(rp, p) and torch.equal(rt, t)
        if not drop_last and n % batch_size:
            assert our_batches[-1][0][0].size(0) == n % batch_size      # the short last batch, as it is


@pytest.mark.parametrize('n,batch_size,drop_last', [(40, 8, True), (37, 8, True), (37, 8, False)])
def test_batcher_shuffling_is_fixed_by_the_torch_seed(n, batch_size, drop_last):
    """Our own shuffling (no reference needed): a permutation fixed by torch.manual_seed, a new one after every pass, the
    reference's batch count and the short last batch as it is."""
    data = TC.synthetic_dataset(n_train=n)
    src, tgt = data['train']['src'], data['train']['tgt']
    torch.manual_seed(3)
    a = TrainBatcher(src, tgt, batch_size, drop_last=drop_last)
    torch.manual_seed(3)
    b = TrainBatcher(src, tgt, batch_size, drop_last=drop_last)
    assert len(a) == (n + batch_size - 1) // batch_size - (1 if drop_last else 0)
    assert np.array_equal(a.order, b.order) and sorted(a.order.tolist()) == list(range(n)) and a.order.tolist() != list(range(n))
    first = a.order.copy()
    batches = list(a)
    assert len(batches) == len(a)
    assert not np.array_equal(a.order, first) and sorted(a.order.tolist()) == list(range(n))
    for bi, ((seq, pos), adj, t) in enumerate(batches):
        idx = first[bi * batch_size:(bi + 1) * batch_size]
        assert adj is None and seq.size(0) == len(idx) == t.size(0)
        for r, i in enumerate(idx):
            assert seq[r, :len(src[i])].tolist() == src[i] and not seq[r, len(src[i]):].any()
            assert pos[r, :len(src[i])].tolist() == list(range(1, len(src[i]) + 1))
            assert t[r, :len(tgt[i])].tolist() == tgt[i]
    if not drop_last:
        assert batches[-1][0][0].size(0) == n % batch_size
    assert [torch.equal(x[0][0], y[0][0]) for x, y in zip(batches, list(b))] == [True] * len(batches)


def test_checkpoint_has_the_reference_keys_and_loads(tmp_path):
    fx = TC.load_fixture()
    model = TC.fixture_model(fx)
    opt = RT.parse(['-data', 'x.pt', '-results_dir', str(tmp_path / 'r'), '-dataset', 'syn', '-d_model', '32', '-n_head', '2'])
    opt.model_name = str(tmp_path / 'run')      # (pytest's directory names contain 'test'; the rule under check is save_model's)
    os.makedirs(opt.model_name)
    # utils.save_model's rule, `>=` as written: the current loss is already in the list, so 'best' writes every time
    for epoch_i, (loss, losses) in enumerate([(0.5, [0.5]), (0.7, [0.5, 0.7])]):
        path = RT.save_model(opt, epoch_i, model, loss, losses)
        assert path == opt.model_name + '/model.chkpt'
        ckpt = torch.load(path, map_location='cpu', weights_only=False)
        assert sorted(ckpt) == ['epoch', 'model', 'settings'] and ckpt['epoch'] == epoch_i
    assert isinstance(ckpt['settings'], argparse.Namespace) and ckpt['settings'].d_model == 32
    assert sorted(ckpt['model']) == sorted(fx['sd'])        # the reference model's own state_dict keys
    fresh = TC.fixture_model(fx)
    with torch.no_grad():
        for p in fresh.parameters():
            p.add_(1.0)
    fresh.load_state_dict(ckpt['model'])
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, fx['sd'][k]), k
    from lamp_amd.run_eval import load_checkpoint_state
    assert sorted(load_checkpoint_state(path)) == sorted(fx['sd'])
    opt.save_mode = 'all'
    assert RT.save_model(opt, 2, model, 0.25, [0.5, 0.7, 0.25]).endswith('/accu_25.000.chkpt')


def _stepped_torch_adam(params, steps=3):
    opt = torch.optim.Adam(params, betas=TC.ADAM_BETAS, lr=2e-4)
    g = torch.Generator().manual_seed(0)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


def test_adam_state_round_trips_through_torch_adam():
    params = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]
    theirs = _stepped_torch_adam(params)
    sd = theirs.state_dict()
    ours = O.Adam(params, betas=TC.ADAM_BETAS, lr=1.0)
    ours.load_state_dict(sd)
    back = ours.state_dict()
    assert sorted(back) == sorted(sd) and back['param_groups'][0]['lr'] == 2e-4
    for i, st in sd['state'].items():
        assert sorted(back['state'][i]) == ['exp_avg', 'exp_avg_sq', 'step']
        for k in st:
            assert torch.equal(back['state'][i][k], st[k]), (i, k)
    again = torch.optim.Adam(params, betas=(0.5, 0.5), lr=1.0)
    again.load_state_dict(copy.deepcopy(back))     # (load_state_dict keeps the tensors it is given: no sharing with `theirs`)
    assert again.param_groups[0]['betas'] == TC.ADAM_BETAS
    for p in params:
        for k in ('step', 'exp_avg', 'exp_avg_sq'):
            assert torch.equal(again.state[p][k], theirs.state[p][k])
    # ... and torch's Adam goes on from it exactly as from its own state
    g = torch.Generator().manual_seed(1)
    grads = [torch.randn(p.shape, generator=g) for p in params]
    before = [p.detach().clone() for p in params]
    for p, gr in zip(params, grads):
        p.grad = gr.clone()
    theirs.step()
    want = [p.detach().clone() for p in params]
    with torch.no_grad():
        for p, b in zip(params, before):
            p.copy_(b)
    again.step()
    for p, w in zip(params, want):
        assert torch.equal(p.detach(), w)
    # a fresh lamp Adam has torch's param_group keys, so its state_dict loads into torch's Adam untouched
    assert set(O.Adam(params).state_dict()['param_groups'][0]) == set(torch.optim.Adam(params).state_dict()['param_groups'][0])


def test_steplr_changes_the_lr_the_next_step_sees(monkeypatch):
    seen = []
    monkeypatch.setattr(N, 'optim_step', lambda entries, kind, step, lr, *a: seen.append((kind, step, lr, len(entries))))
    monkeypatch.setattr(O, '_check', lambda p: p.grad)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: None)
    for cls, kw in ((O.Adam, dict(betas=TC.ADAM_BETAS)), (O.SGD, {})):
        del seen[:]
        params = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(3))]
        opt = cls(params, lr=0.5, **kw)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1, last_epoch=-1)   # main.py:100
        for p in params[:2]:
            p.grad = torch.ones_like(p)       # the third parameter has no gradient: skipped, as torch does
        opt.step()
        sched.step()
        opt.step()
        opt.param_groups[0]['lr'] = 0.25
        opt.step()
        assert [s[2] for s in seen] == [0.5, pytest.approx(0.05), 0.25]
        assert [s[3] for s in seen] == [2, 2, 2]
        if cls is O.Adam:
            assert [s[1] for s in seen] == [1, 2, 3]
            assert params[2] not in opt.state and float(opt.state[params[0]]['step']) == 3.0


@pytest.mark.parametrize('B,L,n_mats', TC.BCE_CASES)
def test_loss_yardstick_torch_fp32_against_fp64(B, L, n_mats):
    """The CPU half of the loss kernel's check (tests/test_train_gpu.py): the gap torch's own fp32 result shows against fp64 on
    the kernel test's inputs, measured and printed here; 4 x this gap (floor: one fp32 ulp) is the kernel's tolerance.  The gap
    must be rounding-sized, or the tolerance derived from it would check nothing."""
    logits, weights, targets = TC.bce_case(B, L, n_mats, seed=B * 1000 + L)
    p64, g64, r64 = TC.bce_reference(logits, weights, targets, torch.float64)
    p32, g32, r32 = TC.bce_reference(logits, weights, targets, torch.float32)
    gaps = {'probs': TC.gap(p32, p64), 'row sums': TC.gap(r32, r64), 'dlogits': max(TC.gap(a, b) for a, b in zip(g32, g64))}
    print('torch fp32 vs fp64, %dx%d x%d: %s' % (B, L, n_mats, ', '.join('%s %.3e' % kv for kv in gaps.items())))
    eps = 2.0 ** -23
    assert gaps['probs'] <= 2 * eps                                   # probabilities are <= 1
    assert gaps['row sums'] <= 2 * eps * float(r64.abs().max()) * max(L, 8) ** 0.5 + 1e-30
    assert gaps['dlogits'] <= 4 * eps * max(weights) / (B * L)


@pytest.mark.parametrize('n_steps', [1, 2, 10])
def test_adam_yardstick_torch_fp32_against_fp64(n_steps):
    """Likewise for the optimizer kernel: torch's fp32 Adam(foreach=True) on the CPU against the fp64 formula."""
    params, grads = TC.optim_case(1, n_steps)
    lrs = [2e-3 if i != 1 else 5e-4 for i in range(n_steps)]
    cpu, _ = TC.torch_adam_fp32(params, grads, lrs)
    want = [TC.adam_reference(p, [grads[i][k] for i in range(n_steps)], lrs) for k, p in enumerate(params)]
    gaps = [TC.gap(c.detach(), w[0]) for c, w in zip(cpu, want)]
    print('torch fp32 Adam vs fp64 after %d steps: %s' % (n_steps, ', '.join('%d el. %.3e' % (p.numel(), g) for p, g in zip(params, gaps))))
    # |w| < 8 here: a few ulp of the parameter per step at the most (Adam's step is <= lr in size)
    assert max(gaps) <= n_steps * 4 * 2.0 ** -21
