"""The imbalanced-label losses on the MI355X (lamp_multilabel_loss_train): the kernel against the fp64
reference of tests/imbalance_loss_common.py under the rule of tests/test_train_gpu.py (per element and per row sum: the larger
of one fp32 ulp at the value and 4 x the gap torch's own fp32 CPU evaluation of the same formula shows against fp64 on the
same inputs), its defaults against lamp_bce_logits_train bit for bit, rows and placement, one train_batch through the model
against autograd on the fp64 oracle, train_epoch, and run_train / run_eval end to end."""
import ctypes
import functools
import json
import os
import tempfile
import threading

import numpy as np
import pytest
import torch

from conftest import max_abs_diff

from lamp_amd import _native as N
from lamp_amd import optim as O
from lamp_amd import train as T

import imbalance_loss_common as IC
import train_common as TC

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _kw(name, pos_weight):
    gp, gn, m, has_w = IC.PARAM_SETS[name]
    return dict(gamma_pos=gp, gamma_neg=gn, clip=m, pos_weight=pos_weight.to(DEV).contiguous() if has_w else None)


@functools.lru_cache(maxsize=None)
def _case(name, B, L, n_mats):
    """The inputs of one kernel case with their fp64 reference and fp32 yardstick, computed once and left unchanged."""
    gp, gn, m, has_w = IC.PARAM_SETS[name]
    logits, weights, targets, pw = IC.loss_case(B, L, n_mats, seed=B * 1000 + L, clip=m)
    w = pw if has_w else None
    ref64 = IC.loss_reference(logits, weights, targets, gp, gn, m, w, torch.float64)
    ref32 = IC.loss_reference(logits, weights, targets, gp, gn, m, w, torch.float32)
    return logits, weights, targets, pw, ref64, ref32


# ------------------------------------------------------------------ 1. the kernel against fp64
@pytest.mark.parametrize('B,L,n_mats', IC.SHAPES)
@pytest.mark.parametrize('name', sorted(IC.PARAM_SETS))
def test_loss_kernel_against_fp64(name, B, L, n_mats):
    logits, weights, targets, pw, (p64, g64, r64), (p32, g32, r32) = _case(name, B, L, n_mats)
    probs, grads, rows = N.multilabel_loss_train([x.to(DEV) for x in logits], weights, targets.to(DEV), **_kw(name, pw))
    torch.cuda.synchronize()
    for a in [probs, rows] + grads:                       # finite inputs, +-1e4 among them: no NaN, no inf anywhere
        assert bool(torch.isfinite(a).all()), name
    what = '%s %dx%d x%d' % (name, B, L, n_mats)
    used = [TC.within(probs, p64, TC.gap(p32, p64), 'probs ' + what),
            TC.within(rows, r64, TC.gap(r32, r64), 'row sums ' + what)]
    for k in range(n_mats):
        used.append(TC.within(grads[k], g64[k], TC.gap(g32[k], g64[k]), 'dlogits[%d] %s' % (k, what)))
    print('%s: worst used fraction of the bar %.3f' % (what, max(used)))


# ------------------------------------------------------------------ 2. defaults
def _raw(xs, weights, t, opts, want_probs=True):
    """lamp_multilabel_loss_train through ctypes with `opts` as given (None = a NULL pointer) -> (status, probs, grads, rows)."""
    n, (B, L) = len(xs), xs[0].shape
    probs = torch.full((B, L), -7.0, device=DEV) if want_probs else None
    grads = [torch.full((B, L), -7.0, device=DEV) for _ in xs]
    rows = torch.full((n, B), -7.0, device=DEV)
    xp = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
    gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
    wp = (ctypes.c_float * n)(*weights)
    st = N.lib().lamp_multilabel_loss_train(xp, wp, gp, n, t.data_ptr(), B, L, N.ptr(probs), L, rows.data_ptr(), B,
                                            None if opts is None else ctypes.byref(opts), N.stream())
    torch.cuda.synchronize()
    return st, probs, grads, rows


def _same(a, b):
    return torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and torch.equal(a[2], b[2])


def test_defaults_are_bce_bit_for_bit_and_probabilities_always_are():
    B, L, n_mats = 7, 130, 3
    logits, weights, targets, pw = IC.loss_case(B, L, n_mats, seed=11)
    xd, td = [x.to(DEV) for x in logits], targets.to(DEV)
    bce = N.bce_logits_train(xd, weights, td)
    assert _same(N.multilabel_loss_train(xd, weights, td), bce)                       # all-zero options
    st, *null = _raw(xd, weights, td, None)                                           # opts == NULL
    assert st == 0 and _same(null, bce)
    st, *zero = _raw(xd, weights, td, N.LossOptions(0.0, 0.0, 0.0, 0, None))
    assert st == 0 and _same(zero, bce)
    for name in sorted(IC.PARAM_SETS):
        p, g, r = N.multilabel_loss_train(xd, weights, td, **_kw(name, pw))
        assert torch.equal(p, bce[0]), name                                           # sigmoid(logits[0]): BCE's bits
        assert not torch.equal(r, bce[2]) and not torch.equal(g[0], bce[1][0]), name  # ... and another objective
    # unit weights are BCE up to rounding, through the other kernel
    p, g, r = N.multilabel_loss_train(xd, weights, td, pos_weight=torch.ones(L, device=DEV))
    assert torch.equal(p, bce[0]) and max_abs_diff(r, bce[2]) <= 8 * 2.0 ** -23 * float(bce[2].abs().max())


def test_refusals_come_before_any_launch_in_the_house_order():
    B, L = 3, 20
    logits, weights, targets, _ = IC.loss_case(B, L, 1, seed=2)
    xd, td = [logits[0].to(DEV)], targets.to(DEV)
    E_DIMS, E_UNSUPPORTED, E_NULL = -1, -4, -5

    def untouched(out):
        return all(bool((a == -7.0).all()) for a in [out[0], out[2]] + out[1])

    for opts in (N.LossOptions(0.5, 0, 0, 0, None), N.LossOptions(0, -1.0, 0, 0, None), N.LossOptions(17.0, 0, 0, 0, None),
                 N.LossOptions(2.0, float('nan'), 0, 0, None), N.LossOptions(0, float('inf'), 0, 0, None),
                 N.LossOptions(0, 0, 1.0, 0, None), N.LossOptions(0, 0, -0.1, 0, None), N.LossOptions(0, 0, float('nan'), 0, None),
                 N.LossOptions(2.0, 2.0, 0, 1, None)):
        st, *out = _raw(xd, weights, td, opts)
        assert st == E_UNSUPPORTED and untouched(out), (opts.gamma_pos, opts.gamma_neg, opts.clip, opts.reserved)
    bad = N.LossOptions(0.5, 0, 0, 0, None)
    lib, s = N.lib(), N.stream()
    xp, wp = (ctypes.c_void_p * 1)(xd[0].data_ptr()), (ctypes.c_float * 1)(1.0)
    # a bad size before a missing pointer before a parameter that is not served
    assert lib.lamp_multilabel_loss_train(xp, wp, None, 1, None, 0, L, None, L, None, B, ctypes.byref(bad), s) == E_DIMS
    assert lib.lamp_multilabel_loss_train(xp, wp, None, 1, None, B, L, None, L, None, B, ctypes.byref(bad), s) == E_NULL
    assert lib.lamp_multilabel_loss_train(xp, wp, None, 1, td.data_ptr(), B, L, None, L, None, B, ctypes.byref(bad), s) == E_UNSUPPORTED
    nine = [xd[0]] * 9
    st, *out = _raw(nine, [1.0] * 9, td, N.LossOptions(2.0, 2.0, 0, 0, None))
    assert st == E_UNSUPPORTED and untouched(out)                                     # 9 matrices: the entry point takes 8
    with pytest.raises(ValueError):
        N.multilabel_loss_train(nine, [1.0] * 9, td, gamma_pos=2.0, gamma_neg=2.0)
    with pytest.raises(ValueError):
        N.multilabel_loss_train(xd, weights, td, pos_weight=torch.ones(L))            # not on the logits' device


# ------------------------------------------------------------------ 3. rows and placement
@pytest.mark.parametrize('name', ['asl_pos_weight', 'focal_2', 'pos_weight', 'margin_only'])
def test_rows_do_not_depend_on_their_batch_and_nan_stays_in_its_row(name):
    B, L = 32, 159
    logits, weights, targets, pw = IC.loss_case(B, L, 3, seed=5, clip=IC.PARAM_SETS[name][2])
    xd, td, kw = [x.to(DEV) for x in logits], targets.to(DEV), _kw(name, pw)
    probs, grads, rows = N.multilabel_loss_train(xd, weights, td, **kw)
    assert _same(N.multilabel_loss_train(xd, weights, td, **kw), (probs, grads, rows))
    for lo, hi in ((0, 1), (31, 32), (5, 12), (0, 16)):
        # the gradient carries 1 / (B L) of the batch the mean is taken over: the same factor through the weights (exact
        # where B / (hi - lo) is a power of two; otherwise probabilities and sums only)
        scale = (hi - lo) / float(B)
        p, g, r = N.multilabel_loss_train([x[lo:hi] for x in xd], [w * scale for w in weights], td[lo:hi], **kw)
        assert torch.equal(p, probs[lo:hi]) and torch.equal(r, rows[:, lo:hi]), (lo, hi)
        if (hi - lo) & (hi - lo - 1) == 0:
            assert all(torch.equal(a, b[lo:hi]) for a, b in zip(g, grads)), (lo, hi)
    bad = [x.clone() for x in xd]
    bad[0][3, 7] = float('nan')
    bad[2][9, 0] = float('nan')
    p, g, r = N.multilabel_loss_train(bad, weights, td, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(p[3, 7]) and torch.isnan(r[0, 3]) and torch.isnan(g[0][3, 7]) and torch.isnan(r[2, 9]) and torch.isnan(g[2][9, 0])
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[3] = False
    assert torch.equal(p[keep], probs[keep]) and torch.equal(r[0][keep], rows[0][keep]) and torch.equal(g[0][keep], grads[0][keep])
    assert torch.equal(r[1], rows[1]) and torch.equal(g[1], grads[1])
    assert int(torch.isnan(p).sum()) == 1 and int(torch.isnan(r).sum()) == 2
    assert int(torch.isnan(g[0]).sum()) == 1 and int(torch.isnan(g[2]).sum()) == 1   # its own element, not its row's gradients


def test_strided_outputs_stay_inside_their_block():
    B, L = 13, 37
    logits, weights, targets, pw = IC.loss_case(B, L, 2, seed=9, clip=IC.PARAM_SETS['asl_pos_weight'][2])
    xd, td, kw = [x.to(DEV) for x in logits], targets.to(DEV), _kw('asl_pos_weight', pw)
    want = N.multilabel_loss_train(xd, weights, td, **kw)
    guard = 12345.0
    big = torch.full((B + 9, L + 3), guard, device=DEV)
    loss = torch.full((2, B + 11), guard, device=DEV)
    N.multilabel_loss_train(xd, weights, td, probs_out=big[4:4 + B, :L], row_loss_out=loss[:, 6:6 + B], **kw)
    torch.cuda.synchronize()
    assert torch.equal(big[4:4 + B, :L], want[0]) and torch.equal(loss[:, 6:6 + B], want[2])
    big[4:4 + B, :L] = guard
    loss[:, 6:6 + B] = guard
    assert bool((big == guard).all()) and bool((loss == guard).all())
    with pytest.raises(ValueError):
        N.multilabel_loss_train(xd, weights, td, probs_out=big[4:4 + B, 1:L + 1].t().contiguous().t(), **kw)
    p, g, r = N.multilabel_loss_train(xd, weights, td, want_grads=False, want_probs=False, **kw)
    assert p is None and g is None and torch.equal(r, want[2])


# ------------------------------------------------------------------ 4. through the model
def _batch0(fx):
    from lamp_amd.data import get_gold_binary
    data = T.TrainBatcher(fx['src'], fx['tgt'], int(fx['batch_size']), shuffle=False, drop_last=False)
    (seq, pos), _, tgt = data.batch(0)
    return seq, pos, get_gold_binary(tgt[:, 1:], int(fx['tgt_vocab_size']))


def test_train_batch_with_asl_and_pos_weight_against_the_fp64_oracle():
    """One train_batch (asymmetric loss + positive weights, dropout 0) on the tiny training model: every parameter's gradient
    against torch.autograd on the fp64 oracle with the fp64 loss.  Tolerance: the rule of tests/test_train_gpu.py's training
    comparisons, max(1e-4, 3 x the oracle's own fp32-vs-fp64 gap) -- the gap taken here from the oracle run in fp32."""
    from oracle import lamp_ref as R
    fx = TC.load_fixture()
    L, h = int(fx['tgt_vocab_size']), int(fx['n_head'])
    seq, pos, gold = _batch0(fx)
    B = gold.size(0)
    gp, gn, m, _ = IC.PARAM_SETS['asl_pos_weight']
    pw = IC.loss_case(B, L, 1, seed=1)[3]
    blocked = R.label_block_mask(torch.from_numpy(fx['label_adj_matrix']), 'prior', L)

    def oracle(dtype):
        sd = {k: (v.detach().clone().to(dtype).requires_grad_(True) if v.is_floating_point() else v) for k, v in fx['sd'].items()}
        logits = R.forward(sd, seq, pos, h, blocked)[0]
        IC.loss_elements(logits, gold.to(dtype), gp, gn, m, pw.to(dtype)).mean().backward()
        return sd, logits.detach()

    sd64, logits64 = oracle(torch.float64)
    sd32, _ = oracle(torch.float32)
    torch.manual_seed(0)
    model = TC.fixture_model(fx).to(DEV)
    model.train()
    opt = TC.train_opt(L)
    opt.loss_options = T.LossOptions(gp, gn, m, pw.to(DEV))
    probs, rows = torch.zeros(B, L, device=DEV), torch.zeros(1, B, device=DEV)
    sgd = torch.optim.SGD(list(model.get_trainable_parameters()), lr=0.0)            # (a step that moves nothing)
    T.train_batch(model, sgd, opt, (seq.to(DEV), pos.to(DEV)), None, gold.to(DEV), probs, rows)
    torch.cuda.synchronize()
    assert max_abs_diff(probs, torch.sigmoid(logits64)) < 1e-4
    plain = TC.fixture_model(fx).to(DEV)
    plain.train()
    T.train_batch(plain, torch.optim.SGD(list(plain.get_trainable_parameters()), lr=0.0), TC.train_opt(L),
                  (seq.to(DEV), pos.to(DEV)), None, gold.to(DEV), torch.zeros_like(probs), torch.zeros_like(rows))
    bce_grads = dict((k, p.grad) for k, p in plain.named_parameters())
    checked, worst, moved = 0, 0.0, 0.0
    for pname, p in model.named_parameters():
        ref, ref32 = sd64[pname].grad, sd32[pname].grad
        if p.grad is None:
            assert ref is None or pname == 'encoder.position_enc.weight', pname        # frozen table / the reference's dead code
            continue
        if pname == 'decoder.tgt_word_emb.weight' and 'tgt_word_proj.weight' in sd64 and sd64['tgt_word_proj.weight'].grad is not None:
            ref, ref32 = ref + sd64['tgt_word_proj.weight'].grad, ref32 + sd32['tgt_word_proj.weight'].grad
        assert ref is not None, pname
        tol = max(1e-4, 3.0 * TC.gap(ref32, ref))
        err = max_abs_diff(p.grad, ref)
        worst = max(worst, err / tol)
        moved = max(moved, max_abs_diff(p.grad, bce_grads[pname]))
        assert err <= tol, (pname, err, tol, float(ref.abs().max()))
        checked += 1
    print('train_batch asl + pos_weight: %d gradients, worst err / tol %.3f; largest distance from the BCE gradient %.3e'
          % (checked, worst, moved))
    assert checked >= 40 and moved > 1e-3                      # (ten tolerances away from the gradient of plain BCE)


# ------------------------------------------------------------------ 5. the epoch
def _epoch(fx, loss_options='absent', seed=0):
    torch.manual_seed(seed)
    model = TC.fixture_model(fx).to(DEV)
    data = T.TrainBatcher(fx['src'], fx['tgt'], int(fx['batch_size']), shuffle=False, drop_last=False)
    optim = O.Adam(list(model.get_trainable_parameters()), betas=TC.ADAM_BETAS, lr=float(fx['lr']))
    opt = TC.train_opt(int(fx['tgt_vocab_size']))
    if loss_options != 'absent':
        opt.loss_options = loss_options
    dres = {}
    out = T.train_epoch(model, data, optim, opt, device=DEV, device_results=dres)
    torch.cuda.synchronize()
    return model, out, dres


def test_train_epoch_defaults_are_todays_epoch_and_focal_is_another():
    fx = TC.load_fixture()
    L = int(fx['tgt_vocab_size'])
    base_model, base, base_res = _epoch(fx)                       # no loss_options attribute at all: the call of before
    for lo in (None, T.LossOptions()):
        model, out, dres = _epoch(fx, lo)
        assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1]) and out[2] == base[2]
        assert torch.equal(dres['row_loss'], base_res['row_loss'])
        for (k, a), b in zip(model.state_dict().items(), base_model.state_dict().values()):
            assert torch.equal(a, b), k
    focal = T.LossOptions(2.0, 2.0)
    model, out, dres = _epoch(fx, focal)
    assert max(max_abs_diff(a, b) for a, b in zip(model.state_dict().values(), base_model.state_dict().values())) > 1e-5
    # the first batch saw the initial weights: its rows of row_loss are the kernel's output for that batch's logits
    seq, pos, gold = _batch0(fx)
    torch.manual_seed(0)
    fresh = TC.fixture_model(fx).to(DEV).train()
    logits = fresh((seq.to(DEV), pos.to(DEV)), None, None, gold.to(DEV), return_attns=False, int_preds=False)[0].detach()
    _, _, rows = N.multilabel_loss_train([logits], [1.0], gold.to(DEV), gamma_pos=2.0, gamma_neg=2.0)
    n0 = gold.size(0)
    assert dres['batches'][0] == (0, n0) and torch.equal(dres['row_loss'][0, :n0], rows[0])
    assert bool((dres['row_loss'][0, :n0] < base_res['row_loss'][0, :n0]).all())     # (1 - p_t)^2 < 1 on the same logits
    assert max_abs_diff(out[0][:n0], torch.sigmoid(logits)) < 1e-6
    want_total = sum(float(dres['row_loss'][0, lo:lo + real].cpu().double().sum()) / (real * L) for lo, real in dres['batches'])
    assert out[2] == want_total                                   # the third return value is the trained loss


def test_train_epoch_with_loss_options_never_waits_for_the_device(monkeypatch):
    fx = TC.load_fixture()
    L = int(fx['tgt_vocab_size'])
    lo = T.LossOptions(0.0, 4.0, IC.f32(0.05), torch.full((L,), 3.0, device=DEV))
    _epoch(fx, lo)                          # warm: allocations, the pinned ring
    me = threading.get_ident()
    state = {'inside': False, 'batches': 0, 'waits': [], 'launches': 0}
    body, launch = T.issue_stage, N.multilabel_loss_train

    def wrapped(*a, **k):
        state['inside'] = True
        try:
            return body(*a, **k)
        finally:
            state['inside'] = False
            state['batches'] += len(a[3].items)

    def counted_launch(*a, **k):
        state['launches'] += 1
        return launch(*a, **k)

    def counting(owner, name, cuda_self):
        real = getattr(owner, name)

        def f(*a, **k):
            if state['inside'] and ((a and a[0].is_cuda) if cuda_self else threading.get_ident() == me):
                state['waits'].append(name)
            return real(*a, **k)
        monkeypatch.setattr(owner, name, f)

    monkeypatch.setattr(T, 'issue_stage', wrapped)
    monkeypatch.setattr(N, 'multilabel_loss_train', counted_launch)
    counting(torch.cuda, 'synchronize', False)
    counting(torch.cuda.Stream, 'synchronize', False)
    counting(torch.cuda.Event, 'synchronize', False)
    for name in ('item', 'cpu', 'tolist', 'numpy', '__bool__', '__float__', '__int__'):
        counting(torch.Tensor, name, True)
    _epoch(fx, lo)
    assert state['batches'] == 3 and state['launches'] == 3 and state['waits'] == [], state      # one loss launch per batch


# ------------------------------------------------------------------ 6. end to end
def test_run_train_with_asl_and_pos_weight_end_to_end_and_run_eval_reads_its_checkpoint():
    from lamp_amd import run_eval, run_train
    with tempfile.TemporaryDirectory(prefix='lamp_run_') as root:   # (save_model writes nothing under a path that contains 'test')
        assert 'test' not in root
        data_path = os.path.join(root, 'train_valid_data.pt')
        torch.save(TC.synthetic_dataset(n_train=208), data_path)
        model_args = ['-data', data_path, '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2',
                      '-label_mask', 'prior', '-batch_size', '16']
        run_args = ['-epoch', '1', '-lr', '0.003', '-dropout', '0.0', '-results_dir', os.path.join(root, 'res'), '-name', 'e2e',
                    '-seed', '1', '-optim_impl', 'lamp']
        bce = run_train.main(model_args + run_args)
        hist = run_train.main(model_args + run_args + ['-loss_fn', 'asl', '-pos_weight', 'inv'])
        json.dumps(hist)
        assert len(hist) == 1 and np.isfinite(hist[0]['train_loss'])
        run_dir = os.path.dirname(hist[0]['checkpoint'])
        bce_dir = os.path.dirname(bce[0]['checkpoint'])
        assert os.path.basename(bce_dir).endswith('.e2e') and 'lossfn' not in bce_dir and 'posw' not in bce_dir
        assert os.path.basename(run_dir) == os.path.basename(bce_dir)[:-len('.e2e')] + '.lossfn_asl_0.0_4.0_0.05.posw_inv_100.0.e2e'
        ckpt = torch.load(hist[0]['checkpoint'], map_location='cpu', weights_only=False)
        st = ckpt['settings']
        assert sorted(ckpt) == ['epoch', 'model', 'settings']
        assert (st.loss_fn, st.asl_gamma_pos, st.asl_gamma_neg, st.asl_clip, st.pos_weight, st.pos_weight_cap) == \
            ('asl', 0.0, 4.0, 0.05, 'inv', 100.0)
        plain = torch.load(bce[0]['checkpoint'], map_location='cpu', weights_only=False)['settings']
        assert not any(hasattr(plain, k) for k in ('loss_fn', 'asl_clip', 'focal_gamma', 'pos_weight', 'pos_weight_cap', 'loss_options'))
        assert set(vars(st)) - set(vars(plain)) == {'loss_fn', 'asl_gamma_pos', 'asl_gamma_neg', 'asl_clip', 'pos_weight', 'pos_weight_cap'}
        row = open(os.path.join(run_dir, 'losses.csv')).read().split()[0].split(',')
        row_bce = open(os.path.join(bce_dir, 'losses.csv')).read().split()[0].split(',')
        assert float(row[1]) == hist[0]['train_loss'] and float(row[1]) != float(row_bce[1])      # the trained loss
        assert (float(row[2]), float(row[3])) == (hist[0]['valid_loss'], hist[0]['test_loss'])
        print('run_train asl + pos_weight: train %.6f (BCE run %.6f), valid %.6f, test %.6f'
              % (hist[0]['train_loss'], bce[0]['train_loss'], hist[0]['valid_loss'], hist[0]['test_loss']))
        # the logged valid and test losses are plain BCE of that checkpoint's predictions: run_eval (lamp_sigmoid_bce_fwd)
        # gives exactly them, from the checkpoint alone
        for split in ('valid', 'test'):
            out = run_eval.main(model_args + ['-checkpoint', hist[0]['checkpoint'], '-split', split])
            assert out['bce_total'] / out['n_samples'] == hist[0]['%s_loss' % split], split
