"""The training layer on the MI355X: lamp_bce_logits_train and lamp_optim_step against fp64 evaluations of their definitions
(tolerance: the larger of one fp32 ulp at the value and 4 x the gap torch's own fp32 CPU result shows against fp64 on the same
inputs -- measured here and printed), train_epoch against the reference's recorded epoch (tests/golden/train_epoch.npz;
tolerance max(1e-4, 3 x the reference's own fp32-vs-fp64 gap)), its determinism / placement / no-host-wait properties,
run_train end to end, and one epoch of the one-hot model."""
import json
import os
import tempfile
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import max_abs_diff

from lamp_amd import _native as N
from lamp_amd import optim as O
from lamp_amd import train as T

import train_common as TC

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


_gap = TC.gap


# ------------------------------------------------------------------ lamp_bce_logits_train
_bce_case = TC.bce_case
BCE_CASES = TC.BCE_CASES


@pytest.mark.parametrize('B,L,n_mats', BCE_CASES)
def test_bce_kernel_against_fp64(B, L, n_mats):
    logits, weights, targets = _bce_case(B, L, n_mats, seed=B * 1000 + L)
    p64, g64, r64 = TC.bce_reference(logits, weights, targets, torch.float64)
    p32, g32, r32 = TC.bce_reference(logits, weights, targets, torch.float32)
    probs, grads, rows = N.bce_logits_train([x.to(DEV) for x in logits], weights, targets.to(DEV))
    torch.cuda.synchronize()
    TC.within(probs, p64, _gap(p32, p64), 'probs %dx%d' % (B, L))
    TC.within(rows, r64, _gap(r32, r64), 'row sums %dx%d x%d' % (B, L, n_mats))
    for k in range(n_mats):
        TC.within(grads[k], g64[k], _gap(g32[k], g64[k]), 'dlogits[%d] %dx%d' % (k, B, L))


def test_bce_rows_do_not_depend_on_their_batch_and_nan_stays_in_its_row():
    B, L = 32, 159
    logits, weights, targets = _bce_case(B, L, 3, seed=5)
    xd, td = [x.to(DEV) for x in logits], targets.to(DEV)
    probs, grads, rows = N.bce_logits_train(xd, weights, td)
    again = N.bce_logits_train(xd, weights, td)
    assert torch.equal(probs, again[0]) and torch.equal(rows, again[2]) and all(torch.equal(a, b) for a, b in zip(grads, again[1]))
    for lo, hi in ((0, 1), (31, 32), (5, 12), (0, 16)):
        # the gradient carries 1 / (B L) of the batch the mean is taken over: the same factor through the weights
        # (B / (hi - lo) is a power of two or the quotient is compared on probabilities and sums only)
        scale = (hi - lo) / float(B)
        p, g, r = N.bce_logits_train([x[lo:hi] for x in xd], [w * scale for w in weights], td[lo:hi])
        assert torch.equal(p, probs[lo:hi]) and torch.equal(r, rows[:, lo:hi]), (lo, hi)
        if (hi - lo) & (hi - lo - 1) == 0:
            assert all(torch.equal(a, b[lo:hi]) for a, b in zip(g, grads)), (lo, hi)
    bad = [x.clone() for x in xd]
    bad[0][3, 7] = float('nan')
    bad[2][9, 0] = float('nan')
    p, g, r = N.bce_logits_train(bad, weights, td)
    torch.cuda.synchronize()
    assert torch.isnan(p[3, 7]) and torch.isnan(r[0, 3]) and torch.isnan(g[0][3, 7]) and torch.isnan(r[2, 9])
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[3] = False
    assert torch.equal(p[keep], probs[keep]) and torch.equal(r[0][keep], rows[0][keep]) and torch.equal(g[0][keep], grads[0][keep])
    assert torch.equal(r[1], rows[1]) and torch.equal(g[1], grads[1])          # another matrix's NaN is not this one's
    assert int(torch.isnan(p).sum()) == 1 and int(torch.isnan(r).sum()) == 2 and int(torch.isnan(g[2]).sum()) == 1


def test_bce_strided_probability_write_stays_inside_its_block():
    B, L = 13, 37
    logits, weights, targets = _bce_case(B, L, 2, seed=9)
    xd, td = [x.to(DEV) for x in logits], targets.to(DEV)
    want = N.bce_logits_train(xd, weights, td)
    guard = 12345.0
    big = torch.full((B + 9, L + 3), guard, device=DEV)
    loss = torch.full((2, B + 11), guard, device=DEV)
    N.bce_logits_train(xd, weights, td, probs_out=big[4:4 + B, :L], row_loss_out=loss[:, 6:6 + B])
    torch.cuda.synchronize()
    assert torch.equal(big[4:4 + B, :L], want[0]) and torch.equal(loss[:, 6:6 + B], want[2])
    big[4:4 + B, :L] = guard
    loss[:, 6:6 + B] = guard
    assert bool((big == guard).all()) and bool((loss == guard).all())
    with pytest.raises(ValueError):
        N.bce_logits_train(xd, weights, td, probs_out=big[4:4 + B, 1:L + 1].t().contiguous().t())
    with pytest.raises(ValueError):
        N.bce_logits_train(xd * 5, weights * 5, td)      # 10 matrices: the entry point takes 8


# ------------------------------------------------------------------ lamp_optim_step
_optim_case = TC.optim_case


def _device_params(params):
    """fp32 device copies; the last one sits one float past a 16-byte boundary (4-byte aligned only)."""
    out = [torch.nn.Parameter(p.to(DEV)) for p in params[:-1]]
    base = torch.empty(params[-1].numel() + 1, device=DEV)
    base[1:] = params[-1].to(DEV)
    odd = torch.nn.Parameter(base[1:])
    assert odd.data_ptr() % 16 == 4 and odd.is_contiguous()
    return out + [odd]


def _misaligned(t):
    base = torch.empty(t.numel() + 1, device=DEV)
    base[1:] = t.to(DEV).reshape(-1)
    return base[1:].view(t.shape)


@pytest.mark.parametrize('n_steps', [1, 2, 10])
def test_adam_kernel_against_fp64(n_steps):
    params, grads = _optim_case(1, n_steps)
    lrs = [2e-3 if i != 1 else 5e-4 for i in range(n_steps)]        # lr changed between steps is honoured
    # torch's own fp32 Adam (foreach) on the CPU against the fp64 formula, on the same fp32 inputs: the yardstick
    cpu = [torch.nn.Parameter(p.clone()) for p in params]
    ref = torch.optim.Adam(cpu, betas=TC.ADAM_BETAS, lr=lrs[0], foreach=True)
    for i in range(n_steps):
        ref.param_groups[0]['lr'] = lrs[i]
        for p, gr in zip(cpu, grads[i]):
            p.grad = gr.clone()
        ref.step()
    want = [TC.adam_reference(p, [grads[i][k] for i in range(n_steps)], lrs) for k, p in enumerate(params)]
    gaps = [_gap(c.detach(), w[0]) for c, w in zip(cpu, want)]

    def run():
        dev = _device_params(params)
        untouched = torch.nn.Parameter(torch.randn(300, device=DEV))
        before = untouched.detach().clone()
        opt = O.Adam(dev + [untouched], betas=TC.ADAM_BETAS, lr=lrs[0])
        for i in range(n_steps):
            opt.param_groups[0]['lr'] = lrs[i]
            for k, (p, gr) in enumerate(zip(dev, grads[i])):
                p.grad = _misaligned(gr) if k == len(dev) - 1 else gr.to(DEV)
            opt.step()
        torch.cuda.synchronize()
        assert torch.equal(untouched.detach(), before) and untouched not in opt.state     # no grad: skipped
        assert float(opt.state[dev[0]]['step']) == n_steps
        return dev, opt

    dev, opt = run()
    for k, (p, w) in enumerate(zip(dev, want)):
        TC.within(p.detach(), w[0], gaps[k], 'Adam param, %d elements, %d steps' % (p.numel(), n_steps))
        TC.within(opt.state[p]['exp_avg'], w[1], _gap(ref.state[cpu[k]]['exp_avg'], w[1]), 'exp_avg %d' % p.numel())
        TC.within(opt.state[p]['exp_avg_sq'], w[2], _gap(ref.state[cpu[k]]['exp_avg_sq'], w[2]), 'exp_avg_sq %d' % p.numel())
    dev2, opt2 = run()
    for a, b in zip(dev, dev2):
        assert torch.equal(a.detach(), b.detach())          # bit-identical from run to run
        assert torch.equal(opt.state[a]['exp_avg_sq'], opt2.state[b]['exp_avg_sq'])
    # the state moves to torch.optim.Adam on the device and back
    there = torch.optim.Adam(opt.param_groups[0]['params'], betas=TC.ADAM_BETAS, lr=1.0)
    there.load_state_dict(opt.state_dict())
    assert all(torch.equal(there.state[p]['exp_avg'], opt.state[p]['exp_avg']) for p in dev)


@pytest.mark.parametrize('n_steps', [1, 2, 10])
def test_sgd_kernel_against_fp64(n_steps):
    params, grads = _optim_case(2, n_steps)
    lrs = [0.05 if i != 1 else 0.2 for i in range(n_steps)]
    cpu = [p.clone() for p in params]
    want = [p.double().clone() for p in params]
    for i in range(n_steps):
        for k in range(len(params)):
            cpu[k] = cpu[k] - lrs[i] * grads[i][k]           # torch.optim.SGD's update: param.add_(grad, alpha=-lr)
            want[k] = want[k] - lrs[i] * grads[i][k].double()
    dev = _device_params(params)
    opt = O.SGD(dev, lr=lrs[0])
    for i in range(n_steps):
        opt.param_groups[0]['lr'] = lrs[i]
        for k, (p, gr) in enumerate(zip(dev, grads[i])):
            p.grad = _misaligned(gr) if k == len(dev) - 1 else gr.to(DEV)
        opt.step()
    torch.cuda.synchronize()
    for k, p in enumerate(dev):
        TC.within(p.detach(), want[k], _gap(cpu[k], want[k]), 'SGD param, %d elements, %d steps' % (p.numel(), n_steps))


def test_optim_table_longer_than_one_launch():
    """More entries than one launch's argument table holds (72), zero-sized tensors among them."""
    g = torch.Generator().manual_seed(4)
    sizes = [(i * 37) % 300 for i in range(200)]
    params = [torch.randn(n, generator=g) for n in sizes]
    grads = [torch.randn(n, generator=g) for n in sizes]
    dev = [torch.nn.Parameter(p.to(DEV)) for p in params]
    for p, gr in zip(dev, grads):
        p.grad = gr.to(DEV)
    O.SGD(dev, lr=0.5).step()
    torch.cuda.synchronize()
    for p, w, gr in zip(dev, params, grads):
        assert torch.equal(p.detach().cpu(), w - 0.5 * gr)


# ------------------------------------------------------------------ lamp_embed_bwd_ordered
@pytest.mark.parametrize('n_tok,d,V', [(300, 32, 17), (9664, 512, 2000), (70, 1100, 5), (1, 8, 3)])
def test_ordered_embedding_gradient(n_tok, d, V):
    """One writer per row, repeated tokens in position order: against an fp64 index_add (tolerance: the kernel rule, with torch's
    own fp32 CPU index_add as the yardstick), bit-identical from run to run, the PAD row untouched, and the atomic entry point
    it stands beside agrees within the same bound."""
    g = torch.Generator().manual_seed(n_tok)
    seq = torch.randint(0, V, (n_tok,), generator=g)
    seq[::5] = 2                                   # one token that repeats a lot
    dout = torch.randn(n_tok, d, generator=g)
    keep = seq != 0
    want = torch.zeros(V, d, dtype=torch.float64).index_add_(0, seq[keep], dout[keep].double())
    cpu32 = torch.zeros(V, d).index_add_(0, seq[keep], dout[keep])
    gap = _gap(cpu32, want)
    sd, dd = seq.to(DEV), dout.to(DEV)
    a = N.embed_bwd(sd, dd, V, pad_idx=0, ordered=True)
    b = N.embed_bwd(sd, dd, V, pad_idx=0, ordered=True)
    c = N.embed_bwd(sd, dd, V, pad_idx=0)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not a[0].any()
    TC.within(a, want, gap, 'ordered embedding gradient %d x %d' % (n_tok, d))
    TC.within(c, want, gap, 'atomic embedding gradient %d x %d' % (n_tok, d))


# ------------------------------------------------------------------ train_epoch
def _fixture_epoch(fx, prefetch=8, streams=1, int_preds=False, optimizer='lamp', device_results=None, seed=0):
    torch.manual_seed(seed)
    model = TC.fixture_model(fx, int_preds=int_preds).to(DEV)
    data = T.TrainBatcher(fx['src'], fx['tgt'], int(fx['batch_size']), shuffle=False, drop_last=False)
    params = list(model.get_trainable_parameters())
    opt = (O.Adam if optimizer == 'lamp' else torch.optim.Adam)(params, betas=TC.ADAM_BETAS, lr=float(fx['lr']))
    dres = {} if device_results is None else device_results
    out = T.train_epoch(model, data, opt, TC.train_opt(int(fx['tgt_vocab_size']), int_preds=int_preds), device=DEV,
                        prefetch=prefetch, streams=streams, device_results=dres)
    torch.cuda.synchronize()
    return model, out, dres


def _batch_means(dres, n_labels, k=0):
    rows = dres['row_loss'][k].cpu().double()
    return torch.stack([rows[lo:lo + real].sum() / (real * n_labels) for lo, real in dres['batches']])


def test_train_epoch_against_the_reference_fixture():
    fx = TC.load_fixture()
    L = int(fx['tgt_vocab_size'])
    model, (preds, targets, bce_total), dres = _fixture_epoch(fx)
    assert [real for _, real in dres['batches']] == [8, 8, 4]             # the short last batch, trained on as it is
    assert torch.equal(targets, torch.from_numpy(fx['all_targets']))      # exact
    bce = _batch_means(dres, L)
    d_bce = float((bce - torch.from_numpy(fx['bce64'])).abs().max())
    d_probs = max_abs_diff(preds, torch.from_numpy(fx['probs64']))
    sd = model.state_dict()
    d_w = max(max_abs_diff(sd[k], v) for k, v in fx['final64'].items())
    moved = max(max_abs_diff(sd[k], fx['sd'][k]) for k in fx['final64'])
    print('per-batch BCE |diff| %.3e (tol %.1e), predictions %.3e (tol %.1e), final weights %.3e (tol %.1e); weights moved %.3e'
          % (d_bce, TC.fixture_tolerance(fx, 'bce'), d_probs, TC.fixture_tolerance(fx, 'probs'), d_w,
             TC.fixture_tolerance(fx, 'weights'), moved))
    assert d_bce <= TC.fixture_tolerance(fx, 'bce')
    assert d_probs <= TC.fixture_tolerance(fx, 'probs')
    assert d_w <= TC.fixture_tolerance(fx, 'weights')
    assert moved > 3 * TC.fixture_tolerance(fx, 'weights')                # the epoch did train
    assert abs(bce_total - float(fx['bce_total64'])) <= 3 * TC.fixture_tolerance(fx, 'bce')
    assert max_abs_diff(preds, dres['probs']) == 0.0 and max_abs_diff(targets, dres['targets']) == 0.0


def test_train_epoch_is_deterministic_in_every_mode_and_rows_land_in_place():
    fx = TC.load_fixture()
    base_model, base, dres = _fixture_epoch(fx)
    for kw in (dict(), dict(prefetch=1), dict(streams=2), dict(prefetch=1, streams=2), dict(prefetch=2)):
        model, out, _ = _fixture_epoch(fx, **kw)
        assert torch.equal(out[0], base[0]) and torch.equal(out[1], base[1]) and out[2] == base[2], kw
        for (k, a), b in zip(model.state_dict().items(), base_model.state_dict().values()):
            assert torch.equal(a, b), (kw, k)
    # row i of the result is instance i of the order the batcher ran, the 4 rows of the short batch included: batch 0's rows are
    # what the first forward of a fresh model gives for those instances
    model = TC.fixture_model(fx).to(DEV).train()
    data = T.TrainBatcher(fx['src'], fx['tgt'], int(fx['batch_size']), shuffle=False, drop_last=False)
    (seq, pos), _, _ = data.batch(0)
    first = torch.sigmoid(model((seq.to(DEV), pos.to(DEV)), None, None, None)[0]).detach().cpu()
    assert max_abs_diff(base[0][:8], first) < 1e-6
    assert bool((base[0][16:20] > 0).all()) and base[0].shape == (20, int(fx['tgt_vocab_size']))
    # with the reference's drop_last the rows of the batch left out stay zero, predictions and targets alike
    torch.manual_seed(0)
    model = TC.fixture_model(fx).to(DEV)
    dropped = T.TrainBatcher(fx['src'], fx['tgt'], 8, shuffle=False, drop_last=True)
    opt = O.Adam(model.get_trainable_parameters(), betas=TC.ADAM_BETAS, lr=float(fx['lr']))
    preds, targets, _ = T.train_epoch(model, dropped, opt, TC.train_opt(int(fx['tgt_vocab_size'])), device=DEV)
    assert torch.equal(preds[:16], base[0][:16]) and not preds[16:].any() and not targets[16:].any()


def test_train_epoch_with_int_preds_agrees_with_the_pieces_it_replaces():
    """The same epoch composed of F.binary_cross_entropy_with_logits, loss.backward() and torch.optim.Adam (train.py:36-48)."""
    fx = TC.load_fixture()
    L = int(fx['tgt_vocab_size'])
    model, (preds, _, bce_total), dres = _fixture_epoch(fx, int_preds=True)
    assert dres['row_loss'].shape[0] == 4           # the final prediction + 3 intermediates of a 2-layer decoder
    torch.manual_seed(0)
    ref = TC.fixture_model(fx, int_preds=True).to(DEV).train()
    data = T.TrainBatcher(fx['src'], fx['tgt'], int(fx['batch_size']), shuffle=False, drop_last=False)
    opt = torch.optim.Adam(ref.get_trainable_parameters(), betas=TC.ADAM_BETAS, lr=float(fx['lr']))
    from lamp_amd.data import get_gold_binary
    bces, probs = [], []
    for (seq, pos), adj, tgt in data:
        gold = get_gold_binary(tgt[:, 1:], L).to(DEV)
        opt.zero_grad()
        pred, _, ints = ref((seq.to(DEV), pos.to(DEV)), adj, None, gold, int_preds=True)
        loss = F.binary_cross_entropy_with_logits(pred, gold, reduction='mean')
        bces.append(loss.item())
        for ip in ints:
            loss = loss + 0.2 * F.binary_cross_entropy_with_logits(ip, gold, reduction='mean')
        loss.backward()
        opt.step()
        probs.append(torch.sigmoid(pred).detach().cpu())
    d_bce = float((_batch_means(dres, L) - torch.tensor(bces, dtype=torch.float64)).abs().max())
    d_probs = max_abs_diff(preds, torch.cat(probs))
    d_w = max(max_abs_diff(a, b) for a, b in zip(model.state_dict().values(), ref.state_dict().values()))
    print('int_preds: BCE |diff| %.3e, predictions %.3e, final weights %.3e' % (d_bce, d_probs, d_w))
    assert d_bce <= TC.fixture_tolerance(fx, 'bce') and d_probs <= TC.fixture_tolerance(fx, 'probs')
    assert d_w <= TC.fixture_tolerance(fx, 'weights')
    plain = _fixture_epoch(fx)[0]
    assert max(max_abs_diff(a, b) for a, b in zip(model.state_dict().values(), plain.state_dict().values())) > 1e-5


def test_train_epoch_never_waits_for_the_device_inside_the_loop(monkeypatch):
    fx = TC.load_fixture()
    _fixture_epoch(fx)                      # warm: allocations, the pinned ring
    me = threading.get_ident()
    state = {'inside': False, 'batches': 0, 'waits': []}
    body = T.issue_stage        # the issuing thread's whole share of a stage: uploads, events, target copies, the loop body

    def wrapped(*a, **k):
        state['inside'] = True
        try:
            return body(*a, **k)
        finally:
            state['inside'] = False
            state['batches'] += len(a[3].items)

    def counting(owner, name, cuda_self):
        real = getattr(owner, name)

        def f(*a, **k):
            if state['inside'] and ((a and a[0].is_cuda) if cuda_self else threading.get_ident() == me):
                state['waits'].append(name)
            return real(*a, **k)
        monkeypatch.setattr(owner, name, f)

    monkeypatch.setattr(T, 'issue_stage', wrapped)
    counting(torch.cuda, 'synchronize', False)
    counting(torch.cuda.Stream, 'synchronize', False)
    counting(torch.cuda.Event, 'synchronize', False)
    for name in ('item', 'cpu', 'tolist', 'numpy', '__bool__', '__float__', '__int__'):
        counting(torch.Tensor, name, True)
    _fixture_epoch(fx)
    assert state['batches'] == 3 and state['waits'] == [], state


# ------------------------------------------------------------------ run_train end to end
def test_run_train_end_to_end_and_run_eval_reads_its_checkpoint():
    with tempfile.TemporaryDirectory(prefix='lamp_run_') as root:   # (save_model writes nothing under a path that contains 'test': runner.py:85)
        assert 'test' not in root
        _run_train_end_to_end(root)


def _run_train_end_to_end(root):
    from lamp_amd import run_eval, run_train
    data_path = os.path.join(root, 'train_valid_data.pt')
    torch.save(TC.synthetic_dataset(n_train=208), data_path)
    model_args = ['-data', data_path, '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2',
                  '-label_mask', 'prior', '-batch_size', '16']
    hist = run_train.main(model_args + ['-epoch', '2', '-lr', '0.003', '-dropout', '0.0', '-results_dir', os.path.join(root, 'res'),
                                        '-name', 'e2e', '-seed', '1', '-optim_impl', 'lamp'])
    assert len(hist) == 2 and hist[1]['train_loss'] < hist[0]['train_loss']
    print('run_train: train loss %.6f -> %.6f, test loss %.6f -> %.6f' % (hist[0]['train_loss'], hist[1]['train_loss'],
                                                                         hist[0]['test_loss'], hist[1]['test_loss']))
    run_dir = os.path.dirname(hist[1]['checkpoint'])
    rows = [l.split(',') for l in open(os.path.join(run_dir, 'losses.csv')).read().split()]
    assert [r[0] for r in rows] == ['1', '2'] and all(len(r) == 4 for r in rows)
    assert float(rows[1][1]) == hist[1]['train_loss'] and float(rows[1][3]) == hist[1]['test_loss']
    assert hist[1]['checkpoint'].endswith('/model.chkpt') and os.path.exists(hist[1]['checkpoint'])
    ckpt = torch.load(hist[1]['checkpoint'], map_location='cpu', weights_only=False)
    assert sorted(ckpt) == ['epoch', 'model', 'settings'] and ckpt['epoch'] == 1
    assert set(hist[1]['metrics']) == {'train', 'valid', 'test'} and 'meanAUC' in hist[1]['metrics']['test']
    json.dumps(hist)
    out = run_eval.main(model_args + ['-checkpoint', hist[1]['checkpoint'], '-split', 'test'])
    assert out['bce_total'] / out['n_samples'] == hist[1]['test_loss']            # exactly the last epoch's test loss
    # -load_pretrained goes on from that checkpoint; torch's optimizers are one flag away
    more = run_train.main(model_args + ['-epoch', '1', '-lr', '0.003', '-dropout', '0.0', '-results_dir', os.path.join(root, 'res'),
                                        '-name', 'e2e', '-seed', '1', '-load_pretrained', '-optim_impl', 'torch'])
    assert run_train.parse(model_args).optim_impl in ('lamp', 'torch')
    assert more[0]['train_loss'] < hist[0]['train_loss']


def test_run_train_with_a_general_head_geometry_and_run_eval_reads_it_from_the_checkpoint():
    """run_train -n_head 2 -n_head2 4 -d_k 8 -d_v 24 at d_model 32 (n_head * d_k = 16, n_head * d_v = 48, the label
    self-attention 32 / 96 wide), one epoch; run_eval is given none of the three flags: it takes them from the checkpoint's
    settings, and its metrics are those of the in-process evaluation."""
    from lamp_amd import run_eval, run_train
    with tempfile.TemporaryDirectory(prefix='lamp_run_') as root:
        assert 'test' not in root
        data_path = os.path.join(root, 'train_valid_data.pt')
        torch.save(TC.synthetic_dataset(n_train=64, n_valid=16, n_test=16), data_path)
        args = ['-data', data_path, '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2', '-label_mask',
                'prior', '-batch_size', '16']
        hist = run_train.main(args + ['-epoch', '1', '-lr', '0.003', '-dropout', '0.0', '-results_dir', os.path.join(root, 'res'),
                                      '-name', 'geo', '-seed', '1', '-n_head2', '4', '-d_k', '8', '-d_v', '24'])
        assert len(hist) == 1 and np.isfinite(hist[0]['train_loss']) and np.isfinite(hist[0]['test_loss'])
        ckpt = torch.load(hist[0]['checkpoint'], map_location='cpu', weights_only=False)
        st = ckpt['settings']
        assert (st.n_head, st.n_head2, st.d_k, st.d_v) == (2, 4, 8, 24)
        sd = ckpt['model']
        assert sd['decoder.layer_stack.0.enc_attn.w_qs.weight'].shape == (16, 32)
        assert sd['decoder.layer_stack.0.enc_attn.w_vs.weight'].shape == (48, 32)
        assert sd['decoder.layer_stack.1.slf_attn.w_ks.weight'].shape == (32, 32)
        assert sd['decoder.layer_stack.1.slf_attn.fc.weight'].shape == (32, 96)
        out = run_eval.main(args + ['-checkpoint', hist[0]['checkpoint'], '-split', 'test'])
        assert out['bce_total'] / out['n_samples'] == hist[0]['test_loss']        # exactly the epoch's own test loss
        mine = hist[0]['metrics']['test']
        for key, name in (('ACC', 'subset_accuracy'), ('HA', 'hamming_accuracy'), ('ebF1', 'example_f1'), ('miF1', 'micro_f1'),
                          ('maF1', 'macro_f1')):
            assert (np.isnan(out[name]) and np.isnan(mine[key])) or abs(out[name] - mine[key]) < 1e-12, (key, out[name], mine[key])
        # a bare state dict carries no settings: the flags say it
        bare = os.path.join(root, 'bare.pt')
        torch.save(sd, bare)
        out2 = run_eval.main(args + ['-checkpoint', bare, '-split', 'test', '-n_head2', '4', '-d_k', '8', '-d_v', '24'])
        assert out2['bce_total'] == out['bce_total']


# ------------------------------------------------------------------ the one-hot model
class _Batches(object):
    def __init__(self, batches, n, batch_size):
        self._batches, self.n_insts, self._batch_size = batches, n, batch_size

    def __len__(self):
        return len(self._batches)

    def __iter__(self):
        return iter(self._batches)


def test_one_epoch_of_the_onehot_model_trains():
    import onehot_common as OC
    L, T_len, B = 23, 64, 8
    torch.manual_seed(0)
    model = OC.build_model(L=L, T_max=T_len, dropout=0.0).to(DEV)
    g = torch.Generator().manual_seed(2)
    batches = []
    for b, rows in enumerate((B, B, 5)):
        seq, pos = OC.make_dna(rows, T_len, lengths=[T_len - 4 * ((b + i) % 5) for i in range(rows)], seed=b)
        labels = (seq[:, :L] % 3 == 0)          # learnable: a label is on iff its base is a multiple of 3
        tgt = torch.zeros(rows, L + 2, dtype=torch.int64)
        for r in range(rows):
            ids = [2] + [4 + int(l) for l in labels[r].nonzero().flatten()] + [3]
            tgt[r, :len(ids)] = torch.tensor(ids)
        batches.append(((seq, pos), None, tgt))
    data = _Batches(batches, 2 * B + 5, B)
    opt = O.Adam(model.get_trainable_parameters(), betas=TC.ADAM_BETAS, lr=2e-3)
    losses = []
    for _ in range(3):
        preds, targets, bce_total = T.train_epoch(model, data, opt, TC.train_opt(L), device=DEV)
        assert torch.isfinite(preds).all() and np.isfinite(bce_total)
        losses.append(bce_total)
    print('one-hot epochs: %s' % losses)
    assert losses[1] < losses[0] and losses[2] < losses[1]
