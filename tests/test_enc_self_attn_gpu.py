"""The live encoder self-attention (LAMP(enc_self_attn=True)) on the GPU against the oracle composition of
tests/enc_live_common.py: eval parity on every route, bit-identity, per-sample input graphs, training gradients."""
import ctypes as C
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

import enc_live_common as EC
import train_common as TC
from conftest import max_abs_diff
from oracle import lamp_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-4   # the project's fp32 tolerance (README)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _run(m, seq, pos, dev, adj=None, **kw):
    with torch.no_grad():
        return m((seq.to(dev), pos.to(dev)), adj, None, None, **kw)


_REF = {}


def _ref(shape, mask, pos):
    """The oracle's result for a (shape, label mask, position embedding) case: computed once, shared, never modified."""
    key = (shape, mask, pos)
    if key not in _REF:
        _, sd, blocked, seq, spos, h = EC.build(shape, mask, pos)
        with torch.no_grad():
            _REF[key] = EC.live_forward_ref(sd, seq, spos, h, blocked)
    return _REF[key]


# ------------------------------------------------------------------ 1. parity, eval
@pytest.mark.parametrize('pos', [True, False])
@pytest.mark.parametrize('mask', ['prior', 'inveye', 'none'])
@pytest.mark.parametrize('shape', ['A', 'B', 'C'])
def test_eval_parity(dev, shape, mask, pos):
    m, sd, blocked, seq, spos, h = EC.build(shape, mask, pos)
    m = m.to(dev).eval()
    ref_logits, ref_enc = _ref(shape, mask, pos)[:2]
    logits, enc, extra = _run(m, seq, spos, dev)
    assert extra is None
    print('%s %s pos=%s: logits %.3e, enc_output (all rows, PAD included) %.3e' %
          (shape, mask, pos, max_abs_diff(logits, ref_logits), max_abs_diff(enc, ref_enc)))
    assert max_abs_diff(logits, ref_logits) < TOL
    assert max_abs_diff(enc, ref_enc) < TOL     # PAD rows included


@pytest.mark.parametrize('shape', ['A', 'B', 'C'])
def test_eval_parity_with_attention_maps(dev, shape):
    m, sd, blocked, seq, spos, h = EC.build(shape, 'prior', True)
    m = m.to(dev).eval()
    ref_logits, ref_enc, ref_maps, (ref_slf, ref_encdec), _ = _ref(shape, 'prior', True)
    logits, enc, enc_attns, (slf, encdec) = _run(m, seq, spos, dev, return_attns=True)
    assert max_abs_diff(logits, ref_logits) < TOL and max_abs_diff(enc, ref_enc) < TOL
    assert len(enc_attns[0]) == 2
    for got, want in zip(enc_attns[0], ref_maps):       # the maps of the attention that was USED
        assert got.shape == want.shape
        assert max_abs_diff(got, want) < TOL
        assert float((got.sum(-1) - 1).abs().max()) < TOL
    for got, want in zip(slf + encdec, ref_slf + ref_encdec):
        assert max_abs_diff(got, want) < TOL
    # the maps do not change the results
    plain = _run(m, seq, spos, dev)
    assert torch.equal(plain[0], logits) and torch.equal(plain[1], enc)


@pytest.mark.parametrize('shape', ['A', 'B', 'C'])
def test_eval_parity_with_int_preds(dev, shape):
    m, sd, blocked, seq, spos, h = EC.build(shape, 'prior', True, int_preds=True)
    m = m.to(dev).eval()
    ref_logits, ref_enc, _, _, ref_int = _ref(shape, 'prior', True)
    logits, enc, ipreds = _run(m, seq, spos, dev, int_preds=True)
    assert max_abs_diff(logits, ref_logits) < TOL and max_abs_diff(enc, ref_enc) < TOL
    assert len(ipreds) == len(ref_int) == 3
    for got, want in zip(ipreds, ref_int):
        assert max_abs_diff(got, want) < TOL


# ------------------------------------------------------------------ 2. bit-identity
def _repad(seq, spos, T):
    return F.pad(seq, (0, T - seq.size(1))), F.pad(spos, (0, T - spos.size(1)))


@pytest.mark.parametrize('shape', ['A', 'B'])
def test_a_samples_bits_do_not_depend_on_its_batch(dev, shape):
    """A sample alone, inside the batch, after re-padding to T + 37 and with the batch order permuted: the same logits and
    live encoder rows, bit for bit.  "Alone" is the sample trimmed to its own length (and, as well, its padded row as a batch of
    one): on shape B that crosses the 256-query and the 64-key boundaries of the attention kernels."""
    m, sd, blocked, seq, spos, h = EC.build(shape, 'prior', True)
    m = m.to(dev).eval()
    lengths = EC.SHAPES[shape]['lengths']
    T = seq.size(1)
    logits, enc, _ = _run(m, seq, spos, dev)
    perm = list(reversed(range(len(lengths))))
    p_logits, p_enc, _ = _run(m, seq[perm], spos[perm], dev)
    r_seq, r_pos = _repad(seq, spos, T + EC.PAD_EXTRA)
    r_logits, r_enc, _ = _run(m, r_seq, r_pos, dev)
    for b, n in enumerate(lengths):
        a_logits, a_enc, _ = _run(m, seq[b:b + 1], spos[b:b + 1], dev)
        assert torch.equal(a_logits[0], logits[b]) and torch.equal(a_enc[0, :n], enc[b, :n])
        assert torch.equal(p_logits[perm.index(b)], logits[b]) and torch.equal(p_enc[perm.index(b), :n], enc[b, :n])
        assert torch.equal(r_logits[b], logits[b]) and torch.equal(r_enc[b, :n], enc[b, :n])
        t_logits, t_enc, _ = _run(m, seq[b:b + 1, :n], spos[b:b + 1, :n], dev)
        assert torch.equal(t_enc[0], enc[b, :n]), (shape, n)
        assert torch.equal(t_logits[0], logits[b]), (shape, n)


@pytest.mark.parametrize('shape', ['A', 'B', 'C', 'D'])
def test_fused_route_equals_module_route_and_chain_equals_separate_launches(dev, shape):
    m, sd, blocked, seq, spos, h = EC.build(shape, 'prior', True)
    m = m.to(dev).eval()
    src = (seq.to(dev), spos.to(dev))
    with torch.no_grad():
        fused = m(src, None, None, None)
        module = m._forward_composite(src, None, None, False, False)
        # without the weights-only packs the live tail runs as separate launches at these row counts (shape D: with them it
        # is one chain launch)
        m.use_chain_packs = False
        m.invalidate_native_cache()
        separate = m(src, None, None, None)
    print('%s: fused - module: logits %.3e, enc_output %.3e; fused - separate launches: logits %.3e, enc_output %.3e' %
          (shape, max_abs_diff(fused[0], module[0]), max_abs_diff(fused[1], module[1]), max_abs_diff(fused[0], separate[0]),
           max_abs_diff(fused[1], separate[1])))
    assert torch.equal(fused[1], module[1]) and torch.equal(fused[0], module[0])
    assert torch.equal(fused[1], separate[1]) and torch.equal(fused[0], separate[0])


# ------------------------------------------------------------------ 2b. the packed route (behind LAMP.use_packed_live_encoder)
def _packed(m):
    m.use_packed_live_encoder = True
    return m


@pytest.mark.parametrize('pos', [True, False])
@pytest.mark.parametrize('shape', ['A', 'B', 'C'])
def test_packed_route_eval_parity(dev, shape, pos):
    m, sd, blocked, seq, spos, h = EC.build(shape, 'prior', pos)
    m = _packed(m.to(dev).eval())
    ref_logits, ref_enc = _ref(shape, 'prior', pos)[:2]
    logits, enc, _ = _run(m, seq, spos, dev)
    print('packed %s pos=%s: logits %.3e, enc_output (all rows, PAD included) %.3e' %
          (shape, pos, max_abs_diff(logits, ref_logits), max_abs_diff(enc, ref_enc)))
    assert max_abs_diff(logits, ref_logits) < TOL
    assert max_abs_diff(enc, ref_enc) < TOL     # PAD rows included: each sample's own PAD row
    m.use_packed_live_encoder = False
    padded = _run(m, seq, spos, dev)
    assert max_abs_diff(padded[0], logits) < TOL and not torch.equal(padded[1], enc)   # it IS another route


@pytest.mark.parametrize('shape', ['A', 'B'])
def test_packed_route_bits_do_not_depend_on_the_batch(dev, shape):
    """The packed route's kernel and summation order are a function of the sample's own rows: trimmed, batched, re-padded,
    permuted and split into micro-batches -- the same bits, PAD rows of enc_output included."""
    m, sd, blocked, seq, spos, h = EC.build(shape, 'prior', True)
    m = _packed(m.to(dev).eval())
    lengths = EC.SHAPES[shape]['lengths']
    T = seq.size(1)
    logits, enc, _ = _run(m, seq, spos, dev)
    perm = list(reversed(range(len(lengths))))
    p_logits, p_enc, _ = _run(m, seq[perm], spos[perm], dev)
    r_seq, r_pos = _repad(seq, spos, T + EC.PAD_EXTRA)
    r_logits, r_enc, _ = _run(m, r_seq, r_pos, dev)
    assert torch.equal(p_logits[perm], logits) and torch.equal(p_enc[perm], enc)
    assert torch.equal(r_logits, logits) and torch.equal(r_enc[:, :T], enc)
    for b, n in enumerate(lengths):
        t_logits, t_enc, _ = _run(m, seq[b:b + 1, :n], spos[b:b + 1, :n], dev)
        assert torch.equal(t_enc[0], enc[b, :n]) and torch.equal(t_logits[0], logits[b]), (shape, n)
    m.workspace_limit_bytes = 1     # one sample per pass
    s_logits, s_enc, _ = _run(m, seq, spos, dev)
    assert torch.equal(s_logits, logits) and torch.equal(s_enc, enc)


def test_packed_route_all_pad_sample_and_fallbacks(dev):
    m, sd, blocked, seq, spos, h = EC.build('A', 'prior', True)
    m = _packed(m.to(dev).eval())
    seq2 = torch.cat([seq[:1], torch.zeros_like(seq[:1]), seq[1:]])
    pos2 = torch.cat([spos[:1], torch.zeros_like(spos[:1]), spos[1:]])
    logits, enc, _ = _run(m, seq, spos, dev)
    l2, e2, _ = _run(m, seq2, pos2, dev)
    assert torch.isnan(l2[1]).all() and torch.isnan(e2[1]).all()
    assert torch.equal(l2[[0, 2, 3]], logits) and torch.equal(e2[[0, 2, 3]], enc)
    # maps and input graphs take the padded route whatever the switch says: the padded route's bits
    adj = EC.random_graphs(EC.SHAPES['A']['lengths'], seed=3)
    with_adj, with_maps = _run(m, seq, spos, dev, adj=adj), _run(m, seq, spos, dev, return_attns=True)
    m.use_packed_live_encoder = False
    assert torch.equal(_run(m, seq, spos, dev, adj=adj)[0], with_adj[0])
    assert torch.equal(_run(m, seq, spos, dev, return_attns=True)[0], with_maps[0])


# ------------------------------------------------------------------ 3. input graphs
def test_input_graphs_reach_the_prediction(dev):
    m, sd, blocked, seq, spos, h = EC.build('A', 'prior', True)
    m = m.to(dev).eval()
    adj = EC.random_graphs(EC.SHAPES['A']['lengths'], seed=3)
    with torch.no_grad():
        ref_logits, ref_enc, ref_maps = EC.live_forward_ref(sd, seq, spos, h, blocked, adj=adj)[:3]
    logits, enc, _ = _run(m, seq, spos, dev, adj=adj)
    assert max_abs_diff(logits, ref_logits) < TOL and max_abs_diff(enc, ref_enc) < TOL
    plain = _run(m, seq, spos, dev)[0]
    moved = (logits - plain).abs().max(dim=1).values
    print('adj: max |logit change| per sample', moved.tolist())
    assert float(moved.max()) > 1e-3          # the graph now reaches the prediction
    # the module-by-module route and the maps see the same graph
    with torch.no_grad():
        module = m._forward_composite((seq.to(dev), spos.to(dev)), adj, None, False, False)
    assert torch.equal(module[0], logits)
    w_maps = _run(m, seq, spos, dev, adj=adj, return_attns=True)
    assert torch.equal(w_maps[0], logits)
    for got, want in zip(w_maps[2][0], ref_maps):
        assert max_abs_diff(got, want) < TOL


# ------------------------------------------------------------------ 4. an all-PAD sample
def test_all_pad_sample_is_nan_and_leaves_its_neighbours_alone(dev):
    m, sd, blocked, seq, spos, h = EC.build('A', 'prior', True)
    m = m.to(dev).eval()
    seq2 = torch.cat([seq[:1], torch.zeros_like(seq[:1]), seq[1:]])
    pos2 = torch.cat([spos[:1], torch.zeros_like(spos[:1]), spos[1:]])
    logits, enc, _ = _run(m, seq, spos, dev)
    l2, e2, _ = _run(m, seq2, pos2, dev)
    assert torch.isnan(l2[1]).all()
    keep = [0, 2, 3]
    assert torch.equal(l2[keep], logits) and torch.equal(e2[keep], enc)


# ------------------------------------------------------------------ 5. training, dropout 0
@pytest.mark.parametrize('with_adj', [False, True])
def test_every_parameter_gradient_matches_oracle_autograd(dev, with_adj):
    m, sd, blocked, seq, spos, h = EC.build('A', 'prior', True)
    m = m.to(dev)
    L = EC.SHAPES['A']['L']
    adj = EC.random_graphs(EC.SHAPES['A']['lengths'], seed=4) if with_adj else None
    tgt = (torch.rand(seq.size(0), L, generator=torch.Generator().manual_seed(1)) < 0.2).float()
    sd64 = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    ref_logits, ref_enc = EC.live_forward_ref(sd64, seq, spos, h, blocked, adj=adj)[:2]
    ref_loss = F.binary_cross_entropy_with_logits(ref_logits, tgt.double())
    ref_loss.backward()

    m.train()
    logits, enc, extra = m((seq.to(dev), spos.to(dev)), adj, None, tgt.to(dev))
    assert extra is None and logits.requires_grad
    assert max_abs_diff(logits, ref_logits.detach()) < TOL and max_abs_diff(enc, ref_enc.detach()) < TOL
    loss = F.binary_cross_entropy_with_logits(logits, tgt.to(dev))
    loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-5
    checked = live = 0
    for pname, p in m.named_parameters():
        ref = sd64[pname].grad
        if pname == 'encoder.position_enc.weight':
            assert p.grad is None
            continue
        if pname == 'decoder.tgt_word_emb.weight' and sd64['tgt_word_proj.weight'].grad is not None:
            ref = ref + sd64['tgt_word_proj.weight'].grad
        assert p.grad is not None and ref is not None, pname
        scale = ref.abs().max().item()
        # the rule of tests/test_gpu_training.py for the decoder's attention parameters
        assert max_abs_diff(p.grad, ref) <= 3e-4 * scale + 1e-9, (pname, max_abs_diff(p.grad, ref), scale)
        if 'encoder.layer_stack' in pname and 'slf_attn' in pname:
            assert float(p.grad.abs().max()) > 0, pname     # None without the feature
            live += 1
        checked += 1
    assert checked >= 50 and live == 12


# ------------------------------------------------------------------ 6. training, dropout 0.1
def test_dropout_matches_the_torch_restatement_with_the_librarys_masks(dev):
    """The encoder of forward_train at dropout 0.1 against a fp64 restatement that applies the library's own counter-based keep
    masks (N.dropout_keep_mask) at the three sites of each live layer, with the seeds forward_train draws."""
    from lamp_amd import _native as N
    p = 0.1
    m, sd, blocked, seq, spos, h = EC.build('A', 'prior', True, dropout=p)
    m = m.to(dev).train()
    s = EC.SHAPES['A']
    B, T, d, H = seq.size(0), seq.size(1), s['d'], s['h']
    dk = d // H
    torch.manual_seed(11)
    base = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())     # training._Seeds

    def seed(k):
        return (base + 0x9E3779B1 * k) & 0xffffffff

    sd64 = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    x = F.embedding(seq, sd64['encoder.src_word_emb.weight']) + F.embedding(spos, sd64['encoder.position_enc.weight'])
    blk = EC.enc_blocked_mask(seq)
    k = 0
    for i in range(2):
        pre = 'encoder.layer_stack.%d.' % i
        wq, wk, wv, fc, g, b = R._mha_params(sd64, pre + 'slf_attn.')
        split = lambda t: t.view(B, T, H, dk).permute(2, 0, 1, 3)  # noqa: E731
        q, kk, v = split(x @ wq.t()), split(x @ wk.t()), split(x @ wv.t())
        P = torch.softmax((q @ kk.transpose(-1, -2) / dk ** 0.5).masked_fill(blk, float('-inf')), -1)
        keep_a = N.dropout_keep_mask(H * B * T * T, p, seed(k + 1)).view(H, B, T, T).cpu()
        a = ((P * keep_a / (1 - p)) @ v).permute(1, 2, 0, 3).reshape(B, T, H * dk)
        keep_o = N.dropout_keep_mask(B * T * d, p, seed(k + 2)).view(B, T, d).cpu()
        x = F.layer_norm((a @ fc.t()) * keep_o / (1 - p) + x, (d,), g, b, 1e-5)
        w1, b1, w2, b2, g2, bb2 = R._ffn_params(sd64, pre + 'pos_ffn.')
        keep_f = N.dropout_keep_mask(B * T * d, p, seed(k + 3)).view(B, T, d).cpu()
        o = torch.relu(x @ w1[:, :, 0].t() + b1) @ w2[:, :, 0].t() + b2
        x = F.layer_norm(o * keep_f / (1 - p) + x, (d,), g2, bb2, 1e-5)
        k += 3
    dy = torch.randn(B, T, d, generator=torch.Generator().manual_seed(5))
    (x * dy.double()).sum().backward()

    torch.manual_seed(11)
    enc = m((seq.to(dev), spos.to(dev)), None, None, None)[1]
    assert max_abs_diff(enc.detach(), x.detach()) < TOL
    (enc * dy.to(dev)).sum().backward()
    for pname, prm in m.named_parameters():
        if pname.startswith('encoder.layer_stack'):
            ref = sd64[pname].grad
            assert prm.grad is not None, pname
            assert max_abs_diff(prm.grad, ref) <= 3e-4 * ref.abs().max().item() + 1e-9, pname


# ------------------------------------------------------------------ 7. a training epoch
def test_training_epoch_is_reproducible_and_moves_the_encoder_attention_weights(dev):
    from lamp_amd import optim as O
    from lamp_amd import train as T
    s = dict(EC.SHAPES['A'], V=4 + 2 * EC.SHAPES['A']['L'])     # the synthetic dataset marks every label with two words
    data = TC.synthetic_dataset(n_train=48, n_labels=s['L'], n_words=s['V'] - 4, max_len=s['T'] - 2, seed=5)

    def epoch():
        m = EC.build(s, 'prior', True, dropout=0.1)[0].to(dev)
        before = {k: v.clone() for k, v in m.state_dict().items()}
        batches = T.TrainBatcher(data['train']['src'], data['train']['tgt'], 16, shuffle=False, drop_last=False)
        assert len(batches) == 3
        opt = O.Adam(list(m.get_trainable_parameters()), betas=TC.ADAM_BETAS, lr=1e-3)
        torch.manual_seed(3)
        preds, _, loss = T.train_epoch(m, batches, opt, TC.train_opt(s['L']), device=dev)
        torch.cuda.synchronize()
        assert loss == loss, 'NaN loss'
        return before, m.state_dict(), preds, loss

    before, after1, preds1, loss1 = epoch()
    _, after2, preds2, loss2 = epoch()
    assert loss1 == loss2 and torch.equal(preds1, preds2)
    assert all(torch.equal(after1[k], after2[k]) for k in after1)
    for k in after1:
        if 'encoder.layer_stack' in k and 'slf_attn' in k:
            assert not torch.equal(after1[k], before[k]), k


def test_run_train_with_the_flag_and_run_eval_takes_it_from_the_checkpoint(dev):
    from lamp_amd import run_eval, run_train
    with tempfile.TemporaryDirectory(prefix='lamp_live_') as root:
        assert 'test' not in root
        data_path = os.path.join(root, 'train_valid_data.pt')
        torch.save(TC.synthetic_dataset(n_train=64), data_path)
        args = ['-data', data_path, '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2', '-label_mask', 'prior',
                '-batch_size', '16']
        hist = run_train.main(args + ['-epoch', '2', '-lr', '0.003', '-dropout', '0.0', '-results_dir', os.path.join(root, 'res'),
                                      '-seed', '1', '-optim_impl', 'lamp', '-enc_self_att'])
        assert hist[1]['train_loss'] < hist[0]['train_loss']
        assert '.enc_self_att' in hist[1]['checkpoint']
        ckpt = torch.load(hist[1]['checkpoint'], map_location='cpu', weights_only=False)
        assert ckpt['settings'].enc_self_att is True
        out = run_eval.main(args + ['-checkpoint', hist[1]['checkpoint'], '-split', 'test'])     # no flag: from the settings
        assert out['bce_total'] / out['n_samples'] == hist[1]['test_loss']


# ------------------------------------------------------------------ 8. the one-hot encoder, live
def _onehot_live_ref(sd, seq, pos, h):
    x = F.embedding(seq, sd['encoder.src_word_emb.weight'], padding_idx=0).transpose(1, 2)
    y = F.relu(F.conv1d(x, sd['encoder.conv1.weight'], sd['encoder.conv1.bias'], padding=8))[:, :, :-1]
    y = F.max_pool1d(y, 2, 2)
    y = F.relu(F.conv1d(y, sd['encoder.conv2.weight'], sd['encoder.conv2.bias'], padding=8).transpose(1, 2))[:, :-1, :]
    T2 = y.size(1)
    y = y + F.embedding(pos[:, :T2], sd['encoder.position_enc.weight'])
    seq2 = seq[:, :T2]
    blk = EC.enc_blocked_mask(seq2)
    for i in range(R.count_layers(sd, 'encoder')):
        p = 'encoder.layer_stack.%d.' % i
        y, _ = R.mha(y, y, blk, *R._mha_params(sd, p + 'slf_attn.'), n_head=h)
        y = R.ffn(y, *R._ffn_params(sd, p + 'pos_ffn.'))
    out = R.decoder_forward(sd, seq2, y, None, h)[0]
    return R.readout(out, sd['tgt_word_proj.linear.weight']), y


def test_onehot_encoder_live(dev):
    import onehot_common as OC
    from lamp_amd.Models import LAMP
    d, h, L, T, B = 128, 2, 16, 64, 2
    torch.manual_seed(0)
    m = LAMP(9, L, T, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=2 * d,
             d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', dropout=0.0, dec_dropout=0.0, dec_dropout2=0.0, onehot=True,
             label_mask='none', enc_self_attn=True)
    seq, pos = OC.make_dna(B, T, lengths=[64, 41], seed=2)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref_logits, ref_enc = _onehot_live_ref(sd, seq, pos, h)
    m = m.to(dev).eval()
    logits, enc, _ = _run(m, seq, pos, dev)
    assert max_abs_diff(logits, ref_logits) < TOL and max_abs_diff(enc, ref_enc) < TOL
    # one gradient check: fp64 autograd on the same composition
    sd64 = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    tgt = (torch.rand(B, L, generator=torch.Generator().manual_seed(1)) < 0.2).float()
    F.binary_cross_entropy_with_logits(_onehot_live_ref(sd64, seq, pos, h)[0], tgt.double()).backward()
    m.train()
    out = m((seq.to(dev), pos.to(dev)), None, None, tgt.to(dev))[0]
    F.binary_cross_entropy_with_logits(out, tgt.to(dev)).backward()
    for pname, prm in m.named_parameters():
        if 'encoder.layer_stack' in pname or pname.startswith('encoder.conv'):
            ref = sd64[pname].grad
            assert prm.grad is not None and ref is not None, pname
            assert max_abs_diff(prm.grad, ref) <= 3e-4 * ref.abs().max().item() + 1e-9, pname


# ------------------------------------------------------------------ 9. the dead mode
def test_dead_mode_is_untouched(dev):
    from lamp_amd import _native as N
    m_off, sd, blocked, seq, spos, h = EC.build('A', 'prior', True, live=False, enc_self_attn=False)
    m_plain = EC.build('A', 'prior', True, live=False)[0]
    m_off, m_plain = m_off.to(dev).eval(), m_plain.to(dev).eval()
    a, b = _run(m_off, seq, spos, dev), _run(m_plain, seq, spos, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # lamp_forward_opts with the flag clear (and with no options at all) is lamp_forward
    model = m_plain._native_model()[0]
    s, p = seq.to(dev), spos.to(dev)
    B, T = s.shape
    L, d = m_plain.n_labels, m_plain.d_model
    lib = N.lib()
    assert lib.lamp_forward_opts_workspace_bytes(C.byref(model), None, B, T, 0) == lib.lamp_forward_workspace_bytes(C.byref(model), B, T, 0)
    ws = N.workspace(lib.lamp_forward_workspace_bytes(C.byref(model), B, T, 0) + 4096, dev)
    for opts in (None, N.FwdOptions(0, 0, None, None)):
        logits = torch.empty((B, L), dtype=torch.float32, device=dev)
        enc = torch.empty((B, T, d), dtype=torch.float32, device=dev)
        N.check(lib.lamp_forward_opts(C.byref(model), C.byref(opts) if opts is not None else None, s.data_ptr(), p.data_ptr(), B, T,
                                      logits.data_ptr(), enc.data_ptr(), None, ws.data_ptr(), ws.numel(), N.stream()),
                'lamp_forward_opts')
        torch.cuda.synchronize()
        assert torch.equal(logits, b[0]) and torch.equal(enc, b[1])
