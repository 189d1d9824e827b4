"""The one-hot genomics encoder on the device (csrc/conv.hip): LAMP(onehot=True) in eval and train() mode against the
test-local fp64 restatement of lamp/Encoders.py:68-73 composed with the oracle (tests/onehot_common.py)."""
import pytest
import torch

from conftest import max_abs_diff
from oracle import lamp_ref as R
from lamp_amd import synthetic

from onehot_common import build_model, fp64_state, make_dna, onehot_forward_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def _blocked(adj, mask, L):
    return R.label_block_mask(adj, mask, L) if mask != 'none' else None


@pytest.mark.parametrize('T,lengths,mask', [(40, None, 'none'), (41, [41, 30, 7], 'prior'), (64, [64, 2], 'none')])
def test_eval_matches_fp64_restatement(dev, T, lengths, mask):
    L = 23
    adj = synthetic.make_adjacency(L, 0.2, 0) if mask == 'prior' else None
    m = build_model(d=64, h=4, L=L, T_max=64, mask=mask, adj=adj.clone() if adj is not None else None)
    B = len(lengths) if lengths else 2
    seq, pos = make_dna(B, T, lengths)
    sd = fp64_state(m)
    ref_logits, ref_enc, _ = onehot_forward_ref(sd, seq, pos, 4, _blocked(adj, mask, L))
    m = m.to(dev).eval()
    with torch.no_grad():
        logits, enc, _ = m((seq.to(dev), pos.to(dev)), None, None, None)
    assert enc.shape == (B, T // 2, 64)
    assert max_abs_diff(enc, ref_enc) < 1e-4
    assert max_abs_diff(logits, ref_logits) < 1e-4


def test_deepsea_shape_against_fp64(dev):
    L, d, T, B = 919, 512, 1000, 32
    for mask in ('none', 'prior'):
        adj = synthetic.make_adjacency(L, 0.05, 1) if mask == 'prior' else None
        m = build_model(d=d, h=4, L=L, T_max=T, dff=1024, mask=mask, adj=adj.clone() if adj is not None else None)
        seq, pos = make_dna(B, T, [T] * (B - 1) + [700], seed=3)
        sd = fp64_state(m)
        m = m.to(dev).eval()
        with torch.no_grad():
            logits, enc, _ = m((seq.to(dev), pos.to(dev)), None, None, None)
        pick = [0, B - 1]   # results do not depend on B: a few samples on the CPU
        ref_logits, ref_enc, _ = onehot_forward_ref(sd, seq[pick], pos[pick], 4, _blocked(adj, mask, L))
        err = max_abs_diff(logits[pick], ref_logits)
        print('deepsea %s: logits max |err| %.3g, enc %.3g' % (mask, err, max_abs_diff(enc[pick], ref_enc)))
        assert err < 1e-4


def test_microbatches_and_batch_size_do_not_change_a_sample(dev):
    m = build_model(d=64, h=4, L=23, T_max=64).to(dev).eval()
    seq, pos = make_dna(5, 50, [50, 20, 50, 3, 44], seed=2)
    seq, pos = seq.to(dev), pos.to(dev)
    with torch.no_grad():
        whole = m((seq, pos), None, None, None)
        m.workspace_limit_bytes = 1   # one sample per micro-batch
        split = m((seq, pos), None, None, None)
        one = m((seq[3:4], pos[3:4]), None, None, None)
    assert torch.equal(whole[0], split[0]) and torch.equal(whole[1], split[1])
    assert torch.equal(whole[0][3:4], one[0]) and torch.equal(whole[1][3:4], one[1])


def test_int_preds_and_attention_maps(dev):
    L, T = 23, 40
    m = build_model(d=64, h=4, L=L, T_max=64, int_preds=True)
    seq, pos = make_dna(2, T, [40, 25])
    sd = fp64_state(m)
    ref_logits, ref_enc, ref_int = onehot_forward_ref(sd, seq, pos, 4, None, int_preds=True)
    _, _, (ref_slf, ref_encdec) = onehot_forward_ref(sd, seq, pos, 4, None)
    m = m.to(dev).eval()
    with torch.no_grad():
        logits, enc, ipreds = m((seq.to(dev), pos.to(dev)), None, None, None, int_preds=True)
        out = m((seq.to(dev), pos.to(dev)), None, None, None, return_attns=True)
    assert max_abs_diff(logits, ref_logits) < 1e-4
    assert len(ipreds) == len(ref_int) and all(max_abs_diff(a, b) < 1e-4 for a, b in zip(ipreds, ref_int))
    enc_attns, (slf, encdec) = out[2][0], out[3]
    assert len(enc_attns) == 2 and enc_attns[0].shape == (4 * 2, T // 2, T // 2)
    assert encdec[0].shape == (4 * 2, L, T // 2)
    for a, b in zip(encdec, ref_encdec):
        assert max_abs_diff(a, b) < 1e-4
    assert max_abs_diff(out[0], ref_logits) < 1e-4


def _grads_ref(sd64, names, seq, pos, n_head, w):
    sd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd64.items()}
    logits, _, _ = onehot_forward_ref(sd, seq, pos, n_head, None)
    (logits * w).sum().backward()
    return {k: sd[k].grad for k in names}


def test_training_gradients_match_fp64_autograd(dev):
    m = build_model(d=64, h=4, L=23, T_max=64)
    seq, pos = make_dna(3, 37, [37, 20, 9], seed=5)
    sd64 = fp64_state(m)
    w = torch.randn(3, 23, generator=torch.Generator().manual_seed(1))
    # the sinusoid table is frozen (lamp/Models.py:97-107); the library gives it no gradient, as on the token path
    names = [k for k, p in m.named_parameters() if k != 'encoder.position_enc.weight']
    ref = _grads_ref(sd64, [k for k in names if k in sd64], seq, pos, 4, w.double())
    m = m.to(dev).train()
    logits, enc, _ = m((seq.to(dev), pos.to(dev)), None, None, None)
    (logits * w.to(dev)).sum().backward()
    worst = 0.0
    for k, p in m.named_parameters():
        if k not in ref or ref[k] is None:
            continue
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        err = max_abs_diff(g, ref[k]) / max(1.0, float(ref[k].abs().max()))
        worst = max(worst, err)
        assert err < 1e-4, (k, err)
    for k in ('encoder.conv1.weight', 'encoder.conv1.bias', 'encoder.conv2.weight', 'encoder.conv2.bias',
              'encoder.src_word_emb.weight'):
        assert k in ref and ref[k] is not None


def test_dropout_uses_the_librarys_counter_based_mask(dev):
    from lamp_amd import _native as N, training
    m = build_model(d=64, h=4, L=23, T_max=64, dropout=0.3).to(dev)
    enc = m.encoder.train()
    seq, pos = make_dna(2, 30, [30, 17], seed=7)
    seq, pos = seq.to(dev), pos.to(dev)
    seed = 12345
    t1 = N.onehot_tap_table(enc.src_word_emb.weight, enc.conv1.weight)
    x = training._OnehotFn.apply(seq, pos, t1, enc.conv1.bias, enc.conv2.weight, enc.conv2.bias,
                                 enc.position_enc.weight, 0.3, seed)
    B, T, d = 2, 30, 64
    keep = N.dropout_keep_mask(B * T * d, 0.3, seed, device=dev).view(B, T, d).transpose(1, 2).double()
    sd = {k: v.detach().double() for k, v in m.state_dict().items()}
    xin = torch.nn.functional.embedding(seq, sd['encoder.src_word_emb.weight']).transpose(1, 2)
    y = torch.nn.functional.conv1d(xin, sd['encoder.conv1.weight'], sd['encoder.conv1.bias'], padding=8)[:, :, :-1]
    y = torch.relu(y * keep / 0.7)
    y = torch.nn.functional.max_pool1d(y, 2, 2)
    y = torch.relu(torch.nn.functional.conv1d(y, sd['encoder.conv2.weight'], sd['encoder.conv2.bias'], padding=8)
                   .transpose(1, 2))[:, :-1, :]
    y = y + torch.nn.functional.embedding(pos[:, :T // 2], sd['encoder.position_enc.weight'])
    assert max_abs_diff(x, y) < 1e-4


def test_optimizer_step_then_eval_rebuilds_the_cached_tables(dev):
    m = build_model(d=64, h=4, L=23, T_max=64).to(dev)
    seq, pos = make_dna(2, 32, [32, 11], seed=9)
    seq, pos = seq.to(dev), pos.to(dev)
    m.eval()
    with torch.no_grad():
        before = m((seq, pos), None, None, None)[0].clone()
    opt = torch.optim.SGD(m.get_trainable_parameters(), lr=0.5)
    m.train()
    logits = m((seq, pos), None, None, None)[0]
    logits.sum().backward()
    opt.step()
    m.eval()
    with torch.no_grad():
        after = m((seq, pos), None, None, None)[0]
    sd = fp64_state(m)
    ref, _, _ = onehot_forward_ref(sd, seq.cpu(), pos.cpu(), 4, None)
    assert not torch.equal(before, after)
    assert max_abs_diff(after, ref) < 1e-4


@pytest.mark.parametrize('name', ['even_none', 'odd_prior', 'ragged_prior', 'maps_none'])
def test_against_the_reference_golden(dev, name):
    """tests/golden/onehot_*.npz, recorded from the reference itself (tests/golden/make_golden_onehot.py)."""
    from onehot_common import golden_model
    m, z, _, _ = golden_model(name)
    m = m.to(dev).eval()
    src = (torch.from_numpy(z['seq']).to(dev), torch.from_numpy(z['pos']).to(dev))
    with torch.no_grad():
        logits, enc, _ = m(src, None, None, None)
    assert max_abs_diff(logits, torch.from_numpy(z['logits_fp64'])) < 1e-4
    assert max_abs_diff(enc, torch.from_numpy(z['enc_fp64'])) < 1e-4
    if 'int_pred0_fp64' not in z:
        return
    with torch.no_grad():
        _, _, ip = m(src, None, None, None, int_preds=True)
        _, _, enc_attns, dec2 = m(src, None, None, None, return_attns=True)
    for i, a in enumerate(ip):
        assert max_abs_diff(a, torch.from_numpy(z['int_pred%d_fp64' % i])) < 1e-4
    # the encoder's maps are over T2 keys, masked by src_seq[:, :T2] read with a row stride of T
    for i, a in enumerate(enc_attns[0]):
        assert max_abs_diff(a, torch.from_numpy(z['enc_attn%d_fp64' % i])) < 1e-4, i
    for j, group in enumerate(dec2):
        for i, a in enumerate(group):
            assert max_abs_diff(a, torch.from_numpy(z['dec_attn%d_%d_fp64' % (j, i)])) < 1e-4, (j, i)


def test_dropout_backward_uses_the_same_mask(dev):
    """p > 0: the front end's gradients (dropout-scaled pool / ReLU backward, tap table, conv1 / conv2) against torch
    autograd on a restatement that uses the library's counter-based keep mask."""
    from lamp_amd import _native as N, training
    F = torch.nn.functional
    p, seed, B, T, d = 0.3, 777, 2, 34, 64
    m = build_model(d=d, h=4, L=23, T_max=64, dropout=p).to(dev)
    enc = m.encoder.train()
    seq, pos = make_dna(B, T, [T, 21], seed=11)
    seq, pos = seq.to(dev), pos.to(dev)
    G = torch.randn(B, T // 2, d, generator=torch.Generator().manual_seed(3)).to(dev)
    t1 = N.onehot_tap_table(enc.src_word_emb.weight, enc.conv1.weight)
    x = training._OnehotFn.apply(seq, pos, t1, enc.conv1.bias, enc.conv2.weight, enc.conv2.bias,
                                 enc.position_enc.weight, p, seed)
    (x * G).sum().backward()
    keep = N.dropout_keep_mask(B * T * d, p, seed, device=dev).view(B, T, d).transpose(1, 2).double()
    ref = {k: v.detach().double().clone().requires_grad_(True) for k, v in
           (('w1', enc.conv1.weight), ('b1', enc.conv1.bias), ('w2', enc.conv2.weight), ('b2', enc.conv2.bias),
            ('e', enc.src_word_emb.weight))}
    xin = F.embedding(seq, ref['e'], padding_idx=0).transpose(1, 2)
    y = F.conv1d(xin, ref['w1'], ref['b1'], padding=8)[:, :, :-1]
    y = F.max_pool1d(torch.relu(y * keep / (1 - p)), 2, 2)
    y = torch.relu(F.conv1d(y, ref['w2'], ref['b2'], padding=8).transpose(1, 2))[:, :-1, :]
    y = y + F.embedding(pos[:, :T // 2], enc.position_enc.weight.double())
    assert max_abs_diff(x, y) < 1e-4
    (y * G.double()).sum().backward()
    for k, prm in (('w1', enc.conv1.weight), ('b1', enc.conv1.bias), ('w2', enc.conv2.weight), ('b2', enc.conv2.bias),
                   ('e', enc.src_word_emb.weight)):
        err = max_abs_diff(prm.grad, ref[k].grad) / max(1.0, float(ref[k].grad.abs().max()))
        assert err < 1e-4, (k, err)


def test_run_eval_on_a_synthetic_onehot_dataset(dev, tmp_path):
    """run_eval -dataset deepsea: the reference's rule (config_args.py:90-91) builds the one-hot model, the checkpoint loads,
    and the metrics are those of LAMP(onehot=True) called batch by batch (each batch padded to its own longest sequence)."""
    import argparse
    import json
    import os
    import subprocess
    import sys
    from lamp_amd import synthetic, data as D
    from lamp_amd.run_eval import multilabel_metrics
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n_lab, T_MAX, bs = 12, 64, 4
    g = torch.Generator().manual_seed(5)

    def split(n):
        src, tgt = [], []
        for _ in range(n):
            ln = int(torch.randint(10, T_MAX + 1, (1,), generator=g))
            src.append(torch.randint(4, 9, (ln,), generator=g).tolist())
            labs = sorted(set(torch.randint(4, 4 + n_lab, (3,), generator=g).tolist()))
            tgt.append([2] + labs + [3])
        return {'src': src, 'tgt': tgt}
    src_dict = {w: i for i, w in enumerate(['<blank>', '<unk>', '<s>', '</s>', 'A', 'C', 'G', 'T', 'N'])}
    tgt_dict = {w: i for i, w in enumerate(['<blank>', '<unk>', '<s>', '</s>'] + ['l%d' % i for i in range(n_lab)])}
    data = {'settings': argparse.Namespace(max_seq_len=T_MAX), 'dict': {'src': src_dict, 'tgt': tgt_dict},
            'train': split(8), 'valid': split(4), 'test': split(10)}
    torch.save(data, tmp_path / 'train_valid_test.pt')
    sd = synthetic.make_onehot_state_dict(n_lab, T_MAX, 64, 128, 4, 2, 2, seed=4)
    torch.save({'model': sd}, tmp_path / 'model.chkpt')
    args = ['-data', str(tmp_path / 'train_valid_test.pt'), '-checkpoint', str(tmp_path / 'model.chkpt'), '-dataset', 'deepsea',
            '-d_model', '64', '-d_inner_hid', '128', '-n_layers_enc', '2', '-n_head', '4', '-label_mask', 'none',
            '-batch_size', str(bs)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'lamp_amd.run_eval'] + args, capture_output=True, text=True, env=env,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert out['onehot'] is True and out['n_samples'] == 10
    r2 = subprocess.run([sys.executable, '-m', 'lamp_amd.run_eval'] + args + ['-merge_stages'], capture_output=True,
                        text=True, env=env, timeout=600, cwd=ROOT)
    assert r2.returncode != 0 and 'merge_stages' in r2.stderr
    m = build_model(d=64, h=4, L=n_lab, T_max=T_MAX, dff=128)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    preds, gold = [], []
    for (seq, pos), _, tgt in D.EvalBatcher(data['test']['src'], data['test']['tgt'], bs):
        with torch.no_grad():
            preds.append(torch.sigmoid(m((seq.to(dev), pos.to(dev)), None, None, None)[0]).cpu())
        gold.append(D.get_gold_binary(tgt[:, 1:], n_lab))
    want = multilabel_metrics(torch.cat(preds), torch.cat(gold), 0.5)
    for k in ('subset_accuracy', 'hamming_accuracy', 'example_f1', 'micro_f1', 'macro_f1'):
        assert abs(out[k] - want[k]) < 1e-9, k
    with pytest.raises(ValueError, match='merge_stage'):
        from lamp_amd.evaluate import test_epoch
        test_epoch(m, D.EvalBatcher(data['test']['src'], data['test']['tgt'], bs), n_lab, bs, dev, merge_stage=True)
