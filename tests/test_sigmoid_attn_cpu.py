"""Sigmoid attention without a GPU: the torch restatement against the reference's fixture, constructors, state_dict layout,
the drivers' flag and the ABI table."""
import argparse
import os
import re

import pytest
import torch

from conftest import ROOT
from oracle import lamp_ref as R
from sigmoid_common import MASKS, load_fixture, mha_state, sigmoid_sdpa

NEW_ENTRIES = ('lamp_sdpa_act_fwd', 'lamp_mha_act_fwd', 'lamp_mha_train_act_fwd', 'lamp_mha_act_bwd', 'lamp_sigmoid_attn_bwd')


@pytest.fixture(scope='module')
def fx():
    return load_fixture()


@pytest.mark.parametrize('mask', MASKS)
def test_restatement_reproduces_the_reference_sdpa(fx, mask):
    m = fx.get('sdpa_mask_' + mask)
    out, attn = sigmoid_sdpa(fx['sdpa_q'], fx['sdpa_k'], fx['sdpa_v'], m)
    assert (attn - fx['sdpa_attn_' + mask]).abs().max().item() <= 1e-6
    assert (out - fx['sdpa_out_' + mask]).abs().max().item() <= 1e-5


@pytest.mark.parametrize('h', (1, 4))
@pytest.mark.parametrize('mask', MASKS)
def test_restatement_reproduces_the_reference_mha(fx, monkeypatch, h, mask):
    monkeypatch.setattr(R, 'sdpa', sigmoid_sdpa)
    sd = mha_state(fx, h)
    pre = 'mha%d_' % h
    out, attn = R.mha(fx[pre + 'xq'], fx[pre + 'xkv'], fx.get(pre + 'mask_' + mask), sd['w_qs.weight'], sd['w_ks.weight'],
                      sd['w_vs.weight'], sd.get('fc.weight'), sd['layer_norm.weight'], sd['layer_norm.bias'], n_head=h)
    assert (attn - fx[pre + 'attn_' + mask]).abs().max().item() <= 1e-6
    assert (out - fx[pre + 'out_' + mask]).abs().max().item() <= 1e-5


def test_fully_blocked_row_is_zero_and_finite(fx):
    m = fx['sdpa_mask_fullrow']
    rows = m.all(dim=2)
    assert rows.any()
    out, attn = sigmoid_sdpa(fx['sdpa_q'], fx['sdpa_k'], fx['sdpa_v'], m)
    for o, a in ((out, attn), (fx['sdpa_out_fullrow'], fx['sdpa_attn_fullrow'])):
        assert torch.isfinite(o).all() and torch.isfinite(a).all()
        assert (a[rows] == 0).all() and (o[rows] == 0).all()
    for h in (1, 4):
        a = fx['mha%d_attn_fullrow' % h]
        mm = fx['mha%d_mask_fullrow' % h].repeat(h, 1, 1)
        assert torch.isfinite(a).all() and torch.isfinite(fx['mha%d_out_fullrow' % h]).all() and (a[mm.all(dim=2)] == 0).all()


def _model(**kw):
    from lamp_amd.Models import LAMP
    return LAMP(30, 7, 12, 7, n_layers_enc=2, n_layers_dec=2, n_head=2, n_head2=2, d_word_vec=16, d_model=16, d_inner_hid=32,
                d_k=8, d_v=8, encoder='graph', decoder='graph', label_mask='none', **kw)


def test_module_constructors():
    from lamp_amd import _native as N
    from lamp_amd.SubLayers import MultiHeadAttention, ScaledDotProductAttention
    assert ScaledDotProductAttention(4.0, attn_type='sigmoid').act == N.LAMP_ATTN_SIGMOID
    assert ScaledDotProductAttention(4.0).act == N.LAMP_ATTN_SOFTMAX
    assert MultiHeadAttention(2, 16, 8, 8, attn_type='sigmoid').attention.act == N.LAMP_ATTN_SIGMOID
    for cls, args in ((ScaledDotProductAttention, (4.0,)), (MultiHeadAttention, (2, 16, 8, 8))):
        with pytest.raises(NotImplementedError):
            cls(*args, attn_type='tanh')


def test_model_opt_in_reaches_the_decoder_blocks_only():
    from lamp_amd import _native as N
    blocks = lambda m: [a.attention.act for l in m.decoder.layer_stack for a in (l.enc_attn, l.slf_attn)]  # noqa: E731
    ignored = _model(attn_type='sigmoid')   # the reference's flag: accepted and dropped (lamp/Layers.py:23-30)
    assert ignored.dec_attn_type is None and blocks(ignored) == [N.LAMP_ATTN_SOFTMAX] * 4
    on = _model(dec_attn_type='sigmoid')
    assert blocks(on) == [N.LAMP_ATTN_SIGMOID] * 4
    assert all(l.slf_attn.attention.act == N.LAMP_ATTN_SOFTMAX for l in on.encoder.layer_stack)
    live = _model(dec_attn_type='sigmoid', enc_self_attn=True)
    assert all(l.slf_attn.attention.act == N.LAMP_ATTN_SOFTMAX for l in live.encoder.layer_stack)
    nodec = _model(dec_attn_type='sigmoid', no_dec_self_att=True)
    assert [l.enc_attn.attention.act for l in nodec.decoder.layer_stack] == [N.LAMP_ATTN_SIGMOID] * 2
    with pytest.raises(NotImplementedError):
        _model(dec_attn_type='tanh')
    a, b = on.state_dict(), _model().state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)


def test_run_train_flag_and_checkpoint_settings_round_trip(tmp_path):
    from lamp_amd import run_eval, run_train
    base = ['-data', 'x.pt', '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2']
    off, on = run_train.parse(base), run_train.parse(base + ['-attn_type', 'sigmoid'])
    assert off.attn_type == 'softmax' and on.attn_type == 'sigmoid'
    assert on.model_name == off.model_name + '.attn_sigmoid'
    with pytest.raises(SystemExit):
        run_train.parse(base + ['-attn_type', 'tanh'])
    sd = {'w': torch.zeros(1)}
    for name, ckpt, want in (('on', {'model': sd, 'settings': run_train.checkpoint_settings(on)}, 'sigmoid'),
                             ('off', {'model': sd, 'settings': run_train.checkpoint_settings(off)}, 'softmax'),
                             ('absent', {'model': sd, 'settings': argparse.Namespace(enc_self_att=True)}, 'softmax'),
                             ('bare', sd, 'softmax')):
        path = str(tmp_path / (name + '.chkpt'))
        torch.save(ckpt, path)
        state, live, attn_type = run_eval.load_checkpoint_settings(path)
        assert attn_type == want and list(state) == ['w'] and live is (name == 'absent')
    assert run_eval.parse(['-data', 'x.pt', '-attn_type', 'sigmoid']).attn_type == 'sigmoid'
    ns = argparse.Namespace(**{k: v for k, v in vars(run_train.parse(base)).items() if k != 'attn_type'})
    assert run_train.derive(ns).attn_type == 'softmax'


def test_header_ctypes_and_library_carry_the_new_entry_points():
    import ctypes
    from lamp_amd import _native as N
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(lamp_[a-z0-9_]+)\s*\(', text))
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and name in N.PROTOTYPES and hasattr(lib, name), name
    assert set(N.PROTOTYPES) == declared   # and vice versa: no row without a declaration
    for macro, value in (('LAMP_ATTN_SOFTMAX', 0), ('LAMP_ATTN_SIGMOID', 1), ('LAMP_FWD_DEC_SIGMOID', 2)):
        assert re.search(r'#define %s %d\b' % (macro, value), text) and getattr(N, macro) == value
    assert N.lib().lamp_version() == 5
