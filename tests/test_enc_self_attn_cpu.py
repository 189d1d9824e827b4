"""The live encoder self-attention's surface, without a GPU: constructors, state_dict layout, the drivers' flags."""
import argparse

import torch

from oracle import lamp_ref as R


def _model(**kw):
    from lamp_amd.Models import LAMP
    return LAMP(30, 7, 12, 7, n_layers_enc=2, n_layers_dec=2, n_head=2, n_head2=2, d_word_vec=16, d_model=16, d_inner_hid=32,
                d_k=8, d_v=8, encoder='graph', decoder='graph', label_mask='none', **kw)


def test_constructs_with_the_flag_and_defaults_to_off():
    live, dead = _model(enc_self_attn=True), _model()
    assert live.enc_self_attn and live.encoder.enc_self_attn and all(l.live_attn for l in live.encoder.layer_stack)
    assert not dead.enc_self_attn and not dead.encoder.enc_self_attn and not any(l.live_attn for l in dead.encoder.layer_stack)


def test_the_new_keyword_comes_last_in_every_signature():
    import inspect
    from lamp_amd.Encoders import GraphEncoder
    from lamp_amd.Layers import EncoderLayer
    from lamp_amd.Models import LAMP
    for cls, name in ((LAMP, 'enc_self_attn'), (GraphEncoder, 'enc_self_attn'), (EncoderLayer, 'live_attn')):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].name == name and params[-1].default is False, cls


def test_state_dict_is_the_same_in_both_modes_and_is_the_reference_layout():
    live, dead = _model(enc_self_attn=True), _model()
    a, b = live.state_dict(), dead.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    ref = R.make_state_dict(30, 7, 12, 16, 32, 2, 2, 2)
    assert set(a) == set(ref) and all(a[k].shape == ref[k].shape for k in ref)
    # a checkpoint of either mode loads into the other
    live.load_state_dict(b)
    dead.load_state_dict(a)
    assert [id(p) for p in live.get_trainable_parameters()] != []
    assert len(list(live.get_trainable_parameters())) == len(list(dead.get_trainable_parameters()))


def test_the_flag_belongs_to_the_graph_encoder():
    import pytest
    from lamp_amd.Models import LAMP
    with pytest.raises(NotImplementedError):
        LAMP(30, 7, 12, 7, n_layers_enc=1, n_layers_dec=1, n_head=1, n_head2=1, d_word_vec=16, d_model=16, d_inner_hid=32,
             d_k=16, d_v=16, encoder='mlp', decoder='graph', label_mask='none', enc_self_attn=True)


def test_run_train_flag_name_suffix_and_checkpoint_setting():
    from lamp_amd import run_train
    base = ['-data', 'x.pt', '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2']
    off, on = run_train.parse(base), run_train.parse(base + ['-enc_self_att'])
    assert off.enc_self_att is False and on.enc_self_att is True
    assert '.enc_self_att' not in off.model_name
    assert on.model_name == off.model_name + '.enc_self_att'
    named = run_train.parse(base + ['-enc_self_att', '-name', 'r1'])
    assert named.model_name.endswith('.enc_self_att.r1')
    assert run_train.checkpoint_settings(on).enc_self_att is True
    assert run_train.checkpoint_settings(off).enc_self_att is False
    # derive() on a namespace of an older caller, which has no such attribute: off
    ns = argparse.Namespace(**{k: v for k, v in vars(run_train.parse(base)).items() if k != 'enc_self_att'})
    assert run_train.derive(ns).enc_self_att is False


def test_run_eval_reads_the_flag_from_the_settings_or_the_command_line(tmp_path):
    from lamp_amd import run_eval
    sd = {'w': torch.zeros(1)}
    for name, ckpt, want in (('on', {'model': sd, 'settings': argparse.Namespace(enc_self_att=True)}, True),
                             ('off', {'model': sd, 'settings': argparse.Namespace(enc_self_att=False)}, False),
                             ('absent', {'model': sd, 'settings': argparse.Namespace()}, False),
                             ('bare', sd, False)):
        path = str(tmp_path / (name + '.chkpt'))
        torch.save(ckpt, path)
        state, live = run_eval.load_checkpoint(path)
        assert live is want and list(state) == ['w']
    assert run_eval.parse(['-data', 'x.pt', '-enc_self_att']).enc_self_att is True
    assert run_eval.parse(['-data', 'x.pt']).enc_self_att is False


def test_options_struct_matches_the_header():
    import ctypes
    from lamp_amd import _native as N
    assert ctypes.sizeof(N.FwdOptions) == 24
    assert [f[0] for f in N.FwdOptions._fields_] == ['enc_self_attn', 'flags', 'enc_mask', 'enc_chain_packs']
    for name in ('lamp_forward_opts', 'lamp_forward_opts_workspace_bytes', 'lamp_onehot_forward_opts',
                 'lamp_onehot_forward_opts_workspace_bytes'):
        assert name in N.PROTOTYPES
