"""The one-hot genomics encoder (GraphEncoder(onehot=True), lamp/Encoders.py:46-51,68-73) without a GPU: construction,
the reference's parameter names and shapes, what stays rejected, the trainable set, the C ABI's new entry points."""
import ctypes

import pytest
import torch

from lamp_amd import _native as N
from lamp_amd.Encoders import GraphEncoder, RNNEncoder
from lamp_amd.Models import LAMP

from onehot_common import build_model


def test_state_dict_names_and_shapes_follow_the_reference():
    m = build_model(d=64, h=4, L=23, T_max=64)
    sd = m.state_dict()
    assert sd['encoder.src_word_emb.weight'].shape == (9, 9)
    assert sd['encoder.conv1.weight'].shape == (64, 9, 16)
    assert sd['encoder.conv1.bias'].shape == (64,)
    assert sd['encoder.conv2.weight'].shape == (64, 64, 16)
    assert sd['encoder.conv2.bias'].shape == (64,)
    assert sd['encoder.position_enc.weight'].shape == (65, 64)
    e = sd['encoder.src_word_emb.weight']
    ref = torch.zeros(9, 9)
    ref[1:, 1:] = torch.eye(8)
    assert torch.equal(e, ref)
    # a checkpoint of the same shape loads
    m2 = build_model(d=64, h=4, L=23, T_max=64, seed=1)
    m2.load_state_dict(sd)
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in sd.items())


def test_out_of_scope_onehot_combinations_raise():
    kw = dict(n_layers=1, n_head=1, d_k=8, d_v=8, d_word_vec=8, d_model=8, d_inner_hid=16, onehot=True)
    GraphEncoder(9, 4, **kw)
    with pytest.raises(NotImplementedError):
        GraphEncoder(10, 4, **kw)
    with pytest.raises(NotImplementedError):
        GraphEncoder(9, 4, no_enc_pos_embedding=True, **kw)
    for t in ('sum', 'mean', 'flatten'):
        with pytest.raises(NotImplementedError):
            GraphEncoder(9, 4, enc_transform=t, **kw)
    with pytest.raises(NotImplementedError):
        RNNEncoder(9, 4, n_layers=1, d_word_vec=8, d_model=8, onehot=True)
    m = build_model(d=16, h=2, L=5, T_max=8)
    seq = torch.ones(1, 8, dtype=torch.long)
    with pytest.raises(NotImplementedError, match='adj'):
        m((seq, seq), [torch.ones(2, 2)], None, None)


def test_trainable_parameters_leave_out_the_identity_table_and_positions():
    m = build_model(d=16, h=2, L=5, T_max=8)
    ids = {id(p) for p in m.get_trainable_parameters()}
    assert id(m.encoder.src_word_emb.weight) not in ids
    assert id(m.encoder.position_enc.weight) not in ids
    assert id(m.encoder.conv1.weight) in ids and id(m.encoder.conv2.bias) in ids
    n_all = len(list(m.parameters()))
    assert len(ids) == n_all - 2
    # the token encoder keeps its embedding trainable
    t = LAMP(10, 5, 8, 5, n_layers_enc=1, n_layers_dec=1, n_head=2, n_head2=2, d_word_vec=16, d_model=16,
             d_inner_hid=32, d_k=8, d_v=8, encoder='graph', decoder='graph', label_mask='none')
    assert id(t.encoder.src_word_emb.weight) in {id(p) for p in t.get_trainable_parameters()}


def test_tap_table_is_a_pure_repack_for_the_identity_embedding():
    m = build_model(d=16, h=2, L=5, T_max=8)
    enc = m.encoder
    t1 = N.onehot_tap_table(enc.src_word_emb.weight, enc.conv1.weight)
    assert t1.shape == (9, 16, 16)
    assert torch.all(t1[0] == 0)
    for v in range(1, 9):
        assert torch.equal(t1[v], enc.conv1.weight[:, v, :].t())


def test_new_entry_points_are_bound_and_validate_before_any_launch():
    lib = N.lib()
    for name in ('lamp_onehot_forward', 'lamp_onehot_forward_workspace_bytes', 'lamp_conv_pack', 'lamp_onehot_front_fwd',
                 'lamp_conv_window_fwd', 'lamp_conv_relu_bwd_pad', 'lamp_onehot_front_bwd',
                 'lamp_onehot_front_bwd_partials_bytes'):
        assert name in N.PROTOTYPES and hasattr(lib, name)
    assert lib.lamp_onehot_forward_workspace_bytes(None, None, 1, 100, 0) == 0
    assert lib.lamp_onehot_forward(None, None, None, None, 1, 100, None, None, None, None, 0, None) == -5
    fe = N.OnehotFrontend(16, 16, 16, 16, 16, 9, 16)
    assert lib.lamp_onehot_front_fwd(16, 1, 100, ctypes.byref(fe), 6, 0.0, 0, 16, None) == -4    # d % 4
    assert lib.lamp_onehot_front_fwd(16, 1, 1, ctypes.byref(fe), 8, 0.0, 0, 16, None) == -1     # T < 2
    bad = N.OnehotFrontend(16, 16, 16, 16, 16, 17, 16)
    assert lib.lamp_onehot_front_fwd(16, 1, 100, ctypes.byref(bad), 8, 0.0, 0, 16, None) == -1  # vocabulary > 16
    assert lib.lamp_conv_window_fwd(None, 1, 4, 20, 8, 16, 8, None, 1, None, 0, None, 0, 16, None, None) == -5
    assert lib.lamp_conv_window_fwd(16, 1, 4, 20, 6, 16, 8, None, 1, None, 0, None, 0, 16, None, None) == -4
    assert lib.lamp_conv_window_fwd(16, 1, 4, 2, 8, 16, 8, None, 1, None, 0, None, 0, 16, None, None) == -1
    assert lib.lamp_conv_pack(None, 4, 4, 16, 0, 16, None) == -5
    assert lib.lamp_conv_relu_bwd_pad(16, 16, 1, 4, 6, 16, None) == -4
    assert lib.lamp_onehot_front_bwd(16, 1, 100, ctypes.byref(fe), 8, 0.0, 0, 16, 16, 16, 0, None) == -3


GOLDEN_CASES = ('even_none', 'odd_prior', 'ragged_prior', 'maps_none')


def test_state_dict_names_and_shapes_equal_the_reference_fixture():
    from onehot_common import golden_model
    m, z, _, _ = golden_model('even_none')
    sd = m.state_dict()
    names = [str(n) for n in z['sd_names']]
    assert sorted(sd) == names
    for k, shp in zip(names, z['sd_shapes']):
        assert list(sd[k].shape) == [int(x) for x in shp if x > 0], k


@pytest.mark.parametrize('name', GOLDEN_CASES)
def test_fp64_restatement_equals_the_reference_fp64_record(name):
    """Pins tests/onehot_common.onehot_forward_ref (which the GPU tests use at full size) to the reference itself."""
    from conftest import max_abs_diff
    from oracle import lamp_ref as R
    from onehot_common import golden_case, onehot_forward_ref, GOLDEN_DIMS
    z, sd, adj = golden_case(name)
    sd = {k: v.double() for k, v in sd.items()}
    seq, pos = torch.from_numpy(z['seq']), torch.from_numpy(z['pos'])
    blocked = R.label_block_mask(adj, 'prior', GOLDEN_DIMS['L']) if adj is not None else None
    logits, enc, _ = onehot_forward_ref(sd, seq, pos, GOLDEN_DIMS['h'], blocked)
    assert enc.shape == z['enc_fp64'].shape
    assert max_abs_diff(enc, torch.from_numpy(z['enc_fp64'])) < 1e-9
    assert max_abs_diff(logits, torch.from_numpy(z['logits_fp64'])) < 1e-9
    if 'int_pred0_fp64' in z:
        _, _, ip = onehot_forward_ref(sd, seq, pos, GOLDEN_DIMS['h'], blocked, int_preds=True)
        for i, a in enumerate(ip):
            assert max_abs_diff(a, torch.from_numpy(z['int_pred%d_fp64' % i])) < 1e-9
