"""The learnable label graph (LAMP(learn_label_bias=True)) without a GPU: the constructor and the state_dict, the runners'
flag, the C ABI of lamp_attn_bias_bwd / lamp_label_bias_fold (symbols and host-side argument checks) and the resource report
of their two kernels."""
import argparse
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

from lamp_amd import _native as N

L = 7
NEW_SYMBOLS = ('lamp_attn_bias_bwd_workspace_bytes', 'lamp_attn_bias_bwd', 'lamp_label_bias_fold')


def _model(**kw):
    from lamp_amd.Models import LAMP
    args = dict(n_layers_enc=2, n_layers_dec=2, n_head=2, n_head2=2, d_word_vec=16, d_model=16, d_inner_hid=32, d_k=8, d_v=8,
                encoder='graph', decoder='graph', label_mask='none')
    args.update(kw)
    return LAMP(30, L, 12, L, **args)


def _prior():
    g = torch.Generator().manual_seed(1)
    adj = (torch.rand(L, L, generator=g) < 0.4).float()
    adj = ((adj + adj.t()) > 0).float()
    adj.fill_diagonal_(1.0)
    assert (adj == 0).any()
    return adj


# ------------------------------------------------------------------ construction
def test_the_default_adds_no_parameter_and_no_key():
    import inspect
    from lamp_amd.Models import LAMP
    from lamp_amd.Decoders import GraphDecoder
    # next to label_bias, as label_bias came in: `enc_self_attn` stays LAMP's last keyword (tests/test_enc_self_attn_cpu.py)
    names = list(inspect.signature(LAMP.__init__).parameters)
    assert names[-3:] == ['label_bias', 'learn_label_bias', 'enc_self_attn']
    assert list(inspect.signature(GraphDecoder.__init__).parameters)[-2:] == ['label_bias', 'learn_label_bias']
    for cls in (LAMP, GraphDecoder):
        assert inspect.signature(cls.__init__).parameters['learn_label_bias'].default is False
    plain, const = _model(), _model(label_bias=torch.randn(L, L))
    assert list(const.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in const.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert not any('label_bias' in n for n, _ in const.named_parameters())
    assert const.decoder.label_bias is None and plain.decoder.label_bias is None
    assert const.decoder.label_bias_f32.requires_grad is False
    off = _model(label_bias=torch.randn(L, L), learn_label_bias=False)
    assert list(off.state_dict()) == list(plain.state_dict())


def test_the_flag_makes_the_bias_a_parameter_in_the_state_dict():
    g = torch.Generator().manual_seed(2)
    bias = torch.randn(L, L, generator=g)
    bias[2, 5] = float('-inf')
    m = _model(label_bias=bias, learn_label_bias=True, label_adj_matrix=_prior(), label_mask='prior')
    p = m.decoder.label_bias
    assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.dtype == torch.float32 and tuple(p.shape) == (L, L)
    assert torch.equal(p.detach(), bias) and p.data_ptr() != bias.data_ptr()       # what the caller passed, -inf included
    sd = m.state_dict()
    assert 'decoder.label_bias' in sd and not any('label_bias_f32' in k for k in sd)
    assert set(sd) - set(_model().state_dict()) == {'decoder.label_bias'}
    assert any(q is p for q in m.parameters()) and any(q is p for q in m.get_trainable_parameters())
    # the buffer the kernels read: padded, mask folded in, non-persistent, no gradient of its own
    buf = m.decoder.label_bias_f32
    blocked = m.decoder.label_mask_u8 != 0
    assert tuple(buf.shape) == (L, 8) and not buf.requires_grad and 'label_bias_f32' in dict(m.decoder.named_buffers())
    want = N.pad_bias_rows(bias.masked_fill(blocked, float('-inf')))
    assert torch.equal(buf, want) and blocked.any() and buf[2, 5] == float('-inf')


def test_learning_without_a_bias_starts_from_zeros():
    m = _model(learn_label_bias=True)
    assert torch.equal(m.decoder.label_bias.detach(), torch.zeros(L, L))
    assert torch.equal(m.decoder.label_bias_f32, torch.zeros(L, 8))
    masked = _model(learn_label_bias=True, label_mask='inveye')
    assert torch.equal(masked.decoder.label_bias.detach(), torch.zeros(L, L))        # the parameter stays finite under the mask
    assert torch.equal(torch.isinf(masked.decoder.label_bias_f32[:, :L]), torch.eye(L) == 0)


def test_the_existing_refusals_apply():
    ok = torch.zeros(L, L)
    for kw in (dict(label_bias=ok), dict()):
        with pytest.raises(ValueError):
            _model(learn_label_bias=True, no_dec_self_att=True, **kw)
        with pytest.raises(NotImplementedError):
            _model(learn_label_bias=True, dec_attn_type='sigmoid', **kw)
        with pytest.raises(NotImplementedError):
            _model(learn_label_bias=True, decoder='mlp', encoder='mlp', **kw)
    with pytest.raises(ValueError):
        _model(learn_label_bias=True, label_bias=torch.full((L, L), float('nan')))
    with pytest.raises(ValueError):
        _model(learn_label_bias=True, label_bias=torch.zeros(L, L - 1))


def test_state_dict_round_trip_and_a_checkpoint_without_the_key():
    g = torch.Generator().manual_seed(3)
    a = _model(label_bias=torch.randn(L, L, generator=g), learn_label_bias=True)
    b = _model(learn_label_bias=True)
    b.load_state_dict(a.state_dict())
    assert torch.equal(b.decoder.label_bias.detach(), a.decoder.label_bias.detach())
    # a constant-bias (or bias-free) checkpoint loads strictly; the learnable model keeps the bias it was built with
    before = a.decoder.label_bias.detach().clone()
    a.load_state_dict(_model().state_dict())
    assert torch.equal(a.decoder.label_bias.detach(), before)
    with pytest.raises(RuntimeError, match='label_bias'):                              # the other way round the key is unexpected
        _model().load_state_dict(b.state_dict())


# ------------------------------------------------------------------ runners
def test_run_train_flag_name_settings_and_run_eval_detection(tmp_path):
    from lamp_amd import run_eval, run_train
    base = ['-data', 'x.pt', '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2']
    off = run_train.parse(base)
    on = run_train.parse(base + ['-learn_label_bias'])
    both = run_train.parse(base + ['-learn_label_bias', '-label_bias', 'logp', '-label_bias_scale', '0.5'])
    assert off.learn_label_bias is False and on.learn_label_bias is True and on.label_bias == 'none'
    assert '.lbias' not in off.model_name
    assert on.model_name == off.model_name + '.lbias_learn'
    assert both.model_name == off.model_name + '.lbias_logp_0.5.lbias_learn'
    assert run_train.parse(base + ['-learn_label_bias', '-name', 'x']).model_name == off.model_name + '.lbias_learn.x'
    # with the flag off the settings are what they were before it existed
    s_off, s_on = run_train.checkpoint_settings(off), run_train.checkpoint_settings(both)
    assert 'learn_label_bias' not in vars(s_off) and s_on.learn_label_bias is True and s_on.label_bias == 'logp'
    assert set(vars(s_on)) - set(vars(s_off)) == {'learn_label_bias'}
    ns = argparse.Namespace(**{k: v for k, v in vars(run_train.parse(base)).items() if k != 'learn_label_bias'})
    assert run_train.derive(ns).learn_label_bias is False                               # an older caller's namespace
    sd = {'w': torch.zeros(1)}
    learned = {'w': torch.zeros(1), 'decoder.label_bias': torch.zeros(2, 2)}
    wrapped = {'module.' + k: v for k, v in learned.items()}
    for name, ckpt, want in (('on', {'model': sd, 'settings': s_on}, True),
                             ('off', {'model': sd, 'settings': s_off}, False),
                             ('key', {'model': learned, 'settings': argparse.Namespace()}, True),
                             ('bare', sd, False), ('bare_learned', learned, True), ('bare_wrapped', wrapped, True)):
        path = str(tmp_path / (name + '.chkpt'))
        torch.save(ckpt, path)
        assert run_eval.load_checkpoint_learn_label_bias(run_eval.load_checkpoint_object(path)) is want, name
    assert run_eval.load_checkpoint_learn_label_bias(None) is False


# ------------------------------------------------------------------ C ABI
def test_header_prototypes_and_library_symbols_agree():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(lamp_[a-z0-9_]+)\s*\(', text))
    assert set(N.PROTOTYPES) == declared and set(NEW_SYMBOLS) <= declared
    lib = N.lib()
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.argtypes == N.PROTOTYPES[name][1] and fn.restype is N.PROTOTYPES[name][0]
    assert lib.lamp_version() == 5 and ctypes.sizeof(N.Mask) == 56 and ctypes.sizeof(N.Model) == 152


def test_argument_errors_come_back_before_any_launch():
    """Dummy pointers, no device: every status below is produced by the host-side checks."""
    lib = N.lib()
    E_DIMS, E_WORKSPACE, E_NULL = -1, -3, -5
    assert [lib.lamp_strerror(e) is not None for e in (E_DIMS, E_WORKSPACE, E_NULL)] == [True] * 3
    need = lib.lamp_attn_bias_bwd_workspace_bytes(130, 90, 90)
    assert need == lib.lamp_colsum_workspace_bytes(130, 90 * 90) == 3 * 90 * 90 * 4        # the column sum's first stage
    assert lib.lamp_attn_bias_bwd_workspace_bytes(64, 24, 24) == 24 * 24 * 4
    assert lib.lamp_attn_bias_bwd_workspace_bytes(0, 24, 24) == 0

    def bwd(dS=16, n=8, lq=5, lk=6, bias=16, stride=8, dbias=16, ld=6, ws=16, nb=1 << 20):
        return lib.lamp_attn_bias_bwd(dS, n, lq, lk, 2.0, bias, stride, dbias, ld, ws, nb, None)
    for bad in (dict(n=0), dict(lq=0), dict(lk=-1), dict(ld=5), dict(stride=5)):
        assert bwd(**bad) == E_DIMS, bad
    assert bwd(dS=None, ld=5) == E_DIMS                                                     # dimensions are checked first
    for bad in (dict(dS=None), dict(dbias=None), dict(ws=None)):
        assert bwd(**bad) == E_NULL, bad
    assert bwd(nb=lib.lamp_attn_bias_bwd_workspace_bytes(8, 5, 6) - 1) == E_WORKSPACE
    assert bwd(ws=None, nb=0) == E_NULL                                                     # ... and NULL before the size

    def fold(param=16, ld_p=7, blocked=16, n=7, out=16):
        return lib.lamp_label_bias_fold(param, ld_p, blocked, n, out, None)
    for bad in (dict(n=0), dict(n=-3), dict(ld_p=6)):
        assert fold(**bad) == E_DIMS, bad
    for bad in (dict(param=None), dict(out=None)):
        assert fold(**bad) == E_NULL, bad


def test_error_codes_are_the_headers():
    text = open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read()
    for name, value in (('LAMP_E_DIMS', -1), ('LAMP_E_WORKSPACE', -3), ('LAMP_E_NULL', -5)):
        assert re.search(r'%s\s*=\s*%d\b' % (name, value), text), name


# ------------------------------------------------------------------ the kernels' resource report
def test_the_two_kernels_use_neither_scratch_nor_agprs():
    from lamp_amd import build as B
    assert 'backward.hip' in B.SOURCES
    res = {k.split('::')[-1]: r for k, r in B.kernel_resources('backward.hip').items()}
    for name in ('attn_bias_bwd_reduce_kernel', 'label_bias_fold_kernel'):
        assert name in res, sorted(res)
        r = res[name]
        assert r['scratch'] == 0 and r['agpr'] == 0 and r['lds'] == 0 and r['vgpr'] <= 64, (name, r)
    assert res['colsum_partial_kernel']['scratch'] == 0                                     # the first stage, as it stands
