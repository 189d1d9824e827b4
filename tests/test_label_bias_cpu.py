"""The weighted label graph (LAMP(label_bias=...), lamp_mask kind LAMP_MASK_BIAS_F32) without a GPU: co-occurrence statistics,
constructors, the runners' flags, the host-side argument checks of the C ABI and the new kernel's resource report."""
import argparse
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from label_bias_common import bias_sdpa, brute_counts, toy_split

from lamp_amd import _native as N
from lamp_amd import data as D


# ------------------------------------------------------------------ statistics
def test_cooccurrence_counts_against_a_brute_force_count():
    rows, n_dict = toy_split()
    L = n_dict - 4
    assert len(rows) == 40 and L == 11
    want = brute_counts(rows, L)
    assert want[1, 5] >= 1 and want[L - 1].sum() == 0 and want[:, L - 1].sum() == 0   # the never-occurring label
    hot = D.label_multihot_t(rows, n_dict)          # the host-side half of label_cooccurrence (the product is the library's)
    assert hot.shape == (L, 40) and hot.dtype == torch.float32 and set(hot.unique().tolist()) <= {0.0, 1.0}
    assert hot[:, 7].sum() == 0                      # the empty sample
    assert hot[:, 3].tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0]   # the duplicated label counts once
    assert torch.equal(hot @ hot.t(), want)
    assert D.label_multihot_t(rows[:5], n_dict).shape == (L, 8)     # samples padded to a multiple of 4 with zero columns
    with pytest.raises(RuntimeError, match='HIP device only'):
        D.label_cooccurrence(rows, n_dict, None)


def test_bias_from_counts():
    rows, n_dict = toy_split()
    L = n_dict - 4
    C = brute_counts(rows, L)
    adj = D.label_bias_from_counts(C, 'adj', 0.5)
    want_adj = D.prior_adjacency(rows, n_dict)
    assert torch.equal(adj, 0.5 * want_adj) and adj[L - 1, L - 1] == 0.5
    logp = D.label_bias_from_counts(C, 'logp', 2.0)
    for i in range(L):
        for j in range(L):
            want = 0.0 if i == j else 2.0 * float(torch.log((C[i, j] + 1) / (C[i, i] + 1)))
            assert abs(float(logp[i, j]) - want) <= 1e-6
    assert torch.isfinite(logp).all() and (logp <= 0).all() and not torch.equal(logp, logp.t())
    assert torch.equal(D.label_bias_from_counts(C, 'logp'), 0.5 * logp)
    with pytest.raises(ValueError):
        D.label_bias_from_counts(C, 'cosine', 1.0)


def test_restatement_blocks_exactly_like_a_mask():
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(2, 5, 8, generator=g, dtype=torch.float64) for _ in range(3))
    blocked = torch.rand(2, 5, 5, generator=g) < 0.4
    blocked[:, :, 0] = False
    from oracle import lamp_ref as R
    o_m, p_m = R.sdpa(q, k, v, blocked)
    o_b, p_b = bias_sdpa(q, k, v, torch.zeros(5, 5).masked_fill(blocked[0], float('-inf')).expand(1, 5, 5), None)
    assert torch.equal(p_b[0], p_m[0]) and torch.equal(o_b[0], o_m[0])
    w = torch.rand(5, 5, generator=g, dtype=torch.float64) + 0.1
    _, p_w = bias_sdpa(q, k, v, torch.log(w))
    _, p0 = bias_sdpa(q, k, v)
    ref = w * p0 / (w * p0).sum(dim=2, keepdim=True)          # softmax(s + log w) = w exp(s) / sum w exp(s)
    assert (p_w - ref).abs().max().item() <= 1e-14


# ------------------------------------------------------------------ construction
def _model(**kw):
    from lamp_amd.Models import LAMP
    args = dict(n_layers_enc=2, n_layers_dec=2, n_head=2, n_head2=2, d_word_vec=16, d_model=16, d_inner_hid=32, d_k=8, d_v=8,
                encoder='graph', decoder='graph', label_mask='none')
    args.update(kw)
    return LAMP(30, 7, 12, 7, **args)


def test_construction_errors():
    ok = torch.zeros(7, 7)
    for bad in (torch.full((7, 7), float('nan')), ok.clone().index_put_((torch.tensor([1]), torch.tensor([2])), torch.tensor(float('inf')))):
        with pytest.raises(ValueError):
            _model(label_bias=bad)
    for bad in (torch.zeros(7, 6), torch.zeros(1, 7, 7), torch.zeros(7, 7, dtype=torch.long)):
        with pytest.raises(ValueError):
            _model(label_bias=bad)
    with pytest.raises(ValueError):
        _model(label_bias=ok, no_dec_self_att=True)
    with pytest.raises(NotImplementedError):
        _model(label_bias=ok, dec_attn_type='sigmoid')
    with pytest.raises(NotImplementedError):
        _model(label_bias=ok, decoder='mlp', encoder='mlp')
    _model(label_bias=ok.masked_fill(torch.eye(7) == 0, float('-inf')))     # -inf is allowed


def test_buffer_layout_state_dict_and_descriptor():
    g = torch.Generator().manual_seed(1)
    bias = torch.randn(7, 7, generator=g)
    adj = (torch.rand(7, 7, generator=g) < 0.4).float()
    adj = ((adj + adj.t()) > 0).float()
    adj[3, :] = 0
    adj[:, 3] = 0                                        # an isolated label still sees itself (build_label_mask)
    plain, m = _model(), _model(label_bias=bias, label_adj_matrix=adj.clone(), label_mask='prior')
    assert list(m.state_dict()) == list(plain.state_dict())
    assert plain.decoder.label_bias_f32 is None
    buf = m.decoder.label_bias_f32
    assert buf.dtype == torch.float32 and tuple(buf.shape) == (7, 8) and buf.size(1) % 4 == 0
    blocked = m.decoder.label_mask_u8 != 0
    assert blocked.any() and not blocked[3, 3]
    assert (buf[:, :7][blocked] == float('-inf')).all() and torch.equal(buf[:, :7][~blocked], bias[~blocked])
    assert 'label_bias_f32' in dict(m.decoder.named_buffers())
    # the descriptor needs a device pointer; its fields are checked on a stand-in
    with pytest.raises(RuntimeError, match='HIP device only'):
        m.decoder.label_mask_struct()
    import unittest.mock as mock
    with mock.patch.object(N, 'require_device', lambda *a: None):
        ms = m.decoder.label_mask_struct()
    assert ms.kind == N.LAMP_MASK_BIAS_F32 == 4 and ms.flags == 0 and not ms.tile_list and ms.tile_list_stride == 0
    assert ms.stride_b == 0 and ms.stride_q == 8 and ms.ptr == buf.data_ptr() and ms.allowed_pairs == 0
    none = _model(label_bias=bias)                       # label_mask='none': the bias alone
    assert torch.equal(none.decoder.label_bias_f32[:, :7], bias) and none.decoder.label_mask_u8 is None


def test_make_mask_keeps_the_reference_float_format():
    import inspect
    import unittest.mock as mock
    with mock.patch.object(N, 'require_device', lambda *a: None):     # a float tensor stays "nonzero = blocked": a byte mask
        ms, m8 = N.make_mask(torch.tensor([[0.0, -2.5, 0.0], [1.0, 0.0, 0.0]]), 1, 2, 3)
    assert ms.kind == N.LAMP_MASK_U8 and m8.dtype == torch.uint8 and m8.view(2, 3).tolist() == [[0, 1, 0], [1, 0, 0]]
    assert inspect.signature(N.make_bias_mask).parameters.keys() == {'bias', 'B', 'lq', 'lk'}
    with pytest.raises(RuntimeError, match='HIP device only'):
        N.make_bias_mask(torch.zeros(3, 5), 1, 3, 5)
    p = N.pad_bias_rows(torch.ones(2, 3, 5))
    assert tuple(p.shape) == (2, 3, 8) and p.is_contiguous() and (p[..., 5:] == 0).all() and (p[..., :5] == 1).all()


# ------------------------------------------------------------------ runners
def test_run_train_flags_name_and_checkpoint_settings_round_trip(tmp_path):
    from lamp_amd import run_eval, run_train
    base = ['-data', 'x.pt', '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-n_layers_enc', '2']
    off = run_train.parse(base)
    on = run_train.parse(base + ['-label_bias', 'logp', '-label_bias_scale', '0.5'])
    assert off.label_bias == 'none' and off.label_bias_scale == 1.0 and '.lbias' not in off.model_name
    assert on.label_bias == 'logp' and on.label_bias_scale == 0.5
    assert on.model_name == off.model_name + '.lbias_logp_0.5'
    assert run_train.parse(base + ['-label_bias', 'adj']).model_name == off.model_name + '.lbias_adj_1.0'
    with pytest.raises(SystemExit):
        run_train.parse(base + ['-label_bias', 'cosine'])
    ns = argparse.Namespace(**{k: v for k, v in vars(run_train.parse(base)).items() if not k.startswith('label_bias')})
    d = run_train.derive(ns)
    assert d.label_bias == 'none' and d.label_bias_scale == 1.0
    sd = {'w': torch.zeros(1)}
    for name, ckpt, want in (('on', {'model': sd, 'settings': run_train.checkpoint_settings(on)}, ('logp', 0.5)),
                             ('off', {'model': sd, 'settings': run_train.checkpoint_settings(off)}, ('none', 1.0)),
                             ('absent', {'model': sd, 'settings': argparse.Namespace(enc_self_att=True)}, None),
                             ('bare', sd, None)):
        path = str(tmp_path / (name + '.chkpt'))
        torch.save(ckpt, path)
        assert run_eval.load_checkpoint_label_bias(run_eval.load_checkpoint_object(path)) == want
        assert len(run_eval.load_checkpoint_settings(path)) == 3          # still the 3-tuple its callers unpack
    e = run_eval.parse(['-data', 'x.pt', '-label_bias', 'adj', '-label_bias_scale', '2'])
    assert e.label_bias == 'adj' and e.label_bias_scale == 2.0 and run_eval.parse(['-data', 'x.pt']).label_bias == 'none'
    data = {'train': {'tgt': toy_split()[0]}, 'dict': {'tgt': list(range(toy_split()[1]))}}
    assert D.build_label_bias(data, 'none', 1.0, None) is None


# ------------------------------------------------------------------ C ABI: constants and host-side argument checks
def test_header_and_ctypes_agree_and_the_abi_did_not_move():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read(), flags=re.S)
    assert re.search(r'LAMP_MASK_BIAS_F32 = 4\b', text) and N.LAMP_MASK_BIAS_F32 == 4
    assert re.search(r'#define LAMP_FWD_LABEL_BIAS 16\b', text) and N.LAMP_FWD_LABEL_BIAS == 16
    assert N.lib().lamp_version() == 5 and ctypes.sizeof(N.Mask) == 56 and ctypes.sizeof(N.Model) == 152
    declared = set(re.findall(r'\b(lamp_[a-z0-9_]+)\s*\(', text))
    assert set(N.PROTOTYPES) == declared


def _sdpa_status(mask, act=None, attn=None):
    lib = N.lib()
    lay = N.AttnLayout(*([4] * 12))
    args = (16, 16, 16, 16, attn, 1, 1, 4, 4, 8, 8, 1.0)
    if act is None:
        return lib.lamp_sdpa_fwd(*args, ctypes.byref(mask), ctypes.byref(lay), None)
    return lib.lamp_sdpa_act_fwd(*args, act, ctypes.byref(mask), ctypes.byref(lay), None)


def test_argument_errors_come_back_before_any_launch():
    """Dummy pointers, no device: every status below is produced by the host-side checks."""
    K = N.LAMP_MASK_BIAS_F32
    assert _sdpa_status(N.Mask(K, 0, 16, 0, 6, None, 0, 0)) == -2             # stride_q % 4
    assert _sdpa_status(N.Mask(K, 0, 16, 6, 4, None, 0, 0)) == -2             # stride_b % 4
    assert _sdpa_status(N.Mask(K, 0, 24, 0, 4, None, 0, 0)) == -2             # pointer not 16-byte aligned
    assert _sdpa_status(N.Mask(K, 0, None, 0, 4, None, 0, 0)) == -5
    assert _sdpa_status(N.Mask(K, 0, 16, 0, 4, None, 0, 0), act=N.LAMP_ATTN_SIGMOID) == -4
    assert _sdpa_status(N.Mask(K, 0, 16, 0, 4, 16, 2, 0)) == -4               # a tile list
    assert _sdpa_status(N.Mask(K, 0, 16, 0, 4, 16, 2, 0), attn=16) == -4      # ... also where maps would make the kernel ignore it
    assert _sdpa_status(N.Mask(K, N.LAMP_MASK_SPARSE_ROWS, 16, 0, 4, None, 0, 0)) == -4
    assert _sdpa_status(N.Mask(K, N.LAMP_MASK_SELF_RAGGED, 16, 0, 4, None, 0, 0)) == -4
    assert _sdpa_status(N.Mask(5, 0, 16, 0, 4, None, 0, 0)) == -4             # there is no kind 5
    lib = N.lib()
    w = N.MhaWeights(16, 16, 16, 16, 16, 16, 2, 1)
    st = lib.lamp_mha_act_fwd(16, 16, 1, 4, 4, 32, 16, 16, ctypes.byref(w), N.LAMP_ATTN_SIGMOID,
                              ctypes.byref(N.Mask(K, 0, 16, 0, 4, None, 0, 0)), 16, None, 16, 1 << 20, None)
    assert st == -4
    st = lib.lamp_mha_fwd(16, 16, 1, 4, 4, 32, 16, 16, ctypes.byref(w), ctypes.byref(N.Mask(K, 0, 16, 0, 5, None, 0, 0)), 16, None,
                          16, 1 << 20, None)
    assert st == -2


def dummy_model(L, d, dff, h, n_enc, n_dec):
    """A lamp_model struct whose pointers are dummies: enough for the argument checks, which launch nothing."""
    enc = (N.EncLayer * max(1, n_enc))(*[N.EncLayer(N.MhaWeights(16, 16, 16, 16, 16, 16, h, 1)) for _ in range(n_enc)])
    dec = (N.DecLayer * n_dec)(*[N.DecLayer(N.MhaWeights(16, 16, 16, 16, 16, 16, h, 1), N.FfnWeights(),
                                            N.MhaWeights(16, 16, 16, 16, 16, 16, h, 1)) for _ in range(n_dec)])
    m = N.Model(1000, 1001, L, d, dff, d // h, d // h, n_enc, n_dec, 0, 16, 16, 16, 16, 0, 0, 0, enc, dec)
    return m, (enc, dec)


def test_forward_flag_is_checked_before_any_launch():
    lib = N.lib()
    m, keep = dummy_model(8, 32, 64, 2, 1, 1)
    ws_plain = lib.lamp_forward_workspace_bytes(ctypes.byref(m), 2, 8, 0)
    opts = N.FwdOptions(0, N.LAMP_FWD_LABEL_BIAS, None, None)
    assert lib.lamp_forward_opts_workspace_bytes(ctypes.byref(m), ctypes.byref(opts), 2, 8, 0) == ws_plain > 0

    def status(flags, **fields):
        mm, kp = dummy_model(8, 32, 64, 2, 1, 1)
        mm.label_mask = 16
        for k, v in fields.items():
            setattr(mm, k, v)
        o = N.FwdOptions(0, flags, None, None)
        return lib.lamp_forward_opts(ctypes.byref(mm), ctypes.byref(o), 16, 16, 1, 8, 16, 16, None, 16, 1 << 30, None)
    F = N.LAMP_FWD_LABEL_BIAS
    assert status(F | N.LAMP_FWD_DEC_SIGMOID) == -4
    assert status(F, label_mask_bits=16) == -4
    assert status(F, label_tiles=16) == -4
    assert status(F, label_mask_flags=N.LAMP_MASK_SPARSE_ROWS) == -4
    assert status(F, label_mask_allowed=5) == -4
    assert status(F, label_mask=24) == -2


# ------------------------------------------------------------------ the kernel's resource report
def test_the_bias_kernel_has_no_scratch_in_any_instantiation():
    from lamp_amd import build as B
    assert 'attention_bias.hip' in B.SOURCES
    res = B.kernel_resources('attention_bias.hip')
    kernels = {k: r for k, r in res.items() if 'attn_bias_kernel' in k}
    assert len(kernels) == 9, sorted(res)                      # 3 head widths x 3 output modes
    for name, r in kernels.items():
        assert r['scratch'] == 0 and r['vgpr'] <= 256 and r['occupancy'] >= 2, (name, r)
