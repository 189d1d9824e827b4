"""CPU-side checks of the imbalanced-label losses (lamp_multilabel_loss_train): the fp64 reference the
GPU tests compare against reduces to the losses it generalises and its closed-form gradients equal autograd; label_pos_weight
against a numpy count; run_train's flags, results name and checkpoint settings; the wrapper's refusals, raised without a
device; the ABI bookkeeping.  Nothing here needs a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

from lamp_amd import _native as N
from lamp_amd import data as D
from lamp_amd import run_train as RT
from lamp_amd import train as T

import imbalance_loss_common as IC
import train_common as TC


def _case(B=6, L=41, seed=0, span=6.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, L, generator=g, dtype=torch.float64) * span).clamp(-30.0, 30.0)
    t = (torch.rand(B, L, generator=g) < 0.2).double()
    w = torch.exp(torch.randn(L, generator=g, dtype=torch.float64))
    return x, t, w


# ------------------------------------------------------------------ the reference itself
def test_reference_reduces_to_bce_focal_and_pos_weight_bce():
    x, t, w = _case()
    bce = F.binary_cross_entropy_with_logits(x, t, reduction='none')
    assert float((IC.loss_elements(x, t) - bce).abs().max()) < 1e-13
    bce_w = F.binary_cross_entropy_with_logits(x, t, reduction='none', pos_weight=w)
    assert float((IC.loss_elements(x, t, pos_weight=w) - bce_w).abs().max()) < 1e-12
    # focal loss written out (Lin et al. 2017, alpha through w = alpha / (1 - alpha)): -(1 - p_t)^gamma log p_t
    for gamma in (1.0, 2.0, 5.0):
        s = torch.sigmoid(x)
        p_t = torch.where(t > 0, s, 1.0 - s)
        log_p_t = torch.where(t > 0, F.logsigmoid(x), F.logsigmoid(-x))
        focal = -(1.0 - p_t) ** gamma * log_p_t
        assert float((IC.loss_elements(x, t, gamma, gamma) - focal).abs().max()) < 1e-12, gamma
    # the margin discards a negative predicted below it outright, and shifts the others
    el = IC.loss_elements(x, torch.zeros_like(x), 0.0, 4.0, 0.05)
    s = torch.sigmoid(x)
    assert bool((el[s <= 0.05] == 0).all()) and bool((el[s > 0.06] > 0).all())
    # a soft target mixes the two branches as written
    soft = torch.full_like(x, 0.3)
    mixed = 0.3 * IC.loss_elements(x, torch.ones_like(x), 1.0, 4.0, 0.05, w) + 0.7 * IC.loss_elements(x, torch.zeros_like(x), 1.0, 4.0, 0.05, w)
    assert float((IC.loss_elements(x, soft, 1.0, 4.0, 0.05, w) - mixed).abs().max()) < 1e-12


@pytest.mark.parametrize('name', sorted(IC.PARAM_SETS))
def test_closed_form_gradients_equal_autograd(name):
    gp, gn, m, has_w = IC.PARAM_SETS[name]
    x, t, w = _case(seed=3)
    if m > 0:       # (away from the kink of max(s - m, 0), where autograd's subgradient is a convention)
        edge = float(np.log(m / (1 - m)))
        x = torch.where((x - edge).abs() < 1e-3, torch.full_like(x, edge + 2e-3), x)
    t[0] = 0.3                                         # a row of soft targets
    x = x.requires_grad_(True)
    IC.loss_elements(x, t, gp, gn, m, w if has_w else None).sum().backward()
    closed = IC.closed_form_gradient(x.detach(), t, gp, gn, m, w if has_w else None)
    err = float((closed - x.grad).abs().max())
    print('%s: closed form vs fp64 autograd %.3e' % (name, err))
    assert err < 1e-12


def test_reference_is_finite_at_the_planted_logits_in_both_precisions():
    """The kernel test's inputs (0, +-30, +-88, +-104, +-1e4 among them) give no NaN or inf in the fp64 reference nor in its
    fp32 evaluation, the yardstick: otherwise the GPU comparison would compare nothing there."""
    for name, (gp, gn, m, has_w) in IC.PARAM_SETS.items():
        logits, weights, targets, pw = IC.loss_case(4, 65, 3, seed=4065, clip=m)
        for dtype in (torch.float64, torch.float32):
            p, g, r = IC.loss_reference(logits, weights, targets, gp, gn, m, pw if has_w else None, dtype)
            assert all(bool(torch.isfinite(a).all()) for a in [p, r] + g), (name, dtype)
        assert any(float(v) in (1e4, -1e4) for v in logits[0].flatten())


# ------------------------------------------------------------------ label_pos_weight
def test_label_pos_weight_against_a_numpy_count():
    data = TC.synthetic_dataset(n_train=57, n_labels=11)
    tgt = [list(s) for s in data['train']['tgt']]
    tgt = [[2] + [v for v in s[1:-1] if v != 4 + 7] + [3] for s in tgt]      # label 7 has no positive
    tgt[0] = tgt[0][:-1] + [tgt[0][1], 3]                                     # a label repeated inside a sample counts once
    n, L = len(tgt), 11
    c = IC.count_labels(tgt, L)
    assert c[7] == 0 and c.max() < n
    raw = (n - c) / np.maximum(c, 1)
    for kind, f in (('inv', lambda v: v), ('sqrt_inv', np.sqrt)):
        for cap in (100.0, 3.0):
            w = D.label_pos_weight(tgt, L + 4, 'cpu', kind, cap)
            assert w.dtype == torch.float32 and tuple(w.shape) == (L,) and w.is_contiguous()
            want = np.where(c > 0, np.minimum(f(raw), cap), cap).astype(np.float32)
            assert np.array_equal(w.numpy(), want), (kind, cap)
            assert float(w[7]) == cap
    assert bool((D.label_pos_weight(tgt, L + 4, 'cpu', 'inv', 3.0) == 3.0).any())      # the cap binds somewhere
    assert D.label_pos_weight(tgt, L + 4, 'cpu').tolist() == D.label_pos_weight(tgt, L + 4, 'cpu', 'inv', 100.0).tolist()
    with pytest.raises(ValueError):
        D.label_pos_weight(tgt, L + 4, 'cpu', 'log')
    with pytest.raises(ValueError):
        D.label_pos_weight(tgt, L + 4, 'cpu', 'inv', 0.0)


# ------------------------------------------------------------------ run_train's flags
BASE = ['-data', 'x.pt', '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-name', 'n1']
NEW_KEYS = ('loss_fn', 'focal_gamma', 'asl_gamma_pos', 'asl_gamma_neg', 'asl_clip', 'pos_weight', 'pos_weight_cap', 'loss_options')


def test_name_and_settings_are_unchanged_without_the_flags():
    opt = RT.parse(BASE)
    assert opt.loss_fn == 'bce' and opt.pos_weight == 'none' and opt.loss == 'ce'
    assert 'lossfn' not in opt.model_name and 'posw' not in opt.model_name and opt.model_name.endswith('.n1')
    st = RT.checkpoint_settings(opt)
    assert not any(hasattr(st, k) for k in NEW_KEYS)
    opt.loss_options = None                 # as run_train.main leaves it for plain BCE
    st2 = RT.checkpoint_settings(opt)
    assert vars(st2) == vars(st)
    assert RT.loss_parameters(opt) == (0.0, 0.0, 0.0)
    assert RT.build_loss_options(opt, None, 'cpu') is None      # train_batch then calls bce_logits_train as it always did


def test_suffixes_and_settings_with_the_flags():
    plain = RT.parse(BASE).model_name
    opt = RT.parse(BASE + ['-loss_fn', 'asl', '-pos_weight', 'inv'])
    assert opt.model_name == plain[:-len('.n1')] + '.lossfn_asl_0.0_4.0_0.05.posw_inv_100.0.n1'
    st = RT.checkpoint_settings(opt)
    assert (st.loss_fn, st.asl_gamma_pos, st.asl_gamma_neg, st.asl_clip, st.pos_weight, st.pos_weight_cap) == \
        ('asl', 0.0, 4.0, 0.05, 'inv', 100.0)
    assert not hasattr(st, 'focal_gamma') and not hasattr(st, 'loss_options')
    assert all(isinstance(v, (bool, int, float, str, type(None))) for v in vars(st).values())
    assert RT.loss_parameters(opt) == (0.0, 4.0, 0.05)
    opt = RT.parse(BASE + ['-loss_fn', 'focal', '-focal_gamma', '3'])
    assert opt.model_name == plain[:-len('.n1')] + '.lossfn_focal_3.0.n1'
    st = RT.checkpoint_settings(opt)
    assert (st.loss_fn, st.focal_gamma) == ('focal', 3.0)
    assert not any(hasattr(st, k) for k in ('asl_gamma_pos', 'asl_gamma_neg', 'asl_clip', 'pos_weight', 'pos_weight_cap'))
    assert RT.loss_parameters(opt) == (3.0, 3.0, 0.0)
    opt = RT.parse(BASE + ['-pos_weight', 'sqrt_inv', '-pos_weight_cap', '20'])
    assert opt.model_name == plain[:-len('.n1')] + '.posw_sqrt_inv_20.0.n1'
    st = RT.checkpoint_settings(opt)
    assert (st.pos_weight, st.pos_weight_cap) == ('sqrt_inv', 20.0) and not hasattr(st, 'loss_fn')
    # the weights come from the TRAIN split's counts; the object train_batch reads holds them and the three floats
    data = TC.synthetic_dataset(n_train=40)
    lo = RT.build_loss_options(RT.parse(BASE + ['-loss_fn', 'asl', '-pos_weight', 'inv']), data, 'cpu')
    assert isinstance(lo, T.LossOptions) and (lo.gamma_pos, lo.gamma_neg, lo.clip) == (0.0, 4.0, 0.05)
    assert torch.equal(lo.pos_weight, D.label_pos_weight(data['train']['tgt'], len(data['dict']['tgt']), 'cpu', 'inv', 100.0))
    lo = RT.build_loss_options(RT.parse(BASE + ['-loss_fn', 'focal']), data, 'cpu')
    assert (lo.gamma_pos, lo.gamma_neg, lo.clip, lo.pos_weight) == (2.0, 2.0, 0.0, None)
    assert 'valid and test losses stay plain BCE' in _help()       # the flag help says what stays comparable


def _help():
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        RT.parse(['-h'])
    return ' '.join(buf.getvalue().split())


@pytest.mark.parametrize('argv', [
    ['-loss_fn', 'hinge'], ['-pos_weight', 'log'],
    ['-loss_fn', 'focal', '-focal_gamma', '0.5'], ['-loss_fn', 'focal', '-focal_gamma', '17'],
    ['-loss_fn', 'focal', '-focal_gamma', '-1'], ['-loss_fn', 'focal', '-focal_gamma', 'nan'],
    ['-loss_fn', 'asl', '-asl_clip', '1.0'], ['-loss_fn', 'asl', '-asl_clip', '-0.1'],
    ['-loss_fn', 'asl', '-asl_gamma_neg', '0.3'], ['-loss_fn', 'asl', '-asl_gamma_pos', 'inf'],
    ['-pos_weight', 'inv', '-pos_weight_cap', '0'], ['-pos_weight', 'inv', '-pos_weight_cap', 'inf'],
])
def test_flag_validation(argv):
    with pytest.raises((ValueError, SystemExit)):
        RT.parse(BASE + argv)


def test_flags_of_an_objective_that_is_not_chosen_are_not_judged():
    assert RT.parse(BASE + ['-focal_gamma', '0.5']).loss_fn == 'bce'                   # (plain BCE: nothing reads it)
    assert RT.parse(BASE + ['-loss_fn', 'focal', '-focal_gamma', '0']).model_name.endswith('.lossfn_focal_0.0.n1')


# ------------------------------------------------------------------ the wrapper's refusals, without a device
@pytest.mark.parametrize('kw', [
    dict(gamma_pos=0.5), dict(gamma_neg=0.5), dict(gamma_pos=-1.0), dict(gamma_neg=17.0), dict(gamma_pos=float('nan')),
    dict(gamma_neg=float('inf')), dict(clip=1.0), dict(clip=-0.1), dict(clip=float('nan')),
    dict(pos_weight=torch.ones(6)), dict(pos_weight=torch.ones(5, dtype=torch.float64)), dict(pos_weight=torch.ones(5, 1)),
    dict(pos_weight=torch.ones(10)[::2]), dict(pos_weight=[1.0] * 5),
])
def test_wrapper_refuses_parameters_before_it_looks_for_a_device(kw, monkeypatch):
    def no_library():
        raise AssertionError('the library was called')
    monkeypatch.setattr(N, 'lib', no_library)
    x, t = torch.zeros(3, 5), torch.zeros(3, 5)              # CPU tensors: a served request would fail on them later
    with pytest.raises(ValueError):
        N.multilabel_loss_train([x], [1.0], t, **kw)
    if 'pos_weight' not in kw:
        with pytest.raises(ValueError):
            T.LossOptions(**kw)                              # and so does the object train_batch reads, when it is made


def test_wrapper_signature_and_matrix_limit():
    sig = inspect.signature(N.multilabel_loss_train)
    assert list(sig.parameters) == ['logits', 'weights', 'targets', 'gamma_pos', 'gamma_neg', 'clip', 'pos_weight', 'probs_out',
                                    'row_loss_out', 'want_grads', 'want_probs']
    assert [sig.parameters[k].default for k in ('gamma_pos', 'gamma_neg', 'clip', 'pos_weight')] == [0.0, 0.0, 0.0, None]
    x = torch.zeros(3, 5)
    with pytest.raises(ValueError):
        N.multilabel_loss_train([x] * 9, [1.0] * 9, x)        # the entry point takes 8
    with pytest.raises(ValueError):
        N.multilabel_loss_train([x] * 2, [1.0], x)
    assert N.check_loss_options(1, 16, 0) == (1.0, 16.0, 0.0)


# ------------------------------------------------------------------ ABI bookkeeping
def test_header_ctypes_and_library_carry_the_entry_point():
    raw = open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    m = re.search(r'\bint\s+lamp_multilabel_loss_train\s*\(([^)]*)\)', text)
    base = re.search(r'\bint\s+lamp_bce_logits_train\s*\(([^)]*)\)', text)
    assert m and base
    n_args, n_base = len(m.group(1).split(',')), len(base.group(1).split(','))
    assert n_args == n_base + 1 and 'const lamp_loss_options* opts' in m.group(1)
    restype, argtypes = N.PROTOTYPES['lamp_multilabel_loss_train']
    assert restype is ctypes.c_int and len(argtypes) == n_args
    assert argtypes[:-2] == N.PROTOTYPES['lamp_bce_logits_train'][1][:-1] and argtypes[-2] == ctypes.POINTER(N.LossOptions)
    assert 'lamp_multilabel_loss_train' in N.LATE_ENTRY_POINTS              # added without an ABI bump
    body = re.search(r'typedef struct lamp_loss_options \{(.*?)\} lamp_loss_options;', text, flags=re.S).group(1)
    fields = re.findall(r'(\w+)\s*[;,]', body)
    assert fields == [f[0] for f in N.LossOptions._fields_] == ['gamma_pos', 'gamma_neg', 'clip', 'reserved', 'pos_weight']
    assert ctypes.sizeof(N.LossOptions) == 24 and N.LossOptions.pos_weight.offset == 16
    assert re.search(r'#define LAMP_HIP_ABI_VERSION 5\b', raw) and N.ABI_VERSION == 5
    lib = ctypes.CDLL(N.LIB_PATH)
    assert hasattr(lib, 'lamp_multilabel_loss_train') and hasattr(lib, 'lamp_bce_logits_train')
    for rule in ('NaN logit', 'inf logit', "caller's responsibility"):          # the header states the rules
        assert rule in ' '.join(raw.split()), rule
    from lamp_amd import build as B
    kernels = B.kernel_resources('train_step.hip')
    mine = {k: r for k, r in kernels.items() if 'multilabel_loss_train_kernel' in k}
    assert len(mine) == 4, sorted(kernels)             # exponent x margin, specialised at compile time
    for name, r in mine.items():
        assert r.get('scratch', 0) == 0 and r.get('agpr', 0) == 0, (name, r)
