"""The fp64 restatements of tests/conv_common.py (which tests/test_conv_kernels_gpu.py holds csrc/conv.hip against) pinned
without a GPU: against F.embedding / F.conv1d / F.max_pool1d in fp64 and torch.autograd on that composition, the decision
margins of the backward cases against an fp32 restatement, and the argument refusals of the five entry points that
tests/test_onehot_cpu.py does not already assert."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

import conv_common as CC
from onehot_common import onehot_encoder_ref


def _weights(d, V=9, T_max=64, seed=0):
    g = CC.gen(seed)
    sd = {'encoder.src_word_emb.weight': torch.randn(V, V, generator=g, dtype=torch.float64),
          'encoder.conv1.weight': torch.randn(d, V, 16, generator=g, dtype=torch.float64) * 0.3,
          'encoder.conv1.bias': torch.randn(d, generator=g, dtype=torch.float64),
          'encoder.conv2.weight': torch.randn(d, d, 16, generator=g, dtype=torch.float64) * 0.2,
          'encoder.conv2.bias': torch.randn(d, generator=g, dtype=torch.float64),
          'encoder.position_enc.weight': torch.randn(T_max + 1, d, generator=g, dtype=torch.float64)}
    return sd


def _tap_table(sd):
    return torch.einsum('vi,cit->vtc', sd['encoder.src_word_emb.weight'], sd['encoder.conv1.weight']).contiguous()


@pytest.mark.parametrize('T', [2, 3, 17, 40])
def test_front_ref_then_conv_window_ref_is_the_torch_composition(T):
    d, B = 12, 3
    sd = _weights(d)
    seq = CC.tokens(B, T, 9, seed=T)
    pos = torch.randint(0, 65, (B, T), generator=CC.gen(T + 1))
    want, _ = onehot_encoder_ref(sd, seq, pos)          # no encoder layers in sd: cut before the FFN stack
    T2 = T // 2
    xpad = CC.front_ref(seq, _tap_table(sd), sd['encoder.conv1.bias'])
    assert xpad.shape == (B * (T2 + 16) + 16, d)
    w_pack = CC.conv_pack_ref(sd['encoder.conv2.weight'], 0)
    out, act, mag, _ = CC.conv_window_ref(xpad, B, T2, T2 + 16, w_pack, sd['encoder.conv2.bias'], True,
                                          sd['encoder.position_enc.weight'], pos)
    assert want.shape == (B, T2, d)
    err = (out.view(B, T2, d) - want).abs().max() / want.abs().max()
    assert err < 1e-12, err
    assert torch.equal(act, torch.relu(act)) and bool((mag >= act.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('T', [2, 3, 17, 40])
def test_backward_refs_equal_autograd_on_the_torch_composition(T):
    d, B = 12, 3
    T2 = T // 2
    sd = {k: v.clone().requires_grad_(True) for k, v in _weights(d, seed=5).items()}
    seq = CC.tokens(B, T, 9, seed=T + 7)
    x = F.embedding(seq, sd['encoder.src_word_emb.weight']).transpose(1, 2)
    y1 = F.conv1d(x, sd['encoder.conv1.weight'], sd['encoder.conv1.bias'], padding=8)[:, :, :-1]
    y1.retain_grad()
    P = F.max_pool1d(F.relu(y1), 2, 2)
    P.retain_grad()
    X = F.relu(F.conv1d(P, sd['encoder.conv2.weight'], sd['encoder.conv2.bias'], padding=8).transpose(1, 2))[:, :-1, :]
    G = torch.randn(B, T2, d, generator=CC.gen(3), dtype=torch.float64)
    (X * G).sum().backward()
    w2 = sd['encoder.conv2.weight'].detach()
    dP, mag = CC.conv_input_grad_ref(G.view(B * T2, d), X.detach().reshape(B * T2, d), w2, B, T2)
    want_dP = P.grad.transpose(1, 2)
    assert (dP.view(B, T2, d) - want_dP).abs().max() <= 1e-12 * max(1.0, float(want_dP.abs().max()))
    assert bool((mag >= dP.abs() * (1 - 1e-12)).all())
    # the same gradient as the library composes it: conv_window over the padded dZ from its second row, flipped repack
    dzp = CC.relu_bwd_pad_ref(G.view(B * T2, d), X.detach().reshape(B * T2, d), B, T2)
    via, _, _, _ = CC.conv_window_ref(dzp[1:], B, T2, T2 + 16, CC.conv_pack_ref(w2, 1))
    assert (via - dP).abs().max() <= 1e-12 * max(1.0, float(dP.abs().max()))
    t1 = _tap_table(sd).detach()
    r = CC.front_bwd_ref(seq, t1, sd['encoder.conv1.bias'].detach(), want_dP.detach().contiguous())
    want_dz = y1.grad.transpose(1, 2)
    assert torch.equal(r['dz'], want_dz)
    # t1 = E x conv1_w: its gradient folds back onto conv1's weight
    dw1 = torch.einsum('vi,vtc->cit', sd['encoder.src_word_emb.weight'].detach(), r['dt1'])
    want = sd['encoder.conv1.weight'].grad
    assert (dw1 - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max()))
    assert (r['dz'].sum((0, 1)) - sd['encoder.conv1.bias'].grad).abs().max() <= 1e-12 * max(1.0, float(want_dz.abs().max()) * B * T)
    assert not r['unsafe'].any()


def test_front_ref_dropout_nan_and_ties():
    V, T, d = 9, 40, 8
    t1, b1 = (a.double() for a in CC.front_weights(V, d, seed=1))
    seq = CC.tokens(2, T, V, seed=2)
    keep = torch.rand(2, T, d, generator=CC.gen(3)) < 0.5
    y = F.conv1d(F.one_hot(seq, V).double().transpose(1, 2), t1.permute(2, 0, 1).contiguous(), b1, padding=8)[:, :, :-1]
    want = F.max_pool1d(F.relu(y * keep.transpose(1, 2) * 2.0), 2, 2).transpose(1, 2)
    got = CC.front_pairs(seq, t1, b1, keep, 2.0)['P']
    assert (got - want).abs().max() < 1e-12
    # an invalid token poisons exactly the positions whose window holds it: p - 8 <= j <= p + 7
    seq[0, 20] = V
    y1, _, _ = CC.front_y1(seq, t1, b1)
    bad = torch.isnan(y1).all(-1)
    assert torch.equal(bad[0], (torch.arange(T) >= 13) & (torch.arange(T) <= 28)) and not bad[1].any()
    assert torch.equal(torch.isnan(y1).any(-1), bad)
    # constant sequences: interior pairs tie exactly and the pooled value is that common value
    seq, t1c, b1c, _ = CC.constant_case()
    fp = CC.front_pairs(seq, t1c.double(), b1c.double())
    q = torch.arange(4, (T - 8) // 2)
    assert torch.equal(fp['z0'][:, q], fp['z1'][:, q]) and bool(fp['same'][:, q].all())
    assert torch.equal(fp['P'][:, q], CC.relu_nan(fp['z0'][:, q]))
    assert not fp['same'][:, :4].any()


def test_pairwise_cover_of_the_front_end_shapes():
    cases = CC.pairwise_front_cases()
    for i, j in itertools.combinations(range(4), 2):
        assert {(c[i], c[j]) for c in cases} == set(itertools.product(CC.FRONT_AXES[i], CC.FRONT_AXES[j]))


def _bwd_margin_check(seq, t1, b1, dP, keep, scale, ties_stay):
    r = CC.front_bwd_ref(seq, t1.double(), b1.double(), dP.double(), keep, scale)
    f = CC.front_bwd_fp32(seq, t1, b1, dP, keep, scale)
    share = float(r['unsafe'].double().mean())
    assert share <= 0.01, share
    safe = ~r['unsafe']
    assert torch.equal(f[safe], r['dz'].float()[safe])
    if ties_stay is not None:
        assert not r['unsafe'][:, ties_stay].any()
    return r, share


@pytest.mark.parametrize('case', CC.BWD_CASES, ids=CC.bwd_case_id)
def test_backward_cases_keep_their_decisions_in_fp32(case):
    """The seeds of the GPU cases: at most 1 % of the elements sit within twice the a-priori bound of a decision boundary (none
    in fact, which the dt1 comparison relies on), and outside them an fp32 evaluation decides as the fp64 one does."""
    seq, t1, b1, dP, p, keep, scale = CC.front_bwd_case(case)
    r, share = _bwd_margin_check(seq, t1, b1, dP, keep, scale, None)
    assert share == 0.0
    if p:
        assert 0.4 < float(keep.double().mean()) < 0.6


def test_constant_and_invalid_cases_keep_their_decisions_in_fp32():
    seq, t1, b1, dP = CC.constant_case()
    T = seq.size(1)
    interior = torch.arange(8, T - 8)
    r, share = _bwd_margin_check(seq, t1, b1, dP, None, 1, interior)
    assert share == 0.0
    # the whole gradient goes to the first element of a tied positive pair, none where the pooled value is 0
    P = r['pairs']['P'][:, 4:(T - 8) // 2]
    first, second = r['dz'][:, 8:T - 8:2], r['dz'][:, 9:T - 8:2]
    assert torch.equal(first, torch.where(P > 0, dP.double()[:, 4:(T - 8) // 2], torch.zeros_like(P)))
    assert not second.any() and bool((P > 0).any()) and bool((P == 0).any())
    seq, t1, b1, dP = CC.invalid_case()
    r, share = _bwd_margin_check(seq, t1, b1, dP, None, 1, None)
    assert share == 0.0 and bool(torch.isfinite(r['dz']).all()) and bool(torch.isfinite(r['dt1']).all())


@pytest.mark.parametrize('B,rows_out,c_in,c_out', [(1, 1, 4, 4), (2, 5, 8, 36), (2, 64, 64, 128), (3, 43, 12, 132), (1, 130, 160, 260)])
def test_the_bound_tells_one_dropped_term(B, rows_out, c_in, c_out):
    """The a-priori bound is loose against typical rounding, yet at every conv_window shape of the GPU file a sum that
    leaves out one product (tap 7, channel 0), or counts it twice, misses it."""
    rows_in = rows_out + 16
    x = CC.f32_randn(B * rows_in, c_in, seed=1).double()
    w = CC.f32_randn(c_out, 16, c_in, seed=2, scale=(16 * c_in) ** -0.5).double()
    _, _, mag, _ = CC.conv_window_ref(x, B, rows_out, rows_in, w)
    m = torch.arange(B * rows_out)
    term = (x[(m // rows_out) * rows_in + m % rows_out + 7, 0][:, None] * w[None, :, 7, 0]).abs()
    assert float((term / CC.sum_bound(16 * c_in, mag)).max()) > 1.0


def test_selection_refs():
    w = torch.arange(5 * 12 * 16, dtype=torch.float32).view(5, 12, 16)
    assert torch.equal(CC.conv_pack_ref(w, 0), w.permute(0, 2, 1))
    assert torch.equal(CC.conv_pack_ref(w, 1), w.flip(2).permute(1, 2, 0))
    dy = torch.tensor([[1., 2., 3., 4.]])
    ro = torch.tensor([[0., -0., 1e-30, 2.]])
    z = CC.relu_bwd_pad_ref(dy, ro, 1, 1)
    assert z.shape == (33, 4) and torch.equal(z[8], torch.tensor([0., 0., 3., 4.])) and z.abs().sum() == 7


# ---------------------------------------------------------------- argument refusals (validated before any launch)
DIMS, ALIGN, UNSUPPORTED, NULL = -1, -2, -4, -5


@pytest.fixture(scope='module')
def lib():
    from lamp_amd import _native as N
    try:
        return N.lib()
    except (RuntimeError, OSError) as e:
        pytest.skip('liblamp_hip.so is not built: %s' % e)


def test_conv_window_refusals(lib):
    def cw(x=16, rows_out=4, rows_in=20, c_in=8, w=16, c_out=8, pos=None, src_pos=None, out=16):
        return lib.lamp_conv_window_fwd(x, 1, rows_out, rows_in, c_in, w, c_out, None, 1, pos, 5 if pos else 0, src_pos, 0,
                                        out, None, None)
    assert cw(rows_in=4 + 14) == DIMS            # 16 rows per window: rows_in >= rows_out + 15
    assert cw(c_in=6) == UNSUPPORTED
    assert cw(pos=16, src_pos=None) == NULL
    assert cw(x=20) == ALIGN and cw(w=24) == ALIGN
    assert lib.lamp_conv_window_fwd(16, 0, 4, 20, 8, 16, 8, None, 1, None, 0, None, 0, 16, None, None) == DIMS


def test_front_and_pack_refusals(lib):
    from lamp_amd import _native as N
    fe = N.OnehotFrontend(16, 16, 16, 16, 16, 9, 16)
    big = N.OnehotFrontend(16, 16, 16, 16, 16, 17, 16)
    nbytes = 1 << 30
    assert lib.lamp_onehot_front_bwd(16, 1, 100, ctypes.byref(big), 8, 0.0, 0, 16, 16, 16, nbytes, None) == DIMS
    assert lib.lamp_onehot_front_bwd(16, 1, 1, ctypes.byref(fe), 8, 0.0, 0, 16, 16, 16, nbytes, None) == DIMS
    assert lib.lamp_onehot_front_bwd(16, 1, 100, ctypes.byref(fe), 6, 0.0, 0, 16, 16, 16, nbytes, None) == UNSUPPORTED
    assert lib.lamp_onehot_front_bwd(16, 1, 100, ctypes.byref(fe), 8, 0.0, 0, 20, 16, 16, nbytes, None) == ALIGN
    assert lib.lamp_onehot_front_bwd(16, 1, 100, None, 8, 0.0, 0, 16, 16, 16, nbytes, None) == NULL
    assert lib.lamp_onehot_front_fwd(16, 1, 100, ctypes.byref(fe), 8, 0.0, 0, 20, None) == ALIGN
    assert lib.lamp_onehot_front_bwd_partials_bytes(19, 27, 9, 36) == 3 * 9 * 16 * 36 * 4
    assert lib.lamp_onehot_front_bwd_partials_bytes(4, 64, 9, 4) == 1 * 9 * 16 * 4 * 4
    assert lib.lamp_conv_pack(16, 4, 0, 16, 0, 16, None) == DIMS
    assert lib.lamp_conv_relu_bwd_pad(16, 16, 1, 0, 8, 16, None) == DIMS
    assert lib.lamp_conv_relu_bwd_pad(16, 20, 1, 4, 8, 16, None) == ALIGN
