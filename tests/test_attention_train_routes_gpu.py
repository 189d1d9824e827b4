"""Training-mode attention beyond 256 queries: the single-pass map write-out (PM == 2: scores + row log2-sum-exp, normalised in
place) of BOTH kernels it can reach, against fp64 torch on the CPU, and the backward that reads those maps against autograd on
the fp64 oracle.  tests/attn_routes_common.py holds the routing rule, the operands, the references and the assertions.

Routes (launch_attn, lamp_amd/csrc/attention.hip; a call with maps and lse):
  attn32   attn_kernel<DP, 1, 2, MK>, 32-query blocks: lq > 256 and lk > 64.  <DP, 2, 2, MK> only through the tuning hook.
  small16  attention_small.hip, 16-query blocks: lq <= 256, or lk <= 64, or LAMP_MASK_SELF_RAGGED, or bit 7 of the tuning hook.
Every parameter list below asserts its route by construction (AC.route); on the tuning build the 16-query kernel's trace hook
confirms it (that kernel stamps the buffer, attn_kernel does not).

MEASURED holds the worst figures of one run on an MI355X beside the bars they are held to."""
import ctypes

import pytest
import torch

import attn_routes_common as AC
from conftest import max_abs_diff
from oracle import lamp_ref as R

pytestmark = pytest.mark.gpu

# (lq, lk) on the 32-query route: one query past a block, a partial last block, key counts one past a 32-key tile / one past 256
SHAPES_ATTN32 = [(257, 65), (289, 97), (300, 130), (321, 257)]
# (lq, lk, self_ragged) on the 16-query kernel beyond 256 queries: the flag; the few-keys rule (lk = 64 is its edge)
SHAPES_SMALL16 = [(300, 300, True), (983, 40, False), (257, 64, False)]
# (d_k, d_v): 24 -> DP = 32, 64 -> DP = 64, 128 -> DP = 128, and d_v != d_k both ways (DP follows the larger)
WIDTHS = [(24, 24), (64, 64), (128, 128), (64, 128), (128, 100)]
KINDS = ['none', 'u8', 'shared', 'keys']
# LAMP_MASK_SELF_RAGGED is a flag of a mask: no maskless call can carry it
SMALL16_CASES = [(lq, lk, rg, kind) for lq, lk, rg in SHAPES_SMALL16 for kind in KINDS if not (rg and kind == 'none')]
FORCED_WIDTHS = [(24, 24), (64, 64), (128, 100)]
# every input of each section-1 test function (the argument tuples of AC.sdpa_case): what its lse yardstick is taken over
INPUTS_ATTN32 = [(lq, lk, dk, dv, kind) for lq, lk in SHAPES_ATTN32 for dk, dv in WIDTHS for kind in KINDS]
INPUTS_SMALL16 = [(lq, lk, dk, dv, kind) for lq, lk, _, kind in SMALL16_CASES for dk, dv in WIDTHS]
INPUTS_FORCED = [(lq, lk, dk, dv, kind) for lq, lk in SHAPES_ATTN32 for dk, dv in FORCED_WIDTHS for kind in KINDS]
TRACE_SLOTS = 8192

MEASURED = """One run on an MI355X, worst figure over all cases of the test beside its bar (bars: tests/attn_routes_common.py).

1. lamp_sdpa_fwd_fast_maps against fp64 (maps bar 5e-6, output 2e-5, row sums 1e-5; lse: 4 x the fp32-CPU-against-fp64 gap)
   test / route                                  cases  maps     output   row sum  lse      fp32 CPU gap  lse / gap
   32-query kernel, attn_kernel<DP, 1, 2>          80   2.6e-6   3.1e-6   2.6e-6   2.0e-5   2.46e-5       0.81
   16-query kernel beyond 256 queries              55   2.7e-6   2.2e-6   2.7e-6   1.3e-5   2.53e-5       0.52
   forced key split 1, attn_kernel<DP, 1, 2>       48   2.6e-6   2.6e-6   2.6e-6   1.9e-5   1.68e-5       1.13
   forced key split 2, attn_kernel<DP, 2, 2>       48   2.6e-6   2.6e-6   2.6e-6   1.9e-5   1.68e-5       1.13
   forced bit 7, 16-query kernel                   48   2.7e-6   1.6e-6   2.7e-6   1.4e-5   1.68e-5       0.85
   The worst lse error of every case sits on a spike row, where lse is the spike's own score (57.7, one fp32 ulp = 3.8e-6):
   it is the rounding of a 24- to 128-term fp32 dot product, in the kernels as in torch.  Against the gap of ITS OWN case
   alone (a maximum over two rows, 2.7e-6 .. 2.5e-5 from case to case) a kernel's error reaches 4.10 x on the 32-query
   kernel (300 x 130, d = 64, byte mask: 1.82e-5 against 4.45e-6) and 3.13 x on the 16-query kernel -- which is why the
   yardstick is taken over all the inputs of a test, as AC.lse_gap_fp32 explains.
   lse of a fully blocked row: -inf in both kernels, every case.

2. MultiHeadAttention.train() at 260 x 70 / 260 x 260 against autograd on the fp64 oracle (output bar 2e-5, map 5e-6, dropped
   map 1e-5, gradients 3e-4 * max|ref| + 1e-9)
   output <= 1.6e-6, map <= 9.2e-7 (p_attn = 0.3 included); every gradient (dxq, dxk, w_qs, w_ks, w_vs, fc, gamma, beta) within
   0.004 of its bar, i.e. ~1e-6 of the gradient's maximum.

3. whole models (logits bar 1e-4, enc_output 5e-5 / 1e-4 live, loss 1e-5, gradients 3e-4 * max|ref| + 1e-9)
   labels260_prior    logits 7.0e-7  enc 6.3e-7  loss 1.3e-8  worst gradient 0.004 of its bar, 63 parameters
   labels260_inveye   logits 6.3e-7  enc 6.3e-7  loss 6.5e-8  worst gradient 0.004 of its bar, 63 parameters
   labels260_sigmoid  logits 5.0e-7  enc 6.3e-7  loss 4.9e-8  worst gradient 0.004 of its bar, 63 parameters
   live_T300          logits 1.8e-6  enc 1.9e-6  loss 1.7e-8  worst gradient 0.011 of its bar, 75 parameters
   The fp32 CPU oracle's own gradients, the condition the seeds were chosen under: 0.003 - 0.004 of the bar, seed 0 each.

That the tests see a fault: with lse of a tail query block written to the wrong row of that block in attn_kernel (a scratch
build, numbers only), the forward's logits do not move (6e-7) and 27 tests fail: all 20 cases of the 32-query test at
lq = 300 (the one shape whose tail block has more than one row), all five tests of section 2 (gradients up to 29 000 x their
bar) and labels260_prior / labels260_inveye of section 3 (gradients 4 000 x their bar and more)."""


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from lamp_amd import _native as N
    N.lib()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def tuning():
    """The -DLAMP_TUNING build of the same sources: lamp_debug_force_attn and the 16-query kernel's trace hook."""
    from lamp_amd import _native as N
    t = N.load_library(N.TUNING_LIB_PATH)
    t.lamp_debug_force_attn.argtypes = [ctypes.c_int]
    t.lamp_debug_force_attn.restype = None
    t.lamp_debug_set_attn_trace.argtypes = [ctypes.c_void_p]
    t.lamp_debug_set_attn_trace.restype = None
    return t


class _Small16Trace(object):
    """with _Small16Trace(tuning, dev, workgroups) as t: ...; t.used() -- did attention_small.hip run inside the block?
    The kernel writes 8 words per workgroup; ``workgroups`` bounds its grid and must fit the buffer."""

    def __init__(self, tuning, dev, workgroups):
        assert workgroups <= TRACE_SLOTS
        self.tuning = tuning
        self.buf = torch.zeros(8 * TRACE_SLOTS, dtype=torch.int64, device=dev)

    def __enter__(self):
        torch.cuda.synchronize()
        self.tuning.lamp_debug_set_attn_trace(self.buf.data_ptr())
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.tuning.lamp_debug_set_attn_trace(None)

    def used(self):
        return bool((self.buf.view(-1, 8)[:, 3] != 0).any().item())


def _workgroups(lq, B, H):
    return (lq + 15) // 16 * B * H       # the 16-query kernel's grid at one query block per workgroup, its largest


# ------------------------------------------------------------------ 1. the single-pass write-out against fp64
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dk,dv', WIDTHS)
@pytest.mark.parametrize('lq,lk', SHAPES_ATTN32)
def test_fast_maps_on_the_32_query_kernel_vs_fp64(dev, lq, lk, dk, dv, kind):
    """Route attn32 -- attn_kernel<DP, 1, /*PM=*/2, MK> (lq > 256, lk > 64), product library.  lamp_sdpa_fwd_fast_maps on
    head-fused operands, B = 2 (3 with the key-token mask), H = 2, every mask kind training hands over, a dead row in the tail
    query block, an all-padding sample, a late spike in the last partial key tile: maps (5e-6), output (2e-5), exact zeros,
    NaN placement, row sums (1e-5) and lse against fp64 torch; lse within 4x the worst gap of fp32 torch on the CPU over this
    test's inputs (measured: gap 2.46e-5, the kernel's worst error 2.0e-5); lse of a fully blocked row is -inf.
    All figures: MEASURED."""
    from lamp_amd import _native as N
    assert AC.route(lq, lk) == 'attn32'
    c = AC.sdpa_case(lq, lk, dk, dv, kind)
    AC.check_fast_maps(c, *AC.run_fast_maps(N, c, dev), gap=AC.lse_gap_fp32(INPUTS_ATTN32), tag='attn32')


@pytest.mark.parametrize('dk,dv', WIDTHS)
@pytest.mark.parametrize('lq,lk,ragged,kind', SMALL16_CASES)
def test_fast_maps_on_the_16_query_kernel_beyond_256_queries_vs_fp64(dev, lq, lk, ragged, kind, dk, dv):
    """Route small16 -- attention_small.hip with PM == 2 beyond 256 queries, product library: through LAMP_MASK_SELF_RAGGED
    (300 x 300: the live encoder at reuters' T) and through the few-keys rule (983 x 40: delicious' enc-dec attention; 257 x 64:
    the rule's edge).  The same assertions as on the 32-query kernel (measured: fp32 CPU gap of lse 2.53e-5, the kernel's
    worst error 1.3e-5).  All figures: MEASURED."""
    from lamp_amd import _native as N
    assert AC.route(lq, lk, self_ragged=ragged) == 'small16' and lq > 256
    c = AC.sdpa_case(lq, lk, dk, dv, kind)
    AC.check_fast_maps(c, *AC.run_fast_maps(N, c, dev, self_ragged=ragged), gap=AC.lse_gap_fp32(INPUTS_SMALL16), tag='small16')


@pytest.mark.parametrize('dk,dv', FORCED_WIDTHS)
@pytest.mark.parametrize('lq,lk', SHAPES_ATTN32)
@pytest.mark.parametrize('mode', [1, 2, 0x80])
def test_fast_maps_forced_variants_vs_fp64(dev, tuning, mode, lq, lk, dk, dv):
    """The tuning build's forced variants with PM == 2 and lq > 256, every mask kind each: key split 1 (attn_kernel<DP, 1, 2>),
    key split 2 (attn_kernel<DP, 2, 2>: two waves per query block merged before lse is written -- reached by nothing else),
    bit 7 (the 16-query kernel for any query count, with its own key-split heuristic).  The same assertions as on the product
    routes; the trace hook of the 16-query kernel says which kernel ran (measured: fp32 CPU gap of lse 1.68e-5, worst
    errors 1.9e-5 / 1.9e-5 / 1.4e-5).  All figures: MEASURED."""
    from lamp_amd import _native as N
    want = AC.route(lq, lk, force=mode)
    assert want == ('small16' if mode == 0x80 else 'attn32')
    for kind in KINDS:
        c = AC.sdpa_case(lq, lk, dk, dv, kind)
        try:
            tuning.lamp_debug_force_attn(mode)
            with _Small16Trace(tuning, dev, _workgroups(lq, c['B'], c['H'])) as trace:
                got = AC.run_fast_maps(N, c, dev, _lib=tuning)
        finally:
            tuning.lamp_debug_force_attn(0)
        assert trace.used() == (want == 'small16'), (mode, kind)
        AC.check_fast_maps(c, *got, gap=AC.lse_gap_fp32(INPUTS_FORCED), tag='forced %#x %s' % (mode, want))


def test_the_heuristic_takes_the_documented_route(dev, tuning):
    """The unforced choice of the tuning build (the same sources as the product library) for every (lq, lk) of this file, and
    either side of both boundaries: the 16-query kernel's trace buffer is stamped exactly where AC.route says small16."""
    from lamp_amd import _native as N
    shapes = [(lq, lk, False) for lq, lk in SHAPES_ATTN32] + SHAPES_SMALL16 + [(256, 65, False), (300, 300, False), (260, 70, False),
                                                                               (260, 260, False), (260, 23, False)]
    for lq, lk, ragged in shapes:
        c = AC.sdpa_case(lq, lk, 24, 24, 'u8')
        with _Small16Trace(tuning, dev, _workgroups(lq, c['B'], c['H'])) as trace:
            AC.run_fast_maps(N, c, dev, self_ragged=ragged, _lib=tuning)
        assert trace.used() == (AC.route(lq, lk, self_ragged=ragged) == 'small16'), (lq, lk, ragged)


# ------------------------------------------------------------------ 2. lamp_mha_train_fwd + lamp_mha_bwd beyond 256 queries
D_MODEL = 64


def _mha_inputs(which, H, seed):
    """-> (xq, xk or None for self-attention, blocked (B, lq, lk) bool, the mask to hand the module (CPU), dy)."""
    g = torch.Generator().manual_seed(seed)
    if which == 'cross':            # 260 queries x 70 keys, key-token mask, ragged lengths (no sample without a key)
        B, lq, lk = 3, 260, 70
        xq, xk = torch.randn(B, lq, D_MODEL, generator=g), torch.randn(B, lk, D_MODEL, generator=g)
        seq = torch.randint(1, 50, (B, lk), generator=g)
        seq[1, 33:] = 0
        seq[2, 65:] = 0             # one key past two 32-key tiles
        blocked = seq.eq(0).unsqueeze(1).expand(B, lq, lk)
        mask = seq
    else:                           # 260 x 260 self-attention, one shared mask, ONE tensor behind query, key and value
        B, lq, lk = 2, 260, 260
        xq, xk = torch.randn(B, lq, D_MODEL, generator=g), None
        shared = torch.rand(lq, lk, generator=g) < 0.5
        shared.fill_diagonal_(False)
        blocked = shared.unsqueeze(0).expand(B, lq, lk)
        mask = shared
    dy = torch.randn(B, lq, D_MODEL, generator=g)
    return xq, xk, blocked, mask, dy


def _mha_restatement(xq, xk, blocked, w, H, keep=None, p=0.0):
    """lamp/SubLayers.py:77-121 in plain torch with attention dropout applied through a given keep mask (H, B, lq, lk):
    the restatement of test_mha_with_dropout_matches_torch_restatement_with_the_same_masks.  -> (out, the dropped map)."""
    B, lq, d = xq.shape
    lk, dk = xk.size(1), w['w_qs.weight'].size(0) // H
    split = lambda t, l: t.view(B, l, H, dk).permute(2, 0, 1, 3)  # noqa: E731
    q, k, v = split(xq @ w['w_qs.weight'].t(), lq), split(xk @ w['w_ks.weight'].t(), lk), split(xk @ w['w_vs.weight'].t(), lk)
    s = (q @ k.transpose(-1, -2)) / dk ** 0.5
    P = torch.softmax(s.masked_fill(blocked.unsqueeze(0), float('-inf')), -1)
    Pd = P * keep / (1 - p) if keep is not None else P
    a = (Pd @ v).permute(1, 2, 0, 3).reshape(B, lq, H * dk)
    o = a @ w['fc.weight'].t() if 'fc.weight' in w else a
    out = torch.nn.functional.layer_norm(o + xq, (d,), w['layer_norm.weight'], w['layer_norm.bias'], 1e-5)
    return out, Pd.reshape(H * B, lq, lk)


def _mha_device_mask(N, which, mask, dev, lk):
    if which == 'cross':
        return N.key_token_mask(mask.to(dev), lk)      # (N.Mask, keepalive)
    return mask.to(dev), None                           # a [lq, lk] bool tensor: the module builds the shared descriptor


def _check_mha(dev, which, H, p_attn):
    from lamp_amd import _native as N
    from lamp_amd import training
    from lamp_amd.SubLayers import MultiHeadAttention
    torch.manual_seed(100 + H)
    mod = MultiHeadAttention(H, D_MODEL, D_MODEL // H, D_MODEL // H, dropout=0.0, dropout2=p_attn).to(dev).train()
    xq, xk, blocked, mask, dy = _mha_inputs(which, H, 7 * H + len(which))
    B, lq, _ = xq.shape
    lk = blocked.size(-1)
    assert lq > 256 and (AC.route(lq, lk) == 'attn32')
    w = {k: v.detach().cpu().double().requires_grad_() for k, v in mod.state_dict().items()}
    xq64 = xq.double().requires_grad_()
    xk64 = xk.double().requires_grad_() if xk is not None else xq64
    keep = None
    if p_attn > 0:      # the seed _MHAFn will draw for its attention dropout, and the library's own keep mask for it
        torch.manual_seed(4321)
        keep = N.dropout_keep_mask(H * B * lq * lk, p_attn, training._Seeds().next()).view(H, B, lq, lk)
        ref, ref_map = _mha_restatement(xq64, xk64, blocked, w, H, keep, p_attn)
        assert 0.6 < keep.float().mean().item() < 0.8
    else:
        ref, ref_map = R.mha(xq64, xk64, blocked, w['w_qs.weight'], w['w_ks.weight'], w['w_vs.weight'], w.get('fc.weight'),
                             w['layer_norm.weight'], w['layer_norm.bias'], H)
    ref.backward(dy.double())

    m, keepalive = _mha_device_mask(N, which, mask, dev, lk)
    xq_d = xq.to(dev).requires_grad_()
    xk_d = xk.to(dev).requires_grad_() if xk is not None else xq_d
    torch.manual_seed(4321)
    out, attn = mod(xq_d, xk_d, xk_d, attn_mask=m)
    out.backward(dy.to(dev))
    torch.cuda.synchronize()
    del keepalive
    fig = {'out': max_abs_diff(out, ref.detach()), 'map': max_abs_diff(attn, ref_map.detach())}
    pairs = [('dxq', xq_d.grad, xq64.grad)] + ([('dxk', xk_d.grad, xk64.grad)] if xk is not None else [])
    pairs += [(n, p.grad, w[n].grad) for n, p in mod.named_parameters()]
    assert len(pairs) == (1 if xk is None else 2) + (6 if H > 1 else 5)
    for n, got, want in pairs:
        assert got is not None and want is not None, n
        fig[n] = max_abs_diff(got, want) / (AC.GRAD_RTOL * want.abs().max().item() + AC.GRAD_ATOL)
    print('mha %s H=%d p_attn=%.1f: out %.2e map %.2e; gradient errors as fractions of the bar: %s' % (
        which, H, p_attn, fig['out'], fig['map'], ' '.join('%s %.3f' % (n, fig[n]) for n, _, _ in pairs)))
    # output and map: the bars of test_mha_with_distinct_key_and_value_sources (2e-5, 5e-6; the dropped map 1e-5 as in
    # test_mha_with_dropout_matches_torch_restatement_with_the_same_masks: kept entries are scaled by 1 / (1 - p)), both
    # inside the rule 3e-4 * max|ref| + 1e-9 the gradients are held to
    assert fig['out'] < 2e-5 and fig['map'] < (1e-5 if p_attn > 0 else 5e-6)
    for n, _, _ in pairs:
        assert fig[n] <= 1.0, (n, fig[n])


@pytest.mark.parametrize('H', [1, 4])
@pytest.mark.parametrize('which', ['cross', 'self'])
def test_mha_train_and_backward_beyond_256_queries_vs_oracle_autograd(dev, which, H):
    """Route attn32 (260 x 70 under a ragged key-token mask; 260 x 260 under a shared mask) -- MultiHeadAttention.train() at
    d_model = 64: lamp_mha_train_fwd writes the maps through attn_kernel<DP, 1, 2>, lamp_mha_bwd reads them.  'self' passes ONE
    tensor as query, key and value source (the dxk == dxq accumulate-in-place branch of lamp_mha_act_bwd); H = 1 has no fc
    (g_a aliases dxq).  Output, map, dxq, dxk, every weight, gamma, beta against torch autograd on the fp64 oracle R.mha,
    gradients within 3e-4 * max|ref| + 1e-9.  Figures: MEASURED."""
    _check_mha(dev, which, H, 0.0)


def test_mha_train_with_attention_dropout_beyond_256_queries(dev):
    """Route attn32, 260 x 260 self-attention, H = 4, p_attn = 0.3: the dropped map feeds the batched Pd.V product and the
    backward at this size.  Reference: the torch restatement with the library's own keep mask (N.dropout_keep_mask) for the
    seed the forward draws.  Figures: MEASURED."""
    _check_mha(dev, 'self', 4, 0.3)


def test_mha_train_routes_on_the_tuning_build(dev, tuning, monkeypatch):
    """The training forward's route at the shapes of this section and of section 3's enc-dec attention, through the trace hook:
    260 x 70 and 260 x 260 leave the 16-query kernel's buffer untouched (attn32), 260 x 23 stamps it (few keys)."""
    from lamp_amd import _native as N
    from lamp_amd.SubLayers import MultiHeadAttention
    monkeypatch.setattr(N, '_lib', tuning)
    torch.manual_seed(5)
    mod = MultiHeadAttention(2, D_MODEL, 32, 32, dropout=0.0).to(dev).train()
    for lq, lk in ((260, 70), (260, 260), (260, 23)):
        xq, xk = torch.randn(2, lq, D_MODEL, device=dev), torch.randn(2, lk, D_MODEL, device=dev)
        with _Small16Trace(tuning, dev, _workgroups(lq, 2, 2)) as trace:
            mod(xq, xk, xk)
        assert trace.used() == (AC.route(lq, lk) == 'small16'), (lq, lk)


# ------------------------------------------------------------------ 3. whole-model gradients on those routes
_MIN_CHECKED = {'softmax': 40, 'sigmoid': 35, 'live': 50}


@pytest.mark.parametrize('name', sorted(AC.MODEL_CASES))
def test_every_parameter_gradient_matches_oracle_autograd_beyond_256_queries(dev, name):
    """loss.backward() through LAMP.train() against autograd on the fp64 oracle, every parameter, with the assertions and the
    tolerance of tests/test_gpu_training.py::test_every_parameter_gradient_matches_oracle_autograd (and of its live-encoder and
    sigmoid counterparts):
      labels260_prior / _inveye   V = 50, L = 260, T = 23, d = 64, dff = 96, h = 2, B = 2, lengths [23, 9]: the label
                                  self-attention is 260 x 260 on attn32, the enc-dec attention 260 x 23 on small16 (few keys)
      labels260_sigmoid           the same model with dec_attn_type = 'sigmoid': launch_sigmoid_bwd and the batched products at
                                  lq > 256, against the restatement of tests/sigmoid_common.py
      live_T300                   enc_self_attn=True at tests/enc_live_common.py shape 'B' (T = 300, lengths [300, 257, 64, 20],
                                  d = 128): the encoder self-attention is 300 x 300 on small16 through LAMP_MASK_SELF_RAGGED,
                                  against EC.live_forward_ref
    The seeds (AC.MODEL_SEEDS) were chosen so that the fp32 CPU oracle's own logits, loss and autograd stay inside these same
    bars against the fp64 oracle (AC.fp32_oracle_is_inside; `python tests/attn_routes_common.py`, no GPU needed): a ReLU kink
    cannot fake a mismatch here, and there is no escape for one.  Figures: MEASURED."""
    import torch.nn.functional as F
    m, sd, blocked, seq, spos, h, tgt, kind = AC.model_case(name)
    ref_logits, ref_enc, ref_loss, g64 = AC.oracle_run(kind, sd, seq, spos, h, blocked, tgt)
    m = m.to(dev).train()
    logits, enc, extra = m((seq.to(dev), spos.to(dev)), None, None, tgt.to(dev))
    assert extra is None and logits.requires_grad and enc.requires_grad
    tol_enc = 1e-4 if kind == 'live' else 5e-5            # tests/test_enc_self_attn_gpu.py holds its encoder to TOL = 1e-4
    e_logits, e_enc = max_abs_diff(logits, ref_logits), max_abs_diff(enc, ref_enc)
    loss = F.binary_cross_entropy_with_logits(logits, tgt.to(dev))
    loss.backward()
    checked = live = 0
    worst = (0.0, None)
    failures = []
    for pname, p in m.named_parameters():
        if pname == 'encoder.position_enc.weight':
            assert p.grad is None       # frozen sinusoid table
            continue
        if kind != 'live' and 'encoder.layer_stack' in pname and 'slf_attn' in pname:
            assert p.grad is None       # dead code in the reference: no gradient there either
            continue
        ref = AC.reference_gradient(g64, pname)
        assert p.grad is not None and ref is not None, pname
        scale = ref.abs().max().item()
        err = max_abs_diff(p.grad, ref)
        frac = err / (AC.GRAD_RTOL * scale + AC.GRAD_ATOL)
        worst = max(worst, (frac, pname))
        if not err <= AC.GRAD_RTOL * scale + AC.GRAD_ATOL:
            failures.append((pname, err, scale))
        if kind == 'live' and 'encoder.layer_stack' in pname and 'slf_attn' in pname:
            assert float(p.grad.abs().max()) > 0, pname
            live += 1
        checked += 1
    print('%s: logits %.2e enc %.2e loss %.2e; worst gradient error %.3f of the bar (%s), %d parameters' % (
        name, e_logits, e_enc, abs(loss.item() - ref_loss), worst[0], worst[1], checked))
    assert e_logits < 1e-4 and e_enc < tol_enc
    assert abs(loss.item() - ref_loss) < 1e-5
    assert not failures, failures
    assert checked >= _MIN_CHECKED[kind] and live == (12 if kind == 'live' else 0)
    if kind == 'softmax':   # eval-mode forward of the same weights agrees with the train-mode forward at dropout 0
        m.eval()
        with torch.no_grad():
            ev, _, _ = m((seq.to(dev), spos.to(dev)), None, None, None)
        assert max_abs_diff(ev, logits.detach()) < 2e-5
