"""-m gpu: the ragged plan (csrc/pointwise.hip: embed_plan_kernel, seq_plan_kernel) at the thresholds of its geometry, and the
fall-back routes of its hand-off that an idle GPU never takes.

Every evaluation forward on a ragged batch starts with embed_plan_kernel: a few plan workgroups count each sample's extents and
publish them as {value, epoch} granules, every gather wave polls them a bounded number of times and otherwise counts what is
missing itself (plan_prefix, plan_scan_sample).  On an idle GPU the granules are there at the first or second poll, so the
fall-backs run only when several processes share the GPU.  The tuning build's lamp_debug_embed_plan_mode withholds the granules
(bit 0: plen, bit 1: off) or skips the dense shortcut (bit 2): the fall-backs then run on every launch and must give the bits
of the ordinary hand-off.

The sweeps (ragged_plan_common.SWEEP x PATTERNS) walk the plan's geometry: n_plan = 1, (nb + 3) / 4 and its cap of 64 workgroups,
the 64-lane prefix chunks, seq_plan_kernel's 64 / 256 / 1024 threads and its wave loop beyond 16 samples (return_attns=True: the
padded route), the 512-position groups of plan_scan_sample and the last partial word of the key mask.  One tiny model keeps a
case to a fraction of a second; tolerances are those of tests/test_gpu_parity.py (and of tests/test_enc_self_attn_gpu.py for the
live encoder)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import enc_live_common as EC
import ragged_plan_common as RP
from conftest import max_abs_diff
from oracle import lamp_ref as R
from test_enc_self_attn_gpu import TOL as TOL_LIVE
from test_gpu_parity import CONFIGS, TOL_ACT, TOL_ATTN, TOL_LOGIT, make_case

pytestmark = pytest.mark.gpu

SWEEP_IDS = ['nb%d_T%d' % c for c in RP.SWEEP]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from lamp_amd import _native as N
    N.lib()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def tuning():
    """The -DLAMP_TUNING build of the same sources: the only library that exports lamp_debug_embed_plan_mode."""
    from lamp_amd import _native as N
    t = N.load_library(N.TUNING_LIB_PATH)
    t.lamp_debug_embed_plan_mode.argtypes = [ctypes.c_int]
    t.lamp_debug_embed_plan_mode.restype = None
    return t


@pytest.fixture(scope='module')
def tiny(dev):
    """{position table?: (model on the device, fp32 state_dict, fp64 state_dict)}: one model for every (nb, T) of the sweeps."""
    out = {}
    for pos in (True, False):
        sd = RP.tiny_state_dict(pos)
        out[pos] = (RP.tiny_model(sd, pos).to(dev).eval(), sd, R.to_dtype(sd, torch.float64))
    return out


_REF = {}


def _ref(name, nb, T, pos, sd, sd64):
    """Pattern, plan restatement and the oracle's results (fp32 and fp64) of one case: computed once, shared, never modified."""
    key = (name, nb, T, pos)
    if key not in _REF:
        seq, spos = RP.make_pattern(name, nb, T)
        with torch.no_grad():
            ref_logits, ref_enc, _ = R.forward(sd, seq, spos, RP.TINY['h'], None)
            ref64, _, _ = R.forward(sd64, seq, spos, RP.TINY['h'], None)
        _REF[key] = dict(seq=seq, pos=spos, logits=ref_logits, enc=ref_enc, logits64=ref64,
                         plan=RP.plan_ref(seq.numpy(), spos.numpy() if pos else None))
    return _REF[key]


def _fwd(m, src, **kw):
    with torch.no_grad():
        return m(src, None, None, None, **kw)


def _assert_oracle_bars(logits, enc, ref, what):
    assert max_abs_diff(enc, ref['enc']) < TOL_ACT, what
    assert torch.equal(torch.isnan(logits).cpu(), torch.isnan(ref['logits'])), what
    # tiny widths make LayerNorm ill-conditioned: the bar scales with the oracle's own fp32-vs-fp64 gap (test_gpu_parity.py)
    gap = max_abs_diff(ref['logits'], ref['logits64'])
    assert max_abs_diff(logits, ref['logits64']) < max(TOL_LOGIT, 4 * gap), (what, gap)


# ------------------------------------------------------------------ the product library over the sweeps
@pytest.mark.parametrize('name', sorted(RP.PATTERNS))
@pytest.mark.parametrize('nb,T', RP.SWEEP, ids=SWEEP_IDS)
def test_plan_geometry_sweep_on_the_product_library(dev, tiny, nb, T, name):
    for pos in (True, False):
        m, sd, sd64 = tiny[pos]
        ref = _ref(name, nb, T, pos, sd, sd64)
        what = (name, nb, T, pos)
        assert RP.forward_passes(m, nb, T) == (1, nb) and RP.forward_passes(m, nb, T, want_attn=True) == (1, nb), what
        src = (ref['seq'].to(dev), ref['pos'].to(dev))
        logits, enc, _ = _fwd(m, src)
        _assert_oracle_bars(logits, enc, ref, what)
        # every position past a sample's rows holds the ONE shared PAD row, bit for bit
        plen = torch.from_numpy(ref['plan']['plen'])
        skipped = torch.arange(T).unsqueeze(0) >= plen.unsqueeze(1)
        rows = enc.cpu()[skipped].view(torch.int32)
        assert rows.size(0) == nb * T - int(ref['plan']['rows'][0])
        assert rows.size(0) == 0 or torch.equal(rows, rows[:1].expand_as(rows)), what
        # the same samples in batches of four: other plan geometry, other offsets, the same bits
        for o in sorted({0, 60, 64, nb - 4}):
            if 0 <= o and o + 4 <= nb:
                part, enc_part, _ = _fwd(m, (src[0][o:o + 4], src[1][o:o + 4]))
                assert RP.same_bits(part, logits[o:o + 4]) and RP.same_bits(enc_part, enc[o:o + 4]), (what, o)
        # the padded route (seq_plan_kernel: 64 / 256 / 1024 threads, its wave loop beyond 16 samples): the same bits again
        lg, en, _, _ = _fwd(m, src, return_attns=True)
        assert RP.same_bits(lg, logits) and RP.same_bits(en, enc), what


# ------------------------------------------------------------------ the forced fall-back routes (tuning library)
def _forced_modes(m, src, hook, modes, what, timings=None):
    """Mode 0 once, then every forced mode three times (a race in the concurrent rewrite of the key-mask words would not
    repeat): logits, enc_output and the intermediate read-outs keep mode 0's bits.  -> mode 0's results."""
    try:
        hook(0)
        want = _fwd(m, src, int_preds=True)
        for mode in modes:
            hook(mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runs = [_fwd(m, src, int_preds=True) for _ in range(3)]
            torch.cuda.synchronize()
            if timings is not None:
                timings[mode] = (time.perf_counter() - t0) / 3
            for got in runs:
                assert RP.same_bits(got[0], want[0]) and RP.same_bits(got[1], want[1]), (what, mode)
                assert len(got[2]) == len(want[2]) > 0 and all(RP.same_bits(a, b) for a, b in zip(got[2], want[2])), (what, mode)
    finally:
        hook(-1)
    return want


def _modes_of(name):
    return (4, 7) if name == 'dense' else (1, 2, 3, 4, 7)


@pytest.mark.parametrize('name', sorted(RP.PATTERNS))
@pytest.mark.parametrize('nb,T', RP.SWEEP, ids=SWEEP_IDS)
def test_forced_fall_back_routes_keep_the_bits(dev, tiny, tuning, monkeypatch, nb, T, name):
    """Bit 0: the scanner and the gather waves count the samples themselves.  Bit 1: every gather wave of a non-dense batch
    runs its own plan_prefix(want = b) -- across several 64-sample chunks beyond 64 samples -- and the PAD-row wave the
    want < 0 form.  Bit 2: a fixed-length batch goes through the hand-off (4) and through the fall-backs (7) as well."""
    from lamp_amd import _native as N
    monkeypatch.setattr(N, '_lib', tuning)
    for pos in (True, False):
        m, sd, sd64 = tiny[pos]
        ref = _ref(name, nb, T, pos, sd, sd64)
        what = (name, nb, T, pos)
        assert RP.forward_passes(m, nb, T) == (1, nb), what
        src = (ref['seq'].to(dev), ref['pos'].to(dev))
        timings = {}
        want = _forced_modes(m, src, tuning.lamp_debug_embed_plan_mode, _modes_of(name), what, timings)
        _assert_oracle_bars(want[0], want[1], ref, what)
        print('forced plan modes %s: %s' % (what, ', '.join('mode %d %.2f ms' % (k, 1e3 * v) for k, v in sorted(timings.items()))))


@pytest.mark.parametrize('nb', [5, 65, 129])
def test_forced_fall_back_routes_on_the_live_packed_encoder(dev, tuning, monkeypatch, nb):
    """enc_self_attn=True behind use_packed_live_encoder (csrc/attention_ragged.hip on the packed rows; scatter_rows_kernel returns
    the granules to "no epoch"): modes 3 and 7 against mode 0 bit for bit, mode 0 against the oracle composition of
    tests/enc_live_common.py at that file's bar."""
    from lamp_amd import _native as N
    T = 33
    rng = np.random.default_rng(nb)
    lengths = [int(n) for n in rng.integers(1, T + 1, size=nb)]
    lengths[0], lengths[nb - 2], lengths[nb - 1] = T, 0, 1
    shape = dict(V=50, L=24, d=128, h=2, dff=256, T=T, lengths=lengths)
    m, sd, blocked, seq, spos, h = EC.build(shape, 'prior', True)
    assert seq.shape == (nb, T)
    m = m.to(dev).eval()
    m.use_packed_live_encoder = True
    with torch.no_grad():
        ref = EC.live_forward_ref(sd, seq, spos, h, blocked)
    monkeypatch.setattr(N, '_lib', tuning)
    src = (seq.to(dev), spos.to(dev))
    want = _forced_modes(m, src, tuning.lamp_debug_embed_plan_mode, (3, 7), ('live_packed', nb))
    assert max_abs_diff(want[0], ref[0]) < TOL_LIVE and max_abs_diff(want[1], ref[1]) < TOL_LIVE
    m.use_packed_live_encoder = False     # the switch did select the packed route
    assert not torch.equal(torch.nan_to_num(_fwd(m, src)[1]), torch.nan_to_num(want[1]))


def test_forced_fall_back_routes_with_the_embedding_fold(dev, tuning, monkeypatch):
    """The reuters_b32_ragged configuration narrowed to d_model 64 and T = 40: encoder layer 0's W1 is folded into the embedding
    tables and the gather leaves row maps for the gathered residual instead of embedded rows (d_inner 512 is a multiple of 32,
    the tables are 16-byte aligned), so a row gathered to the wrong place shows in two ways."""
    from lamp_amd import _native as N
    cfg = list(CONFIGS['reuters_b32_ragged'])
    cfg[2], cfg[3] = 40, 64
    cfg[10] = [40, 20, 15, 7, 21, 33, 28, 9, 4, 5, 16, 17, 39, 1, 3, 38] * 2
    m, sd, blocked, seq, spos, h = make_case(tuple(cfg), dev)
    assert m.fold_embedding and m._native_model()[0].enc0_emb_w1 and m._native_model()[0].enc0_pos_w1
    with torch.no_grad():
        ref_logits, ref_enc, _ = R.forward(sd, seq, spos, h, blocked)
    monkeypatch.setattr(N, '_lib', tuning)
    want = _forced_modes(m, (seq.to(dev), spos.to(dev)), tuning.lamp_debug_embed_plan_mode, (3, 7), 'fold')
    assert max_abs_diff(want[0], ref_logits) < TOL_LOGIT and max_abs_diff(want[1], ref_enc) < TOL_ACT


# ------------------------------------------------------------------ key-token masks outside lamp_forward
def _window_tokens(B, lk, seed):
    """[B, lk] tokens as a column window of a wider matrix (row stride 100 > lk) whose other columns hold tokens too: a kernel
    that read lk-strided rows, or past the window, would see other keys.  Ragged, with a sample without any token (NaN rows),
    a full one and PAD tokens inside."""
    g = torch.Generator().manual_seed(seed)
    wide = torch.randint(1, 9, (B, 100), generator=g)
    seq = wide[:, 13:13 + lk]
    for b in range(B):
        n = int(torch.randint(1, lk + 1, (1,), generator=g))
        seq[b, n:] = 0
    seq[0, :] = wide[0, 0]
    seq[1, :] = 0
    seq[2, 30:34] = 0
    seq[2, 62:66] = 0
    seq[2, lk - 1] = 5
    return wide, seq


@pytest.mark.parametrize('B', [3, 4, 16, 17, 40])
def test_sdpa_key_token_mask_in_a_column_window(dev, B):
    """lamp_sdpa_fwd with a key-token mask whose rows are lk = 70 columns of a wider token matrix (stride_b = 100): out and
    maps against fp64 attention."""
    from lamp_amd import _native as N
    H, lq, lk, dk = 2, 5, 70, 8
    g = torch.Generator().manual_seed(B)
    q, k, v = (torch.randn(B, l, H * dk, generator=g) for l in (lq, lk, lk))
    wide, seq = _window_tokens(B, lk, B)
    wide_dev = wide.to(dev)
    mask, keep = N.key_token_mask(wide_dev[:, 13:13 + lk], lk)
    assert mask.stride_b == 100 and mask.ptr == wide_dev.data_ptr() + 13 * 8
    blocked = seq.eq(0).unsqueeze(1).expand(B, lq, lk)
    split = lambda t, l: t.view(B, l, H, dk).permute(2, 0, 1, 3).reshape(H * B, l, dk)  # noqa: E731
    ref_out, ref_attn = R.sdpa(split(q, lq).double(), split(k, lk).double(), split(v, lk).double(), blocked.repeat(H, 1, 1),
                               dk ** 0.5)
    assert torch.isnan(ref_out[1]).all() and not torch.isnan(ref_out[0]).any()
    for need_attn in (True, False):
        out, attn = N.sdpa_fused(q.to(dev), k.to(dev), v.to(dev), H, mask, 1.0 / dk ** 0.5, need_attn=need_attn)
        got = out.view(B, lq, H, dk).permute(2, 0, 1, 3).reshape(H * B, lq, dk)
        assert max_abs_diff(got, ref_out) < TOL_ATTN, need_attn          # inf when the NaN patterns differ
        if need_attn:
            assert max_abs_diff(attn, ref_attn) < TOL_ATTN


@pytest.mark.parametrize('B', [3, 4, 16, 17, 40])
def test_mha_key_token_mask_in_a_column_window(dev, B):
    """lamp_mha_fwd with the same mask: the attention block counts the samples' keys itself (launch_seq_plan with the mask's row
    stride: seq_plan_kernel's 64 / 256 / 1024 threads, its wave loop at 17 and 40 samples, lk = 70 leaves six bits in the last
    mask word) and reads the plan's bit-packed copy of the mask.  Maps against fp64 at TOL_ATTN, the block's output at TOL_ACT."""
    from lamp_amd import _native as N
    H, lq, lk, d = 2, 5, 70, 32
    dk = d // H
    sd = R.make_state_dict(20, 4, 8, d, 32, H, 1, 1, seed=B)
    par = R._mha_params(sd, 'decoder.layer_stack.0.enc_attn.')
    g = torch.Generator().manual_seed(100 + B)
    xq, xkv = torch.randn(B, lq, d, generator=g), torch.randn(B, lk, d, generator=g)
    wide, seq = _window_tokens(B, lk, B)
    wide_dev = wide.to(dev)
    mask, keep = N.key_token_mask(wide_dev[:, 13:13 + lk], lk)
    blocked = seq.eq(0).unsqueeze(1).expand(B, lq, lk)
    ref_out, ref_attn = R.mha(xq.double(), xkv.double(), blocked, *[p.double() for p in par], n_head=H)
    on_dev = [p.to(dev).contiguous() for p in par]
    w = N.MhaWeights(*[N.ptr(p) for p in on_dev], H, 1)
    out, attn = N.mha(xq.to(dev), xkv.to(dev), w, dk, dk, mask, True)
    assert max_abs_diff(attn, ref_attn) < TOL_ATTN
    assert max_abs_diff(out, ref_out) < TOL_ACT
    assert torch.isnan(out[1]).all() and not torch.isnan(out[0]).any()
