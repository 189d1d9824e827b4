"""-m gpu: the eval forward at head geometries away from d_k = d_v = d_model / n_head and n_head2 = n_head
(tests/head_geometry_common.py: G1 .. G6), where api.hip's hdk != hdv paths run: K and V as separate launches, the per-layer
K/V-ahead projection, a workspace carved for the larger head count of two blocks, the chain launch at k_h != d_model, the
32-query and LDS-tile attention kernels on layouts with q_r != v_r.

Every figure is held against the fp64 oracle at the bars of tests/test_gpu_parity.py -- logits at tests/fuzz_parity.py's rule
max(1e-4, 4 x the fp32 CPU oracle's own gap to fp64) -- and the bit rules the project promises are checked under these
geometries.  The G5 (chain launch) cases carry 'G5' in their names."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import enc_live_common as EC
import head_geometry_common as HG
from conftest import max_abs_diff
from oracle import lamp_ref as R

pytestmark = pytest.mark.gpu

TOL_LOGIT, TOL_ACT, TOL_ATTN = 1e-4, 5e-5, 1e-5     # tests/test_gpu_parity.py
PAD = EC.PAD_EXTRA                                   # the re-padding of the bit-identity tests
SMALL = ['G1', 'G2', 'G3', 'G4a', 'G4b', 'G6']
CHAIN = ['G5a', 'G5b', 'G5b_ff1024', 'G5c']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from lamp_amd import _native as N
    N.lib()  # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def tuning():
    """The -DLAMP_TUNING build of the same sources: the only library that exports the lamp_debug_* hooks."""
    from lamp_amd import _native as N
    t = N.load_library(N.TUNING_LIB_PATH)
    for name in ('lamp_debug_force_chain', 'lamp_debug_chain_geometry'):
        getattr(t, name).argtypes = [ctypes.c_int]
        getattr(t, name).restype = None
    return t


def _build(name, dev, B=None, **kw):
    lengths = HG.chain_lengths(B if B is not None else 6) if name in CHAIN else None
    T = HG.GEOMS[name]['T']
    m, sd, blocked, seq, spos, g = HG.build(name, lengths=lengths, n_max_seq=T + PAD, **kw)
    return m.to(dev).eval(), sd, blocked, seq, spos, g


def _run(m, seq, pos, dev, adj=None, **kw):
    with torch.no_grad():
        return m((seq.to(dev), pos.to(dev)), adj, None, None, **kw)


_REF = {}


def _ref(name, B=None):
    """fp64 oracle of a geometry's default case -> dict; computed once, shared, never modified."""
    key = (name, B)
    if key not in _REF:
        lengths = HG.chain_lengths(B if B is not None else 6) if name in CHAIN else None
        _, sd, blocked, seq, spos, g = HG.build(name, lengths=lengths, n_max_seq=HG.GEOMS[name]['T'] + PAD)
        logits, enc, enc_attns, (slf, encdec) = HG.oracle_forward(sd, seq, spos, g, blocked, return_attns=True)
        ips = HG.oracle_forward(sd, seq, spos, g, blocked, int_preds=True)[2]
        l32 = HG.oracle_forward(sd, seq, spos, g, blocked, dtype=None)[0]
        gap = max_abs_diff(l32, logits)
        _REF[key] = dict(logits=logits, enc=enc, enc_attns=enc_attns[0], slf=slf, encdec=encdec, ips=ips, gap=gap,
                         tol=max(TOL_LOGIT, 4 * gap))
    return _REF[key]


# ------------------------------------------------------------------ 1. parity with the fp64 oracle
def _check_parity(m, seq, spos, g, ref, dev, tag):
    logits, enc, extra = _run(m, seq, spos, dev)
    B, L, T = seq.size(0), g['L'], seq.size(1)
    print('%s: logits %.3e (bar %.3e, fp32 CPU gap %.3e) enc %.3e' % (tag, max_abs_diff(logits, ref['logits']), ref['tol'],
                                                                     ref['gap'], max_abs_diff(enc, ref['enc'])))
    assert extra is None and logits.shape == (B, L) and enc.shape == (B, T, g['d'])
    assert max_abs_diff(logits, ref['logits']) < ref['tol']
    assert max_abs_diff(enc, ref['enc']) < TOL_ACT
    lg, en, enc_attns, (slf, encdec) = _run(m, seq, spos, dev, return_attns=True)
    assert torch.equal(lg, logits) and torch.equal(en, enc)            # the maps do not change the bits
    assert len(enc_attns[0]) == g['n_enc'] and len(slf) == len(encdec) == g['n_dec']
    for got, want in zip(enc_attns[0], ref['enc_attns']):
        assert got.shape == (g['h'] * B, T, T) and max_abs_diff(got, want) < TOL_ATTN
    for got, want in zip(slf, ref['slf']):
        assert got.shape == (g['h2'] * B, L, L) and max_abs_diff(got, want) < TOL_ATTN
    for got, want in zip(encdec, ref['encdec']):
        assert got.shape == (g['h'] * B, L, T) and max_abs_diff(got, want) < TOL_ATTN
    lg, en, ips = _run(m, seq, spos, dev, int_preds=True)
    assert torch.equal(lg, logits) and torch.equal(en, enc)            # nor do the intermediate predictions
    assert len(ips) == len(ref['ips']) == 2 * g['n_dec'] - 1
    for got, want in zip(ips, ref['ips']):
        assert max_abs_diff(got, want) < TOL_LOGIT
    return logits, enc


@pytest.mark.parametrize('name', SMALL)
def test_eval_forward_against_the_fp64_oracle(dev, name):
    m, sd, blocked, seq, spos, g = _build(name, dev)
    _check_parity(m, seq, spos, g, _ref(name), dev, name)


@pytest.mark.parametrize('name,mask,pos', [('G1', 'none', False), ('G1', 'inveye', True), ('G2', 'prior', True),
                                           ('G3', 'none', False), ('G6', 'prior', True)])
def test_eval_forward_other_masks(dev, name, mask, pos):
    """The masks the default cases leave out, and a model without the position table (not every mask on every geometry)."""
    m, sd, blocked, seq, spos, g = _build(name, dev, mask=mask, pos=pos)
    ref, ref_enc, _ = HG.oracle_forward(sd, seq, spos, g, blocked)
    gap = max_abs_diff(HG.oracle_forward(sd, seq, spos, g, blocked, dtype=None)[0], ref)
    logits, enc, _ = _run(m, seq, spos, dev)
    print('%s %s pos=%s: logits %.3e (fp32 CPU gap %.3e) enc %.3e' % (name, mask, pos, max_abs_diff(logits, ref), gap,
                                                                      max_abs_diff(enc, ref_enc)))
    assert max_abs_diff(logits, ref) < max(TOL_LOGIT, 4 * gap) and max_abs_diff(enc, ref_enc) < TOL_ACT


@pytest.mark.parametrize('name', ['G1', 'G2'])
def test_reference_fixture_through_the_gpu(dev, name):
    """tests/golden/geometry.npz: the reference's own modules at G1 / G2, at the bars of test_model_golden."""
    d, sd, g, blocked = HG.load_golden_geometry(name)
    adj = d.get('label_adj_matrix')
    m = HG.build_model(g, sd, adj).to(dev).eval()
    seq, spos = d['src_seq'], d['src_pos']
    logits, enc, _ = _run(m, seq, spos, dev)
    assert max_abs_diff(logits, d['logits']) < TOL_LOGIT and max_abs_diff(enc, d['enc_output']) < TOL_ACT
    lg, _, enc_attns, (slf, encdec) = _run(m, seq, spos, dev, return_attns=True)
    assert torch.equal(lg, logits)
    for i, a in enumerate(enc_attns[0]):
        assert max_abs_diff(a, d['attn_enc_%d' % i]) < TOL_ATTN
    for i, a in enumerate(slf):
        assert max_abs_diff(a, d['attn_dec_slf_%d' % i]) < TOL_ATTN
    for i, a in enumerate(encdec):
        assert max_abs_diff(a, d['attn_dec_enc_%d' % i]) < TOL_ATTN
    lg, _, ips = _run(m, seq, spos, dev, int_preds=True)
    assert len(ips) == 3 and torch.equal(lg, logits)
    for i, p in enumerate(ips):
        assert max_abs_diff(p, d['int_pred_%d' % i]) < TOL_LOGIT


# ------------------------------------------------------------------ 2. the bit rules
def _repad(seq, spos, T):
    return F.pad(seq, (0, T - seq.size(1))), F.pad(spos, (0, T - spos.size(1)))


def _check_bit_rules(m, seq, spos, g, dev):
    """A sample alone (trimmed to its own length, and as its padded row), in the batch, under a micro-batch split and under a
    longer padding: the same logits and encoder rows, bit for bit."""
    lengths, T = g['lengths'], seq.size(1)
    logits, enc, _ = _run(m, seq, spos, dev)
    assert torch.isfinite(logits).all()
    r_logits, r_enc, _ = _run(m, *_repad(seq, spos, T + PAD), dev)
    assert torch.equal(r_logits, logits) and torch.equal(r_enc[:, :T], enc)
    for b, n in enumerate(lengths[:4]):
        a_logits, a_enc, _ = _run(m, seq[b:b + 1], spos[b:b + 1], dev)
        assert torch.equal(a_logits[0], logits[b]) and torch.equal(a_enc[0], enc[b]), (b, n)
        t_logits, t_enc, _ = _run(m, seq[b:b + 1, :n], spos[b:b + 1, :n], dev)
        assert torch.equal(t_logits[0], logits[b]) and torch.equal(t_enc[0], enc[b, :n]), (b, n)
    m.workspace_limit_bytes = 1      # one sample per pass (and no K/V-ahead: the whole batch does not fit)
    try:
        s_logits, s_enc, _ = _run(m, seq, spos, dev)
        _, _, s_enc_attns, (s_slf, s_encdec) = _run(m, seq, spos, dev, return_attns=True)
    finally:
        del m.workspace_limit_bytes
    assert torch.equal(s_logits, logits) and torch.equal(s_enc, enc)
    _, _, enc_attns, (slf, encdec) = _run(m, seq, spos, dev, return_attns=True)
    for a, b in zip(enc_attns[0] + slf + encdec, s_enc_attns[0] + s_slf + s_encdec):
        assert torch.equal(a, b)
    return logits, enc


def _check_switches(m, seq, spos, dev, logits, enc, tol):
    """use_chain_packs and cache_layer0_query off: the same bits.  fold_embedding off: the unfolded route, which the project
    promises within 2e-5 of the folded one (a re-association, test_embedding_fold_against_the_unfolded_route_and_the_oracle)
    and bit-equal to the module-by-module route's encoder rows (test_model_golden)."""
    from lamp_amd import _native as N
    src = (seq.to(dev), spos.to(dev))
    for switch in ('use_chain_packs', 'cache_layer0_query'):
        setattr(m, switch, False)
        m.invalidate_native_cache()
        try:
            off = _run(m, seq, spos, dev)
        finally:
            delattr(m, switch)
            m.invalidate_native_cache()
        assert torch.equal(off[0], logits) and torch.equal(off[1], enc), switch
    with torch.no_grad():
        enc2, _ = m.encoder(src[0], None, src[1])
        y, _ = m.decoder(None, src[0], enc2)
        lg2 = N.diag_logits(y, m.tgt_word_proj.linear.weight)
    assert m.fold_embedding
    assert max_abs_diff(enc2, enc) < 2e-5 and max_abs_diff(lg2, logits) < max(2e-5, tol)
    m.fold_embedding = False
    try:
        logits_u, enc_u, _ = _run(m, seq, spos, dev)
    finally:
        del m.fold_embedding
    print('fold off: logits %.3e enc %.3e; module route - unfolded launcher: logits %.3e' % (
        max_abs_diff(logits_u, logits), max_abs_diff(enc_u, enc), max_abs_diff(lg2, logits_u)))
    assert max_abs_diff(logits_u, logits) < 2e-5 and max_abs_diff(enc_u, enc) < 2e-5
    assert max_abs_diff(enc2, enc_u) == 0.0 and max_abs_diff(lg2, logits_u) < 1e-6


@pytest.mark.parametrize('name', SMALL)
def test_bit_rules(dev, name):
    m, sd, blocked, seq, spos, g = _build(name, dev)
    logits, enc = _check_bit_rules(m, seq, spos, g, dev)
    _check_switches(m, seq, spos, dev, logits, enc, _ref(name)['tol'])


# ------------------------------------------------------------------ 3. options, on G1 (and on G5a below)
def _bias_for(g, blocked, seed=31):
    """A random (L, L) score bias with about 20 % -inf that keeps every row one allowed key (tests/test_label_bias_gpu.py)."""
    L = g['L']
    gen = torch.Generator().manual_seed(seed)
    bias = 2.0 * torch.randn(L, L, generator=gen)
    drop = torch.rand(L, L, generator=gen) < 0.2
    allowed = ~blocked if blocked is not None else torch.ones(L, L, dtype=torch.bool)
    drop[torch.arange(L), allowed.float().argmax(dim=1)] = False
    return bias.masked_fill(drop, float('-inf'))


def _check_options(name, dev, B=None):
    sd64 = None
    # enc_self_attn=True: padded, behind use_packed_live_encoder, and with per-sample graphs (test_enc_self_attn_gpu.py: 1e-4)
    m, sd, blocked, seq, spos, g = _build(name, dev, B=B, enc_self_attn=True)
    sd64 = R.to_dtype(sd, torch.float64)
    with torch.no_grad():
        ref = HG.live_forward_ref(sd64, seq, spos, g, blocked)
    logits, enc, _ = _run(m, seq, spos, dev)
    print('%s live: logits %.3e enc %.3e' % (name, max_abs_diff(logits, ref[0]), max_abs_diff(enc, ref[1])))
    assert max_abs_diff(logits, ref[0]) < 1e-4 and max_abs_diff(enc, ref[1]) < 1e-4
    lg, en, enc_attns, (slf, encdec) = _run(m, seq, spos, dev, return_attns=True)
    assert torch.equal(lg, logits) and torch.equal(en, enc)
    for got, want in zip(enc_attns[0] + slf + encdec, ref[2] + ref[3][0] + ref[3][1]):
        assert got.shape == want.shape and max_abs_diff(got, want) < 1e-4
    m.use_packed_live_encoder = True
    packed = _run(m, seq, spos, dev)
    del m.use_packed_live_encoder
    assert max_abs_diff(packed[0], ref[0]) < 1e-4 and max_abs_diff(packed[1], ref[1]) < 1e-4
    if g['dk'] != g['dv']:      # the packed rows' Q/K/V launch is one width: d_k != d_v keeps the padded route, its bits
        assert torch.equal(packed[0], logits) and torch.equal(packed[1], enc)
    adj = EC.random_graphs(g['lengths'], seed=3)
    with torch.no_grad():
        ref_adj = HG.live_forward_ref(sd64, seq, spos, g, blocked, adj=adj)
    with_adj = _run(m, seq, spos, dev, adj=adj)
    assert max_abs_diff(with_adj[0], ref_adj[0]) < 1e-4 and max_abs_diff(with_adj[1], ref_adj[1]) < 1e-4
    assert float((with_adj[0] - logits).abs().max()) > 1e-3          # the graphs reach the prediction

    # dec_attn_type='sigmoid' (test_sigmoid_attn_gpu.py: 1e-4 / 5e-5 / maps 1e-5)
    m, sd, blocked, seq, spos, g = _build(name, dev, B=B, dec_attn_type='sigmoid')
    with torch.no_grad():
        ref = HG.sigmoid_forward_ref(sd64, seq, spos, g, blocked)
    logits, enc, _ = _run(m, seq, spos, dev)
    print('%s sigmoid: logits %.3e enc %.3e' % (name, max_abs_diff(logits, ref[0]), max_abs_diff(enc, ref[1])))
    assert max_abs_diff(logits, ref[0]) <= 1e-4 and max_abs_diff(enc, ref[1]) <= 5e-5
    lg, _, _, (slf, encdec) = _run(m, seq, spos, dev, return_attns=True)
    assert max_abs_diff(lg, ref[0]) <= 1e-4
    for got, want in zip(slf + encdec, ref[3][0] + ref[3][1]):
        assert max_abs_diff(got, want) <= 1e-5

    # label_bias= a random matrix (test_label_bias_gpu.py: 1e-4 / 5e-5 / maps 1e-5)
    bias = _bias_for(g, blocked)
    m, sd, blocked, seq, spos, g = _build(name, dev, B=B, label_bias=bias)
    with torch.no_grad():
        ref = HG.label_bias_forward_ref(sd64, seq, spos, g, blocked, bias.double())
    logits, enc, _ = _run(m, seq, spos, dev)
    print('%s label_bias: logits %.3e enc %.3e' % (name, max_abs_diff(logits, ref[0]), max_abs_diff(enc, ref[1])))
    assert max_abs_diff(logits, ref[0]) <= 1e-4 and max_abs_diff(enc, ref[1]) <= 5e-5
    lg, _, _, (slf, encdec) = _run(m, seq, spos, dev, return_attns=True)
    assert max_abs_diff(lg, ref[0]) <= 1e-4
    for got, want in zip(slf + encdec, ref[3][0] + ref[3][1]):
        assert max_abs_diff(got, want) <= 1e-5

    # matmul_precision='high' (test_matmul_precision_gpu.py: 1e-4 on logits and encoder rows; another kernel's bits)
    m, sd, blocked, seq, spos, g = _build(name, dev, B=B)
    ref = _ref(name, B)
    highest = _run(m, seq, spos, dev)
    m.matmul_precision = 'high'
    high = _run(m, seq, spos, dev, int_preds=True)
    print('%s high: logits %.3e enc %.3e' % (name, max_abs_diff(high[0], ref['logits']), max_abs_diff(high[1], ref['enc'])))
    assert max_abs_diff(high[0], ref['logits']) <= 1e-4 and max_abs_diff(high[1], ref['enc']) <= 1e-4
    assert not torch.equal(high[0], highest[0])
    for got, want in zip(high[2], ref['ips']):
        assert max_abs_diff(got, want) <= 1e-4

    # no_dec_self_att
    m, sd, blocked, seq, spos, g = _build(name, dev, B=B, no_dec_self_att=True)
    assert not any('decoder.layer_stack.0.slf_attn' in k for k in sd)
    ref, ref_enc, _ = HG.oracle_forward(sd, seq, spos, g, blocked)
    logits, enc, _ = _run(m, seq, spos, dev)
    print('%s no_dec_self_att: logits %.3e enc %.3e' % (name, max_abs_diff(logits, ref), max_abs_diff(enc, ref_enc)))
    assert max_abs_diff(logits, ref) < TOL_LOGIT and max_abs_diff(enc, ref_enc) < TOL_ACT
    lg, _, ips = _run(m, seq, spos, dev, int_preds=True)
    assert torch.equal(lg, logits) and len(ips) == g['n_dec'] - 1


def test_options_at_G1(dev):
    _check_options('G1', dev)


# ------------------------------------------------------------------ 4. G5: the chain launch at k_h != d_model
def _force(tuning, monkeypatch):
    from lamp_amd import _native as N
    monkeypatch.setattr(N, '_lib', tuning)
    return tuning.lamp_debug_force_chain, tuning.lamp_debug_chain_geometry


@pytest.mark.parametrize('name', CHAIN)
def test_G5_eval_forward_against_the_fp64_oracle(dev, name):
    m, sd, blocked, seq, spos, g = _build(name, dev, B=6)      # 540 decoder rows
    _check_parity(m, seq, spos, g, _ref(name, 6), dev, name)


@pytest.mark.parametrize('name,B', [('G5a', 6), ('G5a', 12), ('G5a', 3), ('G5b', 6), ('G5b', 12), ('G5b_ff1024', 6), ('G5c', 6),
                                    ('G5c', 12)])
def test_G5_chain_forced_on_equals_forced_off(dev, tuning, monkeypatch, name, B):
    """The rule of test_decoder_chain_launch_is_bit_identical at k_h = n_head * d_v of 256 / 512 (G5a), 1024 / 512 (G5b; with
    d_inner 1024 as well) and 768 (G5c): chain forced on == forced off, bit for bit, three runs."""
    m, sd, blocked, seq, spos, g = _build(name, dev, B=B)
    force, geom = _force(tuning, monkeypatch)
    try:
        force(0)
        want, enc_want, ip_want = _run(m, seq, spos, dev, int_preds=True)
        force(1)
        for _ in range(3):
            got, enc_got, ip_got = _run(m, seq, spos, dev, int_preds=True)
            assert torch.equal(got, want) and torch.equal(enc_got, enc_want)
            assert all(torch.equal(a, b) for a, b in zip(ip_got, ip_want))
        plain, _, _ = _run(m, seq, spos, dev)
        assert torch.equal(plain, want)
    finally:
        force(-1)
    if B == 6:
        ref = _ref(name, 6)
        assert max_abs_diff(got, ref['logits']) < ref['tol']


# forced panel heights whose panel, operand vectors and LayerNorm operand rows exceed the 160 KiB of LDS (chain_lds): H rows are
# max(k_h, d_ff) wide, so 20 and 24 rows x (512 + 1024) floats (G5b) and 24 rows x (512 + 768) floats (G5c) do not fit beside the
# modulo-residual rows of layer 0 / the read-out rows of the last block
REFUSED = {('G5b', 19), ('G5b', 20), ('G5c', 20)}


@pytest.mark.parametrize('geometry', [0, 8, 11, 12, 15, 16, 17, 18, 19, 20])
@pytest.mark.parametrize('name', ['G5a', 'G5b', 'G5c'])
def test_G5_chain_every_geometry(dev, tuning, monkeypatch, name, geometry):
    """Every geometry number of test_decoder_chain_every_geometry_is_bit_identical, ragged batch with a partial last panel
    (5 x 90 rows).  A forced panel height that does not fit LDS at this call's widths (REFUSED) is refused with
    LAMP_E_UNSUPPORTED before anything is launched; every other geometry gives the bits of the separate launches."""
    from lamp_amd import _native as N
    m, sd, blocked, seq, spos, g = _build(name, dev, B=5)
    force, geom = _force(tuning, monkeypatch)
    try:
        force(0)
        want, _, _ = _run(m, seq, spos, dev)
        force(1)
        geom(geometry)
        if (name, geometry) in REFUSED:
            with pytest.raises(N.LampError, match='not supported'):
                _run(m, seq, spos, dev)
        else:
            for _ in range(3):
                got, _, _ = _run(m, seq, spos, dev)
                assert torch.equal(got, want)
    finally:
        force(-1)
        geom(-1)


def _launches(m, seq, spos, dev):
    """GEMM-class and LayerNorm launches of one forward (lamp_prof_*)."""
    from lamp_amd import _native as N
    N.prof_enable(True)
    try:
        N.prof_reset()
        out = _run(m, seq, spos, dev)
        torch.cuda.synchronize()
        prof = N.prof_read()
    finally:
        N.prof_enable(False)
    return out, prof


@pytest.mark.parametrize('name', CHAIN)
def test_G5_product_library_takes_the_chain_by_row_count(dev, name):
    """PRODUCT library, no hook: 270 rows (B = 3) take the five separate launches, 540 and 1080 rows the chain -- every sample
    the same bits whatever batch it rides in.  That the chain really runs at 540 rows is read off the launch counters: with the
    weight packs each of the 2 x n_dec sub-chains is ONE GEMM-class launch in place of three and no LayerNorm launch in place
    of two; without the packs (34 panels: below the native layouts' threshold) every sub-chain is five launches."""
    from lamp_amd import _native as N
    m, sd, blocked, seq, spos, g = _build(name, dev, B=12)
    full, enc_full, _ = _run(m, seq, spos, dev)                 # 1080 rows
    half, enc_half, _ = _run(m, seq[:6], spos[:6], dev)         # 540 rows
    small, enc_small, _ = _run(m, seq[:3], spos[:3], dev)       # 270 rows
    assert torch.equal(half, full[:6]) and torch.equal(small, full[:3])
    assert torch.equal(enc_half, enc_full[:6]) and torch.equal(enc_small, enc_full[:3])
    tail, _, _ = _run(m, seq[9:], spos[9:], dev)
    assert torch.equal(tail, full[9:])
    ref = _ref(name, 6)
    assert max_abs_diff(half, ref['logits']) < ref['tol']

    def count(prof, cls):
        return int(prof[cls]['launches'])
    packs = m._native_model()[4]
    assert packs is not None and all(packs[i].fc and packs[i].fc4 for i in range(2 * g['n_dec']))
    (with_packs, _, _), p_on = _launches(m, seq[:6], spos[:6], dev)
    (rows270, _, _), p_270 = _launches(m, seq[:3], spos[:3], dev)
    m.use_chain_packs = False
    m.invalidate_native_cache()
    try:
        _run(m, seq[:6], spos[:6], dev)      # rebuilds the weights-only tables (hoisted query, folded embedding: GEMM launches)
        (no_packs, _, _), p_off = _launches(m, seq[:6], spos[:6], dev)
    finally:
        del m.use_chain_packs
        m.invalidate_native_cache()
    assert torch.equal(with_packs, half) and torch.equal(no_packs, half) and torch.equal(rows270, small)
    n_sub = 2 * g['n_dec']
    d_gemm = count(p_off, 'gemm') - count(p_on, 'gemm')
    d_ln = count(p_off, 'layernorm') - count(p_on, 'layernorm')
    print('%s at 540 rows: GEMM-class launches %d -> %d, LayerNorm launches %d -> %d with the packs' % (
        name, count(p_off, 'gemm'), count(p_on, 'gemm'), count(p_off, 'layernorm'),
        count(p_on, 'layernorm')))
    assert d_gemm == 2 * n_sub and d_ln == 2 * n_sub, (name, d_gemm, d_ln)     # every sub-chain, k_h of both blocks, chained
    assert count(p_270, 'gemm') == count(p_off, 'gemm')          # 270 rows: the separate launches


def test_G5_bit_rules_and_options_at_G5a(dev):
    m, sd, blocked, seq, spos, g = _build('G5a', dev, B=6)
    logits, enc = _check_bit_rules(m, seq, spos, g, dev)
    _check_switches(m, seq, spos, dev, logits, enc, _ref('G5a', 6)['tol'])
    _check_options('G5a', dev, B=6)
