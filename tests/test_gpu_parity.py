"""-m gpu: the HIP path (through the C ABI) against the golden vectors captured from the reference and
against the CPU oracle on the same seeded inputs.  Tolerance: 1e-4 absolute on logits (the
north-star bar), tighter on intermediate tensors; NaN patterns must coincide exactly."""
import pytest
import torch

from conftest import golden_names, load_golden, max_abs_diff
from oracle import lamp_ref as R

pytestmark = pytest.mark.gpu

TOL_LOGIT = 1e-4
TOL_ACT = 5e-5
TOL_ATTN = 1e-5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from lamp_amd import _native as N
    N.lib()  # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def tuning():
    """The -DLAMP_TUNING build of the same sources: the only library that exports the lamp_debug_* hooks."""
    import ctypes
    from lamp_amd import _native as N
    t = N.load_library(N.TUNING_LIB_PATH)
    for name in ('lamp_debug_force_gemm_tile', 'lamp_debug_force_attn'):
        getattr(t, name).argtypes = [ctypes.c_int]
        getattr(t, name).restype = None
    return t


# ------------------------------------------------------------------ building blocks
@pytest.mark.parametrize('M,K,N_', [(1, 4, 1), (7, 36, 5), (64, 64, 64), (90, 512, 512), (200, 128, 96),
                                    (2880, 512, 512), (9664, 512, 512), (333, 1024, 2048),
                                    # row-panel counts around the whole-panels-per-XCD placement (gemm.hip: panel_split)
                                    (513, 64, 70), (1024, 512, 64), (4100, 36, 200), (545, 128, 1536)])
def test_linear_vs_torch_fp64(dev, M, K, N_):
    from lamp_amd import _native as N
    g = torch.Generator().manual_seed(M * 7 + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N_, K, generator=g) / K ** 0.5
    b = torch.randn(N_, generator=g)
    r = torch.randn(M, N_, generator=g)
    ref = (x.double() @ w.double().t() + b.double()).clamp_min(0) + r.double()
    out = N.linear(x.to(dev), w.to(dev), b.to(dev), residual=r.to(dev), relu=True)
    assert max_abs_diff(out, ref) < 2e-5
    ref2 = x.double() @ w.double().t()
    assert max_abs_diff(N.linear(x.to(dev), w.to(dev)), ref2) < 2e-5


@pytest.mark.parametrize('cfg', list(range(1, 19)))
def test_linear_every_tile_config(dev, tuning, cfg):
    """Every GEMM tile configuration of the tuning build (32x32x2 and 16x16x4 MFMA variants) against fp64, on shapes with
    ragged M / N edges and a K that is not a multiple of BK."""
    from lamp_amd import _native as N
    force = tuning.lamp_debug_force_gemm_tile
    try:
        force(cfg)
        for M, K, N_ in ((300, 512, 200), (67, 72, 130), (1, 4, 1)):
            g = torch.Generator().manual_seed(cfg * 100 + M)
            x = torch.randn(M, K, generator=g)
            w = torch.randn(N_, K, generator=g) / K ** 0.5
            b = torch.randn(N_, generator=g)
            r = torch.randn(M, N_, generator=g)
            ref = (x.double() @ w.double().t() + b.double()).clamp_min(0) + r.double()
            out = N.linear(x.to(dev), w.to(dev), b.to(dev), residual=r.to(dev), relu=True, _lib=tuning)
            assert max_abs_diff(out, ref) < 2e-5, (cfg, M, K, N_)
    finally:
        force(0)


def test_linear_detects_transposed_or_shifted_tiles(dev):
    """Asymmetric operands: a swapped row/column mapping in the MFMA epilogue cannot pass."""
    from lamp_amd import _native as N
    M, K, N_ = 130, 40, 70
    x = torch.zeros(M, K)
    x[:, :] = torch.arange(M).view(-1, 1) * 0.01
    x[:, 1] = 1.0
    w = torch.zeros(N_, K)
    w[:, 0] = 1.0
    w[:, 1] = torch.arange(N_) * 3.0
    ref = x.double() @ w.double().t()
    assert max_abs_diff(N.linear(x.to(dev), w.to(dev)), ref) < 1e-4


@pytest.mark.parametrize('d,M', [(4, 37), (64, 37), (512, 37), (1024, 37), (2048, 37), (512, 1), (512, 5), (512, 1025),
                                 (512, 2883)])   # row counts around the XCD-contiguous row order (4 rows per workgroup)
def test_layernorm(dev, d, M):
    from lamp_amd import _native as N
    g = torch.Generator().manual_seed(d + M)
    x = torch.randn(M, d, generator=g) * 3 + 1
    gm, bt = torch.randn(d, generator=g), torch.randn(d, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (d,), gm.double(), bt.double(), 1e-5)
    assert max_abs_diff(N.layernorm(x.to(dev), gm.to(dev), bt.to(dev)), ref) < 2e-5


def test_sdpa_golden_all_masks(dev):
    from lamp_amd.SubLayers import ScaledDotProductAttention
    d, _ = load_golden('sdpa')
    mod = ScaledDotProductAttention(temperature=d['q'].size(-1) ** 0.5).eval()
    for name in ('none', 'keypad', 'shared', 'fullrow'):
        m = d.get('mask_' + name)
        out, attn = mod(d['q'].to(dev), d['k'].to(dev), d['v'].to(dev),
                        attn_mask=m.to(dev) if m is not None else None)
        assert max_abs_diff(out, d['out_' + name]) < TOL_ACT, name
        assert max_abs_diff(attn, d['attn_' + name]) < TOL_ATTN, name
        mod.need_attn = False
        out2, none = mod(d['q'].to(dev), d['k'].to(dev), d['v'].to(dev),
                         attn_mask=m.to(dev) if m is not None else None)
        mod.need_attn = True
        assert none is None and max_abs_diff(out2, d['out_' + name]) < TOL_ACT, name
    assert torch.isnan(out[2, 3]).all()  # fully masked row: NaN, and only there (checked by max_abs_diff)


@pytest.mark.parametrize('lq,lk,dk', [(1, 1, 4), (33, 65, 32), (90, 302, 128), (159, 100, 128), (130, 257, 64),
                                      (300, 300, 128)])
def test_sdpa_vs_oracle_shapes(dev, lq, lk, dk):
    from lamp_amd import _native as N
    g = torch.Generator().manual_seed(lq * 1000 + lk)
    n = 5
    q, k, v = (torch.randn(n, l, dk, generator=g) for l in (lq, lk, lk))
    mask = torch.rand(n, lq, lk, generator=g) < 0.3
    mask[:, :, 0] = False
    ref_o, ref_a = R.sdpa(q.double(), k.double(), v.double(), mask)
    o, a = N.sdpa(q.to(dev), k.to(dev), v.to(dev), mask.to(dev), 1.0 / dk ** 0.5, need_attn=True)
    assert max_abs_diff(o, ref_o) < 2e-5 and max_abs_diff(a, ref_a) < 5e-6
    o2, _ = N.sdpa(q.to(dev), k.to(dev), v.to(dev), mask.to(dev), 1.0 / dk ** 0.5, need_attn=False)
    assert max_abs_diff(o2, ref_o) < 2e-5


@pytest.mark.parametrize('mode', [1, 2, 4, 0x12, 0x22, 0x32, 0x42, 0x14, 0x24, 0x34, 0x41])
@pytest.mark.parametrize('lq,lk,dk', [(90, 302, 128), (70, 33, 64), (200, 513, 32), (5, 1, 16), (300, 130, 128), (260, 70, 24), (260, 40, 24)])
def test_sdpa_every_kernel_variant(dev, tuning, mode, lq, lk, dk):
    """The attention kernels (16-query blocks up to 256 queries or 64 keys, 32-query blocks beyond and for exact maps) with
    1/2/4-way key split must agree with the oracle in every variant, masks and dead rows included."""
    from lamp_amd import _native as N
    force = tuning.lamp_debug_force_attn
    g = torch.Generator().manual_seed(lq + lk + mode)
    n = 3
    q, k, v = (torch.randn(n, l, dk, generator=g) for l in (lq, lk, lk))
    mask = torch.rand(n, lq, lk, generator=g) < 0.4
    mask[:, :, 0] = False
    mask[1, lq // 2, :] = True  # a dead row
    ref_o, ref_a = R.sdpa(q.double(), k.double(), v.double(), mask)
    try:
        force(mode)
        o, _ = N.sdpa(q.to(dev), k.to(dev), v.to(dev), mask.to(dev), 1.0 / dk ** 0.5, need_attn=False, _lib=tuning)
        o2, a2 = N.sdpa(q.to(dev), k.to(dev), v.to(dev), mask.to(dev), 1.0 / dk ** 0.5, need_attn=True, _lib=tuning)
    finally:
        force(0)
    assert max_abs_diff(o, ref_o) < 2e-5
    assert max_abs_diff(o2, ref_o) < 2e-5 and max_abs_diff(a2, ref_a) < 5e-6


@pytest.mark.parametrize('lq,lk,dk,dv', [(256, 40, 128, 128), (257, 40, 128, 128), (16, 16, 128, 128), (17, 191, 128, 72),
                                         (90, 302, 128, 100), (90, 302, 64, 128), (255, 3, 36, 20), (1, 500, 8, 8),
                                         (257, 64, 128, 128), (257, 65, 128, 128), (983, 40, 128, 128), (300, 100, 64, 64)])
def test_sdpa_kernel_choice_boundaries(dev, lq, lk, dk, dv):
    """Either side of the 256-query / 64-key rule, d_v != d_k, a d_v that is a multiple of 4 but not of 8 (must stay off the
    16-query kernel at widths beyond 64), one-tile and many-tile key ranges: out and maps against the oracle."""
    from lamp_amd import _native as N
    g = torch.Generator().manual_seed(lq * 7 + lk + dv)
    n = 3
    q, k = torch.randn(n, lq, dk, generator=g), torch.randn(n, lk, dk, generator=g)
    v = torch.randn(n, lk, dv, generator=g)
    mask = torch.rand(n, lq, lk, generator=g) < 0.35
    mask[:, :, 0] = False
    mask[2, lq // 2, :] = True
    ref_o, ref_a = R.sdpa(q.double(), k.double(), v.double(), mask)
    o, _ = N.sdpa(q.to(dev), k.to(dev), v.to(dev), mask.to(dev), 1.0 / dk ** 0.5, need_attn=False)
    o2, a2 = N.sdpa(q.to(dev), k.to(dev), v.to(dev), mask.to(dev), 1.0 / dk ** 0.5, need_attn=True)
    assert max_abs_diff(o, ref_o) < 2e-5 and max_abs_diff(o2, ref_o) < 2e-5 and max_abs_diff(a2, ref_a) < 5e-6
    o3, _ = N.sdpa(q.to(dev), k.to(dev), v.to(dev), None, 1.0 / dk ** 0.5, need_attn=False)
    assert max_abs_diff(o3, R.sdpa(q.double(), k.double(), v.double(), None)[0]) < 2e-5


def test_sdpa_online_rescale_is_forced(dev):
    """A key in a LATE tile dominates every earlier one, so the running max jumps and the online
    rescale branch really runs (guide rule: a rare data-dependent branch needs its own test)."""
    from lamp_amd import _native as N
    g = torch.Generator().manual_seed(5)
    n, lq, lk, dk = 2, 40, 200, 64
    q, k, v = (torch.randn(n, l, dk, generator=g) for l in (lq, lk, lk))
    k[:, 150] = q[:, 7] * 6.0   # spike in tile 4 for query 7
    k[:, 37] = q[:, 20] * 9.0   # spike in tile 1 for query 20
    ref_o, _ = R.sdpa(q.double(), k.double(), v.double(), None)
    o, _ = N.sdpa(q.to(dev), k.to(dev), v.to(dev), None, 1.0 / dk ** 0.5, need_attn=False)
    assert max_abs_diff(o, ref_o) < 5e-5


@pytest.mark.parametrize('h', [1, 4])
def test_mha_golden(dev, h):
    from lamp_amd.SubLayers import MultiHeadAttention
    d, sd = load_golden('mha_h%d' % h)
    mod = MultiHeadAttention(h, 64, 64 // h, 64 // h)
    mod.load_state_dict(sd)
    mod = mod.to(dev).eval()
    xq, xkv = d['xq'].to(dev), d['xkv'].to(dev)
    o, a = mod(xq, xkv, xkv, attn_mask=d['pad'].to(dev))
    assert max_abs_diff(o, d['out_cross']) < TOL_ACT and max_abs_diff(a, d['attn_cross']) < TOL_ATTN
    o, a = mod(xq, xq, xq, attn_mask=d['slf'].to(dev))
    assert max_abs_diff(o, d['out_self']) < TOL_ACT and max_abs_diff(a, d['attn_self']) < TOL_ATTN
    o, a = mod(xq, xkv, xkv)
    assert max_abs_diff(o, d['out_nomask']) < TOL_ACT and max_abs_diff(a, d['attn_nomask']) < TOL_ATTN


def test_ffn_golden(dev):
    from lamp_amd.SubLayers import PositionwiseFeedForward
    d, sd = load_golden('ffn')
    mod = PositionwiseFeedForward(64, 128)
    mod.load_state_dict(sd)
    mod = mod.to(dev).eval()
    assert max_abs_diff(mod(d['x'].to(dev)), d['out']) < TOL_ACT


# ------------------------------------------------------------------ whole model, golden
def _build(name, dev):
    from test_host_cpu import build_from_fixture
    m, d, sd = build_from_fixture(name)
    m.load_state_dict(sd)
    return m.to(dev).eval(), d, sd


@pytest.mark.parametrize('name', golden_names('model_'))
def test_model_golden(dev, name):
    m, d, sd = _build(name, dev)
    src = (d['src_seq'].to(dev), d['src_pos'].to(dev))
    logits, enc, third = m(src, None, None, None)
    assert third is None and logits.shape == d['logits'].shape and logits.grad_fn is None
    tol = max(TOL_LOGIT, 3 * d.get('ref_gap', 0.0))
    assert max_abs_diff(enc, d['enc_output']) < TOL_ACT
    assert max_abs_diff(logits, d['logits']) < tol
    if 'logits_fp64' in d:  # conditioning sweep
        assert max_abs_diff(logits, d['logits_fp64']) <= max(1e-4, 3 * d['ref_gap'])
    if any(k.startswith('attn_') for k in d):
        lg, en, enc_attns, dec2 = m(src, None, None, None, return_attns=True)
        assert max_abs_diff(lg, d['logits']) < tol
        assert len(enc_attns) == 1 and len(dec2) == 2
        for i, a in enumerate(enc_attns[0]):
            assert max_abs_diff(a, d['attn_enc_%d' % i]) < TOL_ATTN
        for i, a in enumerate(dec2[0]):
            assert max_abs_diff(a, d['attn_dec_slf_%d' % i]) < TOL_ATTN
        for i, a in enumerate(dec2[1]):
            assert max_abs_diff(a, d['attn_dec_enc_%d' % i]) < TOL_ATTN
    if 'int_pred_0' in d:
        lg, en, ips = m(src, None, None, None, int_preds=True)
        assert len(ips) == 3 and max_abs_diff(lg, d['logits']) < tol
        for i, p in enumerate(ips):
            assert max_abs_diff(p, d['int_pred_%d' % i]) < TOL_LOGIT
    # module-by-module route (what lamp/Translator.py-style callers use) agrees with the fused launcher: bit for bit with the
    # unfolded launcher (the modules launch encoder layer 0's W1 GEMM), in the last bits with the folded tables
    enc2, _ = m.encoder(src[0], None, src[1])
    y, _ = m.decoder(None, src[0], enc2)
    from lamp_amd import _native as N
    lg2 = N.diag_logits(y, m.tgt_word_proj.linear.weight)
    assert m.fold_embedding
    assert max_abs_diff(enc2, enc) < 2e-5 and max_abs_diff(lg2, logits) < max(2e-5, tol)   # tol: the sharp-softmax fixtures (G13)
    m.fold_embedding = False
    try:
        logits_u, enc_u, _ = m(src, None, None, None)
    finally:
        del m.fold_embedding
    assert max_abs_diff(enc2, enc_u) == 0.0
    assert max_abs_diff(lg2, logits_u) < 1e-6
    assert max_abs_diff(logits_u, d['logits']) < tol and max_abs_diff(enc_u, d['enc_output']) < TOL_ACT


# ------------------------------------------------------------------ whole model, BASELINE sizes vs oracle
CONFIGS = {
    # name: V, L, T, d, dff, h, mask, pos_emb, B, p, lengths
    'reuters_fixed': (23666, 90, 302, 512, 512, 4, 'prior', True, 6, 0.10, None),
    'reuters_ragged': (23666, 90, 302, 512, 512, 4, 'prior', True, 6, 0.10, [302, 20, 150, 77, 201, 33]),
    'bibtex': (1840, 159, 100, 512, 1024, 4, 'prior', False, 4, 0.05, None),
    'delicious': (504, 983, 40, 1024, 2048, 8, 'none', False, 2, 0.0, [40, 17]),
    'inveye_8h': (300, 70, 50, 256, 512, 8, 'inveye', True, 3, 0.0, [50, 1, 23]),
    # 4096 labels (configs[4]'s label graph: 128 key tiles per label row, sparse prior mask), narrow model
    'labels4096': (500, 4096, 64, 256, 512, 2, 'prior', True, 2, 0.05, [64, 30]),
    # BASELINE.json configs[1] / configs[2] at their full batch, directly against the oracle (0.15 / 0.3 s of CPU)
    'reuters_b32': (23666, 90, 302, 512, 512, 4, 'prior', True, 32, 0.10, None),
    'bibtex_b32': (1840, 159, 100, 512, 1024, 4, 'prior', False, 32, 0.05, None),
    'reuters_b32_ragged': (23666, 90, 302, 512, 512, 4, 'prior', True, 32, 0.10,
                           [302, 20, 150, 77, 201, 33, 288, 9, 64, 65, 16, 17, 191, 192, 193, 48] * 2),
    # BASELINE.json configs[4] EXACTLY: 4096 labels x 512 tokens, d_model 1024, 8 heads, d_ff 2048,
    # prior p = 0.05 -- one full and one ragged sample (the oracle needs ~0.8 TFLOP and ~2 GB of host memory), and
    # its fully connected variant
    'synthetic4096_full': (32004, 4096, 512, 1024, 2048, 8, 'prior', True, 2, 0.05, [512, 300]),
    'synthetic4096_full_none': (32004, 4096, 512, 1024, 2048, 8, 'none', True, 1, 0.0, None),
}


def make_case(cfg, dev, seed=0, qk_scale=1.0):
    from lamp_amd.Models import LAMP
    V, L, T, d, dff, h, mask, pos, B, p, lengths = cfg
    sd = R.make_state_dict(V, L, T, d, dff, h, 2, 2, pos_emb=pos, seed=seed)
    if qk_scale != 1.0:   # sharper attention, as trained weights have it
        for k in sd:
            if k.startswith('decoder.') and ('w_qs' in k or 'w_ks' in k):
                sd[k] = sd[k] * qk_scale
    adj = R.make_adjacency(L, p, seed) if mask == 'prior' else None
    seq, spos = R.make_batch(B, V, T, lengths=lengths, seed=seed)
    m = LAMP(V, L, T, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d,
             d_inner_hid=dff, d_k=d // h, d_v=d // h, encoder='graph', decoder='graph',
             no_enc_pos_embedding=not pos, label_adj_matrix=adj.clone() if adj is not None else None,
             label_mask=mask, dec_dropout2=False)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    blocked = R.label_block_mask(adj, mask, L)
    return m, sd, blocked, seq, spos, h


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_model_vs_oracle_at_baseline_sizes(dev, name):
    m, sd, blocked, seq, spos, h = make_case(CONFIGS[name], dev)
    with torch.no_grad():
        ref_logits, ref_enc, _ = R.forward(sd, seq, spos, h, blocked)
    logits, enc, _ = m((seq.to(dev), spos.to(dev)), None, None, None)
    assert max_abs_diff(enc, ref_enc) < TOL_ACT
    assert max_abs_diff(logits, ref_logits) < TOL_LOGIT


@pytest.mark.parametrize('name,B', [('reuters_fixed', 4), ('reuters_ragged', 6), ('delicious', 2)])
def test_sharp_attention_at_real_width(dev, name, B):
    """Conditioning at the BASELINE widths: decoder Q / K weights x3 make the softmax as peaked as
    trained weights do.  The yardstick is the oracle evaluated in fp64; the bar is max(1e-4, 3 x the fp32 oracle's own
    distance from it)."""
    cfg = list(CONFIGS[name])
    cfg[8] = B
    if cfg[10] is not None:
        cfg[10] = cfg[10][:B]
    m, sd, blocked, seq, spos, h = make_case(tuple(cfg), dev, qk_scale=3.0)
    with torch.no_grad():
        ref32, _, _ = R.forward(sd, seq, spos, h, blocked)
        ref64, _, _ = R.forward(R.to_dtype(sd, torch.float64), seq, spos, h, blocked)
    gap = max_abs_diff(ref32, ref64)
    logits, _, _ = m((seq.to(dev), spos.to(dev)), None, None, None)
    assert max_abs_diff(logits, ref64) <= max(1e-4, 3 * gap), (max_abs_diff(logits, ref64), gap)


# ------------------------------------------------------------------ size-independent properties
def test_samples_are_independent_bitwise(dev):
    """Sharding contract: a sample's logits do not depend on what else is in the batch,
    on the batch size, or on the micro-batch split -- bit for bit."""
    cfg = list(CONFIGS['reuters_ragged'])
    cfg[8] = 32
    cfg[10] = [302, 20, 150, 77, 201, 33, 302, 9] * 4
    m, sd, blocked, seq, spos, h = make_case(tuple(cfg), dev)
    seq, spos = seq.to(dev), spos.to(dev)
    full, enc_full, _ = m((seq, spos), None, None, None)
    assert not torch.isnan(full).any()
    for lo, hi in ((0, 16), (16, 32), (5, 6), (31, 32)):
        part, enc_part, _ = m((seq[lo:hi], spos[lo:hi]), None, None, None)
        assert torch.equal(part, full[lo:hi])
        assert torch.equal(enc_part, enc_full[lo:hi])
    # a batch twice as large (other tile / grid choices may apply) still reproduces every sample
    big, _, _ = m((torch.cat([seq, seq]), torch.cat([spos, spos])), None, None, None)
    assert torch.equal(big[:32], full) and torch.equal(big[32:], full)
    perm = torch.randperm(32, generator=torch.Generator().manual_seed(1)).to(dev)
    shuffled, _, _ = m((seq[perm], spos[perm]), None, None, None)
    assert torch.equal(shuffled, full[perm])
    # micro-batching inside lamp_forward: squeeze the workspace so the batch is split
    m.workspace_limit_bytes = 96 << 20
    split, enc_split, _ = m((seq, spos), None, None, None)
    assert torch.equal(split, full) and torch.equal(enc_split, enc_full)


def test_delicious_batch32_properties_bitwise(dev):
    """BASELINE.json configs[3] at its full batch (983 labels, d_model 1024, 8 heads, mask none, B = 32): too large for
    the oracle in seconds, so it is tied to the oracle-checked B = 2 case through the size-independent properties --
    every sample equals its own single-sample / sliced / permuted / micro-batched run bit for bit."""
    cfg = list(CONFIGS['delicious'])
    cfg[8] = 32
    cfg[10] = [40, 17, 5, 33] * 8
    m, sd, blocked, seq, spos, h = make_case(tuple(cfg), dev)
    seq, spos = seq.to(dev), spos.to(dev)
    full, enc_full, _ = m((seq, spos), None, None, None)
    assert torch.isfinite(full).all()
    # samples 0 and 1 are exactly the oracle-checked 'delicious' case (same seed, same lengths)
    with torch.no_grad():
        ref, ref_enc, _ = R.forward(sd, seq[:2].cpu(), spos[:2].cpu(), h, blocked)
    assert max_abs_diff(full[:2], ref) < TOL_LOGIT and max_abs_diff(enc_full[:2], ref_enc) < TOL_ACT
    for lo, hi in ((0, 2), (0, 16), (16, 32), (7, 8)):
        part, enc_part, _ = m((seq[lo:hi], spos[lo:hi]), None, None, None)
        assert torch.equal(part, full[lo:hi]) and torch.equal(enc_part, enc_full[lo:hi])
    perm = torch.randperm(32, generator=torch.Generator().manual_seed(2)).to(dev)
    shuffled, _, _ = m((seq[perm], spos[perm]), None, None, None)
    assert torch.equal(shuffled, full[perm])
    m.workspace_limit_bytes = 512 << 20   # forces micro-batches inside lamp_forward
    split, enc_split, _ = m((seq, spos), None, None, None)
    assert torch.equal(split, full) and torch.equal(enc_split, enc_full)


def test_synthetic4096_micro_batched_share_bitwise(dev):
    """BASELINE.json configs[4] as one GPU runs it: its 1024-sample share does not fit one pass, lamp_forward walks it in
    micro-batches carved from the workspace.  Here 16 samples under a squeezed workspace limit (several micro-batches, the
    last one ragged in size): every sample equals its run in the unsplit batch bit for bit, and samples 0-1 -- the
    oracle-checked 'synthetic4096_full' pair (same seed, same lengths) -- are within the north-star tolerance of the
    oracle."""
    cfg = list(CONFIGS['synthetic4096_full'])
    cfg[8] = 16
    cfg[10] = [512, 300] + [512, 77, 410, 512, 3, 256, 512, 129, 500, 64, 512, 511, 33, 200]
    m, sd, blocked, seq, spos, h = make_case(tuple(cfg), dev)
    seq, spos = seq.to(dev), spos.to(dev)
    full, enc_full, _ = m((seq, spos), None, None, None)
    assert torch.isfinite(full).all()
    with torch.no_grad():
        ref, ref_enc, _ = R.forward(sd, seq[:2].cpu(), spos[:2].cpu(), h, blocked)
    assert max_abs_diff(full[:2], ref) < TOL_LOGIT and max_abs_diff(enc_full[:2], ref_enc) < TOL_ACT
    for limit_mb in (768, 300):
        m.workspace_limit_bytes = limit_mb << 20
        split, enc_split, _ = m((seq, spos), None, None, None)
        assert torch.equal(split, full) and torch.equal(enc_split, enc_full), limit_mb
    pair, _, _ = m((seq[:2], spos[:2]), None, None, None)
    assert torch.equal(pair, full[:2])


@pytest.mark.parametrize('name,B,lengths', [
    ('reuters_b32', 32, None),                      # the headline shape: 2880 rows = 180 full panels
    ('reuters_b32_ragged', 32, 'cfg'),
    ('reuters_fixed', 3, None),                     # 270 rows: 16 full panels and one of 14 rows
    ('reuters_fixed', 1, None),                     # 90 rows: 5 full panels and one of 10 rows
    ('inveye_8h', 3, [50, 1, 23]),                  # d_model 256 (one float4 per lane in the LayerNorm), 8 heads, 70 labels
])
def test_decoder_chain_launch_is_bit_identical(dev, tuning, monkeypatch, name, B, lengths):
    """chain.hip: the attention output projection (+ residual), its LayerNorm and the position-wise feed-forward block of a
    decoder layer as ONE launch over 16-row panels.  lamp_forward picks it from the row count alone, so it must give the
    bits of the five separate launches: logits, intermediate read-outs and encoder rows with the chain forced on and
    forced off (tuning build of the library), plus the oracle bar on the forced-on run."""
    import ctypes
    from lamp_amd import _native as N
    cfg = list(CONFIGS[name])
    cfg[8] = B
    if lengths != 'cfg':
        cfg[10] = lengths
    m, sd, blocked, seq, spos, h = make_case(tuple(cfg), dev)
    monkeypatch.setattr(N, '_lib', tuning)
    force = tuning.lamp_debug_force_chain
    force.argtypes = [ctypes.c_int]
    force.restype = None
    src = (seq.to(dev), spos.to(dev))
    try:
        force(0)
        want, enc_want, ip_want = m(src, None, None, None, int_preds=True)
        force(1)
        for _ in range(3):   # a race between the W stream's LDS-DMA and the fragment reads would not repeat
            got, enc_got, ip_got = m(src, None, None, None, int_preds=True)
            assert torch.equal(got, want) and torch.equal(enc_got, enc_want)
            assert all(torch.equal(a, b) for a, b in zip(ip_got, ip_want))
        plain, _, _ = m(src, None, None, None)
        assert torch.equal(plain, want)
    finally:
        force(-1)
    with torch.no_grad():
        ref, _, _ = R.forward(sd, seq, spos, h, blocked)
    assert max_abs_diff(got, ref) < TOL_LOGIT


@pytest.mark.parametrize('geometry', [0, 8, 11, 12, 15, 16, 17, 18, 19, 20])
def test_decoder_chain_every_geometry_is_bit_identical(dev, tuning, monkeypatch, geometry):
    """Every geometry of the chain launch the product routes to, forced in the tuning build -- native weights through one LDS
    slot per wave (0), the packed stream with the operands from global memory (8), the round-5 kernel on packed weights with
    the LayerNorm / bias operands in LDS (12; 11: the same kernel on two register sets, tuning build only), panels of 4 to 24 rows on the 4x4x1 MFMA (15-20): same k-order -- the bits of the
    separate launches, ragged batch with a partial last panel."""
    import ctypes
    from lamp_amd import _native as N
    cfg = list(CONFIGS['reuters_ragged'])
    cfg[8], cfg[10] = 5, [302, 20, 150, 77, 201]
    m, sd, blocked, seq, spos, h = make_case(tuple(cfg), dev)
    monkeypatch.setattr(N, '_lib', tuning)
    force, geom = tuning.lamp_debug_force_chain, tuning.lamp_debug_chain_geometry
    for f in (force, geom):
        f.argtypes = [ctypes.c_int]
        f.restype = None
    src = (seq.to(dev), spos.to(dev))
    try:
        force(0)
        want, _, _ = m(src, None, None, None)
        force(1)
        geom(geometry)
        for _ in range(3):
            got, _, _ = m(src, None, None, None)
            assert torch.equal(got, want)
    finally:
        force(-1)
        geom(-1)


@pytest.mark.parametrize('seed', range(10))
def test_decoder_chain_random_models_bit_identical(dev, tuning, monkeypatch, seed):
    """Random chain-eligible models (d_model 512; d_ff 512 or 1024 -- the latter fills the 160 KiB of LDS exactly; 4 or 8 heads;
    1-3 decoder layers with or without label self-attention; any label count, batch and ragged lengths, i.e. any number of
    panels incl. a partial last one): chain forced on == chain forced off, bit for bit, and within the north-star bar of the
    oracle."""
    import ctypes
    import random
    from lamp_amd import _native as N
    from lamp_amd.Models import LAMP
    rng = random.Random(900 + seed)
    d, dff, h = 512, rng.choice([512, 1024]), rng.choice([4, 8])
    L, T, B = rng.choice([7, 16, 33, 90, 159]), rng.choice([9, 40, 77]), rng.randint(1, 9)
    n_dec, no_slf, mask, pos = rng.randint(1, 3), rng.random() < 0.3, rng.choice(['prior', 'none', 'inveye']), rng.random() < 0.5
    V = 300
    sd = R.make_state_dict(V, L, T, d, dff, h, 1, n_dec, pos_emb=pos, seed=seed, no_dec_self_att=no_slf)
    adj = R.make_adjacency(L, 0.2, seed) if mask == 'prior' else None
    lengths = [rng.randint(1, T) for _ in range(B)]
    lengths[rng.randrange(B)] = T
    seq, spos = R.make_batch(B, V, T, lengths=lengths, seed=seed)
    m = LAMP(V, L, T, L, n_layers_enc=1, n_layers_dec=n_dec, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=dff,
             d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', no_enc_pos_embedding=not pos, no_dec_self_att=no_slf,
             label_adj_matrix=adj.clone() if adj is not None else None, label_mask=mask, dec_dropout2=False)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    monkeypatch.setattr(N, '_lib', tuning)
    force = tuning.lamp_debug_force_chain
    force.argtypes = [ctypes.c_int]
    force.restype = None
    src = (seq.to(dev), spos.to(dev))
    try:
        force(0)
        want, enc_want, _ = m(src, None, None, None)
        force(1)
        got, enc_got, _ = m(src, None, None, None)
    finally:
        force(-1)
    assert torch.equal(got, want) and torch.equal(enc_got, enc_want), (d, dff, h, L, T, B, n_dec, no_slf)
    with torch.no_grad():
        ref, _, _ = R.forward(sd, seq, spos, h, R.label_block_mask(adj, mask, L))
    assert max_abs_diff(got, ref) < TOL_LOGIT


def test_decoder_chain_without_self_attention_and_odd_batches(dev, tuning, monkeypatch):
    """The chain behind the enc-dec attention of a decoder WITHOUT label self-attention (no_dec_self_att: pos_ffn2 follows
    pos_ffn1 directly and stays a launch of its own), and the row-count rule of the product library: a batch just below and
    just above 256 panels gives every sample the same bits."""
    import ctypes
    from lamp_amd import _native as N
    from lamp_amd.Models import LAMP
    V, L, T, d, dff, h = 500, 90, 40, 512, 512, 4
    sd = R.make_state_dict(V, L, T, d, dff, h, 2, 2, pos_emb=True, seed=3, no_dec_self_att=True)
    adj = R.make_adjacency(L, 0.1, 3)
    m = LAMP(V, L, T, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=dff,
             d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', no_dec_self_att=True,
             label_adj_matrix=adj.clone(), label_mask='prior', dec_dropout2=False)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    seq, spos = R.make_batch(50, V, T, lengths=[40, 7, 33, 12, 1] * 10, seed=3)
    seq, spos = seq.to(dev), spos.to(dev)
    big, _, _ = m((seq, spos), None, None, None)            # 4500 rows: 20-row panels with packed weights (282 sixteen-row panels: separate launches without)
    small, _, _ = m((seq[:45], spos[:45]), None, None, None)  # 4050 rows = 254 panels: the chain
    assert torch.equal(small, big[:45])
    monkeypatch.setattr(N, '_lib', tuning)
    force = tuning.lamp_debug_force_chain
    force.argtypes = [ctypes.c_int]
    force.restype = None
    try:
        force(0)
        off, _, _ = m((seq, spos), None, None, None)
        force(1)
        on, _, _ = m((seq, spos), None, None, None)
    finally:
        force(-1)
    assert torch.equal(on, off) and torch.equal(on, big)
    with torch.no_grad():
        ref, _, _ = R.forward(sd, seq[:4].cpu(), spos[:4].cpu(), h, R.label_block_mask(adj, 'prior', L))
    assert max_abs_diff(big[:4], ref) < TOL_LOGIT


def test_weight_pack_formats_are_exact_rearrangements(dev):
    """lamp_pack_weight (the weights-only repack behind lamp_model.chain_packs): both formats are pure gathers of W -- format 0
    per 16 columns x 32 k the two 16x16x4 fragment chunks lane by lane, format 1 per 64 columns x 16 k the four k-quads column
    by column -- checked element for element against index arithmetic (include/lamp_hip.h: lamp_pack_weight)."""
    from lamp_amd import _native as N
    g = torch.Generator().manual_seed(5)
    for n, k in ((64, 32), (512, 512), (1024, 512), (128, 1024)):
        w = torch.randn(n, k, generator=g)
        p0 = N.weight_pack(w.to(dev), 0).cpu()
        l = torch.arange(64)
        want0 = w.view(n // 16, 16, k // 32, 2, 4, 4)          # [cb, row, kt, c, quad, j]
        want0 = want0.permute(0, 2, 3, 4, 1, 5)                # [cb, kt, c, quad (= lane >> 4), row (= lane & 15), j]
        assert torch.equal(p0, want0.reshape(-1)), (n, k)
        p1 = N.weight_pack(w.to(dev), 1).cpu()
        want1 = w.view(n // 64, 64, k // 16, 4, 4).permute(0, 2, 3, 1, 4)   # [cb, ch, quad, column (= lane), j]
        assert torch.equal(p1, want1.reshape(-1)), (n, k)
    assert N.weight_pack(torch.randn(24, 48).to(dev), 0) is None and N.weight_pack(torch.randn(32, 64).to(dev), 1) is None
    with pytest.raises(N.LampError):   # misaligned source
        big = torch.randn(64 * 32 + 1).to(dev)
        out = torch.empty(64 * 32, device=dev)
        N.check(N.lib().lamp_pack_weight(big.data_ptr() + 4, 64, 32, 32, 0, out.data_ptr(), N.stream()), 'lamp_pack_weight')


def test_chain_routes_of_the_product_library_give_every_sample_the_same_bits(dev):
    """PRODUCT library, no debug hook: the decoder's row-local tail runs, by row count, as five launches (< 512 rows, > 6144),
    as panels of 4, 8, 12, 20 or 24 rows on the 4x4x1 MFMA (<= 1024 / 2048 / 3072 / 5120 / 6144 rows), or as sixteen-row panels
    (3073-4096 rows) -- from packed
    weights -- and from the native weight layouts (use_chain_packs = False: sixteen-row panels for 2049-4096 rows).  One pool
    of samples through every route: each sample's logits, encoder rows and intermediate read-outs come out bit-identical
    whatever batch it rides in, with and without the packs; a weight update through .data invalidates the packs."""
    from lamp_amd.Models import LAMP
    V, L, T, d, dff, h = 400, 90, 24, 512, 512, 4
    sd = R.make_state_dict(V, L, T, d, dff, h, 1, 2, pos_emb=True, seed=11)
    adj = R.make_adjacency(L, 0.1, 11)
    m = LAMP(V, L, T, L, n_layers_enc=1, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=dff,
             d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', label_adj_matrix=adj.clone(), label_mask='prior',
             dec_dropout2=False)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    B = 70   # 6300 rows: the five separate launches
    seq, spos = R.make_batch(B, V, T, lengths=[T, 3, 17, 9, 24] * 14, seed=11)
    seq, spos = seq.to(dev), spos.to(dev)
    assert m.use_chain_packs
    ref, enc_ref, ip_ref = m((seq, spos), None, None, None, int_preds=True)       # 6300 rows: separate launches
    r64, _, ip64 = m((seq[:64], spos[:64]), None, None, None, int_preds=True)     # 5760 rows: 24-row panels
    assert torch.equal(r64, ref[:64]) and all(torch.equal(a, w[:64]) for a, w in zip(ip64, ip_ref))
    packs = m._native_model()[4]
    assert packs is not None and packs[0].fc and packs[0].fc4 and packs[3].w24
    for b in (4, 8, 12, 20, 24, 32, 40, 45, 48):   # 360 (separate), 720, 1080, 1800, 2160, 2880, 3600, 4050, 4320 (20-row panels) rows
        for lo in (0, B - b):
            got, enc, ip = m((seq[lo:lo + b], spos[lo:lo + b]), None, None, None, int_preds=True)
            assert torch.equal(got, ref[lo:lo + b]) and torch.equal(enc, enc_ref[lo:lo + b]), (b, lo)
            assert all(torch.equal(a, w[lo:lo + b]) for a, w in zip(ip, ip_ref)), (b, lo)
            plain, _, _ = m((seq[lo:lo + b], spos[lo:lo + b]), None, None, None)
            assert torch.equal(plain, got), (b, lo)
    try:
        LAMP.use_chain_packs = False
        m.invalidate_native_cache()
        assert m._native_model()[4] is None
        for b in (20, 32, 40):
            got, _, ip = m((seq[:b], spos[:b]), None, None, None, int_preds=True)
            assert torch.equal(got, ref[:b]) and all(torch.equal(a, w[:b]) for a, w in zip(ip, ip_ref)), b
    finally:
        LAMP.use_chain_packs = True
        m.invalidate_native_cache()
    # the packs follow the weights: an in-place update (what an optimiser does) must not leave a stale copy behind
    with torch.no_grad():
        m.decoder.layer_stack[1].pos_ffn2.w_2.weight.mul_(1.5)
    m.invalidate_native_cache()
    upd, _, _ = m((seq[:32], spos[:32]), None, None, None)
    small, _, _ = m((seq[:4], spos[:4]), None, None, None)          # separate launches read the weights themselves
    assert torch.equal(upd[:4], small) and not torch.equal(upd, ref[:32])


def test_chain_over_two_halves_of_a_large_batch(dev):
    """Just past one chain launch's reach (6145-12288 decoder rows) the row-local tail runs as two chain launches over halves of
    the batch, whole samples each (api.hip: mha_tail), when both halves take 24-row panels.  Batch 136 (68 + 68 samples = 6120
    rows each), 128 (2 x 5760) and 105 (53 + 52: 4770 / 4680 rows) take that route; 100 (50 + 50: 4500 rows) and 140 keep the five
    separate launches.  All against the same samples in batches of four (360 rows: separate launches): logits, encoder rows and
    intermediate read-outs bit for bit."""
    from lamp_amd.Models import LAMP
    V, L, T, d, dff, h = 400, 90, 16, 512, 512, 4
    sd = R.make_state_dict(V, L, T, d, dff, h, 1, 2, pos_emb=True, seed=21)
    adj = R.make_adjacency(L, 0.1, 21)
    m = LAMP(V, L, T, L, n_layers_enc=1, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=dff,
             d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', label_adj_matrix=adj.clone(), label_mask='prior',
             dec_dropout2=False)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    B = 140
    seq, spos = R.make_batch(B, V, T, lengths=[T, 3, 11, 9, 16] * 28, seed=21)
    seq, spos = seq.to(dev), spos.to(dev)
    small = {}
    for lo in (0, 48, 51, 52, 64, 66, 68, 100, 132, 136):
        small[lo] = m((seq[lo:lo + 4], spos[lo:lo + 4]), None, None, None, int_preds=True)
    for b in (140, 136, 128, 105, 100):
        got, enc, ip = m((seq[:b], spos[:b]), None, None, None, int_preds=True)
        plain, _, _ = m((seq[:b], spos[:b]), None, None, None)
        assert torch.equal(plain, got), b
        for lo, (w, w_enc, w_ip) in small.items():
            if lo + 4 <= b:
                assert torch.equal(got[lo:lo + 4], w) and torch.equal(enc[lo:lo + 4], w_enc), (b, lo)
                assert all(torch.equal(a[lo:lo + 4], x) for a, x in zip(ip, w_ip)), (b, lo)


def test_chain_with_operand_rows_in_dead_panel_regions_bibtex_shape(dev):
    """d_ff = 1024 at bibtex's 159 labels: batch 32 = 5088 rows = 255 panels of twenty rows, whose LayerNorm operand rows no longer
    fit LDS beside the panel -- the modulo-residual rows of layer 0's first block then live in the unused upper half of the
    hidden rows while the fc step runs, the read-out rows of the last block are loaded into the hidden region after the W2 step
    (chain.hip: res_alias / wout_late).  Same samples through batch 32 (all four sub-chains as chain launches), batch 40
    (6360 rows: five separate launches each) and batch 3 (477 rows: separate launches): bit-identical logits, encoder rows and
    intermediate read-outs; a partial last panel (batch 31: 4929 rows) included."""
    from lamp_amd.Models import LAMP
    V, L, T, d, dff, h = 300, 159, 20, 512, 1024, 4
    sd = R.make_state_dict(V, L, T, d, dff, h, 1, 2, pos_emb=False, seed=5)
    adj = R.make_adjacency(L, 0.05, 5)
    m = LAMP(V, L, T, L, n_layers_enc=1, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=dff,
             d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', label_adj_matrix=adj.clone(), label_mask='prior',
             dec_dropout2=False, no_enc_pos_embedding=True)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    B = 40
    seq, spos = R.make_batch(B, V, T, lengths=[T, 3, 17, 9, 20] * 8, seed=5)
    seq, spos = seq.to(dev), spos.to(dev)
    assert m.use_chain_packs
    ref, enc_ref, ip_ref = m((seq, spos), None, None, None, int_preds=True)       # 6360 rows: separate launches
    for b in (32, 31, 3, 26):                                                     # 5088, 4929 (20-row panels), 477, 4134 rows
        for lo in (0, B - b):
            got, enc, ip = m((seq[lo:lo + b], spos[lo:lo + b]), None, None, None, int_preds=True)
            assert torch.equal(got, ref[lo:lo + b]) and torch.equal(enc, enc_ref[lo:lo + b]), (b, lo)
            assert all(torch.equal(a, w[lo:lo + b]) for a, w in zip(ip, ip_ref)), (b, lo)
            plain, _, _ = m((seq[lo:lo + b], spos[lo:lo + b]), None, None, None)   # without int_preds: the fused read-out
            assert torch.equal(plain, got), (b, lo)
    for _ in range(20):   # a load consumed before it landed would not repeat
        again, _, _ = m((seq[:32], spos[:32]), None, None, None)
        assert torch.equal(again, ref[:32])
    oracle, _, _ = R.forward(R.to_dtype({k: v.detach().cpu() for k, v in m.state_dict().items()}, torch.float64),
                             seq[:32].cpu(), spos[:32].cpu(), h, R.label_block_mask(adj, 'prior', L))
    assert max_abs_diff(ref[:32], oracle) < 1e-4


def test_chain_launches_survive_a_busy_neighbour_stream(dev):
    """The hand-scheduled chain kernels under contention: 300 back-to-back forwards at the headline decoder shape (2880 rows:
    twelve-row panels) and 100 at 3600 rows (sixteen-row panels) while a second stream keeps the K/V-projection GEMM running on
    the same device -- every result equals the first, bit for bit.  A load consumed before it landed would not repeat."""
    from lamp_amd import _native as N
    from lamp_amd.Models import LAMP
    V, L, T, d, dff, h = 400, 90, 30, 512, 512, 4
    sd = R.make_state_dict(V, L, T, d, dff, h, 2, 2, pos_emb=True, seed=2)
    adj = R.make_adjacency(L, 0.1, 2)
    m = LAMP(V, L, T, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=dff,
             d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', label_adj_matrix=adj.clone(), label_mask='prior',
             dec_dropout2=False)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    seq, spos = R.make_batch(40, V, T, seed=2)
    seq, spos = seq.to(dev), spos.to(dev)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(9664, 512, generator=g).to(dev)
    w = (torch.randn(2048, 512, generator=g) / 512 ** 0.5).to(dev)
    side = torch.cuda.Stream(device=dev)
    for b, n in ((32, 300), (40, 100)):
        src = (seq[:b], spos[:b])
        first, enc_first, _ = m(src, None, None, None)
        torch.cuda.synchronize()
        outs = []
        for i in range(n):
            if i % 4 == 0:
                with torch.cuda.stream(side):
                    N.linear(x, w)
            outs.append(m(src, None, None, None)[0])
        torch.cuda.synchronize()
        bad = [i for i, o in enumerate(outs) if not torch.equal(o, first)]
        assert not bad, (b, bad[:10])


@pytest.mark.parametrize('M', [3, 1019, 3067, 5115, 9665, 10235])
def test_slab_gemm_experiment_is_bit_identical(dev, tuning, M):
    """slab.hip (tuning build only; profiles/r05_rejected_experiments.txt): a GEMM over row slabs on the 4x4x1 MFMA from format-1
    weight packs -- one to ten row groups per workgroup, bias / ReLU / residual epilogues, two segments sharing A, and a live
    row count in device memory (ragged batches) -- gives the bits of the tile kernel."""
    import ctypes
    from lamp_amd import _native as N
    fn = tuning.lamp_debug_slab_gemm
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
                   ctypes.c_void_p, ctypes.c_void_p]
    K = Nn = 512
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(dev)
    ws = [(torch.randn(Nn, K, generator=g) / K ** 0.5).to(dev) for _ in range(2)]
    wq = [N.weight_pack(w, 1) for w in ws]
    b = torch.randn(Nn, generator=g).to(dev)
    r = torch.randn(M, Nn, generator=g).to(dev)
    for nseg, bias, res, relu in ((1, b, None, 1), (1, b, r, 0), (2, None, None, 0)):
        want = [N.linear(x, w, bias, residual=res, relu=bool(relu)) for w in ws[:nseg]]
        outs = [torch.full((M, Nn), float('nan'), device=dev) for _ in range(nseg)]
        for _ in range(2):
            N.check(fn(x.data_ptr(), M, K, K, wq[0].data_ptr(), wq[1].data_ptr() if nseg > 1 else None, Nn, N.ptr(bias), N.ptr(res), Nn, relu,
                       outs[0].data_ptr(), outs[1].data_ptr() if nseg > 1 else None, Nn, None, N.stream()), 'slab')
            assert all(torch.equal(a, w_) for a, w_ in zip(outs, want)), (M, nseg)
    if M > 100:   # live rows from device memory: the rows past them stay untouched
        live = M * 3 // 5
        m_dev = torch.tensor([live, live], dtype=torch.int32, device=dev)
        out = torch.full((M, Nn), 7.0, device=dev)
        N.check(fn(x.data_ptr(), M, K, K, wq[0].data_ptr(), None, Nn, N.ptr(b), None, Nn, 1, out.data_ptr(), None, Nn, m_dev.data_ptr(),
                   N.stream()), 'slab')
        assert torch.equal(out[:live], N.linear(x[:live], ws[0], b, relu=True)) and bool((out[live:] == 7.0).all())


def test_requested_maps_do_not_change_logits(dev):
    """Requested maps come from the same single-pass kernels (scores + row log-sum-exp written on the side): the
    logits do not change by a bit when maps or intermediate predictions are asked for, nor under micro-batching."""
    cfg = list(CONFIGS['reuters_ragged'])
    cfg[8] = 7
    cfg[10] = [302, 20, 150, 77, 201, 33, 9]
    m, sd, blocked, seq, spos, h = make_case(tuple(cfg), dev)
    src = (seq.to(dev), spos.to(dev))
    one, enc_one, _ = m(src, None, None, None)
    lg, _, _, _ = m(src, None, None, None, return_attns=True)
    assert torch.equal(lg, one)
    lg2, _, ips = m(src, None, None, None, int_preds=True)
    assert torch.equal(lg2, one) and len(ips) == 3
    m.workspace_limit_bytes = 64 << 20
    split, enc_split, _ = m(src, None, None, None)
    assert torch.equal(split, one) and torch.equal(enc_split, enc_one)


def test_attention_maps_survive_micro_batching(dev):
    """return_attns=True with the batch split into micro-batches (tiny workspace): every (h*B, lq, lk) map must
    equal the single-pass one."""
    m, sd, blocked, seq, spos, h = make_case(CONFIGS['inveye_8h'], dev)
    src = (seq.to(dev), spos.to(dev))
    lg, enc, enc_attns, dec2 = m(src, None, None, None, return_attns=True)
    flat = [a for a in enc_attns[0]] + [a for a in dec2[0]] + [a for a in dec2[1]]
    for limit in (3 << 20, 6 << 20):
        m.workspace_limit_bytes = limit
        lg2, enc2, ea2, d2 = m(src, None, None, None, return_attns=True)
        flat2 = [a for a in ea2[0]] + [a for a in d2[0]] + [a for a in d2[1]]
        assert torch.equal(lg2, lg) and torch.equal(enc2, enc)
        for a, b in zip(flat, flat2):
            assert max_abs_diff(a, b) == 0.0


@pytest.mark.parametrize('name', ['reuters_b32_ragged', 'bibtex', 'inveye_8h'])
def test_embedding_fold_against_the_unfolded_route_and_the_oracle(dev, name):
    """Encoder layer 0's W1 folded into the embedding tables (LAMP.fold_embedding; lamp_model.enc0_emb_w1 / enc0_pos_w1): a
    re-association of relu((Emb[tok] + Pos[p]) W1^T + b1), so the folded forward sits in the last bits of the unfolded one
    and both inside the oracle's tolerance -- with and without a position table, ragged batches, attention maps (padded
    layout) -- and the tables follow in-place weight updates."""
    m, sd, blocked, seq, spos, h = make_case(CONFIGS[name], dev)
    src = (seq.to(dev), spos.to(dev))
    with torch.no_grad():
        ref_logits, ref_enc, _ = R.forward(sd, seq, spos, h, blocked)
    assert m.fold_embedding
    folded, enc_f, _ = m(src, None, None, None)
    built = m._native_model()
    assert built[0].enc0_emb_w1 and bool(built[0].enc0_pos_w1) == hasattr(m.encoder, 'position_enc')
    maps_f = m(src, None, None, None, return_attns=True)
    m.fold_embedding = False
    plain, enc_p, _ = m(src, None, None, None)
    assert not m._native_model()[0].enc0_emb_w1
    for got, got_enc in ((folded, enc_f), (plain, enc_p), (maps_f[0], maps_f[1])):
        assert max_abs_diff(got, ref_logits) < TOL_LOGIT and max_abs_diff(got_enc, ref_enc) < TOL_ACT
    assert max_abs_diff(folded, plain) < 2e-5 and max_abs_diff(enc_f, enc_p) < 2e-5
    assert torch.equal(maps_f[0], folded) and torch.equal(maps_f[1], enc_f)     # packed and padded layouts: same bits
    # the tables are keyed on the weights' versions
    del m.fold_embedding
    with torch.no_grad():
        m.encoder.layer_stack[0].pos_ffn.w_1.weight.mul_(1.25)
        m.encoder.src_word_emb.weight[5:].add_(0.01)
    after, enc_a, _ = m(src, None, None, None)
    m.fold_embedding = False
    after_plain, enc_ap, _ = m(src, None, None, None)
    assert max_abs_diff(after, after_plain) < 2e-5 and max_abs_diff(enc_a, enc_ap) < 2e-5
    assert max_abs_diff(after, folded) > 1e-4


@pytest.mark.parametrize('L,B,H,p', [(1024, 2, 2, 0.05), (1100, 1, 3, 0.10), (2085, 1, 1, 0.02)])
def test_sdpa_pair_kernel_for_sparse_unstructured_masks(dev, tuning, L, B, H, p):
    """csrc/attention_sparse.hip (LAMP_MASK_SPARSE_ROWS): only the allowed (query, key) pairs of a shared bit-packed mask are
    computed.  Exact masked softmax -- against the fp64 oracle arithmetic and against the dense kernels on the same inputs;
    label counts that are no multiple of the 64-key tile / the 128-query block / the 32-bit mask word, a row that allows a
    single key, a row that allows none (NaN, as the reference's softmax of an all -inf row)."""
    import ctypes
    from lamp_amd import _native as N
    dk = 128
    g = torch.Generator().manual_seed(L)
    q = torch.randn(B, L, H * dk, generator=g)
    k = torch.randn(B, L, H * dk, generator=g)
    v = torch.randn(B, L, H * dk, generator=g)
    blocked = (R.make_adjacency(L, p, 1) == 0)
    blocked[3, :] = True
    blocked[3, L - 1] = False        # one key, the very last
    blocked[7, :] = True             # no key at all
    bits = N.pack_mask_bits(blocked.to(torch.uint8)).to(dev)
    allowed = int((~blocked).sum())
    lay = N.AttnLayout(L * H * dk, dk, H * dk, L * H * dk, dk, H * dk, L * H * dk, dk, H * dk, L * H * dk, dk, H * dk)
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    outs = {}
    tuning.lamp_debug_sparse_lpq.argtypes = [ctypes.c_int]
    tuning.lamp_debug_sparse_lpq.restype = None
    # the product library's route, and both lanes-per-query variants forced in the tuning build
    for name, flags, lib, lanes in (('dense', 0, N.lib(), 0), ('pairs', N.LAMP_MASK_SPARSE_ROWS, N.lib(), 0),
                                    ('pairs8', N.LAMP_MASK_SPARSE_ROWS, tuning, 8), ('pairs4', N.LAMP_MASK_SPARSE_ROWS, tuning, 4)):
        o = torch.full((B, L, H * dk), 7.0, device=dev)
        ms = N.Mask(N.LAMP_MASK_BITS_U32, flags, bits.data_ptr(), 0, bits.size(1), None, 0, allowed if flags else 0)
        try:
            if lanes:
                tuning.lamp_debug_sparse_lpq(lanes)
            N.check(lib.lamp_sdpa_fwd(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), None, B, H, L, L, dk, dk,
                                      dk ** -0.5, ctypes.byref(ms), ctypes.byref(lay), N.stream()), 'sdpa')
        finally:
            if lanes:
                tuning.lamp_debug_sparse_lpq(0)
        outs[name] = o.cpu()
    qh = q.view(B, L, H, dk).permute(0, 2, 1, 3).double()
    kh = k.view(B, L, H, dk).permute(0, 2, 1, 3).double()
    vh = v.view(B, L, H, dk).permute(0, 2, 1, 3).double()
    sc = (qh @ kh.transpose(-1, -2)) / dk ** 0.5
    sc = sc.masked_fill(blocked[None, None], float('-inf'))
    ref = (torch.softmax(sc, dim=-1) @ vh).permute(0, 2, 1, 3).reshape(B, L, H * dk)
    assert torch.isnan(ref[:, 7]).all() and max_abs_diff(outs['dense'], ref) < 2e-5
    for name in ('pairs', 'pairs8', 'pairs4'):
        assert torch.isnan(outs[name][:, 7]).all() and max_abs_diff(outs[name], ref) < 2e-5, name
        assert max_abs_diff(outs[name][:, 3], v[:, L - 1]) < 1e-6, name      # softmax over one key = that key's value row
    assert max_abs_diff(outs['pairs'], outs['pairs4']) == 0.0     # product route == the tuning build's forced default variant


def test_model_takes_the_pair_kernel_on_a_sparse_unstructured_label_graph(dev):
    """configs[4]'s label graph (Bernoulli(0.05) prior over 4096 labels: every 32 x 32 tile holds an edge, every row ~5 % of the
    keys): the decoder drops the tile-list hint, flags the mask LAMP_MASK_SPARSE_ROWS, and lamp_forward's label self-attention
    runs attention_sparse.hip -- same logits as with the dense tile kernel up to summation order, both within the oracle's bar;
    a sample's bits do not depend on the micro-batch split."""
    from lamp_amd import _native as N
    m, sd, blocked, seq, spos, h = make_case(CONFIGS['labels4096'], dev)
    # symmetric Bernoulli(0.05) or identity: 1 - 0.95^2 = 9.75 % of the pairs are allowed
    assert m.decoder.label_tiles is None and m.decoder.label_rows_sparse and 0.09 < m.decoder.label_allowed_pairs / 4096 ** 2 < 0.105
    src = (seq.to(dev), spos.to(dev))
    with torch.no_grad():
        ref_logits, ref_enc, _ = R.forward(sd, seq, spos, h, blocked)
    pairs, _, _ = m(src, None, None, None)
    desc = m._native_model()[0]
    assert desc.label_mask_flags == N.LAMP_MASK_SPARSE_ROWS and desc.label_mask_allowed == m.decoder.label_allowed_pairs
    m.use_sparse_label_attention = False
    dense, _, _ = m(src, None, None, None)
    assert m._native_model()[0].label_mask_flags == 0
    assert max_abs_diff(pairs, ref_logits) < TOL_LOGIT and max_abs_diff(dense, ref_logits) < TOL_LOGIT
    assert 0.0 < max_abs_diff(pairs, dense) < 2e-5      # two kernels, two summation orders
    del m.use_sparse_label_attention
    m.workspace_limit_bytes = 200 << 20     # one sample per pass
    split, _, _ = m(src, None, None, None)
    assert torch.equal(split, pairs)
    # the module-by-module route takes the same kernel
    enc2, _ = m.encoder(src[0], None, src[1])
    y, _ = m.decoder(None, src[0], enc2)
    assert max_abs_diff(N.diag_logits(y, m.tgt_word_proj.linear.weight), pairs) < 2e-5


def test_non_finite_key_behind_a_blocked_key_is_a_documented_deviation(dev):
    """the small-shape and tile attention kernels enter blocked keys as a -inf INITIAL accumulator of the QK^T
    chain (attention_small.hip, attention_tile.hip) instead of overwriting the finished score as masked_fill does
    (lamp/SubLayers.py:32): -inf + (+inf or NaN) is NaN, so a non-finite K row behind a BLOCKED key turns the rows of the
    queries that block it into NaN, where the reference stays finite.  Pinned here so that it cannot change unnoticed:
    finite keys behind blocked positions never matter (bit-identical to the same call with those rows zeroed), queries that
    may see the key are NaN in the reference too, and the pair kernel, which never touches a blocked key, matches the
    reference exactly."""
    import ctypes
    from lamp_amd import _native as N
    g = torch.Generator().manual_seed(5)
    for lq, lk, sparse in ((90, 90, False), (1100, 1100, False), (1100, 1100, True)):
        dk, B, H = 128, 1, 2
        q = torch.randn(B, lq, H * dk, generator=g)
        k = torch.randn(B, lk, H * dk, generator=g)
        v = torch.randn(B, lk, H * dk, generator=g)
        blocked = torch.rand(lq, lk, generator=g) < (0.9 if sparse else 0.5)
        blocked[:, 0] = False
        bad = 7
        blocked[: lq // 2, bad] = True      # the first half of the queries block key 7, the second half may see it
        blocked[lq // 2:, bad] = False
        bits = N.pack_mask_bits(blocked.to(torch.uint8)).to(dev)
        lay = N.AttnLayout(lq * H * dk, dk, H * dk, lk * H * dk, dk, H * dk, lk * H * dk, dk, H * dk, lq * H * dk, dk, H * dk)
        flags = N.LAMP_MASK_SPARSE_ROWS if sparse else 0
        ms = N.Mask(N.LAMP_MASK_BITS_U32, flags, bits.data_ptr(), 0, bits.size(1), None, 0, int((~blocked).sum()) if sparse else 0)

        qd, vd = q.to(dev), v.to(dev)

        def run(kk):
            o = torch.empty(B, lq, H * dk, device=dev)
            kd = kk.to(dev)      # (kept alive across the call: the ABI takes raw pointers)
            N.check(N.lib().lamp_sdpa_fwd(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), None, B, H,
                                          lq, lk, dk, dk, dk ** -0.5, ctypes.byref(ms), ctypes.byref(lay), N.stream()), 'sdpa')
            torch.cuda.synchronize()
            return o.cpu()
        k_zero, k_big, k_inf = k.clone(), k.clone(), k.clone()
        k_zero[:, bad] = 0.0
        k_big[:, bad] = 1e30                    # finite: must not matter to the queries that block it
        k_inf[:, bad] = float('inf')
        base, big, inf = run(k_zero), run(k_big), run(k_inf)
        half = lq // 2
        assert torch.isfinite(base).all()
        if sparse:   # (the lazy rescale is taken per WAVE: a wave-mate that sees the huge key moves this row's rounding, not its value)
            assert max_abs_diff(big[:, :half], base[:, :half]) < 1e-6
        else:
            assert torch.equal(big[:, :half], base[:, :half])                # a finite key behind a blocked position is invisible
        assert torch.isnan(inf[:, half:]).all()                              # queries that SEE the key: inf - inf, as in the reference
        if sparse:
            assert max_abs_diff(inf[:, :half], base[:, :half]) < 1e-6        # pair kernel == masked_fill semantics
        else:
            assert torch.isnan(inf[:, :half]).all()                          # the documented deviation of the dense kernels


def test_layer0_query_cache_tracks_weight_updates(dev):
    """The hoisted label-table x W_q projection is bit-identical to projecting per call, and is refreshed
    when either operand is modified in place (load_state_dict / optimiser step keep data_ptr)."""
    m, sd, blocked, seq, spos, h = make_case(CONFIGS['bibtex'], dev)
    src = (seq.to(dev), spos.to(dev))
    cached, _, _ = m(src, None, None, None)
    m.cache_layer0_query = False
    m._native_cache = None
    plain, _, _ = m(src, None, None, None)
    assert torch.equal(cached, plain)
    m.cache_layer0_query = True
    m._native_cache = None
    m(src, None, None, None)
    with torch.no_grad():
        m.decoder.layer_stack[0].enc_attn.w_qs.weight.mul_(1.5)   # in place: same data_ptr, new _version
    after, _, _ = m(src, None, None, None)
    m.cache_layer0_query = False
    m._native_cache = None
    ref, _, _ = m(src, None, None, None)
    assert torch.equal(after, ref) and not torch.equal(after, cached)


def clustered_adjacency(L, n_clusters, seed=0, extra=0.0):
    """Block-diagonal label graph (labels only co-occur inside their cluster) plus optional random edges."""
    adj = torch.zeros(L, L)
    edges = torch.linspace(0, L, n_clusters + 1).long().tolist()
    for lo, hi in zip(edges[:-1], edges[1:]):
        adj[lo:hi, lo:hi] = 1
    if extra > 0:
        g = torch.Generator().manual_seed(seed)
        r = (torch.rand(L, L, generator=g) < extra).float()
        adj = ((adj + r + r.t()) > 0).float()
    return adj


@pytest.mark.parametrize('lq,extra', [(500, 0.0), (500, 0.00005), (100, 0.0)])
def test_sdpa_tile_skipping_is_exact(dev, lq, extra):
    """Sparse-aware attention: with the active-tile list of a clustered label mask the kernel
    visits only tiles holding an edge; the result must equal the dense visit (bitwise when keys are not split
    across waves) and the oracle."""
    import ctypes
    from lamp_amd import _native as N
    g = torch.Generator().manual_seed(lq)
    dk, n = 64, 3
    q, k, v = (torch.randn(n, lq, dk, generator=g) for _ in range(3))
    blocked = (clustered_adjacency(lq, 5, extra=extra) == 0)
    ref_o, _ = R.sdpa(q.double(), k.double(), v.double(), blocked.unsqueeze(0).expand(n, lq, lq))
    mu8 = blocked.to(torch.uint8).to(dev)
    tiles = N.active_tile_list(mu8).to(dev)
    assert tiles[:, 0].float().mean().item() < 0.75 * (tiles.size(1) - 1)  # the hint really removes tiles
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    out = {}
    for name, tl in (('dense', None), ('sparse', tiles)):
        o = torch.empty_like(qd)
        ms = N.Mask(N.LAMP_MASK_U8, 0, mu8.data_ptr(), 0, lq, tl.data_ptr() if tl is not None else None,
                    tl.size(1) if tl is not None else 0)
        lay = N.AttnLayout(lq * dk, 0, dk, lq * dk, 0, dk, lq * dk, 0, dk, lq * dk, 0, dk)
        N.check(N.lib().lamp_sdpa_fwd(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), None, n, 1, lq, lq,
                                      dk, dk, dk ** -0.5, ctypes.byref(ms), ctypes.byref(lay), N.stream()), 'sdpa')
        out[name] = o
    assert max_abs_diff(out['sparse'], ref_o) < 2e-5 and max_abs_diff(out['dense'], ref_o) < 2e-5
    if lq > 128:  # no key split -> same tiles in the same order minus exact zeros
        assert torch.equal(out['sparse'], out['dense'])


@pytest.mark.parametrize('B,H,lq,lk,dk,dv,mask_kind', [
    (2, 2, 300, 256, 128, 128, 'bits'), (1, 2, 983, 983, 128, 128, 'none'), (1, 1, 983, 983, 128, 128, 'bits'),
    (2, 1, 257, 300, 128, 128, 'bits'), (1, 2, 400, 1000, 96, 72, 'bits'), (1, 1, 385, 257, 68, 128, 'none'),
    (1, 1, 1100, 2100, 128, 128, 'tiles'), (2, 1, 600, 600, 128, 100, 'tiles'), (1, 1, 520, 4096, 128, 128, 'bits')])
def test_lds_tile_attention_has_the_bits_of_the_wave_private_kernel(dev, tuning, B, H, lq, lk, dk, dv, mask_kind):
    """attention_tile.hip (K / V tiles shared by a workgroup through LDS-DMA, Q fragments in registers) against attn_kernel
    (bit 8 of the tuning hook keeps it off): the same MFMA sequence on the same operands, so every output bit must agree --
    ragged last tiles, head dimensions below 128 (range-checked chunks must land as ZEROS in LDS), dead rows, a late key
    that forces the online rescale, and the union of the four query blocks' tile lists for a hinted shared mask."""
    import ctypes
    from lamp_amd import _native as N
    force = tuning.lamp_debug_force_attn
    g = torch.Generator().manual_seed(lq * 31 + lk + dk)
    q = torch.randn(B, lq, H * dk, generator=g)
    k = torch.randn(B, lk, H * dk, generator=g)
    v = torch.randn(B, lk, H * dv, generator=g)
    k[:, lk - 7, :dk] = q[:, 5, :dk] * 5.0       # a spike in the last tile: the running max jumps there
    q, k, v = q.to(dev), k.to(dev), v.to(dev)
    if mask_kind == 'tiles':
        blocked = (clustered_adjacency(max(lq, lk), 7, extra=0.00002)[:lq, :lk] == 0).to(torch.uint8)
    else:
        blocked = (torch.rand(lq, lk, generator=g) < 0.5).to(torch.uint8)
    blocked[:, 0] = 0
    blocked[lq // 3, :] = 1                       # a dead row
    bits = N.pack_mask_bits(blocked).to(dev)
    tiles = N.active_tile_list(blocked.to(dev)).to(dev) if mask_kind == 'tiles' else None
    if tiles is not None:
        assert tiles[:, 0].float().mean().item() < 0.75 * (tiles.size(1) - 1)
    ms = None if mask_kind == 'none' else N.Mask(N.LAMP_MASK_BITS_U32, 0, bits.data_ptr(), 0, bits.size(1),
                                                 tiles.data_ptr() if tiles is not None else None,
                                                 tiles.size(1) if tiles is not None else 0)
    lay = N.AttnLayout(lq * H * dk, dk, H * dk, lk * H * dk, dk, H * dk, lk * H * dv, dv, H * dv, lq * H * dv, dv, H * dv)
    out = {}
    for name, mode in (('tile', 0), ('wave', 0x100)):
        # poison what an earlier launch may have left in LDS is not possible from here; the zero fill itself is pinned by
        # tools/probes/lds_dma_oob.hip -- here stale finite values would already show as wrong bits in the d_k = 96 case
        o = torch.full((B, lq, H * dv), float('nan'), device=dev)
        try:
            force(mode)
            N.check(tuning.lamp_sdpa_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), None, B, H, lq, lk, dk, dv,
                                         dk ** -0.5, ctypes.byref(ms) if ms is not None else None, ctypes.byref(lay),
                                         N.stream()), 'sdpa')
        finally:
            force(0)
        out[name] = o
    dead = torch.isnan(out['wave'])
    if mask_kind != 'none':
        assert dead[:, lq // 3].all() and not dead[:, lq // 3 + 1].any()
    assert torch.equal(dead, torch.isnan(out['tile']))
    assert torch.equal(out['tile'][~dead], out['wave'][~dead])
    # and the oracle, on one head
    hq, hk, hv = q[:, :, :dk].cpu().double(), k[:, :, :dk].cpu().double(), v[:, :, :dv].cpu().double()
    ref_o, _ = R.sdpa(hq, hk, hv, blocked.bool().unsqueeze(0).expand(B, lq, lk) if mask_kind != 'none' else None)
    got = out['tile'][:, :, :dv].cpu()
    ok = ~torch.isnan(got)
    assert (got[ok].double() - ref_o[ok]).abs().max().item() < 5e-5


def test_lds_tile_attention_inside_the_forward_ragged_keys_and_tile_lists(dev, tuning, monkeypatch):
    """The same comparison through lamp_forward: 600 labels over ragged sources of up to 320 tokens -- the enc-dec attention
    takes each sample's own key count and first row (AttnParams::kv_len / kv_off: descriptors that end at the sample's last
    key), the label self-attention the model's tile lists."""
    import ctypes
    from lamp_amd import _native as N
    cfg = (500, 600, 320, 256, 512, 2, 'prior', True, 4, 0.05, [320, 257, 31, 1])
    m, sd, blocked, seq, spos, h = make_case(cfg, dev)
    monkeypatch.setattr(N, '_lib', tuning)
    force = tuning.lamp_debug_force_attn
    src = (seq.to(dev), spos.to(dev))
    try:
        force(0x100)
        want, enc_want, _ = m(src, None, None, None)
        force(0)
        for _ in range(3):
            got, enc_got, _ = m(src, None, None, None)
            assert torch.equal(got, want) and torch.equal(enc_got, enc_want)
    finally:
        force(0)
    with torch.no_grad():
        ref, _, _ = R.forward(sd, seq, spos, h, blocked)
    assert max_abs_diff(got, ref) < TOL_LOGIT


@pytest.mark.parametrize('lq,lk', [(90, 90), (159, 159), (70, 130), (33, 31)])
def test_bit_packed_mask_equals_byte_mask(dev, lq, lk):
    """LAMP_MASK_BITS_U32 (one dword per row and 32-key tile) must give exactly the bits of the uint8 mask,
    dead rows and ragged last words included, with and without attention maps."""
    import ctypes
    from lamp_amd import _native as N
    g = torch.Generator().manual_seed(lq * lk)
    dk, n = 32, 4
    q = torch.randn(n, lq, dk, generator=g).to(dev)
    k = torch.randn(n, lk, dk, generator=g).to(dev)
    v = torch.randn(n, lk, dk, generator=g).to(dev)
    blocked = (torch.rand(lq, lk, generator=g) < 0.6).to(torch.uint8)
    blocked[:, 0] = 0
    blocked[lq // 2, :] = 1                       # a dead row
    mu8 = blocked.to(dev)
    bits = N.pack_mask_bits(blocked).to(dev)
    lay = N.AttnLayout(lq * dk, 0, dk, lk * dk, 0, dk, lk * dk, 0, dk, lq * dk, 0, dk)
    res = {}
    for name, ms in (('u8', N.Mask(N.LAMP_MASK_U8, 0, mu8.data_ptr(), 0, lk, None, 0)),
                     ('bits', N.Mask(N.LAMP_MASK_BITS_U32, 0, bits.data_ptr(), 0, bits.size(1), None, 0))):
        for want_p in (False, True):
            o = torch.empty_like(q)
            pm = torch.empty(n, lq, lk, device=dev) if want_p else None
            N.check(N.lib().lamp_sdpa_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), N.ptr(pm), n, 1, lq,
                                          lk, dk, dk, dk ** -0.5, ctypes.byref(ms), ctypes.byref(lay), N.stream()),
                    'sdpa')
            res[(name, want_p)] = (o, pm)
    for want_p in (False, True):
        a, b = res[('u8', want_p)], res[('bits', want_p)]
        assert max_abs_diff(a[0], b[0]) == 0.0
        if want_p:
            assert max_abs_diff(a[1], b[1]) == 0.0
    assert torch.isnan(res[('bits', False)][0][:, lq // 2]).all()


def test_model_with_clustered_label_graph_uses_tile_lists(dev):
    from lamp_amd.Models import LAMP
    V, L, T, d, dff, h, B = 300, 512, 40, 128, 256, 4, 3
    sd = R.make_state_dict(V, L, T, d, dff, h, 1, 2, pos_emb=True, seed=4)
    adj = clustered_adjacency(L, 8)
    seq, spos = R.make_batch(B, V, T, lengths=[40, 11, 25], seed=4)
    m = LAMP(V, L, T, L, n_layers_enc=1, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d,
             d_inner_hid=dff, d_k=d // h, d_v=d // h, encoder='graph', decoder='graph',
             label_adj_matrix=adj.clone(), label_mask='prior', dec_dropout2=False)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    assert m.decoder.label_tiles[:, 0].max().item() <= 3          # 8 clusters of 64 labels: <= 3 tiles per row block
    src = (seq.to(dev), spos.to(dev))
    sparse, _, _ = m(src, None, None, None)
    m.use_label_tiles = False
    dense, _, _ = m(src, None, None, None)
    m.use_mask_bits = False
    bytes_, _, _ = m(src, None, None, None)
    assert torch.equal(bytes_, dense)
    with torch.no_grad():
        ref, _, _ = R.forward(sd, seq, spos, h, R.label_block_mask(adj, 'prior', L))
    assert torch.equal(sparse, dense)
    assert max_abs_diff(sparse, ref) < TOL_LOGIT


def test_trailing_padding_does_not_change_results(dev):
    """Extra PAD columns are blocked keys and PAD rows of the encoder.  The encoder runs on the packed non-PAD rows and
    the enc-dec attention takes its key split from each sample's own key count, so a sample's logits and encoder
    rows do not depend on the padded length of its batch -- bit for bit -- and every PAD position of enc_output
    holds the one shared PAD row."""
    m, sd, blocked, seq, spos, h = make_case(CONFIGS['reuters_ragged'], dev)
    seq, spos = seq.to(dev), spos.to(dev)
    base, enc_base, _ = m((seq[1:4, :210], spos[1:4, :210]), None, None, None)
    wide, enc_wide, _ = m((seq[1:4], spos[1:4]), None, None, None)
    assert torch.equal(base, wide)
    assert torch.equal(enc_base, enc_wide[:, :210])
    pad_row = enc_wide[0, 301]
    lengths = [20, 150, 77]
    for b, n in enumerate(lengths):
        assert torch.equal(enc_wide[b, n:], pad_row.expand(302 - n, -1))
    # a sample alone, padded to its own length, and the same sample inside the 6-sample ragged batch
    full, enc_full, _ = m((seq, spos), None, None, None)
    for b, n in enumerate([302, 20, 150, 77, 201, 33]):
        one, enc_one, _ = m((seq[b:b + 1, :n], spos[b:b + 1, :n]), None, None, None)
        assert torch.equal(one, full[b:b + 1]) and torch.equal(enc_one, enc_full[b:b + 1, :n])


def test_pad_tokens_inside_a_sequence(dev):
    """PAD tokens that are not trailing are ordinary encoder rows and blocked keys; trailing PAD tokens that still carry a
    position index are live rows too (their embedding is not the shared PAD row).  Against the oracle, with and
    without attention maps (packed and padded encoder), bitwise equal between the two."""
    m, sd, blocked, seq, spos, h = make_case(CONFIGS['reuters_ragged'], dev)
    seq, spos = seq.clone(), spos.clone()
    seq[1, 5] = 0                                   # a PAD token inside sample 1 (20 tokens), position index kept
    seq[2, 100:120] = 0
    spos[2, 100:120] = 0                            # a hole of real PAD positions inside sample 2
    spos[3, 77:80] = torch.tensor([78, 79, 80])     # trailing PAD tokens with position indices
    seq[5, :] = 0                                   # no token at all, positions kept: every key blocked
    with torch.no_grad():
        ref_logits, ref_enc, _ = R.forward(sd, seq, spos, h, blocked)
    src = (seq.to(dev), spos.to(dev))
    logits, enc, _ = m(src, None, None, None)
    assert torch.isnan(logits[5]).all() and torch.isnan(ref_logits[5]).all()
    assert max_abs_diff(enc, ref_enc) < TOL_ACT
    assert max_abs_diff(logits[:5], ref_logits[:5]) < TOL_LOGIT
    lg, en, _, _ = m(src, None, None, None, return_attns=True)
    assert torch.equal(lg[:5], logits[:5]) and torch.equal(en, enc)


def test_allpad_row_poisons_only_itself(dev):
    m, sd, blocked, seq, spos, h = make_case(CONFIGS['reuters_ragged'], dev)
    seq, spos = seq.clone(), spos.clone()
    seq[2] = 0
    spos[2] = 0
    logits, _, _ = m((seq.to(dev), spos.to(dev)), None, None, None)
    clean, _, _ = m((seq[[0, 1, 3, 4, 5]].to(dev), spos[[0, 1, 3, 4, 5]].to(dev)), None, None, None)
    assert torch.isnan(logits[2]).all()
    assert torch.equal(logits[[0, 1, 3, 4, 5]], clean)
    # a batch of PAD only: no packed row but the shared PAD row
    seq0, pos0 = torch.zeros(2, 40, dtype=torch.int64, device=dev), torch.zeros(2, 40, dtype=torch.int64, device=dev)
    lg0, enc0, _ = m((seq0, pos0), None, None, None)
    with torch.no_grad():
        _, ref_enc0, _ = R.forward(sd, seq0.cpu(), pos0.cpu(), h, blocked)
    assert torch.isnan(lg0).all() and max_abs_diff(enc0, ref_enc0) < TOL_ACT
    assert torch.equal(enc0, enc0[0, 0].expand_as(enc0))


def test_label_permutation_equivariance(dev):
    """Relabelling the label nodes (embedding rows, read-out rows, adjacency rows+cols) permutes the
    logits the same way -- a property of message passing on the label graph, checked at full size."""
    from lamp_amd.Models import LAMP
    V, L, T, d, dff, h, mask, pos, B, p, lengths = CONFIGS['bibtex']
    m, sd, blocked, seq, spos, _ = make_case(CONFIGS['bibtex'], dev)
    base, _, _ = m((seq.to(dev), spos.to(dev)), None, None, None)
    perm = torch.randperm(L, generator=torch.Generator().manual_seed(3))
    sd2 = dict(sd)
    for k in ('decoder.tgt_word_emb.weight', 'tgt_word_proj.weight', 'tgt_word_proj.linear.weight'):
        sd2[k] = sd[k][perm]
    adj = R.make_adjacency(L, p, 0)[perm][:, perm]
    m2 = LAMP(V, L, T, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d,
              d_inner_hid=dff, d_k=d // h, d_v=d // h, encoder='graph', decoder='graph',
              no_enc_pos_embedding=not pos, label_adj_matrix=adj.clone(), label_mask=mask, dec_dropout2=False)
    m2.load_state_dict(sd2)
    m2 = m2.to(dev).eval()
    out, _, _ = m2((seq.to(dev), spos.to(dev)), None, None, None)
    assert max_abs_diff(out, base[:, perm.to(dev)]) < 2e-5


# ------------------------------------------------------------------ randomized shape sweep
def _random_case(i):
    import random
    rng = random.Random(1000 + i)
    h = rng.choice([1, 2, 3, 4, 8])
    dk = rng.choice([4, 8, 12, 16, 20, 32, 36, 64])
    d = h * dk
    if h == 1:
        d = rng.choice([4, 8, 20, 64, 128])  # no fc: d_v must equal d_model
    dff = rng.choice([4, 12, 64, 100, 200, 516])
    L = rng.choice([1, 2, 17, 31, 32, 33, 64, 95, 129, 300])
    T = rng.choice([1, 2, 5, 31, 32, 33, 97, 150])
    B = rng.randint(1, 6)
    mask = rng.choice(['prior', 'none', 'inveye'])
    pos = rng.random() < 0.5
    n_enc, n_dec = rng.randint(1, 3), rng.randint(1, 3)
    no_slf = rng.random() < 0.2
    lengths = [rng.randint(1, T) for _ in range(B)]
    lengths[rng.randrange(B)] = T
    return dict(h=h, d=d, dff=dff, L=L, T=T, B=B, mask=mask, pos=pos, n_enc=n_enc, n_dec=n_dec, no_slf=no_slf,
                lengths=lengths, V=rng.choice([5, 40, 1000]))


@pytest.mark.parametrize('i', list(range(24)))
def test_random_model_shapes_vs_oracle(dev, i):
    """Seeded sweep over awkward shapes (tiny / non-power-of-two widths, L or T of 1, ragged lengths, 1-3
    layers, every mask kind, with and without decoder self-attention): whole-model logits vs the oracle."""
    from lamp_amd.Models import LAMP
    c = _random_case(i)
    h, d = c['h'], c['d']
    sd = R.make_state_dict(c['V'], c['L'], c['T'], d, c['dff'], h, c['n_enc'], c['n_dec'], pos_emb=c['pos'],
                           seed=i, no_dec_self_att=c['no_slf'])
    adj = R.make_adjacency(c['L'], 0.2, i) if c['mask'] == 'prior' else None
    seq, spos = R.make_batch(c['B'], c['V'], c['T'], lengths=c['lengths'], seed=i)
    m = LAMP(c['V'], c['L'], c['T'], c['L'], n_layers_enc=c['n_enc'], n_layers_dec=c['n_dec'], n_head=h, n_head2=h,
             d_word_vec=d, d_model=d, d_inner_hid=c['dff'], d_k=d // h, d_v=d // h, encoder='graph', decoder='graph',
             no_enc_pos_embedding=not c['pos'], no_dec_self_att=c['no_slf'],
             label_adj_matrix=adj.clone() if adj is not None else None, label_mask=c['mask'], dec_dropout2=False)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    with torch.no_grad():
        ref_logits, ref_enc, _ = R.forward(sd, seq, spos, h, R.label_block_mask(adj, c['mask'], c['L']))
        ref64, _, _ = R.forward(R.to_dtype(sd, torch.float64), seq, spos, h,
                                R.label_block_mask(adj, c['mask'], c['L']))
    logits, enc, _ = m((seq.to(dev), spos.to(dev)), None, None, None)
    assert logits.shape == ref_logits.shape, c
    assert max_abs_diff(enc, ref_enc) < TOL_ACT, c
    # tiny widths make LayerNorm ill-conditioned: scale the bar by the oracle's own fp32-vs-fp64 gap
    gap = max_abs_diff(ref_logits, ref64)
    assert max_abs_diff(logits, ref64) < max(TOL_LOGIT, 4 * gap), (c, gap)


# ------------------------------------------------------------------ error behaviour at the boundary
def test_errors_surface_as_status_codes_not_crashes(dev):
    """SURVEY.md 8b "Errors": unsupported configurations, undersized workspaces and misaligned pointers come back
    as negative lamp_status codes (-> LampError in Python); the device stays usable afterwards."""
    import ctypes
    from lamp_amd import _native as N
    lib = N.lib()
    x = torch.randn(8, 64, device=dev)
    w = torch.randn(32, 64, device=dev)
    out = torch.empty(8, 32, device=dev)
    # misaligned A (offset by one float): LAMP_E_ALIGN
    buf = torch.randn(8 * 64 + 4, device=dev)
    assert lib.lamp_linear_fwd(buf.data_ptr() + 4, 8, 64, 64, w.data_ptr(), 32, 64, None, None, 0, 0,
                               out.data_ptr(), 32, N.stream()) == -2
    # d_k = 130 is not a multiple of 4: LAMP_E_UNSUPPORTED, raised as LampError by the wrapper
    q = torch.randn(2, 5, 130, device=dev)
    with pytest.raises(N.LampError) as ei:
        N.sdpa(q, q, q, None, 1.0)
    assert ei.value.status == -4 and 'not supported' in str(ei.value)
    # d_k = 132 > 128 runs through the general path
    q = torch.randn(2, 5, 132, device=dev)
    o, a = N.sdpa(q, q, q, None, 1.0 / 132 ** 0.5)
    ref_o, ref_a = R.sdpa(q.cpu(), q.cpu(), q.cpu(), None, 132 ** 0.5)
    assert max_abs_diff(o, ref_o) < 5e-5 and max_abs_diff(a, ref_a) < TOL_ATTN
    # workspace one byte short of a single sample: LAMP_E_WORKSPACE
    m, sd, blocked, seq, spos, h = make_case(CONFIGS['inveye_8h'], dev)
    model, enc_arr, dec_arr = m._native_model()[:3]
    B, T = seq.shape
    need = lib.lamp_forward_workspace_bytes(ctypes.byref(model), 1, T, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    logits = torch.empty(B, m.n_labels, device=dev)
    enc = torch.empty(B, T, m.d_model, device=dev)
    s_, p_ = seq.to(dev), spos.to(dev)
    args = (ctypes.byref(model), s_.data_ptr(), p_.data_ptr(), B, T, logits.data_ptr(), enc.data_ptr(), None)
    assert lib.lamp_forward(*args, ws.data_ptr(), need // 2, N.stream()) == -3
    # ... and with exactly one sample's worth it succeeds by micro-batching sample by sample
    assert lib.lamp_forward(*args, ws.data_ptr(), need, N.stream()) == 0
    ref, _, _ = m((s_, p_), None, None, None)
    assert torch.equal(logits, ref)
    # the earlier failures left no sticky error behind
    assert max_abs_diff(N.linear(x, w), x.double() @ w.double().t()) < 1e-4


# ------------------------------------------------------------------ wide heads (d_k, d_v > 128): the general path
@pytest.mark.parametrize('kind', ['none', 'keys', 'shared_u8', 'shared_bits'])
def test_sdpa_wide_heads_vs_oracle(dev, kind):
    """d_k = d_v = 256 (e.g. d_model 512 with 2 heads): S = QK^T, masked softmax, PV as three launches."""
    from lamp_amd import _native as N
    g = torch.Generator().manual_seed(41)
    B, H, lq, lk, dk = 3, 2, 45, 70, 256
    q, k, v = (torch.randn(B, l, H * dk, generator=g) for l in (lq, lk, lk))
    blocked = None
    mask, keep = None, None
    if kind == 'keys':
        seq = torch.randint(1, 9, (B, lk), generator=g)
        seq[0, 40:] = 0
        seq[2, :] = 0                                  # fully padded sample -> NaN rows
        blocked = seq.eq(0).unsqueeze(1).expand(B, lq, lk)
        mask, keep = N.key_token_mask(seq.to(dev), lk)
    elif kind.startswith('shared'):
        m2 = torch.rand(lq, lk, generator=g) < 0.5
        m2[:, 1] = False
        blocked = m2.unsqueeze(0).expand(B, lq, lk)
        if kind == 'shared_u8':
            mask, keep = N.make_mask(m2.to(dev), B, lq, lk)
        else:
            bits = N.pack_mask_bits(m2.to(torch.uint8)).to(dev)
            mask, keep = N.Mask(N.LAMP_MASK_BITS_U32, 0, bits.data_ptr(), 0, bits.size(1), None, 0), bits
    split = lambda t, l: t.view(B, l, H, dk).permute(2, 0, 1, 3).reshape(H * B, l, dk)  # noqa: E731
    ref_out, ref_attn = R.sdpa(split(q, lq), split(k, lk), split(v, lk),
                               blocked.repeat(H, 1, 1) if blocked is not None else None, dk ** 0.5)
    for need_attn in (True, False):
        if not need_attn and kind != 'none':
            continue
        out, attn = N.sdpa_fused(q.to(dev), k.to(dev), v.to(dev), H, mask, 1.0 / dk ** 0.5, need_attn=need_attn)
        got = out.view(B, lq, H, dk).permute(2, 0, 1, 3).reshape(H * B, lq, dk)
        assert torch.equal(torch.isnan(got.cpu()), torch.isnan(ref_out))
        assert max_abs_diff(torch.nan_to_num(got), torch.nan_to_num(ref_out)) < 5e-5
        if need_attn:
            assert max_abs_diff(torch.nan_to_num(attn), torch.nan_to_num(ref_attn)) < TOL_ATTN
        else:
            assert attn is None
    # head-major API (the reference's own layout) and the C boundary without a map buffer
    o2, _ = N.sdpa(split(q, lq).to(dev), split(k, lk).to(dev), split(v, lk).to(dev),
                   blocked.repeat(H, 1, 1).to(dev) if blocked is not None else None, 1.0 / dk ** 0.5, need_attn=False)
    assert max_abs_diff(torch.nan_to_num(o2), torch.nan_to_num(ref_out)) < 5e-5


def test_model_with_wide_heads_vs_oracle(dev):
    """d_model 512 with 2 heads (d_k = 256) and d_model 320 with 1 head: whole-model logits, maps and int_preds."""
    for cfg in ((300, 37, 40, 512, 512, 2, 'prior', True, 3, 0.2, [40, 11, 25]),
                (200, 20, 30, 320, 256, 1, 'none', False, 2, 0.0, [30, 7])):
        m, sd, blocked, seq, spos, h = make_case(cfg, dev)
        with torch.no_grad():
            ref = R.forward(sd, seq, spos, h, blocked, return_attns=True)
            logits, enc, _ = m((seq.to(dev), spos.to(dev)), None, None, None)
            got = m((seq.to(dev), spos.to(dev)), None, None, None, return_attns=True)
        assert max_abs_diff(enc, ref[1]) < TOL_ACT and max_abs_diff(logits, ref[0]) < TOL_LOGIT
        assert max_abs_diff(got[0], ref[0]) < TOL_LOGIT
        for a, b_ in zip(got[3][1], ref[3][1]):
            assert max_abs_diff(a, b_) < TOL_ATTN
        # micro-batching keeps samples bit-identical on this path too
        m.workspace_limit_bytes = 1
        with torch.no_grad():
            lg2, _, _ = m((seq.to(dev), spos.to(dev)), None, None, None)
        assert torch.equal(lg2, logits)
