"""The tall packed-W tiles of the forward GEMM (csrc/gemm.hip: 64x64x32 and 128x64x32, one wave row; forced tiles 19 and 20 of the
tuning build) and the packs of the K / V projection of the encoder rows (lamp_kv_gemm_pack, lamp_forward_packs_kv).

A tile decides where a product is computed, never which products are summed in which order: every comparison is bit for bit
(torch.equal), against the staged heuristic (forced tile 0) and against the 32-row packed tile (forced tile 9).

The gathered residual and A_dense have no entry point of their own (they exist inside the forward only): the forward tests
below run them on every new tile -- encoder layer 0's W2 launch gathers its residual, and the ragged batch projects K / V from
packed rows with m_dev and A_dense set."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

TALL = (19, 20)
MS, NS, KS, NSEGS = (1, 63, 64, 65, 129, 200), (16, 48, 64, 80), (32, 64, 96), (1, 3, 4)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def tuning():
    """The -DLAMP_TUNING build of the same sources: the only library that exports the lamp_debug_* hooks."""
    from lamp_amd import _native as N
    t = N.load_library(N.TUNING_LIB_PATH)
    t.lamp_debug_force_gemm_tile.argtypes = [ctypes.c_int]
    t.lamp_debug_force_gemm_tile.restype = None
    assert getattr(t, 'lamp_linear_packed_fwd', None) and getattr(t, 'lamp_forward_packs_kv', None)
    return t


def launch(t, tile, x, ws, packs, bs=None, r=None, relu=False, pad=0, m_dev=None, fill=0.0):
    """lamp_linear_packed_fwd of the tuning library under forced tile `tile` -> list of [M, N + pad] outputs (ldc = N + pad)"""
    from lamp_amd import _native as N
    M, K, n, Nn = x.size(0), x.size(1), len(ws), ws[0].size(0)
    outs = [torch.full((M, Nn + pad), fill, dtype=torch.float32, device=x.device) for _ in ws]
    arr = lambda ts: (ctypes.c_void_p * n)(*[N.ptr(p) for p in ts])
    t.lamp_debug_force_gemm_tile(tile)
    try:
        N.check(t.lamp_linear_packed_fwd(N.ptr(x), M, K, K, arr(ws), arr(packs) if packs is not None else None, n, Nn, K,
                                         arr(bs) if bs is not None else None, N.ptr(r), Nn, int(relu), arr(outs), Nn + pad,
                                         N.ptr(m_dev), N.stream()), 'lamp_linear_packed_fwd')
    finally:
        t.lamp_debug_force_gemm_tile(0)
    return outs


def same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


EPILOGUES = {'plain': {}, 'bias': dict(b=1), 'bias_relu': dict(b=1, relu=True), 'bias_R': dict(b=1, r=1), 'bias_relu_R': dict(b=1, r=1, relu=True)}


@pytest.fixture(scope='module')
def cases(dev, tuning):
    """Operands of every edge case and their outputs on the staged heuristic (tile 0) and on the 32-row packed tile (tile 9):
    computed once, shared by both tall tiles."""
    from lamp_amd import _native as N
    g = torch.Generator(device=dev).manual_seed(1234)
    out = []
    for M, Nn, K, nseg in itertools.product(MS, NS, KS, NSEGS):
        x = torch.randn(M, K, device=dev, generator=g)
        ws = [torch.randn(Nn, K, device=dev, generator=g) / K ** 0.5 for _ in range(nseg)]
        packs = [N.weight_pack(w, 0) for w in ws]
        assert all(p is not None for p in packs)
        bs = [torch.randn(Nn, device=dev, generator=g) for _ in range(nseg)]
        r = torch.randn(M, Nn, device=dev, generator=g)
        for name, e in EPILOGUES.items():
            if e.get('r') and nseg != 1:   # the residual is a single-segment matter
                continue
            kw = dict(bs=bs if e.get('b') else None, r=r if e.get('r') else None, relu=bool(e.get('relu')))
            staged = launch(tuning, 0, x, ws, None, **kw)
            out.append(dict(id=(M, Nn, K, nseg, name), x=x, ws=ws, packs=packs, kw=kw, staged=staged,
                            packed32=launch(tuning, 9, x, ws, packs, **kw)))
    return out


def test_the_32_row_packed_tile_is_the_staged_heuristic(cases):
    assert len(cases) == len(MS) * len(NS) * len(KS) * (5 + 3 + 3)
    for c in cases:
        assert same(c['packed32'], c['staged']), c['id']


@pytest.mark.parametrize('tile', TALL)
def test_tall_tile_edges(tuning, cases, tile):
    """Partial row tiles and one row past one / two tiles; fragment blocks past N; one, two and three k-tiles (the prologue alone,
    the re-fetch of the last tile, the steady state); 1, 3 and 4 segments; every epilogue."""
    for c in cases:
        got = launch(tuning, tile, c['x'], c['ws'], c['packs'], **c['kw'])
        assert same(got, c['staged']), (tile, c['id'], 'vs staged')
        assert same(got, c['packed32']), (tile, c['id'], 'vs packed 32x64x32')


@pytest.mark.parametrize('tile', TALL)
def test_tall_tile_with_a_wider_ldc(tuning, cases, tile):
    """ldc = N + 8: the output rows are 32 bytes apart from where a dense C would put them; the columns between stay untouched."""
    for c in cases:
        M, Nn, K, nseg, name = c['id']
        if K != 96 or name not in ('plain', 'bias_relu', 'bias_R'):
            continue
        got = launch(tuning, tile, c['x'], c['ws'], c['packs'], pad=8, fill=-7.0, **c['kw'])
        for o, s in zip(got, c['staged']):
            assert torch.equal(o[:, :Nn], s), (tile, c['id'])
            assert bool((o[:, Nn:] == -7.0).all()), (tile, c['id'])


@pytest.mark.parametrize('tile', TALL)
@pytest.mark.parametrize('M,live', [(200, 0), (200, 1), (200, 64), (200, 65), (200, 130), (1400, 1201)])
def test_tall_tile_with_a_device_side_row_count(dev, tuning, tile, M, live):
    """m_dev holds fewer rows than M: the tile walk is rebuilt from it on the device (1400 rows: whole panels per XCD for the
    host's count), rows past it are neither computed nor written."""
    from lamp_amd import _native as N
    g = torch.Generator(device=dev).manual_seed(M + live)
    for nseg in (1, 4):
        x = torch.randn(M, 96, device=dev, generator=g)
        ws = [torch.randn(80, 96, device=dev, generator=g) for _ in range(nseg)]
        bs = [torch.randn(80, device=dev, generator=g) for _ in range(nseg)]
        packs = [N.weight_pack(w, 0) for w in ws]
        m_dev = torch.tensor([live], dtype=torch.int32, device=dev)
        full = launch(tuning, 0, x, ws, None, bs=bs, relu=True)
        part_staged = launch(tuning, 0, x, ws, None, bs=bs, relu=True, m_dev=m_dev, fill=-7.0)
        part = launch(tuning, tile, x, ws, packs, bs=bs, relu=True, m_dev=m_dev, fill=-7.0)
        assert same(part, part_staged), (tile, M, live, nseg)
        for p, f in zip(part, full):
            assert torch.equal(p[:live], f[:live]) and bool((p[live:] == -7.0).all()), (tile, M, live, nseg)


@pytest.mark.parametrize('tile', TALL)
def test_what_the_pack_cannot_express_takes_the_staged_kernel(dev, tuning, tile):
    """N % 16 != 0, K % 32 != 0, a NULL pack on one of four segments, an unaligned bias: the forced tall tile falls back, silently,
    to the same bits -- and reads no pack (the ones handed in hold NaNs)."""
    g = torch.Generator(device=dev).manual_seed(tile)

    def check(M, Nn, K, nseg, null=None, odd_bias=False):
        x = torch.randn(M, K, device=dev, generator=g)
        ws = [torch.randn(Nn, K, device=dev, generator=g) for _ in range(nseg)]
        raw = [torch.randn(Nn + 1, device=dev, generator=g) for _ in range(nseg)]
        bs = [b[1:] if odd_bias else b[:Nn].clone() for b in raw]   # b[1:]: four bytes past a 16-byte boundary
        poison = [None if s == null else torch.full((Nn * K,), float('nan'), device=dev) for s in range(nseg)]
        want = launch(tuning, 0, x, ws, None, bs=bs, relu=True)
        got = launch(tuning, tile, x, ws, poison, bs=bs, relu=True)
        assert same(got, want) and not any(bool(torch.isnan(o).any()) for o in got), (tile, M, Nn, K, nseg, null, odd_bias)

    for M in (65, 200):
        check(M, 72, 64, 1)
        check(M, 64, 48, 1)
        check(M, 64, 64, 4, null=2)
        check(M, 64, 64, 1, odd_bias=True)
        check(M, 64, 64, 3, odd_bias=True)


# ------------------------------------------------------------------ the forward
SMALL = (50, 5, 7, 64, 128, 2, 'prior', True, 3, 0.3, [7, 3, 5])   # V, L, T, d, dff, h, mask, pos_emb, B, p, lengths: one ragged batch


def forward_variants(m, src, tuning, monkeypatch):
    """logits / enc_output of the model through the tuning library: packs with every GEMM forced to each tall tile, packs
    unforced, no K / V packs, no packs at all (lamp_forward)."""
    from lamp_amd import _native as N
    monkeypatch.setattr(N, '_lib', tuning)

    def run(tile, packs=True, kv=True):
        m.use_gemm_packs, m.use_kv_gemm_packs = packs, kv
        tuning.lamp_debug_force_gemm_tile(tile)
        try:
            with torch.no_grad():
                logits, enc, _ = m(src, None, None, None)
            keep = m._native_cache[1][9]
            assert (keep is not None) == packs and (keep is not None and keep[4] is not None) == (packs and kv)
            return logits.clone(), enc.clone()
        finally:
            tuning.lamp_debug_force_gemm_tile(0)
            del m.use_gemm_packs, m.use_kv_gemm_packs

    return {'tile19': run(19), 'tile20': run(20), 'unforced': run(0), 'no kv packs': run(0, kv=False), 'no packs': run(0, packs=False)}


def assert_all_equal(outs):
    want = outs['no packs']
    assert bool(torch.isfinite(want[0]).all()) and bool(want[0].abs().sum() > 0)
    for name, got in outs.items():
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name


def test_forward_with_kv_packs_on_every_tall_tile(dev, tuning, monkeypatch):
    from test_gpu_parity import make_case
    m, sd, blocked, seq, spos, h = make_case(SMALL, dev)
    assert type(m).use_kv_gemm_packs is True
    assert_all_equal(forward_variants(m, (seq.to(dev), spos.to(dev)), tuning, monkeypatch))


def test_forward_with_kv_packs_layer_by_layer(dev, tuning, monkeypatch):
    """Decoder layers that differ in head count: their K / V projections cannot share one segment list (another width), so each
    layer projects on its own -- with its own two packs."""
    from lamp_amd.SubLayers import MultiHeadAttention
    from test_gpu_parity import make_case
    m, sd, blocked, seq, spos, h = make_case(SMALL, dev)
    torch.manual_seed(5)
    m.decoder.layer_stack[1].enc_attn = MultiHeadAttention(4, 64, 32, 32).to(dev).eval()
    m._param_list = m._native_cache = None
    assert m.decoder.layer_stack[0].enc_attn.n_head == 2 and m.decoder.layer_stack[1].enc_attn.w_ks.weight.shape == (128, 64)
    assert_all_equal(forward_variants(m, (seq.to(dev), spos.to(dev)), tuning, monkeypatch))
