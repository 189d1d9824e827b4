"""-m gpu: the packed-W tile of the forward GEMM (csrc/gemm.hip, GemmParams::Wp) against the LDS-staged route.

The packed route changes where a wave's weight fragments come from (a fragment-major copy, lamp_pack_weight format 0, straight
into registers) and nothing about which products are summed in which order: every comparison here is bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from lamp_amd import _native as N
    assert getattr(N.lib(), 'lamp_linear_packed_fwd', None) and getattr(N.lib(), 'lamp_forward_packs', None)
    return torch.device('cuda:0')


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def operands(dev, M, N_, K, nseg, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dev)
    ws = [(torch.randn(N_, K, generator=g) / K ** 0.5).to(dev) for _ in range(nseg)]
    bs = [torch.randn(N_, generator=g).to(dev) for _ in range(nseg)]
    r = torch.randn(M, N_, generator=g).to(dev)
    return x, ws, bs, r


def both_routes(N, x, ws, bs, r, epilogue, **kw):
    """-> (staged outputs, packed outputs); epilogue: bias + ReLU (+ the residual, which only a single segment takes)"""
    packs = [N.weight_pack(w, 0) for w in ws]
    args = dict(biases=bs, residual=r if len(ws) == 1 else None, relu=True) if epilogue else {}
    args.update(kw)
    return N.linear_packed(x, ws, None, **args), N.linear_packed(x, ws, packs, **args), packs


@pytest.mark.parametrize('nseg', [1, 3])
@pytest.mark.parametrize('K', [32, 64, 96, 512])   # 1, 2, 3 (odd: the k loop's tail step) and 16 k-tiles
@pytest.mark.parametrize('N_', [64, 512])
def test_packed_linear_equals_staged(dev, N_, K, nseg):
    from lamp_amd import _native as N
    for M in (1, 31, 32, 33, 90):
        x, ws, bs, r = operands(dev, M, N_, K, nseg, M * 1000 + N_ + K + nseg)
        for epilogue in (False, True):
            staged, packed, packs = both_routes(N, x, ws, bs, r, epilogue)
            assert all(p is not None for p in packs)
            for s, (a, b) in enumerate(zip(staged, packed)):
                assert same_bits(a, b), (M, N_, K, nseg, epilogue, s)
            # ... and the staged route is the one-matrix entry point, so the packed route is it too
            one = N.linear(x, ws[0], bs[0] if epilogue else None, residual=r if epilogue and nseg == 1 else None, relu=epilogue)
            assert same_bits(one, packed[0]), (M, N_, K, nseg, epilogue)


@pytest.mark.parametrize('M,live', [(90, 41), (90, 0), (9664, 9001)])   # 9664 x 512: the launch size of the encoder FFN at batch 32
def test_packed_linear_with_a_device_side_row_count(dev, M, live):
    from lamp_amd import _native as N
    x, ws, bs, r = operands(dev, M, 512, 512, 1, M + live)
    m_dev = torch.tensor([live], dtype=torch.int32, device=dev)
    full_s, full_p, _ = both_routes(N, x, ws, bs, r, True)
    part_s, part_p, _ = both_routes(N, x, ws, bs, r, True, m_dev=m_dev)
    assert same_bits(full_s[0], full_p[0]) and same_bits(part_s[0], part_p[0])
    assert same_bits(part_p[0][:live], full_p[0][:live])
    assert not part_p[0][live:].any()            # rows past the count are not written (the wrapper hands out zeros)


def test_a_shape_the_pack_cannot_express_takes_the_staged_kernel(dev):
    """N = 72 is not a multiple of 16 and K = 48 not of 32: lamp_pack_weight has no format-0 pack for it, and a pointer handed in
    anyway must not be read -- the launch falls back, silently, to the same bits."""
    from lamp_amd import _native as N
    x, ws, bs, r = operands(dev, 90, 72, 48, 1, 7)
    assert N.weight_pack(ws[0], 0) is None
    poison = torch.full((72 * 48,), float('nan'), device=dev)
    for epilogue in (False, True):
        args = dict(biases=bs, residual=r, relu=True) if epilogue else {}
        staged = N.linear_packed(x, ws, None, **args)[0]
        assert same_bits(staged, N.linear_packed(x, ws, [poison], **args)[0])
        assert same_bits(staged, N.linear(x, ws[0], bs[0] if epilogue else None, residual=r if epilogue else None, relu=epilogue))


@pytest.mark.parametrize('name', ['reuters_fixed', 'inveye_8h'])
def test_model_with_and_without_gemm_packs(dev, name):
    from test_gpu_parity import CONFIGS, make_case
    m, sd, blocked, seq, spos, h = make_case(CONFIGS[name], dev)
    src = (seq.to(dev), spos.to(dev))

    def run(packs):
        m.use_gemm_packs = packs
        try:
            with torch.no_grad():
                logits, enc, _ = m(src, None, None, None)
            assert (m._native_cache[1][9] is not None) == packs     # the packs exist exactly when the switch is on
            return logits.clone(), enc.clone()
        finally:
            del m.use_gemm_packs

    assert type(m).use_gemm_packs is True
    on, off = run(True), run(False)
    assert same_bits(on[0], off[0]) and same_bits(on[1], off[1])
    # an in-place update of a packed weight must refresh its pack: new logits, again the packs-off route's
    with torch.no_grad():
        m.decoder.layer_stack[1].slf_attn.w_ks.weight.mul_(1.5)
        m.encoder.layer_stack[1].pos_ffn.w_2.weight.mul_(0.5)
    on2, off2 = run(True), run(False)
    assert not same_bits(on2[0], on[0]) and not same_bits(on2[1], on[1])
    assert same_bits(on2[0], off2[0]) and same_bits(on2[1], off2[1])
