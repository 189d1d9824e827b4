"""The backward composites' workspace sizes cover every product they issue (no GPU: size queries launch nothing).

lamp_ffn_bwd / lamp_mha_bwd hand ONE workspace to all their single-batch products.  lamp_gemm_workspace_bytes is not monotone
in the shape -- an output of 512 tiles or more takes no K split and needs 0 bytes, a smaller non-square one with K >= 1024
wants up to 64 partial copies -- so a bound taken at "the largest square" comes up short, the composite then runs that product
with fewer splits (or none) than lamp_gemm does with its own workspace, and "same bits as the per-launch route" is lost.
These tests hold each size function against the products the header documents, over a grid that crosses the 512-tile and
K = 1024 thresholds in both directions."""
import ctypes as C
import itertools

import pytest

from lamp_amd import _native as N

ROWS = (180, 1024, 2880, 5000, 16384, 40000)
WIDTHS = (32, 64, 128, 256, 512, 1024, 2048, 4096)


def gemm_bytes(M, N_, K):
    return N.lib().lamp_gemm_workspace_bytes(M, N_, K, 1)


def test_gemm_workspace_is_not_monotone_in_the_shape():
    """The premise: the product that a K split helps needs bytes, the 'bigger' square one none."""
    assert gemm_bytes(2048, 2048, 2880) == 0
    assert gemm_bytes(2048, 512, 2880) > 0


def ffn_products(M, d, dff):
    """(name, M, N, K) of the four products of lamp_ffn_bwd (include/lamp_hip.h): dW2 = d_o^T h, dh = d_o W2, dW1 = dh^T x,
    dx += dh W1."""
    return (('dW2', d, dff, M), ('dh', M, dff, d), ('dW1', dff, d, M), ('dx', M, d, dff))


def test_ffn_bwd_workspace_covers_each_of_its_products():
    L = N.lib()
    short = []
    for M, d, dff in itertools.product(ROWS, WIDTHS, WIDTHS):
        have = L.lamp_ffn_bwd_workspace_bytes(M, d, dff)
        for name, m, n, k in ffn_products(M, d, dff):
            need = gemm_bytes(m, n, k)
            if have < need:
                short.append((M, d, dff, name, have, need))
    combos = {s[:3] for s in short}
    assert not short, '%d of %d shapes short, first: %s' % (len(combos), len(ROWS) * len(WIDTHS) ** 2, short[:3])


def test_ffn_bwd_workspace_covers_layernorm_and_colsum():
    L = N.lib()
    for M, d, dff in itertools.product(ROWS, (32, 512, 4096), (32, 512, 4096)):
        have = L.lamp_ffn_bwd_workspace_bytes(M, d, dff)
        assert have >= L.lamp_layernorm_bwd_workspace_bytes(M, d)
        assert have >= L.lamp_colsum_workspace_bytes(M, dff)


def test_ffn_bwd_workspace_documented_example():
    """2880 rows, d_model 512, d_inner 2048: dW1 [2048, 512] over K = 2880 splits K; the square 2048 x 2048 does not."""
    L = N.lib()
    assert L.lamp_ffn_bwd_workspace_bytes(2880, 512, 2048) >= gemm_bytes(2048, 512, 2880) == 16777216


# (B, lq, lk): Mq = B * lq and Mk = B * lk on both sides of K = 1024 and far beyond; lq != lk so dwq and dwk differ in K
MHA_ROWS = ((2, 90, 90), (32, 90, 300), (4, 300, 45), (64, 20, 625), (16, 1000, 70), (8, 128, 1200), (1, 1500, 1500))
MHA_DMODEL = (64, 512, 2048)
MHA_HEADS = ((1, 16), (1, 128), (4, 32), (4, 128), (8, 64), (16, 16), (16, 32), (16, 64), (16, 128), (2, 128))


def mha_products(B, lq, lk, d, H, dk, dv):
    """The eight single-batch products of lamp_mha_bwd (the per-head ones take no workspace)."""
    Mq, Mk, hdk, hdv = B * lq, B * lk, H * dk, H * dv
    return (('dfc', d, hdv, Mq), ('da', Mq, hdv, d), ('dwq', hdk, d, Mq), ('dwk', hdk, d, Mk), ('dwv', hdv, d, Mk),
            ('dxq', Mq, d, hdk), ('dxk', Mk, d, hdk), ('dxv', Mk, d, hdv))


def test_mha_bwd_workspace_covers_each_of_its_products():
    L = N.lib()
    short, total = [], 0
    for (B, lq, lk), d, (H, dh) in itertools.product(MHA_ROWS, MHA_DMODEL, MHA_HEADS):
        total += 1
        desc = N.MhaTrainDesc(B, lq, lk, d, H, dh, dh, dh ** -0.5, 0.0, 0.0, 0, 0)
        have = L.lamp_mha_bwd_workspace_bytes(C.byref(desc))
        assert have >= L.lamp_layernorm_bwd_workspace_bytes(B * lq, d)
        for name, m, n, k in mha_products(B, lq, lk, d, H, dh, dh):
            need = gemm_bytes(m, n, k)
            if have < need:
                short.append((B, lq, lk, d, H, dh, name, have, need))
    combos = {s[:6] for s in short}
    assert not short, '%d of %d shapes short, first: %s' % (len(combos), total, short[:3])


def test_mha_bwd_workspace_with_unequal_head_widths():
    """d_k != d_v: dwq / dwk are [H d_k, d], dwv / dfc are over H d_v."""
    L = N.lib()
    for dk, dv in ((16, 128), (128, 16)):
        desc = N.MhaTrainDesc(32, 90, 300, 512, 16, dk, dv, dk ** -0.5, 0.0, 0.0, 0, 0)
        have = L.lamp_mha_bwd_workspace_bytes(C.byref(desc))
        for name, m, n, k in mha_products(32, 90, 300, 512, 16, dk, dv):
            assert have >= gemm_bytes(m, n, k), (dk, dv, name)


def test_mha_bwd_workspace_documented_example():
    """B = 32, lq = 90, lk = 300, d_model 512, 16 heads of 128: dwk [2048, 512] over K = 9600."""
    desc = N.MhaTrainDesc(32, 90, 300, 512, 16, 128, 128, 128 ** -0.5, 0.0, 0.0, 0, 0)
    assert N.lib().lamp_mha_bwd_workspace_bytes(C.byref(desc)) >= gemm_bytes(2048, 512, 9600) == 16777216


@pytest.mark.parametrize('M,d,dff', [(1024, 64, 1536), (70, 64, 96)])
def test_ffn_bwd_workspace_is_the_maximum_not_more(M, d, dff):
    """Exactly the maximum over what the call issues: a caller's buffer is not inflated."""
    L = N.lib()
    want = max([L.lamp_layernorm_bwd_workspace_bytes(M, d), L.lamp_colsum_workspace_bytes(M, dff)] +
               [gemm_bytes(m, n, k) for _, m, n, k in ffn_products(M, d, dff)])
    assert L.lamp_ffn_bwd_workspace_bytes(M, d, dff) == want
