"""Large extents without a GPU (DESIGN.md "Addressing limits"; the harness is tests/large_extent_common.py):

  * every `*_bytes()` query of the ABI at arguments whose products pass 2^31 and 2^32: the value equals -- or, where the layout
    is private, is at least -- an exact Python-integer restatement of the buffers include/lamp_hip.h documents, never decreases
    when one dimension grows, and is 0 only where the header says 0 means refusal;
  * the host-side guards of the table at their limits: the documented status, before any launch (a launch on a host without a
    GPU would come back as a positive hipError_t; 16 stands in for a pointer, as in test_ranking_cpu.py).  Not here, because
    they sit behind a launch or a kernel attribute and need a device: lamp_colsum's second-stage grid and the tile GEMM's
    tile count;
  * the harness itself: layout, windows, periodic fills, the arena's own checks;
  * the windows of the GPU cases tell a narrowed index: the row- and element-offset arithmetic of the pointer-based kernels
    (dropout's counter, row * d of the row kernels, row * L of the loss and metric matrices, the optimizer's chunk offset)
    restated with the index narrowed to 32 bits (the mutants of large_extent_common.py) differs from the reference beyond the
    case's bar, at window indices only.  A narrowed offset on the WRITE side needs no restatement: it leaves sentinel in the
    output or changes the landing zone, which the arena's own checks (held above) catch."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import large_extent_common as LX
from lamp_amd import _native as N

E_DIMS, E_ALIGN, E_WORKSPACE, E_UNSUPPORTED, E_NULL = -1, -2, -3, -4, -5
I31 = 1 << 31
P = 16            # the stand-in pointer (16-byte aligned, never dereferenced: every call below is refused before a launch)


def align_up(n, a):
    return (n + a - 1) // a * a


def ln_bwd_bytes(M, d):
    return min((M + 3) // 4, 256) * 3 * d * 4


def colsum_bytes(M, Nn):
    return min(512, max(1, (M + 63) // 64)) * Nn * 4


# ====================================================================================== size queries
def grows(fn, base, dims):
    """fn(*args) never decreases when one of the listed argument positions grows with the rest fixed."""
    for i in dims:
        for factor in (2, 3, 17):
            more = list(base)
            more[i] = base[i] * factor
            assert fn(*more) >= fn(*base), (fn.__name__ if hasattr(fn, '__name__') else fn, base, i, factor)


def test_row_kernel_size_queries_are_exact_past_2_32():
    L = N.lib()
    for M, d, dff in (((1 << 22) + 5, 512, 4096), ((1 << 28) + 3, 1028, 2048), (I31 - 1, 4096, 4096)):
        assert M * dff * 4 > 1 << 32
        assert L.lamp_ffn_workspace_bytes(M, d, dff) == align_up(M * dff * 4, 256)
        assert L.lamp_layernorm_bwd_workspace_bytes(M, d) == ln_bwd_bytes(M, d)
        assert L.lamp_colsum_workspace_bytes(M, dff) == colsum_bytes(M, dff)
        assert L.lamp_ffn_bwd_partials_bytes(M, d, dff) == align_up(ln_bwd_bytes(M, d), 256) + colsum_bytes(M, dff)
    # a wide column sum: N itself past 2^31, the product of chunks and N past 2^32
    assert L.lamp_colsum_workspace_bytes(37, I31 + 4) == (I31 + 4) * 4
    assert L.lamp_colsum_workspace_bytes(1 << 20, I31 + 4) == 512 * (I31 + 4) * 4
    assert L.lamp_attn_bias_bwd_workspace_bytes(1 << 17, 70000, 70000) == colsum_bytes(1 << 17, 70000 * 70000) > 1 << 32
    grows(L.lamp_ffn_workspace_bytes, ((1 << 22) + 5, 512, 4096), (0, 2))
    grows(L.lamp_layernorm_bwd_workspace_bytes, (1 << 22, 512), (0, 1))
    grows(L.lamp_colsum_workspace_bytes, ((1 << 22) + 5, 1 << 20), (0, 1))
    grows(L.lamp_attn_bias_bwd_workspace_bytes, (1 << 12, 3000, 3000), (0, 1, 2))
    grows(L.lamp_ffn_bwd_partials_bytes, ((1 << 22) + 5, 512, 4096), (0, 1, 2))
    # 0 means refusal (non-positive sizes; lamp_ffn_bwd_workspace_bytes also M > 0x7fffffff, the row count of its products)
    assert L.lamp_ffn_workspace_bytes(0, 512, 2048) == 0 and L.lamp_colsum_workspace_bytes(4, 4) > 0
    assert L.lamp_attn_bias_bwd_workspace_bytes(0, 4, 4) == 0 and L.lamp_ffn_bwd_partials_bytes(0, 4, 4) == 0
    assert L.lamp_ffn_bwd_workspace_bytes(I31, 64, 64) == 0 and L.lamp_ffn_bwd_workspace_bytes(I31 - 1, 64, 64) > 0


def test_gemm_and_backward_composite_size_queries():
    L = N.lib()
    # lamp_gemm_workspace_bytes: 0 (no K split) or splits x M x N floats with 2 <= splits <= 64
    for M, Nn, K, batch in ((2048, 512, I31 - 1, 1), (64, 64, I31 - 1, 1), (30000, 30000, 4096, 1), (46000, 46000, 1 << 20, 1)):
        b = L.lamp_gemm_workspace_bytes(M, Nn, K, batch)
        assert b % (M * Nn * 4) == 0 and b // (M * Nn * 4) in [0] + list(range(2, 65)), (M, Nn, K, b)
    assert L.lamp_gemm_workspace_bytes(8192, 8192, I31 - 1, 1) in (0,) + tuple(s * 8192 * 8192 * 4 for s in range(2, 65))
    assert L.lamp_gemm_workspace_bytes(0, 4, 4, 1) == 0 and L.lamp_gemm_workspace_bytes(4, 4, 4, 0) == 0
    # the composites are the maximum over what they issue, each part asked for on its own (test_workspace_bounds_cpu.py holds
    # this at small shapes): here with B * lq and M next to 2^31
    for M, d, dff in (((1 << 22) + 5, 512, 2048), (I31 - 1, 64, 128)):
        prods = (('dW2', d, dff, M), ('dh', M, dff, d), ('dW1', dff, d, M), ('dx', M, d, dff))
        want = max([ln_bwd_bytes(M, d), colsum_bytes(M, dff)] + [L.lamp_gemm_workspace_bytes(m, n, k, 1) for _, m, n, k in prods])
        assert L.lamp_ffn_bwd_workspace_bytes(M, d, dff) == want
    for B, lq, lk, d, H, dk in ((1 << 15, 1 << 10, 300, 512, 4, 32), ((1 << 16) - 1, 1 << 15, 1 << 15, 64, 1, 16)):
        desc = N.MhaTrainDesc(B, lq, lk, d, H, dk, dk, dk ** -0.5, 0.0, 0.0, 0, 0)
        Mq, Mk, hd = B * lq, B * lk, H * dk
        assert L.lamp_mha_bwd_partials_bytes(C.byref(desc)) == ln_bwd_bytes(Mq, d)
        prods = ((d, hd, Mq), (Mq, hd, d), (hd, d, Mq), (hd, d, Mk), (hd, d, Mk), (Mq, d, hd), (Mk, d, hd), (Mk, d, hd))
        want = max([ln_bwd_bytes(Mq, d)] + [L.lamp_gemm_workspace_bytes(m, n, k, 1) for m, n, k in prods])
        assert L.lamp_mha_bwd_workspace_bytes(C.byref(desc)) == want
    over = N.MhaTrainDesc(1 << 16, 1 << 15, 300, 64, 1, 16, 16, 0.25, 0.0, 0.0, 0, 0)       # B * lq = 2^31: refused
    assert L.lamp_mha_bwd_workspace_bytes(C.byref(over)) == 0


def test_attention_and_forward_size_queries_do_not_wrap():
    import test_host_cpu as H
    L = N.lib()
    # lamp_mha_workspace_bytes: a private layout; at least the four projections it documents (q, k, v and the head outputs)
    for B, lq, lk, d, h, dk, dv in ((1 << 14, 300, 1000, 512, 4, 128, 128), ((1 << 16) - 1, 983, 983, 512, 4, 32, 64)):
        floor = B * (lq * h * dk + lk * h * dk + lk * h * dv + lq * h * dv) * 4
        assert floor > 1 << 32 and L.lamp_mha_workspace_bytes(B, lq, lk, d, h, dk, dv) >= floor
    grows(L.lamp_mha_workspace_bytes, (1 << 12, 300, 1000, 512, 4, 32, 32), (0, 1, 2, 4, 5, 6))
    assert L.lamp_mha_workspace_bytes(0, 4, 4, 64, 1, 16, 16) == 0
    # the forward's workspace, every variant: exactly affine in the micro-batch up to sizes past 2^32, at least the encoder FFN's
    # hidden rows (micro_batch x T x d_inner floats for the token front end), growing with T
    d, dff, T, Lb = 512, 2048, 1000, 919
    m, keep = H.dummy_model(L=Lb, d=d, dff=dff, h=4, n_enc=2, n_dec=2)
    mo, keep_o = H.dummy_model(L=Lb, d=d, dff=dff, h=4, n_enc=2, n_dec=2, onehot=True)
    fe = N.OnehotFrontend(16, 16, 16, 16, None, 9, 16)
    opts = N.FwdOptions(1, 0, None, None)
    queries = {
        'forward': lambda mb, T_, w: L.lamp_forward_workspace_bytes(C.byref(m), mb, T_, w),
        'forward_opts': lambda mb, T_, w: L.lamp_forward_opts_workspace_bytes(C.byref(m), C.byref(opts), mb, T_, w),
        'onehot': lambda mb, T_, w: L.lamp_onehot_forward_workspace_bytes(C.byref(mo), C.byref(fe), mb, T_, w),
        'onehot_opts': lambda mb, T_, w: L.lamp_onehot_forward_opts_workspace_bytes(C.byref(mo), C.byref(fe), C.byref(opts), mb, T_, w),
    }
    for name, q in queries.items():
        for want_attn in (0, 1):
            one, two = q(1, T, want_attn), q(2, T, want_attn)
            slope, fixed = two - one, 2 * one - two
            assert slope > 0 and fixed >= 0, name
            for mb in (1050, 8192, 1 << 20):
                got = q(mb, T, want_attn)
                assert got == fixed + slope * mb and got > 1 << 32, (name, mb, got)
            t_rows = T if name.startswith('forward') else T // 2
            assert slope >= t_rows * dff * 4, (name, slope)
            assert q(1050, 2 * T, want_attn) >= q(1050, T, want_attn)
            assert q(0, T, want_attn) == 0
    assert queries['forward'](1050, T, 1) > queries['forward'](1050, T, 0)      # the maps' scratch counts


def test_metrics_and_optimizer_size_queries():
    L = N.lib()
    n, Lb = 1168371 + 300, 919               # the (n, L) matrix of the GPU cases: past 2^32 bytes
    assert n * Lb * 4 > 1 << 32
    rk = L.lamp_ranking_metrics_workspace_bytes(n, Lb)
    tu = L.lamp_tune_thresholds_workspace_bytes(n, Lb)
    assert rk >= 2 * n * Lb * 4 and tu >= 2 * n * Lb * 4          # global route: two key buffers (test_ranking_cpu.py)
    grows(L.lamp_ranking_metrics_workspace_bytes, (n, Lb), (0, 1))
    grows(L.lamp_tune_thresholds_workspace_bytes, (n, Lb), (0, 1))
    assert L.lamp_ranking_metrics_workspace_bytes(I31, 1) == 0 and L.lamp_ranking_metrics_workspace_bytes(I31 - 1, 1) > 0
    assert L.lamp_tune_thresholds_workspace_bytes(I31, 1) == 0 and L.lamp_tune_thresholds_workspace_bytes(n, 65535 * 64 + 1) == 0
    ra = L.lamp_rank_at_k_workspace_bytes
    assert ra(I31 - 1, 64) > 1 << 32 and ra(I31, 5) == 0 and ra(n, 65) == 0 and ra(0, 5) == 0
    grows(ra, (n, 3), (0, 1))          # (k stays within 64: 3 x 17 = 51)
    # lamp_grad_norm_workspace_bytes: 8 bytes per 4096-element chunk, exact; 0 for a table of 2^31 chunks or more
    numels = [(1 << 42) + 1, 0, 4097, (1 << 30) + 4099]
    arr = (N.OptimEntry * len(numels))(*[N.OptimEntry(P, P, P, P, k) for k in numels])
    assert L.lamp_grad_norm_workspace_bytes(arr, len(numels)) == 8 * sum((k + 4095) // 4096 for k in numels) > 1 << 32
    rest = sum((k + 4095) // 4096 for k in numels[1:])
    arr[0].numel = (I31 - 1 - rest) * 4096
    assert L.lamp_grad_norm_workspace_bytes(arr, len(numels)) == 8 * (I31 - 1)
    arr[0].numel += 1
    assert L.lamp_grad_norm_workspace_bytes(arr, len(numels)) == 0
    # lamp_onehot_front_bwd_partials_bytes: chunks x n_vocab x 16 x d floats, the chunk count a function of B * T alone
    fb = L.lamp_onehot_front_bwd_partials_bytes
    per_chunk = 9 * 16 * 512 * 4
    big = fb(1 << 15, 1 << 15, 9, 512)
    assert big % per_chunk == 0 and big > 1 << 32 and fb(1 << 15, 1 << 15, 9, 1024) == 2 * big and fb(0, 8, 9, 512) == 0
    grows(fb, (1 << 10, 1 << 10, 9, 512), (0, 1, 2, 3))


# ====================================================================================== guards: the status before any launch
def test_row_launchers_refuse_a_grid_of_more_than_2_31_blocks():
    """grid4 (pointwise.hip), and its restatements in backward.hip and train_step.hip: one wave per row, four rows per
    workgroup, so (rows + 3) / 4 must fit a 31-bit grid.  The last admitted row count passes this check and fails at the next
    (a NULL pointer), which shows where the limit stands without a launch."""
    L = N.lib()
    last, over = 4 * (I31 - 1), 4 * (I31 - 1) + 1
    assert L.lamp_layernorm_fwd(P, over, 512, P, P, 1e-5, P, None) == E_DIMS
    assert L.lamp_layernorm_residual_fwd(P, None, 0, over, 512, P, P, 1e-5, 0.0, 0, P, None) == E_DIMS
    assert L.lamp_embed_fwd(P, P, over, P, 10, P, 10, 512, P, None) == E_DIMS
    assert L.lamp_diag_logits_fwd(P, P, I31 - 1, 5, 512, P, None) == E_DIMS
    assert L.lamp_sigmoid_bce_fwd(P, P, over, 919, P, P, None) == E_DIMS
    assert L.lamp_softmax_bwd(P, P, over, 300, 0.25, P, None) == E_DIMS
    assert L.lamp_embed_bwd(P, over, P, 512, 10, -1, P, None) == E_DIMS
    assert L.lamp_embed_bwd_ordered(P, over, P, 512, 10, -1, P, None) == E_DIMS
    xs, ws = (C.c_void_p * 1)(P), (C.c_float * 1)(1.0)
    assert L.lamp_bce_logits_train(xs, ws, None, 1, P, over + 3, 919, P, 919, P, over + 3, None) == E_UNSUPPORTED
    assert L.lamp_multilabel_loss_train(xs, ws, None, 1, P, over + 3, 919, P, 919, P, over + 3, None, None) == E_UNSUPPORTED
    # one step inside, the limit is not what refuses: the next check does (a NULL output)
    assert L.lamp_softmax_bwd(P, P, last, 300, 0.25, None, None) == E_NULL
    assert L.lamp_embed_bwd(P, last, P, 512, 10, -1, None, None) == E_NULL
    # column-wise grids: 256 (first stage) and 32 (second stage) columns per workgroup
    assert L.lamp_colsum(P, 4, 256 * (I31 - 1) + 1, 256 * (I31 - 1) + 1, P, P, 1 << 62, None) == E_DIMS
    assert L.lamp_attn_bias_bwd(P, 4, 1 << 20, 1 << 20, 1.0, None, 0, P, 1 << 20, P, 1 << 62, None) == E_DIMS
    assert L.lamp_label_bias_fold(P, 0x7ffffff1, None, 0x7ffffff1, P, None) == E_DIMS
    job = N.ReduceJob(P, (1 << 26) + 1, (1 << 26) + 1, (P, P, P), 4, 0)
    assert L.lamp_reduce_partials_grouped(C.byref(job), 1, None) == E_DIMS
    assert L.lamp_ffn_bwd(P, P, P, P, I31, 64, 64, C.byref(N.FfnWeights(P, P, P, P, P, P)), 0.0, 0, P, P, P, P, P, P, P, P, P, P, 1 << 62,
                          None, 0, None, None) == E_DIMS


def test_tile_gemm_refuses_leading_dimensions_beyond_its_32_bit_tile_offsets():
    """gemm.hip: launch_cfg2, gemm_split.hip: launch_split2 -- max(lda, ldw, ldc) * max(BM, BN) * 4 >= 0x7fffffff and
    ldr * BM * 4 >= 0x7fffffff are LAMP_E_UNSUPPORTED.  M = 35, N = 68 takes the 32 x 64 tile (fewer than 1200 64 x 64 tiles):
    the last admitted leading dimension is 8388604, that of the residual 16777212."""
    L = N.lib()
    ld = 8388604
    assert ld * 64 * 4 < 0x7fffffff <= (ld + 4) * 64 * 4 and 16777212 * 32 * 4 < 0x7fffffff <= 16777216 * 32 * 4
    for prec in (0, 1, 2):
        def call(lda, ldw, ldr, ldc):
            return L.lamp_linear_prec_fwd(P, 35, 64, lda, P, 68, ldw, None, P, ldr, 0, P, ldc, prec, None)
        assert call(ld + 4, 64, 68, 68) == E_UNSUPPORTED
        assert call(64, ld + 4, 68, 68) == E_UNSUPPORTED
        assert call(64, 64, 68, ld + 4) == E_UNSUPPORTED
        if prec == 0:       # (the split kernels' tiles are taller: their own limit stands lower)
            assert call(64, 64, 16777216, 68) == E_UNSUPPORTED
    assert L.lamp_linear_fwd(P, 35, 64, ld + 4, P, 68, 64, None, None, 0, 0, P, 68, None) == E_UNSUPPORTED
    Ws, Cs = (C.c_void_p * 1)(P), (C.c_void_p * 1)(P)
    assert L.lamp_linear_packed_fwd(P, 35, 64, ld + 4, Ws, None, 1, 68, 64, None, None, 0, 0, Cs, 68, None, None) == E_UNSUPPORTED


def gemm_desc(M, Nn, K, ars, acs, brs, bcs, ldc, batch=(1, 1), mask=None, ld_mask=0):
    return N.GemmDesc(P, P, P, M, Nn, K, batch[0], batch[1], 0, ars, acs, 0, 0, brs, bcs, 0, 0, ldc, 0, 0, mask, ld_mask, 1.0, 0)


def test_general_gemm_refuses_spans_beyond_its_32_bit_offsets():
    """gemm_gen.hip: a k-contiguous operand spans 64 * ld + K floats per tile, a k-strided one K * ld; either span times 4, and
    64 * ldc * 4 (64 * ld_mask * 4), must stay below 0x7fffffff -> LAMP_E_UNSUPPORTED; batch0 * batch1 > 65535 -> LAMP_E_DIMS.
    A grouped call with ONE description beyond a guard is refused whole."""
    L = N.lib()
    K = 4096
    lim = 0x7fffffff
    ld_row = (lim - 1) // 4 - K          # 64 * ld + K < lim / 4
    ld_row = (ld_row // 64)
    assert (64 * ld_row + K) * 4 < lim <= (64 * (ld_row + 1) + K) * 4
    ld_k = (lim - 1) // 4 // K
    assert K * ld_k * 4 < lim <= K * (ld_k + 1) * 4
    ldc = (lim - 1) // 256
    assert 64 * ldc * 4 < lim <= 64 * (ldc + 1) * 4

    def run(d):
        return L.lamp_gemm(C.byref(d), None, 0, None)
    assert run(gemm_desc(64, 64, K, ld_row + 1, 1, K, 1, 64)) == E_UNSUPPORTED           # row-major A
    assert run(gemm_desc(64, 64, K, K, 1, ld_row + 1, 1, 64)) == E_UNSUPPORTED           # row-major B
    assert run(gemm_desc(64, 64, K, 1, ld_k + 1, 1, 64, 64)) == E_UNSUPPORTED            # k-strided A (dW = dY^T X)
    assert run(gemm_desc(64, 64, K, 1, 64, 1, ld_k + 1, 64)) == E_UNSUPPORTED
    assert run(gemm_desc(64, 64, K, K, 1, K, 1, ldc + 1)) == E_UNSUPPORTED
    assert run(gemm_desc(64, 64, K, K, 1, K, 1, 64, mask=P, ld_mask=ldc + 1)) == E_UNSUPPORTED
    assert run(gemm_desc(64, 64, K, K, 1, K, 1, 64, batch=(256, 256))) == E_DIMS
    descs = (N.GemmDesc * 3)(gemm_desc(64, 64, K, 1, 64, 1, 64, 64), gemm_desc(64, 64, K, 1, ld_k + 1, 1, 64, 64),
                             gemm_desc(64, 64, K, 1, 64, 1, 64, 64))
    assert L.lamp_gemm_grouped(descs, 3, None) == E_UNSUPPORTED


def test_attention_refuses_slices_beyond_its_32_bit_offsets():
    """attention.hip: launch_attn -- inside one (sample, head) slice the offsets are 32-bit: lq * q_r * 4, lk * k_r * 4,
    lk * v_r * 4, (lq * stride_q + lk) bytes of a u8 mask (x 4 for bit-packed words), (lq * stride_q + lk + 3) * 4 of a bias,
    each >= 0x7fffffff -> LAMP_E_UNSUPPORTED."""
    L = N.lib()
    lq = lk = 300
    r_max = (0x7fffffff - 1) // (4 * lq) // 4 * 4
    assert lq * r_max * 4 < 0x7fffffff <= lq * (r_max + 4) * 4

    def call(lay, mask=None):
        return L.lamp_sdpa_fwd(P, P, P, P, None, 2, 2, lq, lk, 32, 32, 1.0, None if mask is None else C.byref(mask),
                               C.byref(N.AttnLayout(*lay)), None)
    ok_lay = [lq * 64, 32, 64] * 4
    for which in (2, 5, 8):                      # q_r, k_r, v_r
        lay = list(ok_lay)
        lay[which] = r_max + 4
        assert call(lay) == E_UNSUPPORTED, which
    sq_u8 = (0x7fffffff - lk) // lq + 1
    assert lq * sq_u8 + lk >= 0x7fffffff > lq * (sq_u8 - 1) + lk
    assert call(ok_lay, N.Mask(1, 0, P, 0, sq_u8, None, 0, 0)) == E_UNSUPPORTED
    sq_bits = ((0x7fffffff + 3) // 4 - lk) // lq + 1
    assert call(ok_lay, N.Mask(3, 0, P, 0, sq_bits, None, 0, 0)) == E_UNSUPPORTED
    sq_bias = (((0x7fffffff + 3) // 4 - lk - 3) // lq + 1 + 3) // 4 * 4
    assert call(ok_lay, N.Mask(4, 0, P, 0, sq_bias, None, 0, 0)) == E_UNSUPPORTED


def test_metrics_ranking_and_optimizer_refuse_2_31_rows_and_chunks():
    L = N.lib()
    big = 1 << 62
    assert L.lamp_ranking_metrics(P, 919, P, 919, I31, 919, 0.5, P, P, P, None, None, P, big, None) == E_UNSUPPORTED
    assert L.lamp_tune_thresholds(P, 919, P, 919, I31, 919, 0, 0.5, P, P, P, P, P, None, P, big, None) == E_UNSUPPORTED
    assert L.lamp_topk_labels(P, 919, I31, 919, 5, P, 5, None, 0, None) == E_UNSUPPORTED
    disc, ideal = (C.c_double * 5)(), (C.c_double * 6)()
    assert L.lamp_rank_at_k(P, 5, P, 919, I31, 919, 5, disc, ideal, P, P, P, P, P, big, None) == E_UNSUPPORTED
    rows = I31           # the per-label counts are int32
    assert L.lamp_threshold_counts(P, 919, P, 919, rows, 919, 0.5, P, P, P, P, P, P, P, None) == E_UNSUPPORTED
    assert L.lamp_threshold_counts_vec(P, 919, P, 919, rows, 919, P, P, P, P, P, P, P, P, None) == E_UNSUPPORTED
    # 2^31 chunks of 4096 elements in one table
    arr = (N.OptimEntry * 2)(N.OptimEntry(P, P, P, P, (I31 - 1) * 4096), N.OptimEntry(P, P, P, P, 1))
    assert L.lamp_grad_norm(arr, 2, 1.0, P, big, P, None, None) == E_UNSUPPORTED
    one = (N.OptimEntry * 1)(N.OptimEntry(P, P, P, P, I31 * 4096))
    assert L.lamp_optim_step(one, 1, N.LAMP_OPTIM_ADAM, 1, 1e-3, 0.9, 0.98, 1e-8, None) == E_UNSUPPORTED
    wd = (C.c_float * 1)(0.01)
    ext = N.OptimExt(wd, None, 0.0, N.LAMP_OPTIM_DECOUPLED_DECAY, 0)
    assert L.lamp_optim_step_ext(one, 1, N.LAMP_OPTIM_ADAM, 1, 1e-3, 0.9, 0.98, 1e-8, C.byref(ext), None) == E_UNSUPPORTED
    fe = N.OnehotFrontend(P, P, P, P, None, 9, 16)
    assert L.lamp_onehot_front_bwd(P, 1 << 15, 1 << 15, C.byref(fe), 512, 0.0, 0, P, P, P, big, None) == E_DIMS


def test_composites_the_forward_and_the_remaining_guards_refuse_before_any_launch():
    """api.hip: lamp_mha_act_bwd -- B * lq, B * lk > 0x7fffffff and H * B > 65535 are LAMP_E_DIMS (lamp_mha_bwd forwards to it);
    conv.hip: launch_conv_window -- more than 0x7fffffff row tiles; the attention launchers' workgroup count; rank_at_k.hip --
    k > 64 and L > 32768 through the calls; pointwise.hip: launch_seq_plan -- nb * T >= 0x7fffffff is LAMP_E_DIMS, the first
    thing a pass of lamp_forward does on the padded route (the encoder maps are asked for) once the workspace holds the whole
    batch; the packed route counts its rows inside the gather's launch and has no such launcher.  One guard of the table
    cannot be reached with a stand-in pointer: lamp_colsum's second-stage limit, (N + 31) / 32 > 0x7fffffff, is checked after
    the first stage has been launched; for N that large the first stage's own limit, (N + 255) / 256, is the one a host sees."""
    import test_host_cpu as H
    L = N.lib()
    big = 1 << 62

    def mha_bwd(B, lq, lk, heads, act=None, ws_bytes=big):
        desc = N.MhaTrainDesc(B, lq, lk, 64, heads, 16, 16, 0.25, 0.0, 0.0, 0, 0)
        w = N.MhaWeights(P, P, P, P, P, P, heads, 0)
        ptrs = [P] * 26
        if act is None:
            return L.lamp_mha_bwd(C.byref(desc), C.byref(w), *ptrs, P, ws_bytes, None, 0, None, None)
        return L.lamp_mha_act_bwd(C.byref(desc), C.byref(w), act, *ptrs, P, ws_bytes, None, 0, None, None)
    for act in (None, 0, 1):
        assert mha_bwd(1 << 16, 1 << 15, 300, 1, act) == E_DIMS          # B * lq = 2^31
        assert mha_bwd(1 << 16, 300, 1 << 15, 1, act) == E_DIMS          # B * lk = 2^31
        assert mha_bwd(16384, 300, 300, 4, act) == E_DIMS                # H * B = 65536
        # one step inside, the limit is not what refuses: the workspace is (65535 = 3 x 21845 slices)
        assert mha_bwd(21845, 300, 300, 3, act, ws_bytes=0) == E_WORKSPACE
    m, keep = H.dummy_model(L=24, d=64, dff=128, h=4, n_enc=2, n_dec=2)
    maps = (C.c_void_p * 2)(P, P)
    aux = N.Aux(maps, None, None, None, 0, 0)
    assert (1 << 21) * 1024 >= 0x7fffffff
    assert L.lamp_forward(C.byref(m), P, P, 1 << 21, 1024, P, P, C.byref(aux), P, big, None) == E_DIMS
    del keep
    # 2^40 output rows: more than 0x7fffffff row tiles of any height up to 256
    assert L.lamp_conv_window_fwd(P, 1 << 20, 1 << 20, (1 << 20) + 16, 64, P, 64, P, 1, None, 0, None, 0, P, P, None) == E_DIMS
    # 2^32 (sample, head) slices: the workgroup count of every attention launcher passes 0x7fffffff
    lay = N.AttnLayout(*([300 * 64, 32, 64] * 4))
    for lq, lk in ((100, 40), (300, 70)):        # attention_small.hip, attn_kernel
        assert L.lamp_sdpa_fwd(P, P, P, P, None, 1 << 16, 1 << 16, lq, lk, 32, 32, 1.0, None, C.byref(lay), None) == E_DIMS
    assert L.lamp_sdpa_act_fwd(P, P, P, P, None, 1 << 16, 1 << 16, 300, 70, 32, 32, 1.0, 1, None, C.byref(lay), None) == E_DIMS
    disc, ideal = (C.c_double * 65)(), (C.c_double * 66)()
    assert L.lamp_rank_at_k(P, 65, P, 919, 100, 919, 65, disc, ideal, P, P, P, P, P, big, None) == E_UNSUPPORTED
    assert L.lamp_rank_at_k(P, 5, P, 32769, 100, 32769, 5, disc, ideal, P, P, P, P, P, big, None) == E_UNSUPPORTED
    assert L.lamp_topk_labels(P, 919, 100, 919, 65, P, 65, None, 0, None) == E_UNSUPPORTED
    assert L.lamp_topk_labels(P, 32769, 100, 32769, 5, P, 5, None, 0, None) == E_UNSUPPORTED


# ====================================================================================== the harness itself
def test_layout_windows_and_the_arena_on_the_host():
    spans, total, landing = LX.layout([('w', 100), ('x', 9 << 30), ('y', 5 << 30)])
    assert landing >= 9 << 30 and spans['w'][0] >= landing + LX.ZONE and all(a % LX.ALIGN == 0 for a, _ in spans.values())
    assert spans['x'][0] >= spans['w'][1] + LX.ZONE and total >= spans['y'][1] + LX.ZONE
    assert LX.need_bytes([('x', 17 << 30)]) < LX.BUDGET < LX.need_bytes([('x', 20 << 30)])
    assert LX.crossings((1 << 31) + 4) == ['B31'] and LX.crossings(1 << 31) == [] and LX.crossings((1 << 34) + 4)[-1] == 'E32'
    M, d = LX.LN_E31
    wins = LX.windows(M, d * 4)
    assert wins[0] == (0, 128) and wins[-1][1] == M and wins[-1][0] <= M - 128 - M % 128
    for at in (LX.B31, LX.B32, LX.E31):
        r = at // (d * 4)
        assert any(a <= r - 128 and min(r + 128, M - 1) < b for a, b in wins), at
    assert sum(b - a for a, b in wins) < 2000
    old, LX.CHUNK = LX.CHUNK, 1 << 12
    try:
        ar = LX.BigArena(torch.device('cpu'), LX.FILL_NAN, [('a', 4000), ('b', 4099 * 3 * 4 * 3 + 8)])
        ar.check_zones()
        ar.check_untouched('b')
        per = torch.randn(4099, 3)
        v = ar.view('b')[:4099 * 9].view(-1, 3)
        LX.fill_periodic_rows(v, per)
        LX.assert_bit_periodic(v, 4099, 'b')
        LX.assert_rows_equal_generator(v, per, LX.windows(4099 * 3, 12, 16), 'b')
        with pytest.raises(AssertionError, match='never written'):
            ar.check_written('b')                                   # the last two words still hold the sentinel
        with pytest.raises(AssertionError, match='refused call wrote'):
            ar.check_untouched('b')
        v[5000, 1] += 1
        with pytest.raises(AssertionError, match='not periodic'):
            LX.assert_bit_periodic(v, 4099, 'b')
        ar.mem[ar.landing - 9] = 1                         # the landing zone's last words
        with pytest.raises(AssertionError, match='landing zone'):
            ar.check_zones()
    finally:
        LX.CHUNK = old


# ====================================================================================== each case fails under its bug
def beyond(diff, bar):
    return not (diff <= bar)         # NaN (a sentinel read) counts as beyond


def rows_past(wins, first):
    return torch.cat([torch.arange(max(a, first), b) for a, b in wins if b > first])


def test_dropout_windows_tell_a_narrowed_counter():
    n, p, seed = LX.DROPOUT_N, 0.1, 1234
    for a, b in LX.windows(n, 4, LX.FLAT_WINDOW):
        true = N.dropout_keep_mask(b - a, p, seed, start=a)
        for narrow in (LX.narrow_i32, LX.narrow_u32):
            wrong = LX.mutant_keep_mask(b - a, p, seed, a, narrow)
            crossed = b > ((1 << 31) if narrow is LX.narrow_i32 else (1 << 32))
            assert torch.equal(true, wrong) != crossed, (a, b, narrow.__name__)
    # the window above E32 under the unsigned mutant IS the mask of the first 2^20 + 3 elements: what the GPU case rules out
    m = n - (1 << 32)
    assert torch.equal(LX.mutant_keep_mask(m, p, seed, 1 << 32, LX.narrow_u32), N.dropout_keep_mask(m, p, seed))
    assert not torch.equal(N.dropout_keep_mask(m, p, seed, start=1 << 32), N.dropout_keep_mask(m, p, seed))
    assert torch.equal(N.dropout_keep_mask(100, p, seed, start=50), N.dropout_keep_mask(150, p, seed)[50:])


def test_row_kernel_windows_tell_a_narrowed_row_offset():
    """lamp_layernorm_fwd / _residual_fwd and the softmax backward at E31 (an `int` row * d), the B32 cases under an unsigned
    32-bit byte offset: the rows such a kernel would read give results beyond the case's bar in the windows past the boundary."""
    g = torch.Generator().manual_seed(3)
    M, d = LX.LN_E31
    period = torch.randn(LX.PERIOD, d, generator=g) * 2 + 0.5
    rows = rows_past(LX.windows(M, d * 4), (1 << 31) // d)
    ref = F.layer_norm(LX.periodic_rows(period, rows).double(), (d,))
    bad = F.layer_norm(LX.mutant_periodic_rows(period, rows).double(), (d,))
    assert len(rows) == M - (1 << 22) and torch.isnan(bad).all()  # every row past E31 reads the landing zone's sentinel
    rows32 = rows_past(LX.windows(M, d * 4), (1 << 32) // (d * 4))
    bad = F.layer_norm(LX.mutant_periodic_rows(period, rows32, narrow=LX.narrow_u32, unit=4).double(), (d,))
    ref = F.layer_norm(LX.periodic_rows(period, rows32).double(), (d,))
    assert beyond(float((bad - ref).abs().max()), 2e-5) and float((bad - ref).abs().amax(1).min()) > 2e-5
    # rows before the boundary are untouched by either mutant: the windows there agree
    early = torch.arange(0, 128)
    assert torch.equal(LX.mutant_periodic_rows(period, early), LX.periodic_rows(period, early))
    for (n_rows, cols), bar, unit, narrow, first in (
            (LX.SOFTMAX_E31, 1e-5, 1, LX.narrow_i32, (1 << 31) // 300 + 1),
            # the (n, 919) matrix of G6: the loss launch, and the same row * ld of the threshold counts, top-k / rank-at-k, ranking
            # and tune kernels
            (LX.BCE_B32, 1e-6, 4, LX.narrow_u32, (1 << 32) // (919 * 4) + 1),
            # lamp_embed_fwd's t * d at its case's shape (d = 512); lamp_layernorm_bwd and lamp_diag_logits_bwd read the rows of
            # the LayerNorm / read-out shapes in this list
            (((1 << 30) // 512 + 2 * LX.WINDOW + 37, 512), 1e-6, 4, LX.narrow_u32, (1 << 32) // (512 * 4) + 1),
            (LX.COLSUM_TALL, 1e-5, 4, LX.narrow_u32, (1 << 32) // (1028 * 4) + 1),
            ((LX.DIAG_B32[0] * LX.DIAG_B32[1], LX.DIAG_B32[2]), 2e-5, 4, LX.narrow_u32, (1 << 32) // (512 * 4) + 1)):
        per = torch.randn(LX.PERIOD, cols, generator=g)
        rows = rows_past(LX.windows(n_rows, cols * 4), first)
        assert len(rows) >= 128
        diff = (LX.mutant_periodic_rows(per, rows, narrow=narrow, unit=unit).double() - LX.periodic_rows(per, rows).double()).abs()
        assert beyond(float(diff.amax(1).min()), bar), (n_rows, cols)


def test_flat_windows_tell_a_narrowed_element_offset():
    """The optimizer's chunk offset (chunk * 4096 as `int` bytes or elements) at B31 / B32 of its 2^30 + 4099 element entry."""
    n = LX.OPTIM_NUMEL[0]
    per = torch.randn(LX.PERIOD, 1, generator=torch.Generator().manual_seed(19))
    for narrow, first in ((LX.narrow_i32, 1 << 29), (LX.narrow_u32, 1 << 30)):
        e = rows_past(LX.windows(n, 4, LX.FLAT_WINDOW), first)
        assert len(e) >= 4096
        wrong = LX.mutant_periodic_rows(per, e, cols=1, narrow=narrow, unit=4)
        diff = (wrong - LX.periodic_rows(per, e)).abs()
        assert beyond(float(diff.mean()), 1e-3)
