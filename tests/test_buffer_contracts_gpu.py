"""Every entry point against the buffers it was given (tests/redzone_common.py): exactly-sized, 256-byte aligned buffers
carved out of one allocation, with 64 KiB sentinel red zones around each, workspaces and partials of exactly the bytes the
`*_bytes()` functions return.  Each case runs under both sentinel fills and asserts

  * Arena.check(): no byte outside the writable buffers changed (red zones and inputs), row padding of strided outputs
    intact, no output element left unwritten;
  * outputs bit-equal between the NaN fill and the large-finite fill: nothing depends on memory outside the contract or on
    what the workspace held before;
  * outputs bit-equal to the same call through the lamp_amd/_native.py wrapper where one exists for the same layout;
  * outputs within the bar that op already has against fp64 torch (tests/test_gpu_parity.py, test_gpu_backward.py,
    test_gpu_training.py, test_onehot_gpu.py, test_train_gpu.py, attn_routes_common.py) -- no new tolerances.  Of the
    whole-forward variants only 'default' and 'onehot' are held against the fp64 oracle here; the others (live encoder,
    sigmoid decoder, bf16x3, label bias, enc_mask, no packs) are compared with LAMP.forward bit for bit, and their own files
    hold that against fp64 -- one option at a time; tests/test_combo_gpu.py holds their combinations against fp64.

Every overrun these tests can see lands in memory the arena owns.

Weights of the whole-forward cases stay in the module's own tensors (the lamp_model struct of lamp_amd/Models.py is reused);
tokens, logits, enc_output, every aux output, the enc_mask and the workspace are in the arena."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import redzone_common as RZ
from conftest import max_abs_diff
from oracle import lamp_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def N():
    from lamp_amd import _native
    _native.lib()
    return _native


def p(t):
    return None if t is None else t.data_ptr()


def ok(rc, what):
    assert rc == 0, '%s returned %d' % (what, rc)


def rnd(seed):
    return torch.Generator().manual_seed(seed)


def run_both(dev, body, capacity=32 << 20, unordered=()):
    """body(arena) -> {name: tensor view}.  Runs it under both fills, checks the arena, -> the (fill-independent) outputs.
    unordered: outputs summed by atomic adds, whose last bits are documented to vary from run to run."""
    got = []
    for fill in RZ.FILLS:
        ar = RZ.Arena(dev, fill, capacity)
        outs = body(ar)
        ar.check()
        got.append(dict((k, v.clone()) for k, v in outs.items()))
    for k in got[0]:
        if k not in unordered:
            assert RZ.bit_equal(got[0][k], got[1][k]), 'output %r depends on the sentinel fill' % k
    return got[0]


def same_bits(got, want, what):
    assert RZ.bit_equal(got.contiguous(), want.contiguous().view(got.shape)), '%s: not the bits of the wrapper route' % what


# ------------------------------------------------------------------ lamp_linear_fwd
@pytest.mark.parametrize('pad', [True, False])
@pytest.mark.parametrize('full', [True, False])
@pytest.mark.parametrize('M,K,N_', [(67, 72, 130), (1, 4, 1), (513, 64, 70)])
def test_linear_fwd(dev, N, M, K, N_, full, pad):
    g = rnd(M * 7 + K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N_, K, generator=g) / K ** 0.5
    b, r = torch.randn(N_, generator=g), torch.randn(M, N_, generator=g)
    lda, ldw, ldc, ldr = (K + 4, K + 8, N_ + 3, N_ + 5) if pad else (K, K, N_, N_)

    def body(ar):
        A, W = ar.inp(x, 'A', ld=lda), ar.inp(w, 'W', ld=ldw)
        bias = ar.inp(b, 'bias') if full else None
        res = ar.inp(r, 'residual', ld=ldr) if full else None
        Cv = ar.out((M, N_), 'C', ld=ldc)
        ok(N.lib().lamp_linear_fwd(p(A), M, K, lda, p(W), N_, ldw, p(bias), p(res), ldr, int(full), p(Cv), ldc, N.stream()),
           'lamp_linear_fwd')
        return {'C': Cv}
    got = run_both(dev, body)
    ref = x.double() @ w.double().t()
    if full:
        ref = (ref + b.double()).clamp_min(0) + r.double()
    assert max_abs_diff(got['C'], ref) < 2e-5
    if not pad:
        want = N.linear(x.to(dev), w.to(dev), b.to(dev) if full else None, residual=r.to(dev) if full else None, relu=full)
        same_bits(got['C'], want, 'lamp_linear_fwd')


# ------------------------------------------------------------------ lamp_gemm
def operand(ar, data, transposed, pad, name):
    """data (rows, k) -> (arena view of the stored matrix, row stride, col stride): k-contiguous rows `ld` apart, or stored
    transposed (k, rows) so that the rows index is the contiguous one."""
    rows, k = data.shape
    if transposed:
        ld = rows + pad
        return ar.inp(data.t().contiguous(), name, ld=ld), 1, ld
    ld = k + pad
    return ar.inp(data, name, ld=ld), ld, 1


def gemm_call(N, ar, A, ars, acs, Bm, brs, bcs, Cv, M, Nn, K, ldc, ws_bytes='exact', accumulate=False, alpha=1.0, mask=None,
              ld_mask=0, batch=(1, 1), a_b=(0, 0), b_b=(0, 0), c_b=(0, 0)):
    L = N.lib()
    need = L.lamp_gemm_workspace_bytes(M, Nn, K, batch[0] * batch[1])
    nbytes = {'exact': need, 'short': max(need - 1, 0), 'null': 0}[ws_bytes]
    ws = ar.scratch(nbytes, 'workspace') if ws_bytes != 'null' else None
    d = N.GemmDesc(p(A), p(Bm), p(Cv), M, Nn, K, batch[0], batch[1], int(accumulate), ars, acs, a_b[0], a_b[1],
                   brs, bcs, b_b[0], b_b[1], ldc, c_b[0], c_b[1], p(mask), ld_mask, float(alpha), 0)
    ok(L.lamp_gemm(C.byref(d), p(ws) if nbytes else None, nbytes, N.stream()), 'lamp_gemm')
    return need


@pytest.mark.parametrize('pad', [3, 0])
@pytest.mark.parametrize('ta', [False, True])
@pytest.mark.parametrize('tb', [False, True])
@pytest.mark.parametrize('M,Nn,K', [(67, 130, 72), (5, 129, 1030)])
def test_gemm_operand_forms(dev, N, M, Nn, K, ta, tb, pad):
    g = rnd(M * 7 + Nn * 3 + K + ta * 2 + tb)
    a, b = torch.randn(M, K, generator=g), torch.randn(Nn, K, generator=g)
    ldc = Nn + pad

    def body(ar):
        A, ars, acs = operand(ar, a, ta, pad, 'A')
        Bm, brs, bcs = operand(ar, b, tb, pad, 'B')
        Cv = ar.out((M, Nn), 'C', ld=ldc)
        gemm_call(N, ar, A, ars, acs, Bm, brs, bcs, Cv, M, Nn, K, ldc)
        return {'C': Cv}
    got = run_both(dev, body)
    assert max_abs_diff(got['C'], a.double() @ b.double().t()) < 3e-5 * max(1.0, K ** 0.5)
    if not pad:
        ad = a.t().contiguous().to(dev).t() if ta else a.to(dev)
        bd = b.t().contiguous().to(dev).t() if tb else b.to(dev)
        same_bits(got['C'], N.matmul_nt(ad, bd), 'lamp_gemm')


@pytest.mark.parametrize('pad', [4, 0])
@pytest.mark.parametrize('M,Nn,K,tol', [(130, 96, 70, 1e-4), (64, 64, 4096, 2e-3)])
def test_gemm_relu_mask_accumulate_alpha_strided(dev, N, M, Nn, K, tol, pad):
    """ldc > N and ld_mask > N, accumulate into C, alpha, the ReLU mask -- direct and through the split-K reduction."""
    g = rnd(11 + K)
    deep = K >= 1024                                    # the weight-gradient form: both operands stored [K, rows]
    a, b = torch.randn(M, K, generator=g), torch.randn(Nn, K, generator=g)
    h, c0 = torch.randn(M, Nn, generator=g), torch.randn(M, Nn, generator=g)
    alpha = 2.0 if deep else 0.25
    ldc, ldm = Nn + pad, Nn + 2 * pad

    def body(ar):
        A, ars, acs = operand(ar, a, deep, 0, 'A')
        Bm, brs, bcs = operand(ar, b, True, 0, 'B')
        mask = ar.inp(h, 'relu_mask', ld=ldm)
        Cv = ar.inout(c0, 'C', ld=ldc)
        need = gemm_call(N, ar, A, ars, acs, Bm, brs, bcs, Cv, M, Nn, K, ldc, accumulate=True, alpha=alpha, mask=mask, ld_mask=ldm)
        assert (need > 0) == deep
        return {'C': Cv}
    got = run_both(dev, body)
    ref = (a.double() @ b.double().t()) * alpha * (h.double() > 0) + c0.double()
    assert max_abs_diff(got['C'], ref) < tol
    if not pad:
        out = c0.clone().to(dev)
        ad = a.t().contiguous().to(dev).t() if deep else a.to(dev)
        N.matmul_nt(ad, b.t().contiguous().to(dev).t(), out=out, alpha=alpha, accumulate=True, relu_mask=h.to(dev))
        same_bits(got['C'], out, 'lamp_gemm with relu mask')


def test_gemm_batched_head_views(dev, N):
    """A 2 x 3 batch (head, sample) over head-split views of fused [B, l, H*d] buffers: S = Q K^T into (H*B, lq, lk) maps, and
    dK = S^T Q written back INTO a head-split view, where a wrong head stride lands in a neighbour head's columns."""
    g = rnd(9)
    B, H, lq, lk, dk = 3, 2, 37, 23, 16
    q, k = torch.randn(B, lq, H * dk, generator=g), torch.randn(B, lk, H * dk, generator=g)
    s = torch.randn(H * B, lq, lk, generator=g)

    def body(ar):
        Q, Kt, S = ar.inp(q, 'q'), ar.inp(k, 'k'), ar.inp(s, 'S')
        out_s = ar.out((H * B, lq, lk), 'scores')
        gemm_call(N, ar, Q, H * dk, 1, Kt, H * dk, 1, out_s, lq, lk, dk, lk, alpha=0.5, batch=(H, B), a_b=(dk, lq * H * dk),
                  b_b=(dk, lk * H * dk), c_b=(B * lq * lk, lq * lk))
        out_k = ar.out((B, lk, H * dk), 'dk')
        gemm_call(N, ar, S, 1, lk, Q, 1, H * dk, out_k, lk, dk, lq, H * dk, batch=(H, B), a_b=(B * lq * lk, lq * lk),
                  b_b=(dk, lq * H * dk), c_b=(dk, lk * H * dk))
        return {'scores': out_s, 'dk': out_k}
    got = run_both(dev, body)
    qh = q.double().view(B, lq, H, dk).permute(2, 0, 1, 3)
    kh = k.double().view(B, lk, H, dk).permute(2, 0, 1, 3)
    s4 = s.double().view(H, B, lq, lk)
    assert max_abs_diff(got['scores'].view(H, B, lq, lk), 0.5 * qh @ kh.transpose(-1, -2)) < 1e-4
    ref_dk = (s4.transpose(-1, -2) @ qh).permute(1, 2, 0, 3).reshape(B, lk, H * dk)
    assert max_abs_diff(got['dk'], ref_dk) < 1e-4
    qd, kd, sd = q.to(dev), k.to(dev), s.to(dev)
    qv, kv = qd.view(B, lq, H, dk).permute(2, 0, 1, 3), kd.view(B, lk, H, dk).permute(2, 0, 1, 3)
    same_bits(got['scores'], N.matmul_nt(qv, kv, alpha=0.5), 'batched scores')
    buf = torch.zeros(B, lk, H * dk, device=dev)
    N.matmul_nt(sd.view(H, B, lq, lk).transpose(-1, -2), qv.transpose(-1, -2), out=buf.view(B, lk, H, dk).permute(2, 0, 1, 3))
    same_bits(got['dk'], buf, 'batched dK into a head-split view')


@pytest.mark.parametrize('ws_bytes', ['exact', 'short', 'null'])
@pytest.mark.parametrize('M,Nn,K', [(64, 64, 4096), (130, 96, 2048)])
def test_gemm_split_k_with_exact_short_and_no_workspace(dev, N, M, Nn, K, ws_bytes):
    """The weight-gradient form.  exact: lamp_gemm_workspace_bytes() and not a byte more.  short: one byte less -- the launcher
    clamps the split count to what fits (by design), the result stays correct and nothing leaves the buffer.  null: no split,
    the bits of the unsplit launch lamp_gemm_grouped promises."""
    from test_gpu_backward import _gemm_one_launch_no_split
    g = rnd(5 + K)
    dy, x = torch.randn(K, M, generator=g), torch.randn(K, Nn, generator=g)

    def body(ar):
        A, Bm = ar.inp(dy, 'dy'), ar.inp(x, 'x')
        Cv = ar.out((M, Nn), 'dW')
        need = gemm_call(N, ar, A, 1, M, Bm, 1, Nn, Cv, M, Nn, K, Nn, ws_bytes=ws_bytes)
        assert need >= 2 * M * Nn * 4
        return {'dW': Cv}
    got = run_both(dev, body)
    assert max_abs_diff(got['dW'], dy.double().t() @ x.double()) < 3e-5 * K ** 0.5
    if ws_bytes == 'exact':
        same_bits(got['dW'], N.matmul_nt(dy.to(dev).t(), x.to(dev).t()), 'split-K lamp_gemm')
    if ws_bytes == 'null':
        same_bits(got['dW'], _gemm_one_launch_no_split(N, dy.to(dev).t(), x.to(dev).t()), 'unsplit lamp_gemm')


def test_gemm_grouped(dev, N):
    """Three products of mixed K in one launch, the middle one accumulating; each the bits of its own unsplit launch."""
    from test_gpu_backward import _gemm_one_launch_no_split
    g = rnd(13)
    shapes = [(70, 130, 1000), (5, 129, 1030), (64, 64, 16)]
    ops = [(torch.randn(K, M, generator=g), torch.randn(K, Nn, generator=g)) for M, Nn, K in shapes]
    c1 = torch.randn(5, 129, generator=g)

    def body(ar):
        descs, outs = (N.GemmDesc * 3)(), {}
        for i, ((M, Nn, K), (a, b)) in enumerate(zip(shapes, ops)):
            A, Bm = ar.inp(a, 'A%d' % i), ar.inp(b, 'B%d' % i)
            Cv = ar.inout(c1, 'C1') if i == 1 else ar.out((M, Nn), 'C%d' % i)
            descs[i] = N.GemmDesc(p(A), p(Bm), p(Cv), M, Nn, K, 1, 1, int(i == 1), 1, M, 0, 0, 1, Nn, 0, 0, Nn, 0, 0, None, 0,
                                  1.0, 0)
            outs['C%d' % i] = Cv
        ok(N.lib().lamp_gemm_grouped(descs, 3, N.stream()), 'lamp_gemm_grouped')
        return outs
    got = run_both(dev, body)
    for i, ((M, Nn, K), (a, b)) in enumerate(zip(shapes, ops)):
        ref = a.double().t() @ b.double() + (c1.double() if i == 1 else 0)
        assert max_abs_diff(got['C%d' % i], ref) < 3e-5 * max(1.0, K ** 0.5) * 4
        want = _gemm_one_launch_no_split(N, a.to(dev).t(), b.to(dev).t(), accumulate_into=c1.clone().to(dev) if i == 1 else None)
        same_bits(got['C%d' % i], want, 'lamp_gemm_grouped problem %d' % i)


# ------------------------------------------------------------------ lamp_reduce_partials_grouped
def test_reduce_partials_grouped_against_fp64(dev, N):
    """Two jobs over five partial rows: n_total = 3 n_seg (three outputs) and 2 n_seg (two; out[2] NULL)."""
    g = rnd(17)
    rows, segs = 5, (36, 130)
    parts = [torch.randn(rows, 3 * segs[0], generator=g), torch.randn(rows, 2 * segs[1], generator=g)]

    def body(ar):
        jobs, outs = (N.ReduceJob * 2)(), {}
        for j, (part, seg) in enumerate(zip(parts, segs)):
            P = ar.inp(part, 'partial%d' % j)
            o = [ar.out((seg,), 'out%d_%d' % (j, i)) for i in range(part.size(1) // seg)]
            for i, t in enumerate(o):
                outs['out%d_%d' % (j, i)] = t
            jobs[j] = N.ReduceJob(p(P), part.size(1), seg, (C.c_void_p * 3)(*([p(t) for t in o] + [None] * (3 - len(o)))), rows, 0)
        ok(N.lib().lamp_reduce_partials_grouped(jobs, 2, N.stream()), 'lamp_reduce_partials_grouped')
        return outs
    got = run_both(dev, body)
    assert len(got) == 5
    for j, (part, seg) in enumerate(zip(parts, segs)):
        total = part.double().sum(0)
        for i in range(part.size(1) // seg):
            assert max_abs_diff(got['out%d_%d' % (j, i)], total[i * seg:(i + 1) * seg]) < 1e-5 * max(1.0, rows ** 0.5) * 4


# ------------------------------------------------------------------ layer norm
LN_SHAPES = [(5, 36, 0), (37, 2048, 0), (1025, 512, 41)]


def ln_inputs(M, d, r_rows):
    g = rnd(M + d)
    x, res = torch.randn(M, d, generator=g), torch.randn(r_rows or M, d, generator=g)
    gamma, beta, dy = 1 + 0.3 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g), torch.randn(M, d, generator=g)
    return x, res, gamma, beta, dy


def ln_reference(N, x, res, gamma, beta, dy, r_rows, pdrop, seed):
    M, d = x.shape
    xd, rd = x.double().requires_grad_(), res.double().requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    keep = N.dropout_keep_mask(M * d, pdrop, seed).view(M, d) if pdrop else 1.0
    z = xd * keep / (1 - pdrop) + (rd.repeat(M // r_rows, 1) if r_rows else rd)
    z.retain_grad()                           # dz: the gradient of z row by row, also where the residual is broadcast
    y = F.layer_norm(z, (d,), gd, bd, 1e-5)
    y.backward(dy.double())
    return y.detach(), xd.grad, z.grad, gd.grad, bd.grad


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('M,d,_r', LN_SHAPES)
def test_layernorm_fwd(dev, N, M, d, _r, in_place):
    x, _, gamma, beta, _ = ln_inputs(M, d, 0)

    def body(ar):
        G, Bt = ar.inp(gamma, 'gamma'), ar.inp(beta, 'beta')
        X = ar.inout(x, 'x=y') if in_place else ar.inp(x, 'x')
        Y = X if in_place else ar.out((M, d), 'y')
        ok(N.lib().lamp_layernorm_fwd(p(X), M, d, p(G), p(Bt), 1e-5, p(Y), N.stream()), 'lamp_layernorm_fwd')
        return {'y': Y}
    got = run_both(dev, body)
    assert max_abs_diff(got['y'], F.layer_norm(x.double(), (d,), gamma.double(), beta.double(), 1e-5)) < 2e-5
    same_bits(got['y'], N.layernorm(x.to(dev), gamma.to(dev), beta.to(dev)), 'lamp_layernorm_fwd')


@pytest.mark.parametrize('pdrop', [0.0, 0.3])
@pytest.mark.parametrize('M,d,r_rows', LN_SHAPES)
def test_layernorm_residual_fwd_and_bwd(dev, N, M, d, r_rows, pdrop):
    """Forward, and the backward with dbias and a workspace of exactly lamp_layernorm_bwd_workspace_bytes().  p = 0: dx is
    documented as not written (the gradient of x is dz) -- it is passed NULL."""
    x, res, gamma, beta, dy = ln_inputs(M, d, r_rows)
    seed = 77
    L = N.lib()

    def body(ar):
        X, Rs, G, Bt, DY = (ar.inp(t, n) for t, n in ((x, 'x'), (res, 'residual'), (gamma, 'gamma'), (beta, 'beta'), (dy, 'dy')))
        Y = ar.out((M, d), 'y')
        ok(L.lamp_layernorm_residual_fwd(p(X), p(Rs), r_rows, M, d, p(G), p(Bt), 1e-5, pdrop, seed, p(Y), N.stream()),
           'lamp_layernorm_residual_fwd')
        dz, dx = ar.out((M, d), 'dz'), (ar.out((M, d), 'dx') if pdrop else None)
        dg, db, dbias = ar.out((d,), 'dgamma'), ar.out((d,), 'dbeta'), ar.out((d,), 'dbias')
        nb = L.lamp_layernorm_bwd_workspace_bytes(M, d)
        ws = ar.scratch(nb, 'workspace')
        ok(L.lamp_layernorm_bwd(p(X), p(Rs), r_rows, M, d, p(G), 1e-5, pdrop, seed, p(DY), p(dz), p(dx), p(dg), p(db), p(dbias),
                                p(ws), nb, N.stream()), 'lamp_layernorm_bwd')
        outs = {'y': Y, 'dz': dz, 'dgamma': dg, 'dbeta': db, 'dbias': dbias}
        if pdrop:
            outs['dx'] = dx
        return outs
    got = run_both(dev, body)
    y_ref, dx_ref, dz_ref, dg_ref, db_ref = ln_reference(N, x, res, gamma, beta, dy, r_rows, pdrop, seed)
    bar = 1e-4 * max(1.0, (M / 100) ** 0.5)
    assert max_abs_diff(got['y'], y_ref) < (3e-5 if pdrop else 2e-5)
    assert max_abs_diff(got['dx'] if pdrop else got['dz'], dx_ref) < (5e-5 if pdrop else 3e-5)
    assert max_abs_diff(got['dz'], dz_ref) < (5e-5 if pdrop else 3e-5)
    assert max_abs_diff(got['dgamma'], dg_ref) < bar and max_abs_diff(got['dbeta'], db_ref) < bar
    assert max_abs_diff(got['dbias'], dx_ref.sum(0)) < bar
    xd, rd, gd, bd, dyd = (t.to(dev) for t in (x, res, gamma, beta, dy))
    same_bits(got['y'], N.layernorm_residual(xd, rd, gd, bd, dropout_p=pdrop, seed=seed), 'lamp_layernorm_residual_fwd')
    wdz, wdx, wdg, wdb, wdbias = N.layernorm_bwd(xd, rd, gd, dyd, dropout_p=pdrop, seed=seed, want_dbias=True)
    for name, want in (('dz', wdz), ('dgamma', wdg), ('dbeta', wdb), ('dbias', wdbias)) + ((('dx', wdx),) if pdrop else ()):
        same_bits(got[name], want, 'lamp_layernorm_bwd ' + name)


# ------------------------------------------------------------------ colsum, dropout, softmax / sigmoid backward
@pytest.mark.parametrize('M,Nn,ldx', [(129, 257, 260), (129, 257, 257), (4100, 36, 36)])
def test_colsum(dev, N, M, Nn, ldx):
    x = torch.randn(M, Nn, generator=rnd(M + Nn))
    L = N.lib()

    def body(ar):
        X, out = ar.inp(x, 'x', ld=ldx), ar.out((Nn,), 'out')
        nb = L.lamp_colsum_workspace_bytes(M, Nn)
        ws = ar.scratch(nb, 'workspace')
        ok(L.lamp_colsum(p(X), M, Nn, ldx, p(out), p(ws), nb, N.stream()), 'lamp_colsum')
        return {'out': out}
    got = run_both(dev, body)
    assert max_abs_diff(got['out'], x.double().sum(0)) < 1e-5 * max(1.0, M ** 0.5) * 4
    if ldx == Nn:
        same_bits(got['out'], N.colsum(x.to(dev)), 'lamp_colsum')


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('n', [1, 1023, 1025])
def test_dropout(dev, N, n, in_place):
    x = torch.randn(n, generator=rnd(n))
    pdrop, seed = 0.1, 1234

    def body(ar):
        X = ar.inout(x, 'x=y') if in_place else ar.inp(x, 'x')
        Y = X if in_place else ar.out((n,), 'y')
        ok(N.lib().lamp_dropout(p(X), n, pdrop, seed, p(Y), N.stream()), 'lamp_dropout')
        return {'y': Y}
    got = run_both(dev, body)
    xd = x.to(dev)
    keep = N.dropout_keep_mask(n, pdrop, seed).to(dev)
    assert torch.equal(got['y'], torch.where(keep, xd * (1.0 / (1.0 - pdrop)), torch.zeros_like(xd)))
    same_bits(got['y'], N.dropout(xd, pdrop, seed), 'lamp_dropout')


@pytest.mark.parametrize('alias', [False, True])
@pytest.mark.parametrize('rows,lk', [(3, 5), (77, 90)])
def test_softmax_bwd_and_sigmoid_attn_bwd(dev, N, rows, lk, alias):
    g = rnd(rows + lk)
    s = torch.randn(rows, lk, generator=g).double()
    blocked = torch.rand(rows, lk, generator=g) < 0.3
    blocked[:, 0] = False
    s = s.masked_fill(blocked, float('-inf')).requires_grad_()
    P = torch.softmax(s * 0.25, -1)
    dP = torch.randn(rows, lk, generator=g)
    P.backward(dP.double())
    P32 = P.detach().float()
    Ps = torch.sigmoid(s.detach() * 0.25).float()       # blocked entries: sigmoid(-inf) = 0

    def body(ar):
        outs = {}
        for name, Pm in (('softmax', P32), ('sigmoid', Ps)):
            Pv = ar.inp(Pm, 'P_' + name)
            G = ar.inout(dP, 'dP=dS_' + name) if alias else ar.inp(dP, 'dP_' + name)
            dS = G if alias else ar.out((rows, lk), 'dS_' + name)
            if name == 'softmax':
                ok(N.lib().lamp_softmax_bwd(p(Pv), p(G), rows, lk, 0.25, p(dS), N.stream()), 'lamp_softmax_bwd')
            else:
                ok(N.lib().lamp_sigmoid_attn_bwd(p(Pv), p(G), rows, lk, 0.25, 0.0, 0, p(dS), N.stream()), 'lamp_sigmoid_attn_bwd')
            outs[name] = dS
        return outs
    got = run_both(dev, body)
    assert max_abs_diff(got['softmax'], s.grad) < 1e-5
    assert (got['softmax'].cpu()[blocked] == 0).all() and (got['sigmoid'].cpu()[blocked] == 0).all()
    assert max_abs_diff(got['sigmoid'], 0.25 * Ps.double() * (1 - Ps.double()) * dP.double()) < 1e-5
    same_bits(got['softmax'], N.softmax_bwd(P32.to(dev), dP.to(dev), 0.25), 'lamp_softmax_bwd')
    same_bits(got['sigmoid'], N.sigmoid_attn_bwd(Ps.to(dev), dP.to(dev), 0.25), 'lamp_sigmoid_attn_bwd')


# ------------------------------------------------------------------ embedding, read-out, loss
def test_embed_fwd_and_bwd_with_pad_rows(dev, N):
    g = rnd(8)
    B, T, d, V, n_pos = 5, 23, 36, 50, 24
    seq = torch.randint(1, V, (B, T), generator=g)
    seq[:, -4:] = 0
    seq[2, 7] = 0                                       # a PAD inside a sequence
    pos = torch.arange(1, T + 1).repeat(B, 1) * (seq != 0)
    emb, ptab = torch.randn(V, d, generator=g), torch.randn(n_pos, d, generator=g)
    dout, base = torch.randn(B, T, d, generator=g), torch.randn(V, d, generator=g)
    L = N.lib()

    def body(ar):
        S, Pp, E, Pt, D = ar.inp(seq, 'src_seq'), ar.inp(pos, 'src_pos'), ar.inp(emb, 'emb'), ar.inp(ptab, 'pos'), ar.inp(dout, 'dout')
        out = ar.out((B, T, d), 'out')
        ok(L.lamp_embed_fwd(p(S), p(Pp), B * T, p(E), V, p(Pt), n_pos, d, p(out), N.stream()), 'lamp_embed_fwd')
        acc, ordered = ar.inout(base, 'd_emb'), ar.inout(base, 'd_emb_ordered')
        ok(L.lamp_embed_bwd(p(S), B * T, p(D), d, V, 0, p(acc), N.stream()), 'lamp_embed_bwd')
        ok(L.lamp_embed_bwd_ordered(p(S), B * T, p(D), d, V, 0, p(ordered), N.stream()), 'lamp_embed_bwd_ordered')
        return {'out': out, 'ordered': ordered, 'atomic': acc}
    got = run_both(dev, body, unordered=('atomic',))      # lamp_embed_bwd: atomic adds, the order of a repeated token's rows is not fixed
    assert max_abs_diff(got['out'], emb[seq].double() + ptab[pos].double()) < 1e-6
    same_bits(got['out'], N.embed(seq.to(dev), pos.to(dev), emb.to(dev), ptab.to(dev)), 'lamp_embed_fwd')
    ref = torch.nn.Embedding(V, d, padding_idx=0).double()
    ref(seq).backward(dout.double())
    want = base.double() + ref.weight.grad
    assert max_abs_diff(got['atomic'], want) < 1e-4 and max_abs_diff(got['ordered'], want) < 1e-4
    assert torch.equal(got['ordered'][0].cpu(), base[0]) and torch.equal(got['atomic'][0].cpu(), base[0])   # the PAD row: untouched


def test_diag_logits_fwd_bwd_and_sigmoid_bce(dev, N):
    g = rnd(21)
    B, Lb, d = 5, 37, 36
    y, w, dl = torch.randn(B, Lb, d, generator=g), torch.randn(Lb, d, generator=g), torch.randn(B, Lb, generator=g)
    z = (torch.rand(B, Lb, generator=g) < 0.3).float()
    L = N.lib()

    def body(ar):
        Y, W, DL, Z = ar.inp(y, 'y'), ar.inp(w, 'w_out'), ar.inp(dl, 'dlogits'), ar.inp(z, 'targets')
        logits = ar.out((B, Lb), 'logits')
        ok(L.lamp_diag_logits_fwd(p(Y), p(W), B, Lb, d, p(logits), N.stream()), 'lamp_diag_logits_fwd')
        dy, dw = ar.out((B, Lb, d), 'dy'), ar.out((Lb, d), 'dw')
        ok(L.lamp_diag_logits_bwd(p(Y), p(W), p(DL), B, Lb, d, p(dy), p(dw), N.stream()), 'lamp_diag_logits_bwd')
        probs, loss = ar.out((B, Lb), 'probs'), ar.out((B,), 'row_loss')
        ok(L.lamp_sigmoid_bce_fwd(p(DL), p(Z), B, Lb, p(probs), p(loss), N.stream()), 'lamp_sigmoid_bce_fwd')
        return {'logits': logits, 'dy': dy, 'dw': dw, 'probs': probs, 'row_loss': loss}
    got = run_both(dev, body)
    yd, wd = y.double().requires_grad_(), w.double().requires_grad_()
    ref = (yd * wd.unsqueeze(0)).sum(-1)
    ref.backward(dl.double())
    assert max_abs_diff(got['logits'], ref.detach()) < 2e-5
    assert max_abs_diff(got['dy'], yd.grad) < 1e-5 and max_abs_diff(got['dw'], wd.grad) < 1e-5
    assert max_abs_diff(got['probs'], torch.sigmoid(dl.double())) < 1e-6
    ref_loss = F.binary_cross_entropy_with_logits(dl.double(), z.double(), reduction='none').sum(1)
    assert max_abs_diff(got['row_loss'], ref_loss) < 1e-4
    same_bits(got['logits'], N.diag_logits(y.to(dev), w.to(dev)), 'lamp_diag_logits_fwd')
    wdy, wdw = N.diag_logits_bwd(y.to(dev), w.to(dev), dl.to(dev))
    same_bits(got['dy'], wdy, 'lamp_diag_logits_bwd dy')
    same_bits(got['dw'], wdw, 'lamp_diag_logits_bwd dw')
    wp, wl = N.sigmoid_bce(dl.to(dev), z.to(dev))
    same_bits(got['probs'], wp, 'lamp_sigmoid_bce_fwd probs')
    same_bits(got['row_loss'], wl, 'lamp_sigmoid_bce_fwd row_loss')


# ------------------------------------------------------------------ eval sub-layers: lamp_mha_fwd, lamp_mha_act_fwd, lamp_ffn_fwd
def sublayer_weights(d, dff, H, dk, g, dv=None):
    dv = dk if dv is None else dv
    w = dict(wq=torch.randn(H * dk, d, generator=g) * 0.2, wk=torch.randn(H * dk, d, generator=g) * 0.2,
             wv=torch.randn(H * dv, d, generator=g) * 0.2, fc=torch.randn(d, H * dv, generator=g) * 0.2 if H > 1 else None,
             ln_g=1 + 0.1 * torch.randn(d, generator=g), ln_b=0.1 * torch.randn(d, generator=g),
             w1=torch.randn(dff, d, generator=g) * 0.1, b1=torch.randn(dff, generator=g) * 0.1,
             w2=torch.randn(d, dff, generator=g) * 0.1, b2=torch.randn(d, generator=g) * 0.1)
    return w


def arena_mha_weights(N, ar, w, H):
    t = dict((k, ar.inp(w[k], k)) for k in ('wq', 'wk', 'wv', 'ln_g', 'ln_b'))
    fc = ar.inp(w['fc'], 'fc') if w['fc'] is not None else None
    return N.MhaWeights(p(t['wq']), p(t['wk']), p(t['wv']), p(fc), p(t['ln_g']), p(t['ln_b']), H, 1)


def arena_ffn_weights(N, ar, w):
    t = dict((k, ar.inp(w[k], k)) for k in ('w1', 'b1', 'w2', 'b2', 'ln_g', 'ln_b'))
    return N.FfnWeights(p(t['w1']), p(t['b1']), p(t['w2']), p(t['b2']), p(t['ln_g']), p(t['ln_b']))


class _Mod(object):   # what _native.mha_weights / ffn_weights read off a module
    pass


def torch_mha_weights(N, w, H, dev):
    keep = dict((k, v.to(dev)) for k, v in w.items() if v is not None)
    return N.MhaWeights(p(keep['wq']), p(keep['wk']), p(keep['wv']), p(keep.get('fc')), p(keep['ln_g']), p(keep['ln_b']), H, 1), keep


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('self_attn', [False, True])
@pytest.mark.parametrize('H,d,dk,dv', [(4, 64, 16, 16), (1, 16, 16, 16), (3, 64, 24, 40), (1, 64, 48, 64), (2, 64, 160, 32)],
                         ids=['4', '1', '3-d64-dk24-dv40', '1-d64-dk48-dv64', '2-d64-dk160-dv32'])
def test_mha_fwd_exact_workspace(dev, N, H, d, dk, dv, self_attn, act):
    """lamp_mha_fwd / lamp_mha_act_fwd with a workspace of exactly lamp_mha_workspace_bytes(), maps requested, and xkv
    aliasing xq (self-attention: one buffer is query, key and value source).  Beside d_k = d_v = d_model / n_head: n_head * d_k
    != n_head * d_v != d_model (K and V are two launches), one head without fc at d_v = d_model != d_k, and d_k > 128 (the
    score scratch of the general route is part of the workspace)."""
    g = rnd(30 + H if dk == dv else 300 + H + dk + dv)
    B, lq, lk = 2, 37, 37 if self_attn else 23
    w = sublayer_weights(d, 96, H, dk, g, dv)
    xq, xkv = torch.randn(B, lq, d, generator=g), torch.randn(B, lk, d, generator=g)
    blocked = torch.rand(lq, lk, generator=g) < 0.3
    blocked[:, 0] = False
    L = N.lib()

    def body(ar):
        wts = arena_mha_weights(N, ar, w, H)
        XQ = ar.inp(xq, 'xq')
        XKV = XQ if self_attn else ar.inp(xkv, 'xkv')
        Mb = ar.inp(blocked.to(torch.uint8), 'mask')
        mask = N.Mask(N.LAMP_MASK_U8, 0, p(Mb), 0, lk, None, 0, 0)
        out, attn = ar.out((B, lq, d), 'out'), ar.out((H * B, lq, lk), 'attn')
        nb = L.lamp_mha_workspace_bytes(B, lq, lk, d, H, dk, dv)
        ws = ar.scratch(nb, 'workspace')
        if act:
            ok(L.lamp_mha_act_fwd(p(XQ), p(XKV), B, lq, lk, d, dk, dv, C.byref(wts), act, C.byref(mask), p(out), p(attn), p(ws),
                                  nb, N.stream()), 'lamp_mha_act_fwd')
        else:
            ok(L.lamp_mha_fwd(p(XQ), p(XKV), B, lq, lk, d, dk, dv, C.byref(wts), C.byref(mask), p(out), p(attn), p(ws), nb,
                              N.stream()), 'lamp_mha_fwd')
        return {'out': out, 'attn': attn}
    got = run_both(dev, body)
    src = xq if self_attn else xkv
    if act:
        import sigmoid_common
        saved, R.sdpa = R.sdpa, sigmoid_common.sigmoid_sdpa
    try:
        ref_out, ref_attn = R.mha(xq.double(), src.double(), blocked, w['wq'].double(), w['wk'].double(), w['wv'].double(),
                                  w['fc'].double() if H > 1 else None, w['ln_g'].double(), w['ln_b'].double(), H)
    finally:
        if act:
            R.sdpa = saved
    assert max_abs_diff(got['out'], ref_out) < 5e-5 and max_abs_diff(got['attn'], ref_attn) < 1e-5   # TOL_ACT, TOL_ATTN
    wts, keep = torch_mha_weights(N, w, H, dev)
    md = blocked.to(dev)
    mstruct, mkeep = N.make_mask(md, B, lq, lk)
    xqd = xq.to(dev)
    wout, wattn = N.mha(xqd, xqd if self_attn else xkv.to(dev), wts, dk, dv, mstruct, True, act=act)
    same_bits(got['out'], wout, 'lamp_mha_fwd out')
    same_bits(got['attn'], wattn, 'lamp_mha_fwd attn')


@pytest.mark.parametrize('in_place', [False, True])
def test_ffn_fwd_exact_workspace(dev, N, in_place):
    g = rnd(40)
    M, d, dff = 70, 64, 96
    w = sublayer_weights(d, dff, 4, 16, g)
    x = torch.randn(M, d, generator=g)
    L = N.lib()

    def body(ar):
        wts = arena_ffn_weights(N, ar, w)
        X = ar.inout(x, 'x=out') if in_place else ar.inp(x, 'x')
        out = X if in_place else ar.out((M, d), 'out')
        nb = L.lamp_ffn_workspace_bytes(M, d, dff)
        assert nb == M * dff * 4
        ws = ar.scratch(nb, 'workspace')
        ok(L.lamp_ffn_fwd(p(X), M, d, dff, C.byref(wts), p(out), p(ws), nb, N.stream()), 'lamp_ffn_fwd')
        return {'out': out}
    got = run_both(dev, body)
    ref = R.ffn(x.double(), w['w1'].double().unsqueeze(-1), w['b1'].double(), w['w2'].double().unsqueeze(-1), w['b2'].double(),
                w['ln_g'].double(), w['ln_b'].double())
    assert max_abs_diff(got['out'], ref) < 5e-5
    keep = dict((k, v.to(dev)) for k, v in w.items() if v is not None)
    wts = N.FfnWeights(p(keep['w1']), p(keep['b1']), p(keep['w2']), p(keep['b2']), p(keep['ln_g']), p(keep['ln_b']))
    same_bits(got['out'], N.ffn(x.to(dev), wts, dff), 'lamp_ffn_fwd')


# ------------------------------------------------------------------ training composites: lamp_ffn_train_fwd + lamp_ffn_bwd
def ffn_reference(N, x, w, dy, pdrop, seed):
    M, d = x.shape
    leaves = dict((k, w[k].double().requires_grad_()) for k in ('w1', 'b1', 'w2', 'b2', 'ln_g', 'ln_b'))
    X = x.double().requires_grad_()
    h = torch.relu(X @ leaves['w1'].t() + leaves['b1'])
    o = h @ leaves['w2'].t() + leaves['b2']
    keep = N.dropout_keep_mask(M * d, pdrop, seed).view(M, d) if pdrop else 1.0
    y = F.layer_norm(o * keep / (1 - pdrop) + X, (d,), leaves['ln_g'], leaves['ln_b'], 1e-5)
    y.backward(dy.double())
    return dict(h=h.detach(), o=o.detach(), y=y.detach(), dx=X.grad, dW1=leaves['w1'].grad, dW2=leaves['w2'].grad,
                db1=leaves['b1'].grad, db2=leaves['b2'].grad, dgamma=leaves['ln_g'].grad, dbeta=leaves['ln_b'].grad)


def ffn_arena_run(N, ar, x, w, dy, M, d, dff, pdrop, seed, defer):
    """lamp_ffn_train_fwd + lamp_ffn_bwd on arena buffers, exact workspace (and partials when defer) -> outputs."""
    L = N.lib()
    wts = arena_ffn_weights(N, ar, w)
    X, DY = ar.inp(x, 'x'), ar.inp(dy, 'dy')
    h, o, y = ar.out((M, dff), 'h'), ar.out((M, d), 'o'), ar.out((M, d), 'y')
    ok(L.lamp_ffn_train_fwd(p(X), M, d, dff, C.byref(wts), pdrop, seed, p(h), p(o), p(y), N.stream()), 'lamp_ffn_train_fwd')
    dx, d_o, dh = ar.out((M, d), 'dx'), (ar.out((M, d), 'd_o') if pdrop else None), ar.out((M, dff), 'dh')
    dW1, dW2 = ar.out((dff, d), 'dW1'), ar.out((d, dff), 'dW2')
    db1, db2, dg, db = ar.out((dff,), 'db1'), ar.out((d,), 'db2'), ar.out((d,), 'dgamma'), ar.out((d,), 'dbeta')
    nb = L.lamp_ffn_bwd_workspace_bytes(M, d, dff)
    ws = ar.scratch(nb, 'workspace')
    part, npb, jobs = None, 0, None
    if defer:
        npb = L.lamp_ffn_bwd_partials_bytes(M, d, dff)
        part, jobs = ar.scratch(npb, 'partials'), (N.ReduceJob * 2)()
    ok(L.lamp_ffn_bwd(p(X), p(h), p(o), p(DY), M, d, dff, C.byref(wts), pdrop, seed, p(dx), p(d_o), p(dh), p(dW1), p(dW2),
                      p(db1), p(db2), p(dg), p(db), p(ws) if nb else None, nb, p(part), npb, jobs, N.stream()), 'lamp_ffn_bwd')
    if defer:
        ok(L.lamp_reduce_partials_grouped(jobs, 2, N.stream()), 'lamp_reduce_partials_grouped')
    outs = dict(h=h, o=o, y=y, dx=dx, dh=dh, dW1=dW1, dW2=dW2, db1=db1, db2=db2, dgamma=dg, dbeta=db)
    if pdrop:
        outs['d_o'] = d_o
    return outs


def ffn_per_launch(N, x, w, dy, pdrop, seed, dev):
    """The per-launch route of lamp_amd/training.py (_FFNFn with COMPOSITE_CALLS off), launch by launch."""
    t = dict((k, v.to(dev)) for k, v in w.items() if v is not None)
    xd, dyd = x.to(dev), dy.to(dev)
    h = N.linear(xd, t['w1'], t['b1'], relu=True)
    o = N.linear(h, t['w2'], t['b2'])
    y = N.layernorm_residual(o, xd, t['ln_g'], t['ln_b'], dropout_p=pdrop, seed=seed)
    dz, do, dg, db, db2 = N.layernorm_bwd(o, xd, t['ln_g'], dyd, dropout_p=pdrop, seed=seed, want_dbias=True)
    dW2 = N.matmul_nt(do.t(), h.t())
    dh = N.matmul_nt(do, t['w2'].t(), relu_mask=h)
    db1 = N.colsum(dh)
    dW1 = N.matmul_nt(dh.t(), xd.t())
    d_o = do.clone()
    dx = N.matmul_nt(dh, t['w1'].t(), out=dz, accumulate=True)
    return dict(h=h, o=o, y=y, dx=dx, d_o=d_o, dh=dh, dW1=dW1, dW2=dW2, db1=db1, db2=db2, dgamma=dg, dbeta=db)


def check_ffn(got, ref, K=None):
    assert max_abs_diff(got['y'], ref['y']) < 2e-5 and max_abs_diff(got['h'], ref['h']) < 2e-5
    assert max_abs_diff(got['o'], ref['o']) < 2e-5
    for k in ('dx', 'dW1', 'dW2', 'db1', 'db2', 'dgamma', 'dbeta'):
        err, scale = max_abs_diff(got[k], ref[k]), ref[k].abs().max().item()
        print('ffn %-6s max|err| %.3e (scale %.3e)' % (k, err, scale))
        assert err <= 2e-4 * scale + 1e-9, k
        if K is not None and k in ('dW1', 'dW2'):
            assert err < 3e-5 * K ** 0.5, k


@pytest.mark.parametrize('defer', [False, True])
@pytest.mark.parametrize('pdrop', [0.0, 0.3])
def test_ffn_train_fwd_and_bwd(dev, N, pdrop, defer):
    g = rnd(50)
    M, d, dff, seed = 70, 64, 96, 4242
    w = sublayer_weights(d, dff, 4, 16, g)
    x, dy = torch.randn(M, d, generator=g), torch.randn(M, d, generator=g)
    got = run_both(dev, lambda ar: ffn_arena_run(N, ar, x, w, dy, M, d, dff, pdrop, seed, defer))
    check_ffn(got, ffn_reference(N, x, w, dy, pdrop, seed))
    want = ffn_per_launch(N, x, w, dy, pdrop, seed, dev)
    for k in got:     # deferred or not, arena or torch memory: the bits of the per-launch route
        same_bits(got[k], want[k], 'lamp_ffn_bwd ' + k)


@pytest.mark.parametrize('pdrop', [0.0, 0.1])
def test_ffn_bwd_weight_gradients_split_k_like_the_per_launch_route(dev, N, pdrop):
    """M = 1024, d_model = 64, d_inner = 1536: dW1 [1536, 64] and dW2 [64, 1536] over K = 1024 rows take a K split
    (1 572 864 bytes of partial sums), the square 1536 x 1536 product the size function used to be bounded by takes none
    (196 608 bytes came back).  With a workspace of exactly lamp_ffn_bwd_workspace_bytes() every output must have the bits
    of the per-launch route, where each lamp_gemm gets its own lamp_gemm_workspace_bytes()."""
    g = rnd(60)
    M, d, dff, seed = 1024, 64, 1536, 99
    w = sublayer_weights(d, dff, 4, 16, g)
    x, dy = torch.randn(M, d, generator=g), torch.randn(M, d, generator=g)
    L = N.lib()
    assert L.lamp_gemm_workspace_bytes(dff, d, M, 1) == 1572864 <= L.lamp_ffn_bwd_workspace_bytes(M, d, dff)
    got = run_both(dev, lambda ar: ffn_arena_run(N, ar, x, w, dy, M, d, dff, pdrop, seed, False), capacity=64 << 20)
    check_ffn(got, ffn_reference(N, x, w, dy, pdrop, seed), K=M)
    want = ffn_per_launch(N, x, w, dy, pdrop, seed, dev)
    wrapped = N.ffn_bwd(x.to(dev), want['h'], want['o'], dy.to(dev), w['w1'].to(dev), w['w2'].to(dev), w['ln_g'].to(dev), pdrop,
                        seed, True, True)
    for k, t in zip(('dx', 'd_o', 'dh', 'dW1', 'dW2', 'db1', 'db2', 'dgamma', 'dbeta'), wrapped):
        if k != 'd_o' or pdrop:       # without dropout d_o IS dx
            same_bits(t, want[k], 'lamp_ffn_bwd through the wrapper, ' + k)
    for k in got:
        same_bits(got[k], want[k], 'lamp_ffn_bwd ' + k)


# ------------------------------------------------------------------ training composites: lamp_mha_train_fwd + lamp_mha_bwd
def mha_reference(N, xq, xkv, w, blocked, dy, H, dk, p_attn, p_out, s_attn, s_out, dv=None):
    dv = dk if dv is None else dv
    B, lq, d = xq.shape
    lk = xkv.size(1)
    names = ['wq', 'wk', 'wv', 'ln_g', 'ln_b'] + (['fc'] if w['fc'] is not None else [])
    lv = dict((k, w[k].double().requires_grad_()) for k in names)
    XQ, XKV = xq.double().requires_grad_(), xkv.double().requires_grad_()
    split = lambda t, l: t.view(B, l, H, -1).permute(2, 0, 1, 3)  # noqa: E731
    q, k, v = XQ @ lv['wq'].t(), XKV @ lv['wk'].t(), XKV @ lv['wv'].t()
    s = (split(q, lq) @ split(k, lk).transpose(-1, -2)) / dk ** 0.5
    P = torch.softmax(s.masked_fill(blocked, float('-inf')), -1)
    keep_a = N.dropout_keep_mask(H * B * lq * lk, p_attn, s_attn).view(H, B, lq, lk) if p_attn else 1.0
    Pd = P * keep_a / (1 - p_attn)
    a = (Pd @ split(v, lk)).permute(1, 2, 0, 3).reshape(B, lq, H * dv)
    o = a @ lv['fc'].t() if 'fc' in lv else a
    keep_o = N.dropout_keep_mask(B * lq * d, p_out, s_out).view(B, lq, d) if p_out else 1.0
    y = F.layer_norm(o * keep_o / (1 - p_out) + XQ, (d,), lv['ln_g'], lv['ln_b'], 1e-5)
    y.backward(dy.double())
    ref = dict(y=y.detach(), P=P.detach().reshape(H * B, lq, lk), Pd=Pd.detach().reshape(H * B, lq, lk), q=q.detach(), k=k.detach(),
               v=v.detach(), a=a.detach(), dxq=XQ.grad.reshape(B * lq, d), dxk=XKV.grad.reshape(B * lk, d), dwq=lv['wq'].grad,
               dwk=lv['wk'].grad, dwv=lv['wv'].grad, dgamma=lv['ln_g'].grad, dbeta=lv['ln_b'].grad)
    if 'fc' in lv:
        ref['dfc'], ref['o'] = lv['fc'].grad, o.detach().reshape(B * lq, d)
    return ref


def mha_arena_run(N, ar, xq, xkv, w, blocked, dy, H, dk, p_attn, p_out, s_attn, s_out, defer, dv=None):
    L = N.lib()
    dv = dk if dv is None else dv
    B, lq, d = xq.shape
    lk, hd, hdv = xkv.size(1), H * dk, H * dv
    desc = N.MhaTrainDesc(B, lq, lk, d, H, dk, dv, 1.0 / dk ** 0.5, p_attn, p_out, s_attn, s_out)
    wts = arena_mha_weights(N, ar, w, H)
    has_fc = w['fc'] is not None
    XQ, XKV, DY = ar.inp(xq, 'xq'), ar.inp(xkv, 'xkv'), ar.inp(dy, 'dy')
    Mb = ar.inp(blocked.to(torch.uint8), 'mask')
    mask = N.Mask(N.LAMP_MASK_U8, 0, p(Mb), 0, lk, None, 0, 0)
    q, k, v, a = ar.out((B, lq, hd), 'q'), ar.out((B, lk, hd), 'k'), ar.out((B, lk, hdv), 'v'), ar.out((B, lq, hdv), 'a')
    P = ar.out((H * B, lq, lk), 'P')
    Pd = ar.out((H * B, lq, lk), 'Pd') if p_attn else None
    lse = ar.scratch(H * B * lq * 4, 'lse')
    o = ar.out((B * lq, d), 'o') if has_fc else None
    y = ar.out((B, lq, d), 'y')
    ok(L.lamp_mha_train_fwd(C.byref(desc), C.byref(wts), p(XQ), p(XKV), p(XKV), C.byref(mask), p(q), p(k), p(v), p(a), p(P), p(Pd),
                            p(lse), p(o), p(y), N.stream()), 'lamp_mha_train_fwd')
    dxq, d_o = ar.out((B * lq, d), 'dxq'), (ar.out((B * lq, d), 'd_o') if p_out else None)
    da = ar.scratch(B * lq * hdv * 4, 'da') if has_fc else None
    dP = ar.scratch(H * B * lq * lk * 4, 'dP')
    dq, dk_, dv_ = ar.out((B * lq, hd), 'dq'), ar.out((B * lk, hd), 'dk'), ar.out((B * lk, hdv), 'dv')
    dxk = ar.out((B * lk, d), 'dxk')
    dg, db = ar.out((d,), 'dgamma'), ar.out((d,), 'dbeta')
    dwq, dwk, dwv = ar.out((hd, d), 'dwq'), ar.out((hd, d), 'dwk'), ar.out((hdv, d), 'dwv')
    dfc = ar.out((d, hdv), 'dfc') if has_fc else None
    nb = L.lamp_mha_bwd_workspace_bytes(C.byref(desc))
    ws = ar.scratch(nb, 'workspace')
    part, npb, job = None, 0, None
    if defer:
        npb = L.lamp_mha_bwd_partials_bytes(C.byref(desc))
        part, job = ar.scratch(npb, 'partials'), (N.ReduceJob * 1)()
    ok(L.lamp_mha_bwd(C.byref(desc), C.byref(wts), p(XQ), p(XKV), p(XKV), p(q), p(k), p(v), p(a), p(P), p(Pd), p(o), p(DY), p(dxq),
                      p(d_o), p(da), p(dP), p(dq), p(dk_), p(dv_), p(dxk), None, p(dg), p(db), p(dwq), p(dwk), p(dwv), p(dfc),
                      p(ws), nb, p(part), npb, job, N.stream()), 'lamp_mha_bwd')
    if defer:
        ok(L.lamp_reduce_partials_grouped(job, 1, N.stream()), 'lamp_reduce_partials_grouped')
    outs = dict(q=q, k=k, v=v, a=a, P=P, y=y, dxq=dxq, dxk=dxk, dq=dq, dk=dk_, dv=dv_, dgamma=dg, dbeta=db, dwq=dwq, dwk=dwk, dwv=dwv)
    if has_fc:
        outs['o'], outs['dfc'] = o, dfc
    if p_attn:
        outs['Pd'] = Pd
    if p_out:
        outs['d_o'] = d_o
    return outs


def mha_autograd_route(N, xq, xkv, w, blocked, dy, H, p_attn, p_out, s_attn, s_out, dev, composite):
    """lamp_amd/training.py's _MHAFn through autograd with torch-allocated buffers: the composite calls (through the wrappers
    and workspace()) or the per-launch route -> gradients by the names of mha_arena_run."""
    from lamp_amd import training
    B, lq, d = xq.shape
    lk = xkv.size(1)
    names = ['xq', 'xkv', 'wq', 'wk', 'wv', 'fc', 'ln_g', 'ln_b']
    t = dict(w, xq=xq, xkv=xkv)
    lv = [t[k].to(dev).requires_grad_() if t[k] is not None else None for k in names]
    mask, keep = N.make_mask(blocked.to(dev), B, lq, lk)
    saved = training.COMPOSITE_CALLS
    training.COMPOSITE_CALLS = composite
    try:
        y, Pm = training._MHAFn.apply(*lv, H, mask, keep, p_attn, p_out, s_attn, s_out)
        y.backward(dy.to(dev))
    finally:
        training.COMPOSITE_CALLS = saved
    out = dict(y=y.detach(), dxq=lv[0].grad.view(B * lq, d), dxk=lv[1].grad.view(B * lk, d), dwq=lv[2].grad, dwk=lv[3].grad,
               dwv=lv[4].grad, dgamma=lv[6].grad, dbeta=lv[7].grad)
    if lv[5] is not None:
        out['dfc'] = lv[5].grad
    return out


def check_mha(got, ref, Kq=None, Kk=None):
    assert max_abs_diff(got['y'], ref['y']) < 3e-5
    assert max_abs_diff(got['P'], ref['P']) < 1e-5
    if 'Pd' in got:
        assert max_abs_diff(got['Pd'], ref['Pd']) < 1e-5
    for k in ('dxq', 'dxk', 'dwq', 'dwk', 'dwv', 'dfc', 'dgamma', 'dbeta'):
        if k not in ref:
            continue
        err, scale = max_abs_diff(got[k], ref[k]), ref[k].abs().max().item()
        print('mha %-6s max|err| %.3e (scale %.3e)' % (k, err, scale))
        assert err <= 3e-4 * scale + 1e-9, k
        if Kq is not None and k in ('dwq', 'dfc'):
            assert err < 3e-5 * Kq ** 0.5, k
        if Kk is not None and k in ('dwk', 'dwv'):
            assert err < 3e-5 * Kk ** 0.5, k


@pytest.mark.parametrize('defer', [False, True])
@pytest.mark.parametrize('p_attn,p_out', [(0.0, 0.0), (0.25, 0.2)])
def test_mha_train_fwd_and_bwd(dev, N, p_attn, p_out, defer):
    mha_train_case(dev, N, 4, 64, 16, 16, p_attn, p_out, defer, seed=70)


def mha_train_case(dev, N, H, d, dk, dv, p_attn, p_out, defer, seed):
    g = rnd(seed)
    B, lq, lk = 2, 37, 23
    w = sublayer_weights(d, 96, H, dk, g, dv)
    xq, xkv, dy = torch.randn(B, lq, d, generator=g), torch.randn(B, lk, d, generator=g), torch.randn(B, lq, d, generator=g)
    blocked = torch.rand(lq, lk, generator=g) < 0.3
    blocked[:, 0] = False
    got = run_both(dev, lambda ar: mha_arena_run(N, ar, xq, xkv, w, blocked, dy, H, dk, p_attn, p_out, 99, 100, defer, dv))
    check_mha(got, mha_reference(N, xq, xkv, w, blocked, dy, H, dk, p_attn, p_out, 99, 100, dv))
    for composite in (True, False):     # the wrapper route, and the per-launch route: the same bits
        want = mha_autograd_route(N, xq, xkv, w, blocked, dy, H, p_attn, p_out, 99, 100, dev, composite)
        for k in want:
            same_bits(got[k], want[k], 'lamp_mha_bwd %s (composite=%s)' % (k, composite))


@pytest.mark.parametrize('defer', [False, True])
@pytest.mark.parametrize('p_attn,p_out', [(0.0, 0.0), (0.25, 0.2)])
@pytest.mark.parametrize('H,d,dk,dv', [(3, 64, 24, 40), (1, 64, 48, 64)])
def test_mha_train_fwd_and_bwd_general_head_geometry(dev, N, H, d, dk, dv, p_attn, p_out, defer):
    """test_mha_train_fwd_and_bwd with n_head * d_k != n_head * d_v != d_model (MhaBwdProds over (d, hdk, hdv), the attention
    dropout counter over H * B * lq * lk, q / k buffers hdk wide and v / a buffers hdv wide), and with one head without fc at
    d_v = d_model != d_k.  (d_k or d_v > 128 is not a composite shape: lamp_amd/training.py keeps the per-launch route.)"""
    mha_train_case(dev, N, H, d, dk, dv, p_attn, p_out, defer, seed=700 + H + dk + dv)


@pytest.mark.parametrize('p_attn,p_out', [(0.0, 0.0), (0.1, 0.1)])
def test_mha_bwd_weight_gradients_split_k_like_the_per_launch_route(dev, N, p_attn, p_out):
    """B * lk = 1200 key rows, n_head * d_k = 2048 != d_model = 64: dwk / dwv [2048, 64] over K = 1200 take a K split, the
    2048 x 2048 square the size function used to be bounded by takes none.  Exact workspace; every output the bits of the
    per-launch route."""
    g = rnd(80)
    B, lq, lk, H, dk, d = 8, 20, 150, 16, 128, 64
    w = sublayer_weights(d, 96, H, dk, g)
    for k in ('wq', 'wk', 'wv', 'fc'):
        w[k] = w[k] * 0.25
    xq, xkv, dy = torch.randn(B, lq, d, generator=g), torch.randn(B, lk, d, generator=g), torch.randn(B, lq, d, generator=g)
    blocked = torch.rand(lq, lk, generator=g) < 0.3
    blocked[:, 0] = False
    L = N.lib()
    desc = N.MhaTrainDesc(B, lq, lk, d, H, dk, dk, 1.0 / dk ** 0.5, p_attn, p_out, 99, 100)
    need = L.lamp_gemm_workspace_bytes(H * dk, d, B * lk, 1)
    assert need > 0 and L.lamp_gemm_workspace_bytes(H * dk, H * dk, B * lk, 1) == 0
    assert L.lamp_mha_bwd_workspace_bytes(C.byref(desc)) >= need
    got = run_both(dev, lambda ar: mha_arena_run(N, ar, xq, xkv, w, blocked, dy, H, dk, p_attn, p_out, 99, 100, False),
                   capacity=96 << 20)
    check_mha(got, mha_reference(N, xq, xkv, w, blocked, dy, H, dk, p_attn, p_out, 99, 100), Kq=B * lq, Kk=B * lk)
    for composite in (True, False):
        want = mha_autograd_route(N, xq, xkv, w, blocked, dy, H, p_attn, p_out, 99, 100, dev, composite)
        for k in want:
            same_bits(got[k], want[k], 'lamp_mha_bwd %s (composite=%s)' % (k, composite))


@pytest.mark.parametrize('p_attn,p_out', [(0.0, 0.0), (0.1, 0.1)])
@pytest.mark.parametrize('H,dk,dv', [(16, 128, 64), (16, 64, 128), (3, 24, 40), (1, 48, 64)])
def test_mha_bwd_weight_gradients_split_k_with_hdk_not_hdv(dev, N, H, dk, dv, p_attn, p_out):
    """The shape of test_mha_bwd_weight_gradients_split_k_like_the_per_launch_route (B * lk = 1200 key rows, d_model = 64) with
    n_head * d_k != n_head * d_v: 2048 / 1024, 1024 / 2048, 72 / 120 and one head of 48 / 64.  dwk [hdk, 64] and dwv [hdv, 64]
    over K = 1200 are two products of different heights, each with its own K split: the workspace of exactly
    lamp_mha_bwd_workspace_bytes() must hold the larger, and every output has the bits of the per-launch route."""
    g = rnd(800 + H + dk + dv)
    B, lq, lk, d = 8, 20, 150, 64
    w = sublayer_weights(d, 96, H, dk, g, dv)
    for k in ('wq', 'wk', 'wv', 'fc'):
        if w[k] is not None:
            w[k] = w[k] * 0.25
    xq, xkv, dy = torch.randn(B, lq, d, generator=g), torch.randn(B, lk, d, generator=g), torch.randn(B, lq, d, generator=g)
    blocked = torch.rand(lq, lk, generator=g) < 0.3
    blocked[:, 0] = False
    L = N.lib()
    desc = N.MhaTrainDesc(B, lq, lk, d, H, dk, dv, 1.0 / dk ** 0.5, p_attn, p_out, 99, 100)
    need = max(L.lamp_gemm_workspace_bytes(H * dk, d, B * lk, 1), L.lamp_gemm_workspace_bytes(H * dv, d, B * lk, 1),
               L.lamp_gemm_workspace_bytes(H * dk, d, B * lq, 1), L.lamp_gemm_workspace_bytes(d, H * dv, B * lq, 1))
    if H == 16:
        assert L.lamp_gemm_workspace_bytes(2048, d, B * lk, 1) > 0 and L.lamp_gemm_workspace_bytes(2048, 2048, B * lk, 1) == 0
    assert L.lamp_mha_bwd_workspace_bytes(C.byref(desc)) >= need
    got = run_both(dev, lambda ar: mha_arena_run(N, ar, xq, xkv, w, blocked, dy, H, dk, p_attn, p_out, 99, 100, False, dv),
                   capacity=96 << 20)
    check_mha(got, mha_reference(N, xq, xkv, w, blocked, dy, H, dk, p_attn, p_out, 99, 100, dv), Kq=B * lq, Kk=B * lk)
    for composite in (True, False):
        want = mha_autograd_route(N, xq, xkv, w, blocked, dy, H, p_attn, p_out, 99, 100, dev, composite)
        for k in want:
            same_bits(got[k], want[k], 'lamp_mha_bwd %s (composite=%s)' % (k, composite))


# ------------------------------------------------------------------ optimizer, weight repack, prior graph
def test_optim_step_adam(dev, N):
    """One Adam update over five tensors (sizes 1, 3, 4095, 3 * 4096 + 5, 1001: vector bodies and scalar tails) with the
    parameters and both moments updated in place in the arena; the bar of tests/test_train_gpu.py (train_common.within:
    one fp32 ulp or 4 x the gap torch's own fp32 Adam shows against fp64)."""
    import train_common as TC
    params, grads = TC.optim_case(3, 1)
    gsd = rnd(4)
    m0 = [torch.randn(q.shape, generator=gsd) * 0.05 for q in params]
    v0 = [torch.rand(q.shape, generator=gsd) * 0.01 for q in params]
    lr, step, (b1, b2), eps = 2e-3, 5, TC.ADAM_BETAS, 1e-8

    def body(ar):
        arr, outs = (N.OptimEntry * len(params))(), {}
        for i, (q, g, m, v) in enumerate(zip(params, grads[0], m0, v0)):
            P, G = ar.inout(q, 'param%d' % i), ar.inp(g, 'grad%d' % i)
            M, V = ar.inout(m, 'exp_avg%d' % i), ar.inout(v, 'exp_avg_sq%d' % i)
            arr[i] = N.OptimEntry(p(P), p(G), p(M), p(V), q.numel())
            outs.update({'p%d' % i: P, 'm%d' % i: M, 'v%d' % i: V})
        ok(N.lib().lamp_optim_step(arr, len(params), N.LAMP_OPTIM_ADAM, step, lr, b1, b2, eps, N.stream()), 'lamp_optim_step')
        return outs
    got = run_both(dev, body)
    for i, (q, g, m, v) in enumerate(zip(params, grads[0], m0, v0)):
        want = TC.adam_reference(q, [g], [lr], m=m, v=v, step0=step - 1)
        m32 = m + (g - m) * (1 - b1)                 # torch's own fp32 arithmetic on the CPU: the yardstick
        v32 = v * b2 + (1 - b2) * g * g
        p32 = q - lr / (1 - b1 ** step) * m32 / (v32.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
        for name, w64, w32 in (('p', want[0], p32), ('m', want[1], m32), ('v', want[2], v32)):
            TC.within(got['%s%d' % (name, i)], w64, TC.gap(w32, w64), 'adam %s[%d]' % (name, i))
    dp = [q.clone().to(dev) for q in params]
    dm, dv = [t.clone().to(dev) for t in m0], [t.clone().to(dev) for t in v0]
    N.optim_step([(a, g.to(dev), b, c) for a, g, b, c in zip(dp, grads[0], dm, dv)], N.LAMP_OPTIM_ADAM, step, lr, b1, b2, eps)
    for i in range(len(params)):
        same_bits(got['p%d' % i], dp[i], 'lamp_optim_step param %d' % i)
        same_bits(got['m%d' % i], dm[i], 'lamp_optim_step exp_avg %d' % i)
        same_bits(got['v%d' % i], dv[i], 'lamp_optim_step exp_avg_sq %d' % i)


@pytest.mark.parametrize('fmt,n,k', [(0, 48, 96), (1, 128, 48)])
def test_pack_weight_both_formats(dev, N, fmt, n, k):
    """An exact rearrangement: every value of W exactly once, none invented; W's rows ldw = k + 4 apart."""
    w = torch.randn(n, k, generator=rnd(fmt))
    ldw = k + 4

    def body(ar):
        W, out = ar.inp(w, 'W', ld=ldw), ar.out((n * k,), 'packed')
        ok(N.lib().lamp_pack_weight(p(W), n, k, ldw, fmt, p(out), N.stream()), 'lamp_pack_weight')
        return {'packed': out}
    got = run_both(dev, body)
    assert torch.equal(got['packed'].cpu().sort().values, w.flatten().sort().values)
    same_bits(got['packed'], N.weight_pack(w.to(dev), fmt), 'lamp_pack_weight')


def test_prior_graph_build(dev, N):
    g = rnd(31)
    Ln, n_samples = 37, 20
    sets = [sorted(set(torch.randint(0, Ln - 1, (int(torch.randint(0, 5, (1,), generator=g)),), generator=g).tolist()))
            for _ in range(n_samples)]                  # label Ln - 1 never occurs; some samples are empty
    ids = torch.tensor([l for s in sets for l in s], dtype=torch.int64)
    off = torch.tensor([0] + [len(s) for s in sets], dtype=torch.int64).cumsum(0)

    def body(ar):
        I, O = ar.inp(ids, 'label_ids'), ar.inp(off, 'offsets')
        adj, blocked = ar.out((Ln, Ln), 'adj'), ar.out((Ln, Ln), 'blocked', dtype=torch.uint8)
        ok(N.lib().lamp_prior_graph_build(p(I), p(O), n_samples, Ln, p(adj), p(blocked), N.stream()), 'lamp_prior_graph_build')
        return {'adj': adj, 'blocked': blocked}
    got = run_both(dev, body)
    Y = torch.zeros(n_samples, Ln, dtype=torch.float64)
    for i, s in enumerate(sets):
        Y[i, s] = 1
    want = (((Y.t() @ Y) > 0) | torch.eye(Ln, dtype=torch.bool)).float()
    assert torch.equal(got['adj'].cpu(), want) and torch.equal(got['blocked'].cpu(), (want == 0).to(torch.uint8))
    wadj, wblocked = N.prior_graph(ids.to(dev), off.to(dev), Ln, want_blocked=True)
    same_bits(got['adj'], wadj, 'adj')
    same_bits(got['blocked'], wblocked, 'blocked')


# ------------------------------------------------------------------ the pair kernel (LAMP_MASK_SPARSE_ROWS)
def test_sdpa_pair_kernel(dev, N):
    """A shared bit-packed mask of an unstructured 5 % graph over 1030 labels (no multiple of the 64-key tile, the 128-query
    block or the 32-bit mask word); a row with one allowed key (the last) and a dead row in the last partial query block."""
    Ln, B, H, dk = 1030, 1, 2, 128
    g = rnd(Ln)
    q, k, v = (torch.randn(B, Ln, H * dk, generator=g) for _ in range(3))
    blocked = (R.make_adjacency(Ln, 0.05, 1) == 0)
    blocked[3, :] = True
    blocked[3, Ln - 1] = False
    blocked[Ln - 2, :] = True
    words = N.pack_mask_bits(blocked.to(torch.uint8))
    allowed = int((~blocked).sum())

    def call(Q, K_, V, Wd, out):
        ms = N.Mask(N.LAMP_MASK_BITS_U32, N.LAMP_MASK_SPARSE_ROWS, p(Wd), 0, words.size(1), None, 0, allowed)
        lay = N.AttnLayout(Ln * H * dk, dk, H * dk, Ln * H * dk, dk, H * dk, Ln * H * dk, dk, H * dk, Ln * H * dk, dk, H * dk)
        ok(N.lib().lamp_sdpa_fwd(p(Q), p(K_), p(V), p(out), None, B, H, Ln, Ln, dk, dk, dk ** -0.5, C.byref(ms), C.byref(lay),
                                 N.stream()), 'lamp_sdpa_fwd')

    def body(ar):
        Q, K_, V, Wd = ar.inp(q, 'q'), ar.inp(k, 'k'), ar.inp(v, 'v'), ar.inp(words, 'mask_bits')
        out = ar.out((B, Ln, H * dk), 'out')
        call(Q, K_, V, Wd, out)
        return {'out': out}
    got = run_both(dev, body)
    heads = lambda t: t.view(B, Ln, H, dk).permute(0, 2, 1, 3).double()  # noqa: E731
    sc = (heads(q) @ heads(k).transpose(-1, -2)) / dk ** 0.5
    ref = (torch.softmax(sc.masked_fill(blocked[None, None], float('-inf')), -1) @ heads(v)).permute(0, 2, 1, 3).reshape(B, Ln, H * dk)
    out = got['out'].cpu()
    assert torch.isnan(ref[:, Ln - 2]).all() and torch.isnan(out[:, Ln - 2]).all() and max_abs_diff(out, ref) < 2e-5
    assert max_abs_diff(out[:, 3], v[:, Ln - 1]) < 1e-6
    qd, kd, vd, wd = q.to(dev), k.to(dev), v.to(dev), words.to(dev)
    # no lamp_amd/_native.py wrapper passes LAMP_MASK_SPARSE_ROWS to lamp_sdpa_fwd directly (the model sets it in lamp_model):
    # the comparison is the same raw call on ordinary torch memory
    want = torch.empty(B, Ln, H * dk, device=dev)
    call(qd, kd, vd, wd, want)
    same_bits(got['out'], want, 'pair kernel output')


# ------------------------------------------------------------------ the one-hot blocks
@pytest.mark.parametrize('pdrop', [0.0, 0.3])
def test_onehot_blocks_forward_and_backward(dev, N, pdrop):
    """lamp_conv_pack (both flips), lamp_onehot_front_fwd, lamp_conv_window_fwd (conv2 with its epilogue, and its input
    gradient on the flipped repack), lamp_conv_relu_bwd_pad, lamp_onehot_front_bwd with partials of exactly
    lamp_onehot_front_bwd_partials_bytes() and their lamp_colsum, chained as lamp_amd/training.py: _OnehotFn chains them, at
    the smallest shape of tests/test_onehot_gpu.py.  The forward against the fp64 restatement (1e-4, that file's bar); every
    block against the same chain through the wrappers, bit for bit."""
    from onehot_common import build_model, make_dna
    B, T, d, seed, V = 2, 30, 64, 12345, 9
    T2 = T // 2
    Tp = T2 + 16
    enc = build_model(d=d, h=4, L=23, T_max=64, dropout=pdrop).encoder
    seq, pos = make_dna(B, T, [30, 17], seed=7)
    t1 = N.onehot_tap_table(enc.src_word_emb.weight, enc.conv1.weight).detach()
    b1, w2, b2 = enc.conv1.bias.detach(), enc.conv2.weight.detach().contiguous(), enc.conv2.bias.detach()
    pw = enc.position_enc.weight.detach()
    dx = torch.randn(B * T2, d, generator=rnd(5))
    L = N.lib()
    cols = V * 16 * d

    def body(ar):
        S, Pp, T1, B1, W2, B2, PW, DX = (ar.inp(t, n) for t, n in ((seq, 'src_seq'), (pos, 'src_pos'), (t1, 't1'), (b1, 'conv1_b'),
                                                                   (w2, 'conv2_w'), (b2, 'conv2_b'), (pw, 'pos'), (dx, 'dx')))
        pack, flip = ar.out((d, 16, d), 'pack'), ar.out((d, 16, d), 'pack_flipped')
        ok(L.lamp_conv_pack(p(W2), d, d, 16, 0, p(pack), N.stream()), 'lamp_conv_pack')
        ok(L.lamp_conv_pack(p(W2), d, d, 16, 1, p(flip), N.stream()), 'lamp_conv_pack(flip)')
        fe = N.OnehotFrontend(p(T1), p(B1), p(W2), p(B2), p(pack), V, 16)
        xpad = ar.out((B * Tp + 16, d), 'xpad')
        ok(L.lamp_onehot_front_fwd(p(S), B, T, C.byref(fe), d, pdrop, seed, p(xpad), N.stream()), 'lamp_onehot_front_fwd')
        out, ro = ar.out((B * T2, d), 'out'), ar.out((B * T2, d), 'relu_out')
        ok(L.lamp_conv_window_fwd(p(xpad), B, T2, Tp, d, p(pack), d, p(B2), 1, p(PW), pw.size(0), p(Pp), T, p(out), p(ro),
                                  N.stream()), 'lamp_conv_window_fwd')
        dz2 = ar.out((B * Tp + 16, d), 'dz2')
        ok(L.lamp_conv_relu_bwd_pad(p(DX), p(ro), B, T2, d, p(dz2), N.stream()), 'lamp_conv_relu_bwd_pad')
        dP = ar.out((B * T2, d), 'dP')
        ok(L.lamp_conv_window_fwd(p(dz2) + d * 4, B, T2, Tp, d, p(flip), d, None, 0, None, 0, None, 0, p(dP), None, N.stream()),
           'lamp_conv_window_fwd(input gradient)')
        fe2 = N.OnehotFrontend(p(T1), p(B1), p(W2), p(B2), None, V, 16)
        dz1 = ar.out((B, T, d), 'dz1')
        nb = L.lamp_onehot_front_bwd_partials_bytes(B, T, V, d)
        assert nb > 0 and nb % (cols * 4) == 0
        part = ar.scratch(nb, 'partials')
        ok(L.lamp_onehot_front_bwd(p(S), B, T, C.byref(fe2), d, pdrop, seed, p(dP), p(dz1), p(part), nb, N.stream()),
           'lamp_onehot_front_bwd')
        rows = nb // (cols * 4)
        dt1 = ar.out((cols,), 'dt1')
        cb = L.lamp_colsum_workspace_bytes(rows, cols)
        ws = ar.scratch(cb, 'workspace')
        ok(L.lamp_colsum(p(part), rows, cols, cols, p(dt1), p(ws), cb, N.stream()), 'lamp_colsum')
        return dict(pack=pack, flip=flip, xpad=xpad, out=out, relu_out=ro, dz2=dz2, dP=dP, dz1=dz1, dt1=dt1)
    got = run_both(dev, body)
    assert torch.equal(got['pack'].cpu(), w2.permute(0, 2, 1)) and torch.equal(got['flip'].cpu(), w2.flip(2).permute(1, 2, 0))
    sd = dict((k_, v_.detach().double()) for k_, v_ in enc.state_dict().items())
    keep = N.dropout_keep_mask(B * T * d, pdrop, seed).view(B, T, d).transpose(1, 2).double() if pdrop else 1.0
    y = F.conv1d(F.embedding(seq, sd['src_word_emb.weight']).transpose(1, 2), sd['conv1.weight'], sd['conv1.bias'], padding=8)[:, :, :-1]
    y = F.max_pool1d(torch.relu(y * keep / (1 - pdrop)), 2, 2)
    y = torch.relu(F.conv1d(y, sd['conv2.weight'], sd['conv2.bias'], padding=8).transpose(1, 2))[:, :-1, :]
    assert max_abs_diff(got['relu_out'].view(B, T2, d), y) < 1e-4
    assert max_abs_diff(got['out'].view(B, T2, d), y + F.embedding(pos[:, :T2], sd['position_enc.weight'])) < 1e-4
    # the same chain through the wrappers
    sq, ps, t1d, b1d, w2d, b2d, pwd = (t.to(dev) for t in (seq, pos, t1, b1, w2, b2, pw))
    wpack, wflip = N.conv_pack(w2d), N.conv_pack(w2d, flip=True)
    fe = N.onehot_frontend(t1d, b1d, w2d, b2d, wpack)
    wxpad = N.onehot_front_fwd(sq, fe, d, pdrop, seed)
    wout, wro = N.conv_window(wxpad, B, T2, Tp, wpack, b2d, True, pwd, ps, relu_out=True)
    wdz2 = N.conv_relu_bwd_pad(dx.to(dev), wro, B, T2)
    wdP = N.conv_window(wdz2[1:], B, T2, Tp, wflip)
    wdz1, wdt1 = N.onehot_front_bwd(sq, N.onehot_frontend(t1d, b1d, w2d, b2d, None), d, wdP, pdrop, seed)
    for name, want in (('pack', wpack), ('flip', wflip), ('xpad', wxpad), ('out', wout), ('relu_out', wro), ('dz2', wdz2),
                       ('dP', wdP), ('dz1', wdz1), ('dt1', wdt1)):
        same_bits(got[name], want, 'one-hot block ' + name)


# ------------------------------------------------------------------ attention: one shape per row of the routing table
# (lq, lk, dk, dv, mask kind of attn_routes_common.sdpa_case): outputs in the fused [B, l, H*d] layout, so a wrong head stride
# lands in a neighbour head's columns; the 'u8' / 'shared' cases carry a dead (fully blocked) row as the LAST query, i.e. in the
# last partial query block; 'keys' a sample whose keys are all padding.
SDPA_CASES = [(33, 65, 32, 32, 'u8'),       # the 16-query kernel (attention_small.hip)
              (257, 65, 32, 32, 'u8'),      # the 32-query kernel: lq > 256 and lk > 64
              (260, 70, 24, 24, 'keys'),    # ... with per-sample key counts
              (33, 65, 32, 32, 'shared'),
              (33, 65, 132, 132, 'u8')]     # wide heads: the general three-launch route, scores kept in the map buffer


def sdpa_arena_operands(N, ar, c):
    B, H, lq, lk, dk, dv = c['B'], c['H'], c['lq'], c['lk'], c['dk'], c['dv']
    q, k, v = ar.inp(c['q'], 'q'), ar.inp(c['k'], 'k'), ar.inp(c['v'], 'v')
    lay = N.AttnLayout(lq * H * dk, dk, H * dk, lk * H * dk, dk, H * dk, lk * H * dv, dv, H * dv, lq * H * dv, dv, H * dv)
    mask = None
    if c['kind'] == 'u8':
        m = ar.inp(c['blocked'].to(torch.uint8), 'mask')
        mask = N.Mask(N.LAMP_MASK_U8, 0, p(m), lq * lk, lk, None, 0, 0)
    elif c['kind'] == 'shared':
        m = ar.inp(c['shared'].to(torch.uint8), 'mask')
        mask = N.Mask(N.LAMP_MASK_U8, 0, p(m), 0, lk, None, 0, 0)
    elif c['kind'] == 'keys':
        m = ar.inp(c['seq'], 'src_seq')
        mask = N.Mask(N.LAMP_MASK_KEY_TOKENS_I64, 0, p(m), lk, 0, None, 0, 0)
    return q, k, v, lay, mask


def check_sdpa(c, out, P, wide=False):
    """NaN exactly in the dead rows; everything else within the bars of attn_routes_common / test_sdpa_wide_heads_vs_oracle."""
    import attn_routes_common as AR
    tol_out, tol_map = (5e-5, 1e-5) if wide else (AR.TOL_OUT, AR.TOL_MAP)
    out = out.double().cpu()
    assert torch.equal(torch.isnan(out), torch.isnan(c['ref_O']))
    assert max_abs_diff(torch.nan_to_num(out), torch.nan_to_num(c['ref_O'])) < tol_out
    if P is not None:
        P = P.double().cpu()
        assert torch.equal(torch.isnan(P), torch.isnan(c['ref_P']))
        assert max_abs_diff(torch.nan_to_num(P), torch.nan_to_num(c['ref_P'])) < tol_map


# wide heads keep their scores in the map buffer: the map is required, and there is no single-pass write-out
SDPA_RUNS = [c + (mode,) for c in SDPA_CASES for mode in ('out_only', 'exact_maps', 'fast_maps') if c[2] <= 128 or mode == 'exact_maps']


@pytest.mark.parametrize('lq,lk,dk,dv,kind,mode', SDPA_RUNS)
def test_sdpa_fwd_routes(dev, N, lq, lk, dk, dv, kind, mode):
    import attn_routes_common as AR
    wide = dk > 128
    c = AR.sdpa_case(lq, lk, dk, dv, kind)
    B, H = c['B'], c['H']
    L = N.lib()
    if mode == 'fast_maps':     # the table of attn_routes_common.route: which kernel a maps-and-lse call reaches
        assert AR.route(lq, lk) == ('small16' if lq <= 256 else 'attn32')

    def body(ar):
        q, k, v, lay, mask = sdpa_arena_operands(N, ar, c)
        out = ar.out((B, lq, H * dv), 'out')
        P = ar.out((H * B, lq, lk), 'attn') if mode != 'out_only' else None
        mp = C.byref(mask) if mask is not None else None
        outs = {'out': out}
        if mode == 'fast_maps':
            lse = ar.out((H * B, lq), 'lse')
            ok(L.lamp_sdpa_fwd_fast_maps(p(q), p(k), p(v), p(out), p(P), p(lse), B, H, lq, lk, dk, dv, c['scale'], mp, C.byref(lay),
                                         N.stream()), 'lamp_sdpa_fwd_fast_maps')
            outs['lse'] = lse
        else:
            ok(L.lamp_sdpa_fwd(p(q), p(k), p(v), p(out), p(P), B, H, lq, lk, dk, dv, c['scale'], mp, C.byref(lay), N.stream()),
               'lamp_sdpa_fwd')
        if P is not None:
            outs['attn'] = P
        return outs
    got = run_both(dev, body, capacity=16 << 20)
    check_sdpa(c, got['out'], got.get('attn'), wide)
    m, keep = AR.device_mask(N, c, dev)
    qd, kd, vd = c['q'].to(dev), c['k'].to(dev), c['v'].to(dev)
    if mode == 'fast_maps':
        lse = got['lse'].double().cpu()
        live = c['live']
        assert (lse[~live] == float('-inf')).all() and torch.isfinite(lse[live]).all()
        gap = AR.lse_gap_fp32([k_[:5] for k_ in SDPA_CASES if k_[2] <= 128])
        assert (lse[live] - c['ref_lse'][live]).abs().max().item() <= AR.LSE_FACTOR * gap
        wo, wp, wl = N.sdpa_fused(qd, kd, vd, H, m, c['scale'], need_attn=True, fast_maps=True, return_lse=True)
        same_bits(got['lse'], wl, 'lse')
    else:
        wo, wp = N.sdpa_fused(qd, kd, vd, H, m, c['scale'], need_attn=mode != 'out_only')
    same_bits(got['out'], wo, 'attention output')
    if mode != 'out_only':
        same_bits(got['attn'], wp, 'attention maps')


@pytest.mark.parametrize('maps', [False, True])
def test_sdpa_act_fwd_sigmoid(dev, N, maps):
    import attn_routes_common as AR
    from sigmoid_common import sigmoid_sdpa
    c = AR.sdpa_case(33, 65, 32, 32, 'u8')
    B, H, lq, lk, dk, dv = c['B'], c['H'], c['lq'], c['lk'], c['dk'], c['dv']

    def body(ar):
        q, k, v, lay, mask = sdpa_arena_operands(N, ar, c)
        out = ar.out((B, lq, H * dv), 'out')
        P = ar.out((H * B, lq, lk), 'attn') if maps else None
        ok(N.lib().lamp_sdpa_act_fwd(p(q), p(k), p(v), p(out), p(P), B, H, lq, lk, dk, dv, c['scale'], N.LAMP_ATTN_SIGMOID,
                                     C.byref(mask), C.byref(lay), N.stream()), 'lamp_sdpa_act_fwd')
        return {'out': out, 'attn': P} if maps else {'out': out}
    got = run_both(dev, body, capacity=16 << 20)
    heads = lambda t, l, w: t.double().view(B, l, H, w).permute(2, 0, 1, 3).reshape(H * B, l, w)  # noqa: E731
    blocked = c['blocked'].unsqueeze(0).expand(H, B, lq, lk).reshape(H * B, lq, lk)
    ref_o, ref_p = sigmoid_sdpa(heads(c['q'], lq, dk), heads(c['k'], lk, dk), heads(c['v'], lk, dv), blocked)
    ref_o = ref_o.view(H, B, lq, dv).permute(1, 2, 0, 3).reshape(B, lq, H * dv)
    assert max_abs_diff(got['out'], ref_o) < AR.TOL_OUT          # a fully blocked row is 0, not NaN
    assert (got['out'][0, lq - 1] == 0).all()
    m, keep = AR.device_mask(N, c, dev)
    wo, wp = N.sdpa_fused(c['q'].to(dev), c['k'].to(dev), c['v'].to(dev), H, m, c['scale'], need_attn=maps, act=N.LAMP_ATTN_SIGMOID)
    same_bits(got['out'], wo, 'sigmoid attention output')
    if maps:
        assert max_abs_diff(got['attn'], ref_p) < AR.TOL_MAP and (got['attn'].cpu()[blocked] == 0).all()
        same_bits(got['attn'], wp, 'sigmoid attention maps')


@pytest.mark.parametrize('mode', ['out_only', 'exact_maps', 'fast_maps'])
def test_sdpa_bias_kernel_three_output_modes(dev, N, mode):
    """LAMP_MASK_BIAS_F32: a shared fp32 score bias with -inf = blocked, rows padded to a multiple of 4 floats (65 -> 68; the
    padding holds the sentinel, which the kernel may load but must never use)."""
    import attn_routes_common as AR
    c = AR.sdpa_case(33, 65, 32, 32, 'shared')
    B, H, lq, lk, dk, dv = c['B'], c['H'], c['lq'], c['lk'], c['dk'], c['dv']
    bias = torch.randn(lq, lk, generator=rnd(3)).masked_fill(c['shared'], float('-inf'))
    ld = (lk + 3) & ~3
    L = N.lib()

    def body(ar):
        q, k, v, lay, _ = sdpa_arena_operands(N, ar, dict(c, kind='none'))
        bv = ar.inp(bias, 'bias', ld=ld)
        mask = N.Mask(N.LAMP_MASK_BIAS_F32, 0, p(bv), 0, ld, None, 0, 0)
        out = ar.out((B, lq, H * dv), 'out')
        P = ar.out((H * B, lq, lk), 'attn') if mode != 'out_only' else None
        outs = {'out': out}
        if mode == 'fast_maps':
            lse = ar.out((H * B, lq), 'lse')
            ok(L.lamp_sdpa_fwd_fast_maps(p(q), p(k), p(v), p(out), p(P), p(lse), B, H, lq, lk, dk, dv, c['scale'], C.byref(mask),
                                         C.byref(lay), N.stream()), 'lamp_sdpa_fwd_fast_maps')
            outs['lse'] = lse
        else:
            ok(L.lamp_sdpa_fwd(p(q), p(k), p(v), p(out), p(P), B, H, lq, lk, dk, dv, c['scale'], C.byref(mask), C.byref(lay),
                               N.stream()), 'lamp_sdpa_fwd')
        if P is not None:
            outs['attn'] = P
        return outs
    got = run_both(dev, body, capacity=16 << 20)
    heads = lambda t, l, w: t.double().view(B, l, H, w).permute(2, 0, 1, 3)  # noqa: E731
    s = heads(c['q'], lq, dk) @ heads(c['k'], lk, dk).transpose(-1, -2) * c['scale'] + bias.double()
    ref_p = torch.softmax(s, -1)
    ref_o = (ref_p @ heads(c['v'], lk, dv)).permute(1, 2, 0, 3).reshape(B, lq, H * dv)
    ref = dict(c, ref_O=ref_o, ref_P=ref_p.reshape(H * B, lq, lk))
    check_sdpa(ref, got['out'], got.get('attn'))
    if mode == 'fast_maps':
        lse, want = got['lse'].double().cpu().view(H, B, lq), torch.logsumexp(s, -1) / math.log(2.0)
        live = torch.isfinite(want)
        assert (lse[~live] == float('-inf')).all()
        assert (lse[live] - want[live]).abs().max().item() <= AR.LSE_FACTOR * AR.lse_gap_fp32([k_[:5] for k_ in SDPA_CASES if k_[2] <= 128])
    m, keep = N.make_bias_mask(bias.to(dev), B, lq, lk)
    qd, kd, vd = c['q'].to(dev), c['k'].to(dev), c['v'].to(dev)
    if mode == 'fast_maps':
        wo, wp, wl = N.sdpa_fused(qd, kd, vd, H, m, c['scale'], need_attn=True, fast_maps=True, return_lse=True)
        same_bits(got['lse'], wl, 'lse under a bias')
    else:
        wo, wp = N.sdpa_fused(qd, kd, vd, H, m, c['scale'], need_attn=mode != 'out_only')
    same_bits(got['out'], wo, 'output under a bias')
    if mode != 'out_only':
        same_bits(got['attn'], wp, 'maps under a bias')


def test_sdpa_tile_list_route(dev, N):
    """A shared byte mask with its active-tile list, no maps: tiles not listed are skipped, the list is only read."""
    g = rnd(100)
    lq, dk, n = 100, 64, 3
    q, k, v = (torch.randn(n, lq, dk, generator=g) for _ in range(3))
    blocked = torch.ones(lq, lq, dtype=torch.bool)
    for lo in range(0, lq, 20):                     # five clusters of twenty labels: whole 32-key tiles without an edge
        blocked[lo:lo + 20, lo:lo + 20] = False
    tiles = N.active_tile_list(blocked.to(torch.uint8))
    assert tiles[:, 0].float().mean().item() < tiles.size(1) - 1

    def body(ar):
        Q, K_, V = ar.inp(q, 'q'), ar.inp(k, 'k'), ar.inp(v, 'v')
        Mb, Tl = ar.inp(blocked.to(torch.uint8), 'mask'), ar.inp(tiles, 'tile_list')
        out = ar.out((n, lq, dk), 'out')
        ms = N.Mask(N.LAMP_MASK_U8, 0, p(Mb), 0, lq, p(Tl), tiles.size(1), 0)
        lay = N.AttnLayout(lq * dk, 0, dk, lq * dk, 0, dk, lq * dk, 0, dk, lq * dk, 0, dk)
        ok(N.lib().lamp_sdpa_fwd(p(Q), p(K_), p(V), p(out), None, n, 1, lq, lq, dk, dk, dk ** -0.5, C.byref(ms), C.byref(lay),
                                 N.stream()), 'lamp_sdpa_fwd')
        return {'out': out}
    got = run_both(dev, body, capacity=16 << 20)
    ref_o, _ = R.sdpa(q.double(), k.double(), v.double(), blocked.unsqueeze(0).expand(n, lq, lq))
    assert max_abs_diff(got['out'], ref_o) < 2e-5      # (no _native wrapper takes a tile list: fp64 and the two fills only)


# ------------------------------------------------------------------ the whole forward
# V, L, T, d, dff, h, mask, pos_emb, B, p_adj, lengths: the tiny models of tests/test_gpu_training.py::CASES at B = 3, ragged
FWD_CASES = {'tiny_prior_h4': (50, 37, 23, 64, 96, 4, 'prior', True, 3, 0.2, [23, 5, 14]),
             'tiny_none_h1': (40, 20, 17, 32, 48, 1, 'none', False, 3, 0.0, [17, 9, 4])}
# the one-hot front end (lamp_onehot_forward / _opts): tests/test_onehot_gpu.py's small model, T = 41 (odd, T2 = 20), ragged
ONEHOT = dict(d=64, h=4, L=23, T_max=64, T=41, lengths=[41, 30, 7])
FWD_VARIANTS = {'default': ({}, {}),      # chain packs, the hoisted layer-0 query and the embedding fold: Models.py's defaults
                'plain': ({}, dict(use_chain_packs=False, cache_layer0_query=False, fold_embedding=False)),
                'live': (dict(enc_self_attn=True), {}),
                'live_packed': (dict(enc_self_attn=True), dict(use_packed_live_encoder=True)),
                'dec_sigmoid': (dict(dec_attn_type='sigmoid'), {}),
                'bf16x3': ({}, dict(matmul_precision='high')),
                'label_bias': (dict(label_bias=True), {}),       # LAMP_FWD_LABEL_BIAS: an (L, L) fp32 score bias, made per case
                'enc_mask': (dict(enc_self_attn=True), {})}      # live encoder under per-sample input graphs (lamp_fwd_options.enc_mask)
_MODELS = {}


def fwd_model(case, variant, dev):
    key = (case, variant)
    if key not in _MODELS and case == 'onehot':
        from onehot_common import build_model, fp64_state, make_dna, onehot_forward_ref
        o = ONEHOT
        adj = R.make_adjacency(o['L'], 0.2, 0)
        m = build_model(d=o['d'], h=o['h'], L=o['L'], T_max=o['T_max'], mask='prior', adj=adj.clone())
        seq, spos = make_dna(len(o['lengths']), o['T'], o['lengths'])
        sd = fp64_state(m)
        m = m.to(dev).eval()
        for k, v in FWD_VARIANTS[variant][1].items():
            setattr(m, k, v)
        if variant == 'dec_sigmoid':
            m.dec_attn_type = 'sigmoid'
        _MODELS[key] = (m, sd, R.label_block_mask(adj, 'prior', o['L']), seq, spos, o['h'], None)
    if key not in _MODELS:
        from lamp_amd.Models import LAMP
        import enc_live_common as EC
        import label_bias_common as LB
        V, L, T, d, dff, h, mask, pos, B, pa, lengths = FWD_CASES[case]
        ctor, attrs = FWD_VARIANTS[variant]
        if 'label_bias' in ctor:
            ctor = dict(label_bias=LB.random_bias(L, L, rnd(5)))
        graphs = EC.random_graphs(lengths, seed=1) if variant == 'enc_mask' else None
        sd = R.make_state_dict(V, L, T, d, dff, h, 2, 2, pos_emb=pos, seed=0)
        adj = R.make_adjacency(L, pa, 0) if mask == 'prior' else None
        seq, spos = R.make_batch(B, V, T, lengths=lengths, seed=0)
        m = LAMP(V, L, T, L, n_layers_enc=2, n_layers_dec=2, n_head=h, n_head2=h, d_word_vec=d, d_model=d, d_inner_hid=dff,
                 d_k=d // h, d_v=d // h, encoder='graph', decoder='graph', dropout=0.0, dec_dropout=0.0,
                 no_enc_pos_embedding=not pos, label_adj_matrix=adj.clone() if adj is not None else None, label_mask=mask,
                 dec_dropout2=False, **ctor)
        m.load_state_dict(sd)
        m = m.to(dev).eval()
        for k, v in attrs.items():
            setattr(m, k, v)
        _MODELS[key] = (m, sd, R.label_block_mask(adj, mask, L), seq, spos, h, graphs)
    return _MODELS[key]


def fwd_options(N, m, built):
    """lamp_fwd_options as lamp_amd/Models.py: forward builds them (None: plain lamp_forward)."""
    opts = None
    if m.enc_self_attn:
        opts = N.FwdOptions(1, N.LAMP_FWD_PACKED_ENCODER if m.use_packed_live_encoder else 0, None, built[8])
    flags = (N.LAMP_FWD_DEC_SIGMOID if m.dec_attn_type == 'sigmoid' else 0) | N.matmul_precision(m.matmul_precision)[1]
    if getattr(m.decoder, 'label_bias_f32', None) is not None:
        flags |= N.LAMP_FWD_LABEL_BIAS
    if flags:
        if opts is None:
            opts = N.FwdOptions(0, 0, None, None)
        opts.flags |= flags
    return opts


def fwd_arena_call(N, m, ar, seq, spos, mb, aux_kind, short=0, graphs=None):
    """lamp_forward / lamp_forward_opts / lamp_onehot_forward / lamp_onehot_forward_opts with every caller-owned buffer in the
    arena and a workspace of exactly bytes(mb) - short.  -> (status, outputs)."""
    L = N.lib()
    built = m._native_model()
    model = built[0]
    opts = fwd_options(N, m, built)
    fe = built[7][0] if m.onehot else None
    B, T_in = seq.shape
    T = T_in // 2 if fe is not None else T_in
    Ln, d = m.n_labels, m.d_model
    S, Pp = ar.inp(seq, 'src_seq'), ar.inp(spos, 'src_pos')
    if graphs is not None:
        from lamp_amd.Encoders import adj_attn_mask
        m8 = ar.inp(adj_attn_mask(seq, graphs[:B]), 'enc_mask')
        mstruct = N.Mask(N.LAMP_MASK_U8, 0, p(m8), T * T, T, None, 0, 0)
        opts.enc_mask = C.pointer(mstruct)
    logits, enc = ar.out((B, Ln), 'logits'), ar.out((B, T, d), 'enc_output')
    outs = {'logits': logits, 'enc_output': enc}
    aux, keep = None, []
    dec = m.decoder.layer_stack
    if aux_kind == 'int_preds':
        n_int = sum(2 if hasattr(l, 'slf_attn') else 1 for l in dec) - 1
        ip = [ar.out((B, Ln), 'int_pred%d' % i) for i in range(n_int)]
        arr = (C.c_void_p * n_int)(*[p(t) for t in ip])
        keep.append(arr)
        aux = N.Aux(None, None, None, arr, n_int, 0)
        outs.update(('int_pred%d' % i, t) for i, t in enumerate(ip))
    elif aux_kind == 'attn':
        ea = [ar.out((l.slf_attn.n_head * B, T, T), 'enc_self_attn%d' % i) for i, l in enumerate(m.encoder.layer_stack)]
        sa = [ar.out((l.slf_attn.n_head * B, Ln, Ln), 'dec_self_attn%d' % i) for i, l in enumerate(dec)]
        xa = [ar.out((l.enc_attn.n_head * B, Ln, T), 'dec_enc_attn%d' % i) for i, l in enumerate(dec)]
        arrs = [(C.c_void_p * len(ts))(*[p(t) for t in ts]) for ts in (ea, sa, xa)]
        keep += arrs
        aux = N.Aux(arrs[0], arrs[1], arrs[2], None, 0, 0)
        for kind, ts in (('a_enc_self_attn', ea), ('b_dec_self_attn', sa), ('c_dec_enc_attn', xa)):
            outs.update(('%s%d' % (kind, i), t) for i, t in enumerate(ts))
    want = int(aux_kind == 'attn')
    if opts is not None and fe is not None:
        nb = L.lamp_onehot_forward_opts_workspace_bytes(C.byref(model), C.byref(fe), C.byref(opts), mb, T_in, want) - short
    elif opts is not None:
        nb = L.lamp_forward_opts_workspace_bytes(C.byref(model), C.byref(opts), mb, T, want) - short
    elif fe is not None:
        nb = L.lamp_onehot_forward_workspace_bytes(C.byref(model), C.byref(fe), mb, T_in, want) - short
    else:
        nb = L.lamp_forward_workspace_bytes(C.byref(model), mb, T, want) - short
    ws = ar.scratch(nb, 'workspace')
    ap = C.byref(aux) if aux is not None else None
    if opts is not None and fe is not None:
        rc = L.lamp_onehot_forward_opts(C.byref(model), C.byref(fe), C.byref(opts), p(S), p(Pp), B, T_in, p(logits), p(enc), ap,
                                        p(ws), nb, N.stream())
    elif opts is not None:
        rc = L.lamp_forward_opts(C.byref(model), C.byref(opts), p(S), p(Pp), B, T, p(logits), p(enc), ap, p(ws), nb, N.stream())
    elif fe is not None:
        rc = L.lamp_onehot_forward(C.byref(model), C.byref(fe), p(S), p(Pp), B, T_in, p(logits), p(enc), ap, p(ws), nb, N.stream())
    else:
        rc = L.lamp_forward(C.byref(model), p(S), p(Pp), B, T, p(logits), p(enc), ap, p(ws), nb, N.stream())
    del keep
    return rc, outs


FWD_RUNS = [(c, v) for c in sorted(FWD_CASES) for v in sorted(FWD_VARIANTS)] + [('onehot', 'default'), ('onehot', 'dec_sigmoid')]


@pytest.mark.parametrize('aux_kind', [None, 'attn', 'int_preds'])
@pytest.mark.parametrize('case,variant', FWD_RUNS)
def test_forward_with_exact_workspace_and_every_micro_batch_split(dev, N, case, variant, aux_kind):
    """Workspace of exactly bytes(mb) for mb = 1, 2 (an uneven 2 + 1 split of B = 3) and 3; logits, enc_output and the aux
    outputs in the arena.  The same bits for every split, under both fills, and through LAMP.forward (lamp_amd/Models.py),
    whose grow-only workspace takes the whole batch in one pass.  One byte less than bytes(1): LAMP_E_WORKSPACE and not one
    word of the arena touched.

    A token model given less than bytes(B) drops its K/V-ahead buffers, which bytes(mb) counts: at mb < B those bytes are slack
    behind the last region in use, and only mb = B is tight.  So the first mb samples are also run alone (B = mb) with
    bytes(mb): tight at every size, and the same bits, as a sample's results do not depend on its batch."""
    m, sd, blocked, seq, spos, h, graphs = fwd_model(case, variant, dev)

    def body(mb, n=3):
        def run(ar):
            rc, outs = fwd_arena_call(N, m, ar, seq[:n], spos[:n], mb, aux_kind, graphs=graphs)
            ok(rc, 'lamp_forward(B=%d, mb=%d)' % (n, mb))
            return outs
        return run
    got = dict((mb, run_both(dev, body(mb), capacity=16 << 20)) for mb in (1, 2, 3))
    for mb in (1, 2):
        for k in got[3]:
            assert RZ.bit_equal(got[mb][k], got[3][k]), '%s differs between micro-batches of %d and 3' % (k, mb)
        alone = run_both(dev, body(mb, n=mb), capacity=16 << 20)
        for k in ('logits', 'enc_output'):
            assert RZ.bit_equal(alone[k], got[3][k][:mb].contiguous()), '%s of the first %d samples alone differs' % (k, mb)
    with torch.no_grad():
        res = m((seq.to(dev), spos.to(dev)), graphs, None, None, return_attns=aux_kind == 'attn', int_preds=aux_kind == 'int_preds')
    same_bits(got[3]['logits'], res[0], 'logits')
    same_bits(got[3]['enc_output'], res[1], 'enc_output')
    names = sorted(k for k in got[3] if k not in ('logits', 'enc_output'))
    if aux_kind == 'int_preds':
        assert len(names) == len(res[2]) == 3
        for k, t in zip(names, res[2]):
            same_bits(got[3][k], t, k)
    elif aux_kind == 'attn':
        maps = list(res[2][0]) + list(res[3][0]) + list(res[3][1])
        assert len(names) == len(maps) == 6
        for k, t in zip(names, maps):
            same_bits(got[3][k], t, k)
    if variant == 'default':     # and against the oracle, at the bars of tests/test_gpu_parity.py (TOL_LOGIT, TOL_ACT)
        if case == 'onehot':     # tests/test_onehot_gpu.py's restatement and bar
            from onehot_common import onehot_forward_ref
            ref_logits, ref_enc, _ = onehot_forward_ref(sd, seq, spos, h, blocked)
            assert max_abs_diff(got[3]['logits'], ref_logits) < 1e-4 and max_abs_diff(got[3]['enc_output'], ref_enc) < 1e-4
        else:
            ref_logits, ref_enc, _ = R.forward(R.to_dtype(sd, torch.float64), seq, spos, h, blocked)
            assert max_abs_diff(got[3]['logits'], ref_logits) < 1e-4 and max_abs_diff(got[3]['enc_output'], ref_enc) < 5e-5
    for fill in RZ.FILLS:
        ar = RZ.Arena(dev, fill, 16 << 20)
        rc, _ = fwd_arena_call(N, m, ar, seq, spos, 1, aux_kind, short=1, graphs=graphs)
        assert rc == -3, 'bytes(1) - 1 must be LAMP_E_WORKSPACE, got %d' % rc
        assert ar.untouched(), 'a refused call wrote into the arena'
