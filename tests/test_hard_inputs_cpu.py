"""The hard-input families of tests/hard_inputs_common.py, judged from the references alone (no GPU): every generator has the
property it claims, every family meets the conditions that keep the GPU bounds from being vacuous, and the families have
teeth -- each CPU mutant of a restatement (a mistake the randn tests cannot see) violates the rule on some family and passes
it on the randn inputs of the existing tests.

Conditions, for every generated case: (1) the fp32 restatement is finite exactly where the fp64 one is; (2) 4 x gap32 <= 1e-2 x
the output's scale (1 for probabilities, max|ref64| of the tensor or row else; the scale the GPU bound uses where the issue
names one); (3) the offset family at +-120 nats has gap32 <= 2e-5 on maps and <= 8e-5 on outputs, LayerNorm on
1000 + 0.1 randn has gap32 of the order of 1e-3; no element is left out."""
import pytest
import torch

import hard_inputs_common as H
import train_common as TC


def _finite_alike(a32, a64, what):
    assert torch.equal(torch.isfinite(a32), torch.isfinite(a64)), what + ': fp32 and fp64 restatements are not finite alike'
    assert torch.equal(torch.isnan(a32), torch.isnan(a64)), what


def _gap(a32, a64, scale=1.0, per_row=False):
    ok = torch.isfinite(a64)
    g = torch.where(ok, (a32.double() - a64).abs(), torch.zeros_like(a64)) / torch.as_tensor(scale, dtype=torch.float64).clamp_min(1e-300)
    return g.amax(-1) if per_row else float(g.max())


def _violates(got, want64, ref32, floor, **kw):
    """True when `got` breaks the rule (a NaN / inf mismatch counts)."""
    try:
        return H.ratio(got, want64, ref32, floor, **kw) > 1.0
    except AssertionError:
        return True


# ------------------------------------------------------------------ softmax attention
@pytest.mark.parametrize('lq,lk,dk', H.ATTN_SHAPES)
def test_attention_families_meet_the_conditions(lq, lk, dk):
    cases = H.attention_cases(lq, lk, dk)
    assert len(cases) == 1 + 3 + 2 + 8 + 1 + 1
    for c in cases:
        o64, p64 = H.sdpa_ref(c, torch.float64)
        o32, p32 = H.sdpa_ref(c, torch.float32)
        _finite_alike(p32, p64, c['name'])
        _finite_alike(o32, o64, c['name'])
        gp, go = _gap(p32, p64), _gap(o32, o64, c['oscale'])
        print('%dx%d d%d %-22s gap32: maps %.2e, out / scale %.2e' % (lq, lk, dk, c['name'], gp, go))
        assert 4 * gp <= 1e-2 and 4 * go <= 1e-2, (c['name'], gp, go)
        s = H.scores_log2(c)
        if c['name'] == 'offset':
            assert _gap(p32, p64) <= 2e-5 and _gap(o32, o64) <= 8e-5
            plain = dict(c, k=c['k'].clone())
            plain['k'][..., -1] = 0.0                      # the same case without the control coordinate: the same softmax
            shift = (s - H.scores_log2(plain)) * H.LN2
            ok = torch.isfinite(shift)
            for n, cval in ((0, 120.0), (1, -120.0)):      # ONE shift per slice (c sqrt(dk) rounded to fp32 once)
                sh = shift[n][ok[n]]
                assert float((sh - cval).abs().max()) < 1e-4 and float(sh.max() - sh.min()) < 1e-9
            assert _gap(H.sdpa_ref(plain, torch.float64)[1], p64) < 1e-12
            assert torch.isnan(p64[1, lq // 2]).all() and int(torch.isnan(p64).any(-1).sum()) == 1
        if c['name'].startswith('stair'):
            delta = float(c['name'].split('(')[1][:-1])
            tmax = torch.stack([s[..., t:t + 16].amax(-1) for t in range(0, lk, 16)], -1)     # (N, lq, tiles)
            step = tmax[..., 1:] - tmax[..., :-1]
            sign = 1.0 if 'up' in c['name'] else -1.0
            assert step.numel() == 0 or float((step - sign * delta).abs().max()) < 1.0, (c['name'], step)
        if c['name'].startswith('disparity'):
            tile, split = (int(x[1:]) for x in c['name'].split('(')[1].split(',')[:2])
            share = (torch.arange(lk) // tile) % split
            blocked = c['blocked'][0, 0]
            assert not blocked[c['onehot']] and torch.equal(blocked, share == (int(share[c['onehot']]) + 1) % split)
            others = s[..., ~blocked & (torch.arange(lk) != c['onehot'])]
            assert others.numel() == 0 or float((others - s[..., c['onehot']].unsqueeze(-1) + 300).abs().max()) < 1.0
        if c['onehot'] is not None:                        # one-hot in fp32: the GPU test asserts these bits
            r = p64.float()
            assert (r[..., c['onehot']] == 1.0).all()
            if not c['name'].startswith('stair') or c['name'].endswith('(200)'):
                assert float(r.sum()) == r.size(0) * lq    # everything else rounds to exactly 0
        if c['name'] == 'flat':
            assert lk == 1 or lk & (lk - 1)
            assert _gap(p64, torch.full_like(p64, 1.0 / lk)) < 1e-15
            mag = c['v'].abs().amax(-1)
            assert lk == 1 or (float(mag[:, -1].min() / mag[:, 0].max()) > 1e4)
        if c['name'] == 'allneg':
            assert float(s[torch.isfinite(s)].max()) * H.LN2 < -280
        extra = H.lse_extra(c)
        assert torch.isfinite(extra).all() and float(extra.max()) <= 1e-3


def test_bias_and_sigmoid_and_backward_pieces_meet_the_conditions():
    for lq, lk, dk in H.ATTN_SHAPES:
        for c in H.attention_cases(lq, lk, dk, which=('offset', 'stair_up', 'allneg')):
            c = dict(c, bias=H.hard_bias(lq, lk, H._gen(lq, lk, 11)), blocked=None)
            assert lk < 20 or all((c['bias'] == val).any() for val in (100.0, -100.0, float('-inf')))
            (o64, p64), (o32, p32) = H.sdpa_ref(c, torch.float64), H.sdpa_ref(c, torch.float32)
            _finite_alike(p32, p64, c['name'])
            _finite_alike(o32, o64, c['name'])
            assert 4 * _gap(p32, p64) <= 1e-2 and 4 * _gap(o32, o64, c['oscale']) <= 1e-2, c['name']
        c = H.sigmoid_case(lq, lk, dk)
        (o64, p64), (o32, p32) = H.sigmoid_ref(c, torch.float64), H.sigmoid_ref(c, torch.float32)
        _finite_alike(p32, p64, 'sigmoid')
        _finite_alike(o32, o64, 'sigmoid')
        scale = torch.bmm(p64, c['v'].double().abs())
        assert 4 * _gap(p32, p64) <= 1e-2 and 4 * _gap(o32, o64, scale.clamp_min(1e-30)) <= 1e-2
        s = torch.bmm(c['q'].double(), c['k'].double().transpose(1, 2)) / dk ** 0.5
        for val in H.SIGMOID_SCORES[:lk]:
            assert bool(((s - val).abs() <= 1e-6 * abs(val)).any()), val
        r = p64.float()
        assert (r[c['blocked']] == 0).all()
        if lk >= len(H.SIGMOID_SCORES):
            assert (r == 1.0).any() and ((r == 0.0) & ~c['blocked']).any()
    P, dP = H.softmax_bwd_case()
    assert float(dP.abs().max()) > 1e5 and (P[0] == 1).sum() == 1 and (P[0] == 0).sum() == P.size(1) - 1
    assert ((P > 0) & (P < 2.0 ** -126)).any() and ((dP[:, 1:] * dP[:, :-1]) < 0).all()
    d64, d32 = H.softmax_bwd_ref(P, dP, 0.25, torch.float64), H.softmax_bwd_ref(P, dP, 0.25, torch.float32)
    _finite_alike(d32, d64, 'softmax_bwd')
    scale = 0.25 * (P.double() * dP.double()).abs().sum(-1, keepdim=True)
    assert float(4 * _gap(d32, d64, scale, per_row=True).max()) <= 1e-2
    assert (d64[0] == 0).all()          # a one-hot row: P (dP - dP) = 0 exactly
    P, dP = H.sigmoid_bwd_case()
    d64, d32 = H.sigmoid_bwd_ref(P, dP, 0.5, torch.float64), H.sigmoid_bwd_ref(P, dP, 0.5, torch.float32)
    _finite_alike(d32, d64, 'sigmoid_bwd')
    assert ((P == 0) | (P == 1)).float().mean() > 0.3 and (d64[(P == 0) | (P == 1)] == 0).all()
    assert 4 * _gap(d32, d64, (0.5 * dP.double()).abs()) <= 1e-2


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize('d', H.LN_DIMS)
def test_layernorm_families_meet_the_conditions(d):
    from lamp_amd import _native as N
    for family in H.LN_FAMILIES + ('mixed',):
        M = 67 if family == 'mixed' else 5
        c = H.ln_case(family, M, d)
        for p in (0.0, 0.3):
            keep = N.dropout_keep_mask(M * d, p, 77).view(M, d) if p else None
            r64, r32 = H.ln_ref(c, torch.float64, keep, p), H.ln_ref(c, torch.float32, keep, p)
            for name in ('y', 'dz', 'dx'):
                _finite_alike(r32[name], r64[name], family + ' ' + name)
                rows = _gap(r32[name], r64[name], r64[name].abs().amax(-1, keepdim=True).clamp_min(1e-300), per_row=True)
                worst = int(rows.argmax())
                print('d %4d p %.1f %-9s %-2s worst row gap32 / scale %.2e (a %s row)' % (d, p, family, name, float(rows.max()),
                                                                                         c['rows'][worst]))
                assert float(4 * rows.max()) <= 1e-2, (family, name, p, float(rows.max()))
            for name in ('dgamma', 'dbeta', 'dbias'):
                _finite_alike(r32[name], r64[name], family + ' ' + name)
                assert 4 * _gap(r32[name], r64[name], float(r64[name].abs().max())) <= 1e-2, (family, name, p)
            if family == 'near_1000':
                g = _gap(r32['y'], r64['y'])
                assert 1e-5 <= g <= 4e-3 and 2 < float(r64['y'].abs().max()) < 8, g      # about 1e-3 on outputs of scale about 3
            if family == 'constant':
                z = c['x'] + c['res']
                assert (z == 1024).all()
                if d & (d - 1) == 0:
                    run = torch.cumsum(z, 1)                                             # every partial sum is exact in fp32
                    assert torch.equal(run, 1024.0 * torch.arange(1, d + 1).float().expand(M, d))
                    assert torch.equal(r64['y'], c['beta'].double().expand(M, d)) and torch.equal(r32['y'], c['beta'].expand(M, d))
            if family == 'tiny':
                assert float(r64['y'].sub(c['beta'].double()).abs().max()) < 5e-3        # 3e-4 randn x gamma: eps is inside the root
    c = H.ln_case('mixed', 67, d)
    assert set(c['rows']) == set(H.LN_FAMILIES)
    # a row's result does not depend on its neighbours
    whole = H.ln_ref(c, torch.float64)['y']
    for i in (0, 1, 2, 3, 4, 66):
        one = {k: (v[i:i + 1] if k in ('x', 'res', 'dy') else v) for k, v in c.items()}
        assert torch.equal(H.ln_ref(one, torch.float64)['y'], whole[i:i + 1])


# ------------------------------------------------------------------ BCE, optimisers, GEMM
@pytest.mark.parametrize('B,L', H.BCE_SHAPES)
def test_bce_families_meet_the_conditions(B, L):
    seen = set()
    for n_mats in (1, 3):
        logits, weights, targets = H.bce_case(B, L, n_mats)
        for x in logits:
            seen |= {(float(a), float(t)) for a, t in zip(x.flatten(), targets.flatten())}
        p64, g64, r64 = H.bce_ref(logits, weights, targets, torch.float64)
        p32, g32, r32 = H.bce_ref(logits, weights, targets, torch.float32)
        for a32, a64, name in [(p32, p64, 'probs'), (r32.t(), r64.t(), 'rows')] + [(a, b, 'dlogits') for a, b in zip(g32, g64)]:
            _finite_alike(a32, a64, name)
            # a row's scale is no smaller than the smallest normal fp32 number: below it there is no relative precision to ask for
            rows = _gap(a32, a64, a64.abs().amax(-1, keepdim=True).clamp_min(2.0 ** -126), per_row=True)
            assert float(4 * rows.max()) <= 1e-2, (name, rows)
        sat = ((logits[0] >= 104) & (targets == 1)) | ((logits[0] <= -104) & (targets == 0))
        assert sat.any() and (g64[0].float()[sat] == 0).all()      # where the GPU test asserts an exact 0
    f32 = lambda x: float(torch.tensor(x))   # noqa: E731
    if L > 1:
        assert seen == {(f32(x), t) for x in H.BCE_LOGITS for t in H.BCE_TARGETS}
    else:
        assert {x for x, _ in seen} == {f32(x) for x in H.BCE_LOGITS}


@pytest.mark.parametrize('kind', ['zero', 'mixed', 'big_param'])
def test_optimiser_families_meet_the_conditions(kind):
    for n in H.OPTIM_SIZES:
        for step0 in (0, 999):
            p, grads = H.optim_case(kind, n, 10 if kind == 'zero' else 2)
            w64, w32 = H.adam_ref(p, grads, torch.float64, step0), H.adam_ref(p, grads, torch.float32, step0)
            for a32, a64, name in zip(w32, w64, ('p', 'm', 'v')):
                _finite_alike(a32, a64, name)
                assert 4 * _gap(a32, a64, a64.abs().clamp_min(1e-300)) <= 1e-2, (kind, n, name)     # elementwise relative
            if kind == 'zero':
                assert torch.equal(w32[0], p) and not w32[1].any() and not w32[2].any()
            if kind == 'mixed':
                g2 = grads[0].double() ** 2
                assert float(g2.min()) >= 2.0 ** -126 and float(g2.max()) < 3e38 and float(grads[0].abs().min()) < 1e-17
            if kind == 'big_param':
                assert torch.equal(w32[0], p) and float((w64[0] - p.double()).abs().max()) < 4.0     # below the ulp of 8 at 1e8
            s64, s32 = H.sgd_ref(p, grads, torch.float64), H.sgd_ref(p, grads, torch.float32)
            _finite_alike(s32, s64, 'sgd')


@pytest.mark.parametrize('family', H.GEMM_FAMILIES)
def test_gemm_families_meet_the_conditions(family):
    for M, N_, K in ((67, 72, 130), (1, 1, 4), (130, 132, 36)):
        A, W, bias, res = H.gemm_case(M, N_, K, family)
        for relu in (False, True):
            c64, adds = H.linear_ref(A, W, bias, res, relu, torch.float64)
            c32, _ = H.linear_ref(A, W, bias, res, relu, torch.float32)
            _finite_alike(c32, c64, family)
            bound = H.gemm_bound(A, W, K, adds)
            r = H.gemm_ratio(c32, c64, bound, family)
            print('%s %dx%dx%d relu %d: cpu fp32 err / bound %.3f' % (family, M, N_, K, relu, r))
            assert r <= 1.0            # the analytic bound holds for a plain fp32 product: it is no tighter than fp32 allows
    if family == 'scaled':
        A, W, _, _ = H.gemm_case(67, 72, 130, family)
        ra, rw = A.abs().amax(1), W.abs().amax(1)
        assert float(ra.max() / ra.min()) > 2.0 ** 40 and float(rw.max() / rw.min()) > 2.0 ** 40
    if family == 'cancel':
        A, W, _, _ = H.gemm_case(67, 72, 130, family)
        c64 = A.double() @ W.double().t()
        assert float((c64.abs() / (A.double().abs() @ W.double().abs().t())).max()) < 1e-2      # the products cancel


# ------------------------------------------------------------------ the families have teeth
def test_softmax_without_max_subtraction_is_caught():
    lq, lk, dk = 70, 33, 64
    c = H.attention_cases(lq, lk, dk, which=('offset',))[0]
    (o64, p64), (o32, p32) = H.sdpa_ref(c, torch.float64), H.sdpa_ref(c, torch.float32)
    o, p = H.sdpa_no_max_subtraction(c)
    assert _violates(p, p64, p32, H.FLOOR['attn_map']) and _violates(o, o64, o32, H.FLOOR['attn_out'], scale=c['oscale'])
    assert torch.isinf(p[0]).any() or torch.isnan(p[0]).any()          # +120 nats: exp overflows
    assert torch.isnan(p[1]).all()                                     # -120 nats: the row sum is 0
    c = H.randn_attention_case(lq, lk, dk)
    (o64, p64), (o32, p32) = H.sdpa_ref(c, torch.float64), H.sdpa_ref(c, torch.float32)
    o, p = H.sdpa_no_max_subtraction(c)
    assert not _violates(p, p64, p32, H.FLOOR['attn_map']) and not _violates(o, o64, o32, H.FLOOR['attn_out'], scale=c['oscale'])


def test_a_merge_that_forgets_the_common_maximum_is_caught():
    lq, lk, dk = 90, 302, 128
    hit = []
    for c in H.attention_cases(lq, lk, dk, which=('offset', 'allneg', 'disparity')):
        o64, o32 = H.sdpa_ref(c, torch.float64)[0], H.sdpa_ref(c, torch.float32)[0]
        good = H.sdpa_split_merge(c)[0]
        assert not _violates(good, o64, o32, H.FLOOR['attn_out'], scale=c['oscale']), c['name']     # the right merge passes
        if _violates(H.sdpa_split_merge(c, mutant=True)[0], o64, o32, H.FLOOR['attn_out'], scale=c['oscale']):
            hit.append(c['name'])
    print('merge mutant caught by:', hit)
    assert 'offset' in hit and 'allneg' in hit
    c = H.randn_attention_case(lq, lk, dk)
    o64, o32 = H.sdpa_ref(c, torch.float64)[0], H.sdpa_ref(c, torch.float32)[0]
    assert not _violates(H.sdpa_split_merge(c, mutant=True)[0], o64, o32, H.FLOOR['attn_out'], scale=c['oscale'])


@pytest.mark.parametrize('mutant,family', [(H.ln_one_pass_variance, 'near_1000'), (H.ln_one_pass_variance, 'near_-1e4'),
                                           (H.ln_eps_outside, 'tiny')])
def test_layernorm_mutants_are_caught(mutant, family):
    d = 512
    c = H.ln_case(family, 5, d)
    r64, r32 = H.ln_ref(c, torch.float64), H.ln_ref(c, torch.float32)
    bad = H.ln_ref(c, torch.float32, fn=mutant)
    scale = r64['y'].abs().amax(-1, keepdim=True)
    assert _violates(bad['y'], r64['y'], r32['y'], H.FLOOR['ln_fwd'], scale=scale, per_row=True)
    mixed = H.ln_case('mixed', 67, d)
    r64, r32 = H.ln_ref(mixed, torch.float64), H.ln_ref(mixed, torch.float32)
    assert _violates(H.ln_ref(mixed, torch.float32, fn=mutant)['y'], r64['y'], r32['y'], H.FLOOR['ln_fwd'],
                     scale=r64['y'].abs().amax(-1, keepdim=True), per_row=True)
    # test_layernorm's randn operands, its own form (2e-5 absolute).  The one-pass variance passes at every width.  eps outside
    # the root is off by 2.8e-6 |gamma xhat| there (std 3): 0.8e-5 at d = 4, 1.9e-5 at d = 64 -- inside the tolerance -- and
    # 2.4e-5 .. 3.4e-5 from d = 512 on, where the largest |gamma xhat| of 19000+ elements carries it 1.2 to 1.7 times past
    # 2e-5: seen by the margin of one element, against 20000 x the floor on the tiny family (an error of the size of y itself)
    for dd in (4, 64) if mutant is H.ln_eps_outside else (4, 64, 512, 2048):
        c = H.randn_ln_case(37, dd)
        r64, r32 = H.ln_ref(c, torch.float64), H.ln_ref(c, torch.float32)
        bad = H.ln_ref(c, torch.float32, fn=mutant)
        assert not _violates(bad['y'], r64['y'], r32['y'], H.FLOOR['ln_fwd']), dd
        assert not _violates(bad['dz'], r64['dz'], r32['dz'], H.FLOOR['ln_bwd']), dd
    c = H.randn_ln_case(37, 2048)
    r64, r32 = H.ln_ref(c, torch.float64), H.ln_ref(c, torch.float32)
    on_randn = H.ratio(H.ln_ref(c, torch.float32, fn=mutant)['y'], r64['y'], r32['y'], H.FLOOR['ln_fwd'])
    c = H.ln_case(family, 5, d)
    r64, r32 = H.ln_ref(c, torch.float64), H.ln_ref(c, torch.float32)
    try:
        on_hard = H.ratio(H.ln_ref(c, torch.float32, fn=mutant)['y'], r64['y'], r32['y'], H.FLOOR['ln_fwd'],
                          scale=r64['y'].abs().amax(-1, keepdim=True), per_row=True)
    except AssertionError:          # a negative one-pass variance: NaN rows
        on_hard = float('inf')
    print('%s: err / bound %.2f on randn rows (d = 2048), %.3g on %s rows' % (mutant.__name__, on_randn, on_hard, family))
    assert on_randn < 2.0 and on_hard > 10.0


def _bce_violations(logits, weights, targets, **mut):
    p64, g64, r64 = H.bce_ref(logits, weights, targets, torch.float64)
    p32, g32, r32 = H.bce_ref(logits, weights, targets, torch.float32)
    _, gm, rm = H.bce_ref(logits, weights, targets, torch.float32, **mut)
    rows = _violates(rm.t(), r64.t(), r32.t(), TC.ulp32(r64.t()), per_row=True)
    grads = any(_violates(a, b, c, TC.ulp32(b), per_row=True) for a, b, c in zip(gm, g64, g32))
    return rows, grads


def test_bce_mutants_are_caught():
    for B, L in H.BCE_SHAPES:
        case = H.bce_case(B, L, 3)
        assert _bce_violations(*case, softplus=H.softplus_naive)[0], (B, L)      # exp overflows from x = 89 on
    assert _bce_violations(*H.bce_case(5, 1, 3), sig_minus_t=H.sig_minus_t_naive)[1]   # sigmoid(20) - 1 cancels to 0
    assert _bce_violations(*H.bce_case(5, 1, 3)) == (False, False)
    for B, L, n_mats in TC.BCE_CASES:                                            # the existing test's randn cases
        logits, weights, targets = TC.bce_case(B, L, n_mats, seed=B * 1000 + L)
        p64, g64, r64 = TC.bce_reference(logits, weights, targets, torch.float64)
        p32, g32, r32 = TC.bce_reference(logits, weights, targets, torch.float32)
        _, gm, rm = H.bce_ref(logits, weights, targets, torch.float32, softplus=H.softplus_naive, sig_minus_t=H.sig_minus_t_naive,
                              seq=False)
        TC.within(rm, r64, TC.gap(r32, r64), 'naive softplus on randn logits')   # test_bce_kernel_against_fp64's own rule
        for k in range(n_mats):
            TC.within(gm[k], g64[k], TC.gap(g32[k], g64[k]), 'naive sigmoid - t on randn logits')
