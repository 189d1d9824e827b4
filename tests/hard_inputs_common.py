"""Extreme-magnitude and ill-conditioned inputs for the kernels: seeded generators, plain restatements of every operation that
run in fp64 and in fp32 on the CPU, CPU mutants of those restatements (the mistakes the randn tests cannot see), and the one
tolerance rule of tests/test_hard_inputs_cpu.py and tests/test_hard_inputs_gpu.py.  Importable without a GPU.

The rule (train_common.within and test_sharp_attention_at_real_width, applied everywhere):
  expected  the fp64 restatement on the SAME fp32 inputs;
  gap32     the distance of the CPU fp32 restatement from it -- per row where rows differ in magnitude (LayerNorm, BCE, the
            backward pieces), else per tensor;
  bound     max(floor x scale, 4 x gap32), floor being the absolute tolerance of the kernel's existing randn test (FLOOR below)
            and scale the size of the output (max|v| for an attention output, 1 for probabilities, sum_k P|v| where the issue
            says "relative to");
  GEMMs     analytic instead: K 2^-24 sum_k |a_k w_k| plus one fp32 ulp per epilogue add (2^-14 sum|a w| for 'high').
NaN positions must coincide and infinities must be equal; no element is left out of a comparison.

Scores are steered through ONE control coordinate (the last one): q[.., -1] = 1 and k[.., j, -1] = s_j sqrt(d_k), so key j's score
is s_j nats plus the randn part of the other coordinates.  The control coordinate is the last so that a kernel that accumulates
q.k in coordinate order rounds at the large magnitude once, as the exp2-domain arithmetic is what these families are after."""
import math

import torch
import torch.nn.functional as F

import train_common as TC
from label_bias_common import bias_sdpa
from oracle import lamp_ref as R
from sigmoid_common import sigmoid_sdpa

LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
LN_EPS = 1e-5

# absolute tolerances of the existing randn tests (tests/test_gpu_parity.py, test_gpu_backward.py, test_sigmoid_attn_gpu.py)
FLOOR = {
    'attn_out': 2e-5, 'attn_map': 5e-6,                  # test_sdpa_every_kernel_variant
    'sig_out': 1e-5, 'sig_map': 1e-6, 'sig_bwd': 1e-7,   # test_sigmoid_attn_gpu.py
    'softmax_bwd': 1e-5,                                 # test_softmax_bwd_vs_autograd
    'ln_fwd': 2e-5, 'ln_fwd_drop': 3e-5,                 # test_layernorm_residual_fwd_and_bwd_vs_autograd
    'ln_bwd': 3e-5, 'ln_bwd_drop': 5e-5, 'ln_dparam': 1e-4,
}

ATTN_SHAPES = [(5, 1, 16), (70, 33, 64), (260, 40, 24), (90, 302, 128)]   # (lq, lk, dk): one key | three tiles, ragged last |
#                                                       the 32-query kernels beyond 256 queries | four key shares, many tiles
STAIR_DELTAS = (31.0, 33.0, 200.0)   # log2 units: both sides of RESCALE_THR = 32, and far beyond exp2's range per step
N_SLICES = 2


# ------------------------------------------------------------------ the rule
def _f64(t):
    return t.detach().cpu().double()


def ratio(got, want64, ref32, floor, scale=1.0, per_row=False, extra=0.0, what=''):
    """-> worst |got - want64| / bound over every element, bound = scale x max(floor, 4 x gap32) + extra with gap32 =
    max |ref32 - want64| / scale over the tensor (per_row: over each last-dim row).  floor, scale and extra are numbers or
    tensors that broadcast.  NaNs must coincide and infinities be equal (asserted); those elements then count as exact."""
    got, want64, ref32 = _f64(got), _f64(want64), _f64(ref32)
    assert got.shape == want64.shape == ref32.shape, (what, got.shape, want64.shape, ref32.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(want64)), what + ': NaN positions differ'
    special = ~torch.isfinite(want64)
    assert torch.equal(got[special & ~torch.isnan(want64)], want64[special & ~torch.isnan(want64)]), what + ': infinities differ'
    scale = torch.as_tensor(scale, dtype=torch.float64).clamp_min(1e-300).expand_as(want64)
    err = torch.where(special, torch.zeros_like(got), (got - want64).abs()) / scale
    g = torch.where(special | ~torch.isfinite(ref32), torch.zeros_like(got), (ref32 - want64).abs()) / scale
    gap = g.amax(dim=-1, keepdim=True) if per_row else g.max() if g.numel() else g.sum()
    bound = torch.maximum(torch.as_tensor(floor, dtype=torch.float64).expand_as(want64), 4.0 * gap)
    bound = bound + torch.as_tensor(extra, dtype=torch.float64) / scale
    return float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0


def check(worst, what, got, want64, ref32, floor, **kw):
    """ratio(), printed in one line and asserted <= 1; `worst` (a dict) keeps the largest ratio per name."""
    r = ratio(got, want64, ref32, floor, what=what, **kw)
    print('%s: worst err / bound %.3f' % (what, r))
    key = what.split(' | ')[0]
    worst[key] = max(worst.get(key, 0.0), r)
    assert r <= 1.0, (what, r)
    return r


def exact_where_fp32_saturates(P, p64, what, ones=True):
    """Where the fp64 probability rounds to exactly 0 or (ones) exactly 1 in fp32, the kernel's must be that value bit for bit.
    ones=False for the single-pass maps, exp2(score - lse): lse carries a rounding at the magnitude of the scores by design."""
    P, r = P.detach().cpu(), p64.float()
    for val in (0.0, 1.0) if ones else (0.0,):
        at = r == val
        assert bool((P[at] == val).all()), (what, val, int((P[at] != val).sum()))


def gemm_bound(A, W, K, adds=()):
    """K 2^-24 sum_k |a_k w_k| per element (the form of test_matmul_precision_gpu._check with fp32's unit roundoff) plus one
    fp32 ulp at the result of each epilogue add in `adds` (fp64 tensors)."""
    b = K * 2.0 ** -24 * (A.double().abs() @ W.double().abs().t())
    for r in adds:
        b = b + TC.ulp32(r)
    return b


def gemm_ratio(got, want64, bound, what=''):
    got, want64 = _f64(got), _f64(want64)
    assert torch.isfinite(want64).all() and torch.isfinite(got).all(), what
    return float(((got - want64).abs() / bound.clamp_min(1e-300)).max())


# ------------------------------------------------------------------ softmax attention
def _gen(*seed):
    s = 0
    for v in seed:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def steer(lq, lk, dk, key_nats, g, noise=1.0):
    """q (N, lq, dk), k (N, lk, dk) whose scores q.k / sqrt(dk) are key_nats[n, j] plus noise^2 x (a randn score)."""
    q = noise * torch.randn(N_SLICES, lq, dk, generator=g)
    k = noise * torch.randn(N_SLICES, lk, dk, generator=g)
    q[..., -1] = 1.0
    k[..., -1] = (key_nats * dk ** 0.5).float()
    return q, k


def random_mask(lq, lk, g, dead_row=True):
    """About 40 % blocked, key 0 always allowed, one fully blocked row (NaN, as the reference) in slice 1."""
    m = torch.rand(N_SLICES, lq, lk, generator=g) < 0.4
    m[:, :, 0] = False
    if dead_row:
        m[1, lq // 2, :] = True
    return m


def stair_levels(lk, delta, up=True, tile=16):
    """log2 scores of a staircase over `tile`-key tiles: tile t's leader sits at delta * t (up) -- the LAST key leads the last
    tile, the first key of the tile every other one -- and everybody else one step (plus 1..4) below their leader, so each
    tile's maximum exceeds the previous one's by delta and the softmax is one-hot on the last key.  Down: the mirror image."""
    T = (lk + tile - 1) // tile
    j = torch.arange(lk)
    t = j // tile
    lev = delta * (t - 1).double() - (1.0 + 3.0 * torch.rand(lk, generator=torch.Generator().manual_seed(lk)).double())
    lead = t * tile
    lead[t == T - 1] = lk - 1
    lev[j == lead] = delta * t[j == lead].double()
    if not up:
        lev = lev.flip(0)
    return lev


def disparity(lk, tile, split, where):
    """-> (log2 levels [lk], blocked keys [lk], dominant key): tiles go round-robin to `split` key shares; the dominant key (0)
    lies in the first share (key 0) or in the last one (the last key of a tile t with t % split == split - 1, else the last key),
    every other key 300 log2 units below, and the share after the dominant one's is blocked completely."""
    t = torch.arange(lk) // tile
    share = t % split
    if where == 'first':
        dom = 0
    else:
        cand = (share == split - 1).nonzero().flatten()
        dom = int(cand[-1]) if cand.numel() else lk - 1
    lev = torch.full((lk,), -300.0, dtype=torch.float64)
    lev[dom] = 0.0
    blocked = share == (int(share[dom]) + 1) % split
    return lev, blocked, dom


def attention_cases(lq, lk, dk, dv=None, which=None):
    """The softmax families at one shape -> [dict(name, q, k, v, blocked, onehot, oscale)], N_SLICES slices each.  `blocked`
    is (N, lq, lk) bool or None; `onehot` the key every row must put exactly 1.0 on (or None); `oscale` the scale of the
    output bound: max|v|, or the tensor sum_k P|v| for the flat family."""
    dv = dv or dk
    out = []

    def add(name, q, k, v, blocked=None, onehot=None, oscale=None):
        if which is None or name.split('(')[0] in which:
            out.append(dict(name=name, q=q, k=k, v=v, blocked=blocked, onehot=onehot,
                            oscale=float(v.abs().max()) if oscale is None else oscale))

    g = _gen(lq, lk, dk, 1)
    v = torch.randn(N_SLICES, lk, dv, generator=g)
    # 1. offset: slice 0 shifted by +120 nats, slice 1 by -120
    nats = torch.tensor([120.0, -120.0]).view(2, 1).expand(2, lk)
    q, k = steer(lq, lk, dk, nats, g)
    add('offset', q, k, v, random_mask(lq, lk, g))
    # 2. / 3. staircases (both slices alike up to the randn part: 0.1 nats)
    for delta in STAIR_DELTAS:
        q, k = steer(lq, lk, dk, (stair_levels(lk, delta) * LN2).expand(2, lk), g, noise=0.3)
        add('stair_up(%g)' % delta, q, k, v, None, onehot=lk - 1)
    for delta in (33.0, 200.0):
        q, k = steer(lq, lk, dk, (stair_levels(lk, delta, up=False) * LN2).expand(2, lk), g, noise=0.3)
        add('stair_down(%g)' % delta, q, k, v, None, onehot=0)
    # 4. share disparity: 16- and 32-key tiles, 2 and 4 shares, the dominant key in the first and in the last share
    for tile in (16, 32):
        for split in (2, 4):
            for where in ('first', 'last'):
                lev, blk, dom = disparity(lk, tile, split, where)
                q, k = steer(lq, lk, dk, (lev * LN2).expand(2, lk), g, noise=0.3)
                add('disparity(t%d,s%d,%s)' % (tile, split, where), q, k, v, blk.view(1, 1, lk).expand(N_SLICES, lq, lk).clone(),
                    onehot=dom)
    # 5. flat: q = 0, P = 1 / lk, |v| over six decades across the keys
    k = torch.randn(N_SLICES, lk, dk, generator=g)
    dec = 10.0 ** (6.0 * torch.arange(lk).double() / max(lk - 1, 1) - 3.0)
    vf = (torch.randn(N_SLICES, lk, dv, generator=g).double() * dec.view(1, lk, 1)).float()
    add('flat', torch.zeros(N_SLICES, lq, dk), k, vf, None, oscale=vf.double().abs().mean(1, keepdim=True).expand(N_SLICES, lq, dv))
    # 6. all-negative: every allowed score near -300 nats
    q, k = steer(lq, lk, dk, torch.full((2, lk), -300.0), g)
    add('allneg', q, k, v, random_mask(lq, lk, g))
    return out


def randn_attention_case(lq, lk, dk):
    """The operands of test_sdpa_every_kernel_variant (the randn baseline every mutant must pass)."""
    g = _gen(lq, lk, dk, 2)
    q, k, v = (torch.randn(N_SLICES, l, dk, generator=g) for l in (lq, lk, lk))
    return dict(name='randn', q=q, k=k, v=v, blocked=random_mask(lq, lk, g), onehot=None, oscale=float(v.abs().max()))


def scores_log2(case, dtype=torch.float64):
    """The scaled scores in log2 units (blocked = -inf), (N, lq, lk)."""
    q, k = case['q'].to(dtype), case['k'].to(dtype)
    s = torch.bmm(q, k.transpose(1, 2)) / q.size(-1) ** 0.5 * LOG2E
    if case.get('bias') is not None:
        s = s + case['bias'].to(dtype) * LOG2E
    if case['blocked'] is not None:
        s = s.masked_fill(case['blocked'], float('-inf'))
    return s


def sdpa_ref(case, dtype):
    """oracle.lamp_ref.sdpa (label_bias_common.bias_sdpa with a bias) in `dtype` -> (out, maps)."""
    q, k, v = (case[n].to(dtype) for n in 'qkv')
    if case.get('bias') is not None:
        return bias_sdpa(q, k, v, case['bias'].to(dtype), case['blocked'])
    return R.sdpa(q, k, v, case['blocked'])


def lse_extra(case):
    """The single-pass (lse) route stores fp32 log2 scores and subtracts the row's fp32 log2-sum-exp: lse is rounded at the
    magnitude of the scores, up to ulp32(|s|_max) in the log2 domain, i.e. a relative ln2 ulp32(|s|_max) on every probability
    of the row (d/dx 2^x = ln2 2^x).  -> that term, (N, lq, lk); 0 where the row has no allowed key."""
    s = scores_log2(case)
    smax = torch.nan_to_num(s.masked_fill(torch.isinf(s), 0.0).abs().amax(-1, keepdim=True))
    p64 = case['p64'] if 'p64' in case else sdpa_ref(case, torch.float64)[1]
    return torch.nan_to_num(LN2 * TC.ulp32(smax) * p64)


def hard_bias(lq, lk, g):
    """A score bias N(0, 1) with entries of +100, -100 and -inf (about 10 % each); key 0 stays finite in every row."""
    b = torch.randn(lq, lk, generator=g)
    u = torch.rand(lq, lk, generator=g)
    b[u < 0.1] = 100.0
    b[(u >= 0.1) & (u < 0.2)] = -100.0
    b[(u >= 0.2) & (u < 0.3)] = float('-inf')
    b[:, 0] = 0.5
    return b


# ---- mutants (fp32, CPU)
def sdpa_no_max_subtraction(case):
    """softmax as exp(s) / sum exp(s)."""
    q, k, v = case['q'], case['k'], case['v']
    s = torch.bmm(q, k.transpose(1, 2)) / q.size(-1) ** 0.5
    if case['blocked'] is not None:
        s = s.masked_fill(case['blocked'], float('-inf'))
    e = torch.exp(s)
    p = e / e.sum(-1, keepdim=True)
    return torch.bmm(p, v), p


def sdpa_split_merge(case, split=4, tile=16, mutant=False):
    """Online softmax over `split` round-robin key shares, merged by weights exp(m_share - m_all); mutant: exp(m_share)."""
    q, k, v = case['q'], case['k'], case['v']
    s = torch.bmm(q, k.transpose(1, 2)) / q.size(-1) ** 0.5
    if case['blocked'] is not None:
        s = s.masked_fill(case['blocked'], float('-inf'))
    share = (torch.arange(s.size(-1)) // tile) % split
    ms, ls, os_ = [], [], []
    for i in range(split):
        si = s[..., share == i]
        if si.size(-1) == 0:
            continue
        m = si.amax(-1, keepdim=True)
        mu = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        e = torch.exp(si - mu)
        ms.append(m)
        ls.append(e.sum(-1, keepdim=True))
        os_.append(torch.bmm(e, v[:, share == i]))
    m_all = torch.stack(ms).amax(0)
    mu = torch.where(torch.isinf(m_all), torch.zeros_like(m_all), m_all)
    w = [torch.exp(m) if mutant else torch.exp(m - mu) for m in ms]
    l = sum(li * wi for li, wi in zip(ls, w))
    return sum(oi * wi for oi, wi in zip(os_, w)) / l, None


# ------------------------------------------------------------------ sigmoid attention
SIGMOID_SCORES = (0.0, 1e-6, -1e-6, 20.0, -20.0, 88.0, -88.0, 130.0, -130.0, 1e4, -1e4)


def sigmoid_case(lq, lk, dk):
    """q = +-e_last (the sign alternates over the queries), k's control coordinate walks SIGMOID_SCORES: the scores are those
    values up to one rounding.  About 30 % of the keys blocked."""
    g = _gen(lq, lk, dk, 3)
    q = torch.zeros(N_SLICES, lq, dk)
    q[..., -1] = torch.where(torch.arange(lq) % 2 == 0, 1.0, -1.0)
    k = torch.randn(N_SLICES, lk, dk, generator=g)
    vals = torch.tensor(SIGMOID_SCORES, dtype=torch.float64)[(torch.arange(lk) + 3 * torch.arange(N_SLICES).view(-1, 1)) % len(SIGMOID_SCORES)]
    k[..., -1] = (vals * dk ** 0.5).float()
    v = torch.randn(N_SLICES, lk, dk, generator=g)
    return dict(name='sigmoid', q=q, k=k, v=v, blocked=torch.rand(N_SLICES, lq, lk, generator=g) < 0.3)


def sigmoid_ref(case, dtype):
    return sigmoid_sdpa(case['q'].to(dtype), case['k'].to(dtype), case['v'].to(dtype), case['blocked'])


# ------------------------------------------------------------------ attention backward pieces
def softmax_bwd_ref(P, dP, scale, dtype):
    """dS = scale P (dP - sum_k P dP)."""
    P, dP = P.to(dtype), dP.to(dtype)
    return scale * P * (dP - (P * dP).sum(-1, keepdim=True))


def sigmoid_bwd_ref(P, dP, scale, dtype):
    P, dP = P.to(dtype), dP.to(dtype)
    return scale * P * (1 - P) * dP


def softmax_bwd_case(rows=37, lk=70):
    """fp32 P rows: exactly one-hot; one-hot beside fp32-denormal probabilities; ordinary softmax rows.  |dP| up to 1e6 with
    alternating sign.  -> (P, dP)."""
    g = _gen(rows, lk, 4)
    P = torch.softmax(3.0 * torch.randn(rows, lk, generator=g).double(), -1).float()
    for r in range(0, rows, 3):
        P[r] = 0.0
        P[r, (7 * r) % lk] = 1.0
    for r in range(1, rows, 3):
        P[r] = 1e-40 * (1 + torch.arange(lk))
        P[r, (5 * r) % lk] = 1.0
    dP = torch.randn(rows, lk, generator=g) * 10.0 ** (6.0 * torch.rand(rows, 1, generator=g))
    dP = dP.abs() * torch.where(torch.arange(lk) % 2 == 0, 1.0, -1.0)
    return P, dP


def sigmoid_bwd_case(rows=37, lk=70):
    g = _gen(rows, lk, 5)
    P = torch.sigmoid(4.0 * torch.randn(rows, lk, generator=g))
    u = torch.rand(rows, lk, generator=g)
    P[u < 0.2] = 0.0
    P[u > 0.8] = 1.0
    P[0, :4] = torch.tensor([1e-40, 1 - 2.0 ** -24, 2.0 ** -24, 0.5])
    dP = torch.randn(rows, lk, generator=g) * 10.0 ** (6.0 * torch.rand(rows, 1, generator=g))
    dP = dP.abs() * torch.where(torch.arange(lk) % 2 == 0, 1.0, -1.0)
    return P, dP


# ------------------------------------------------------------------ LayerNorm
LN_FAMILIES = ('near_1000', 'near_-1e4', 'tiny', 'huge', 'constant')
LN_DIMS = (36, 64, 512, 4096)


def ln_rows(family, M, d, g):
    """(x, residual) rows of one family: the offset lives in the residual and the spread in x, so the row keeps its family's
    conditioning when dropout thins x."""
    r = torch.randn(M, d, generator=g)
    if family == 'near_1000':      # mean 1000, std 0.1: a one-pass fp32 variance is negative here
        return 0.1 * r, torch.full((M, d), 1000.0)
    if family == 'near_-1e4':
        return r, torch.full((M, d), -1e4)
    if family == 'tiny':           # variance 1e-12 << eps: y is 3e-4 randn with eps inside the root, O(1) with eps outside
        return 1e-6 * r, torch.zeros(M, d)
    if family == 'huge':           # squares stay finite (1e30 x a few)
        return 1e15 * r, 1e15 * torch.randn(M, d, generator=g)
    if family == 'constant':       # every sum is exact in any order when d is a power of two: y == beta bit for bit
        return torch.zeros(M, d), torch.full((M, d), 1024.0)
    raise KeyError(family)


def ln_case(family, M, d):
    """-> dict(x, res, gamma, beta, dy, rows): family 'mixed' takes its rows from every family in turn (rows[i] names row i's)."""
    g = _gen(M, d, 6, LN_FAMILIES.index(family) if family in LN_FAMILIES else 9)
    if family == 'mixed':
        fams = [LN_FAMILIES[i % len(LN_FAMILIES)] for i in range(M)]
        parts = [ln_rows(f, 1, d, g) for f in fams]
        x, res = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    else:
        fams = [family] * M
        x, res = ln_rows(family, M, d, g)
    return dict(x=x, res=res, gamma=1 + 0.3 * torch.randn(d, generator=g), beta=0.1 * torch.randn(d, generator=g),
                dy=torch.randn(M, d, generator=g), rows=fams)


def ln_input(case, dtype, keep=None, p=0.0):
    x, res = case['x'].to(dtype), case['res'].to(dtype)
    return (x * keep / (1 - p) if keep is not None else x), res


def ln_ref(case, dtype, keep=None, p=0.0, fn=None):
    """y and the gradients (dz of the residual branch, dx, dgamma, dbeta) of y = LayerNorm(dropout(x) + res) by autograd in
    `dtype`.  fn: a replacement for the normalisation (the mutants)."""
    x, res, gm, bt = (case[n].detach().to(dtype).clone().requires_grad_() for n in ('x', 'res', 'gamma', 'beta'))
    z = (x * keep / (1 - p) if keep is not None else x) + res
    y = F.layer_norm(z, (z.size(-1),), gm, bt, LN_EPS) if fn is None else fn(z, gm, bt)
    y.backward(case['dy'].to(dtype))
    return dict(y=y.detach(), dz=res.grad, dx=x.grad, dgamma=gm.grad, dbeta=bt.grad, dbias=x.grad.sum(0))


def ln_one_pass_variance(z, gm, bt):
    """mutant: var = E[z^2] - E[z]^2."""
    mean = z.mean(-1, keepdim=True)
    var = (z * z).mean(-1, keepdim=True) - mean * mean
    return (z - mean) / torch.sqrt(var + LN_EPS) * gm + bt


def ln_eps_outside(z, gm, bt):
    """mutant: (z - mean) / (std + eps)."""
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    return (z - mean) / (torch.sqrt(var) + LN_EPS) * gm + bt


def randn_ln_case(M, d):
    """The operands of test_gpu_parity.test_layernorm (rows of 3 randn + 1), with a zero residual."""
    g = _gen(M, d, 7)
    return dict(x=torch.randn(M, d, generator=g) * 3 + 1, res=torch.zeros(M, d), gamma=torch.randn(d, generator=g),
                beta=torch.randn(d, generator=g), dy=torch.randn(M, d, generator=g), rows=['randn'] * M)


# ------------------------------------------------------------------ BCE
BCE_LOGITS = (0.0, 1e-8, -1e-8, 20.0, -20.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4)
BCE_MAGS = (0.0, 1e-8, 20.0, 87.0, 89.0, 104.0, 1e4)
BCE_TARGETS = (0.0, 1.0, 0.5)
BCE_SHAPES = [(7, 37), (5, 1)]
# the (5, 1) case: one target per row, shared by the matrices.  A row is its own yardstick here, so the pairs are those whose
# result is an fp32 normal number or rounds to exactly 0 (a relative gap32 means nothing on a denormal; +-87 and +-89 next to
# the saturating target, which give denormal gradients, are in the rows of the (7, 37) case)
BCE_SINGLE_TARGETS = (1.0, 1.0, 0.0, 1.0, 0.0)
BCE_SINGLES = ((20.0, 1e4, -104.0, 104.0, 1e-8),     # sigmoid(x) - 1 cancels | exactly 0 | rounds to 0 | rounds to 0 | 0.5
               (-20.0, -1e4, -20.0, -89.0, 89.0),    # -1 | loss 1e4 | 2e-9 | loss 89 | loss 89
               (-87.0, 0.0, 87.0, -1e-8, -1e4))


def bce_case(B, L, n_mats):
    """-> (logits [n_mats], weights, targets).  L > 1: row b of matrix k holds ONE magnitude, BCE_MAGS[(b + k) % 7] (rows differ
    in magnitude, so each row is judged by its own gap32), column j its sign (+ for even j) and the target BCE_TARGETS[(j // 2)
    % 3]: with L >= 6 every (logit, target) pair occurs.  L == 1 (each element its own row, judged by its own gap32): the pairs
    where a naive formula cancels or overflows, BCE_SINGLES."""
    idx = torch.arange(B * L).view(B, L)
    if L > 1:
        j = torch.arange(L)
        targets = torch.tensor(BCE_TARGETS)[(j // 2) % 3].expand(B, L).clone()
        sign = torch.where(j % 2 == 0, 1.0, -1.0)
        logits = [(torch.tensor(BCE_MAGS)[(torch.arange(B) + k) % len(BCE_MAGS)].view(B, 1) * sign).contiguous() for k in range(n_mats)]
    else:
        targets = torch.tensor(BCE_SINGLE_TARGETS)[idx % len(BCE_SINGLE_TARGETS)]
        logits = [torch.tensor(BCE_SINGLES[k])[idx % len(BCE_SINGLES[k])] for k in range(n_mats)]
    return logits, [1.0, 0.2, 0.5][:n_mats], targets


def _seq_sum(t):
    """Row sums in plain left-to-right order (the fp32 restatement's: no pairwise tree)."""
    acc = torch.zeros_like(t[:, 0])
    for j in range(t.size(1)):
        acc = acc + t[:, j]
    return acc


def bce_ref(logits, weights, targets, dtype, softplus=None, sig_minus_t=None, seq=True):
    """-> (probs of matrix 0, [dlogits_k], row_loss (n_mats, B)) in `dtype`: sigmoid; (1 - t) sigmoid(x) - t sigmoid(-x) times
    w_k / (B L) (sigmoid(x) - t without its cancellation next to t = 1); max(x, 0) - x t + log1p(exp(-|x|)) summed per row, left
    to right (seq=False: torch's own sum, as train_common.bce_reference).  softplus / sig_minus_t: replacements (the mutants)."""
    t = targets.to(dtype)
    B, L = t.shape
    probs, grads, rows = None, [], []
    for k, (x, w) in enumerate(zip(logits, weights)):
        x = x.to(dtype)
        if k == 0:
            probs = torch.sigmoid(x)
        d = (1 - t) * torch.sigmoid(x) - t * torch.sigmoid(-x) if sig_minus_t is None else sig_minus_t(x, t)
        grads.append(d * (torch.tensor(w, dtype=dtype) / (B * L)))
        if softplus is None:
            terms = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
        else:
            terms = softplus(x) - x * t
        rows.append(_seq_sum(terms) if seq else terms.sum(1))
    return probs, grads, torch.stack(rows)


def softplus_naive(x):
    """mutant: log(1 + exp(x))."""
    return torch.log(1 + torch.exp(x))


def sig_minus_t_naive(x, t):
    """mutant: 1 / (1 + exp(-x)) - t, nothing guarding exp's overflow or the cancellation."""
    return 1 / (1 + torch.exp(-x)) - t


# ------------------------------------------------------------------ Adam / SGD
OPTIM_SIZES = (1, 4099, 8192 + 3)
ADAM_HP = dict(lr=2e-3, beta1=0.9, beta2=0.98, eps=1e-8)


def optim_case(kind, n, n_steps):
    """-> (param, [grad per step]).  kind: 'zero' (gradients exactly 0), 'mixed' (|g| in {1e-18, 1e-6, 1, 1e6, 1e18} side by
    side, signs alternating, another draw every step), 'big_param' (|p| = 1e8, updates below its ulp of 8)."""
    g = _gen(n, n_steps, 8, len(kind))
    p = torch.randn(n, generator=g)
    if kind == 'zero':
        grads = [torch.zeros(n) for _ in range(n_steps)]
    elif kind == 'mixed':
        mags = torch.tensor([1e-18, 1e-6, 1.0, 1e6, 1e18])
        grads = [mags[(torch.arange(n) + s) % 5] * (1 + torch.rand(n, generator=g)) * torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0)
                 for s in range(n_steps)]
    elif kind == 'big_param':
        p = 1e8 * torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0) * (1 + torch.rand(n, generator=g))
        grads = [torch.randn(n, generator=g) for _ in range(n_steps)]
    else:
        raise KeyError(kind)
    return p, grads


def adam_ref(p, grads, dtype, step0=0, m=None, v=None, lr=ADAM_HP['lr'], beta1=ADAM_HP['beta1'], beta2=ADAM_HP['beta2'],
             eps=ADAM_HP['eps']):
    """torch.optim.Adam's update (no weight decay, no amsgrad) in `dtype`, the scalar factors in Python doubles; the first
    gradient is step step0 + 1.  -> (p, m, v)."""
    p = p.to(dtype).clone()
    m = torch.zeros_like(p) if m is None else m.to(dtype).clone()
    v = torch.zeros_like(p) if v is None else v.to(dtype).clone()
    for i, gr in enumerate(grads):
        gr = gr.to(dtype)
        step = step0 + i + 1
        m = m + (gr - m) * (1 - beta1)
        v = v * beta2 + (1 - beta2) * gr * gr
        denom = v.sqrt() / (1 - beta2 ** step) ** 0.5 + eps
        p = p - lr / (1 - beta1 ** step) * (m / denom)
    return p, m, v


def sgd_ref(p, grads, dtype, lr=0.05):
    p = p.to(dtype).clone()
    for gr in grads:
        p = p - lr * gr.to(dtype)
    return p


# ------------------------------------------------------------------ GEMM
def gemm_case(M, N, K, family, seed=0):
    """-> (A [M, K], W [N, K], bias [N] or None, residual [M, N] or None).
    'scaled': rows of A and of W scaled by powers of two from 2^-40 to 2^40 (the bound is per element);
    'cancel': A rows [b, -b, small ...] with b = 2^20 against W rows whose first two entries are equal;
    'epi_big' / 'epi_small': bias and residual 2^20 times larger / smaller than the product."""
    g = _gen(M, N, K, 10, seed)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias = res = None
    if family == 'scaled':
        A = A * 2.0 ** torch.randint(-40, 41, (M, 1), generator=g).float()
        W = W * 2.0 ** torch.randint(-40, 41, (N, 1), generator=g).float()
    elif family == 'cancel':
        A[:, 0] = 2.0 ** 20
        if K > 1:
            A[:, 1] = -2.0 ** 20
            W[:, 1] = W[:, 0]
    elif family in ('epi_big', 'epi_small'):
        f = 2.0 ** 20 if family == 'epi_big' else 2.0 ** -20
        bias = torch.randn(N, generator=g) * f * K ** 0.5
        res = torch.randn(M, N, generator=g) * f * K ** 0.5
    else:
        raise KeyError(family)
    return A, W, bias, res


GEMM_FAMILIES = ('scaled', 'cancel', 'epi_big', 'epi_small')


def linear_ref(A, W, bias, res, relu, dtype):
    """-> (result, [the fp64-meaningful intermediate after each epilogue add]) of relu(A W^T + bias) + res in `dtype`."""
    c = A.to(dtype) @ W.to(dtype).t()
    adds = []
    if bias is not None:
        c = c + bias.to(dtype)
        adds.append(c)
    if relu:
        c = c.clamp(min=0)
    if res is not None:
        c = c + res.to(dtype)
        adds.append(c)
    return c, adds
