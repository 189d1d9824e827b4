"""Shared pieces of the kernel-level tests of the one-hot front end (csrc/conv.hip): fp64 restatements of its five entry points
written as index arithmetic from the formulas of include/lamp_hip.h ("the one-hot genomics encoder", "Building blocks"), the
a-priori error bounds, the decision margins of the backward, and the inputs that the CPU and the GPU file share.  Nothing here
calls the library (front_keep takes the dropout counter from lamp_amd._native.dropout_keep_mask, which is torch integer
arithmetic only).

Tolerance: an fp32 sum of n terms in any order is within (n + 2) * 2^-24 * mag of the exact sum, mag = the sum of the terms'
magnitudes taken from the fp64 restatement.  conv_window: n = 16 c_in (bias and position row counted into mag); front end: n =
17 (16 taps and the bias); dt1: n = contributing rows + chunks.  Selections, copies and the padding are exact.  A max and a
ReLU are 1-Lipschitz, so the bound of a pooled value is the larger bound of its pair."""
import torch

U = 2.0 ** -24
TAPS = 16
NAN = float('nan')


def sum_bound(n, mag):
    return (n + 2) * U * mag


# ---------------------------------------------------------------- front end, forward
def window_tokens(seq, ps=None):
    """[B, P, 16] int64: the token under tap t of position ps[i], seq[b, ps[i] + t - 8], or -1 outside [0, T)."""
    B, T = seq.shape
    ps = torch.arange(T) if ps is None else ps
    j = ps[:, None] + torch.arange(TAPS)[None, :] - 8            # [P, 16]
    inside = (j >= 0) & (j < T)
    tok = seq[:, j.clamp(0, T - 1).reshape(-1)].view(B, ps.numel(), TAPS)
    return torch.where(inside[None], tok, torch.full_like(tok, -1)), inside


def front_y1(seq, t1, b1, ps=None):
    """fp64 y1[b, p, :] = b1 + sum_{t < 16, 0 <= p + t - 8 < T} t1[seq[b, p + t - 8], t, :] at the positions ps (all of them
    by default), summed in the order t = 0 .. 15, so equal windows give equal bits.  -> (y1 with NaN where the window holds a
    token outside [0, n_vocab), mag = |b1| + sum |t1[..]|, window tokens)."""
    V, _, d = t1.shape
    win, inside = window_tokens(seq, ps)
    B, P, _ = win.shape
    y = b1.view(1, 1, d).expand(B, P, d).clone()
    mag = b1.abs().view(1, 1, d).expand(B, P, d).clone()
    bad = torch.zeros(B, P, dtype=torch.bool)
    for t in range(TAPS):
        tok = win[:, :, t]
        live = inside[None, :, t].expand(B, P)
        ok = live & (tok >= 0) & (tok < V)
        bad |= live & ~ok
        term = t1[tok.clamp(0, V - 1), t, :] * ok[:, :, None].to(t1.dtype)     # + 0.0 is exact
        y = y + term
        mag = mag + term.abs()
    y = torch.where(bad[:, :, None], torch.full_like(y, NAN), y)
    return y, mag, win


def relu_nan(y):
    """The ReLU that lets a NaN through (torch.relu's)."""
    return torch.where((y > 0) | torch.isnan(y), y, torch.zeros_like(y))


def pair_max(a0, a1):
    """max_pool1d's choice: the first element wins ties, a NaN is propagated."""
    return torch.where((a1 > a0) | torch.isnan(a1), a1, a0)


def dropped(y, keep, scale):
    """Dropout as the library applies it: kept elements times scale, the others exactly 0 (a dropped NaN too)."""
    if keep is None:
        return y
    return torch.where(keep, y * scale, torch.zeros_like(y))


def front_pairs(seq, t1, b1, keep=None, scale=1, qs=None):
    """The pooled pairs q (all T // 2 by default): dict of z0 / z1 = dropout(y1) of the pair's two positions (pre-ReLU), their
    a-priori bounds e0 / e1 (0 where dropped: a dropped element is exact), a0 / a1 = relu, P = the pair max, bound = max(e0, e1),
    same = the two positions have the same token window and keep state (then z0 == z1 bit for bit in any precision)."""
    B, T = seq.shape
    T2 = T // 2
    qs = torch.arange(T2) if qs is None else qs
    ps = torch.stack([2 * qs, 2 * qs + 1], 1).reshape(-1)
    y, mag, win = front_y1(seq, t1, b1, ps)
    e = sum_bound(17, mag) * scale
    if keep is not None:
        k = keep[:, ps, :]
        y = dropped(y, k, scale)
        e = torch.where(k, e, torch.zeros_like(e))
        k0, k1 = k[:, 0::2], k[:, 1::2]
        same_keep = k0 == k1
    else:
        same_keep = True
    z0, z1 = y[:, 0::2], y[:, 1::2]
    a0, a1 = relu_nan(z0), relu_nan(z1)
    same = (win[:, 0::2] == win[:, 1::2]).all(-1)[:, :, None] & same_keep
    e0, e1 = e[:, 0::2], e[:, 1::2]
    return dict(z0=z0, z1=z1, e0=e0, e1=e1, a0=a0, a1=a1, P=pair_max(a0, a1), bound=torch.maximum(e0, e1), same=same)


def to_xpad(P):
    """[B, T2, d] -> the xpad layout [B * (T2 + 16) + 16, d]: row b * (T2 + 16) + 8 + q = P[b, q], zeros in every other row."""
    B, T2, d = P.shape
    x = torch.zeros(B, T2 + 16, d, dtype=P.dtype)
    x[:, 8:8 + T2] = P
    return torch.cat([x.view(-1, d), torch.zeros(16, d, dtype=P.dtype)], 0)


def xpad_data_rows(B, T2):
    """Row indices of the data rows of an xpad, in (b, q) order."""
    return (torch.arange(B)[:, None] * (T2 + 16) + 8 + torch.arange(T2)[None, :]).reshape(-1)


def front_ref(seq, t1, b1, keep=None, scale=1):
    """lamp_onehot_front_fwd in fp64: the xpad of P = pair max of relu(dropout(y1)); an odd T drops its last position."""
    return to_xpad(front_pairs(seq, t1, b1, keep, scale)['P'])


# ---------------------------------------------------------------- conv_window
def conv_window_ref(x, B, rows_out, rows_in, w_pack, bias=None, relu=False, pos_table=None, src_pos=None):
    """lamp_conv_window_fwd in fp64: v[b * rows_out + q][n] = sum_{t, ci} x[b * rows_in + q + t][ci] w_pack[n][t][ci] + bias[n],
    relu_out = act(v), out = relu_out + pos_table[src_pos[b][q]] (a NaN row where that index is outside the table).
    -> (out, relu_out, mag = sum |x w| + |bias| (+ |position row| for out only, returned as mag_out))."""
    c_out, taps, c_in = w_pack.shape
    m = torch.arange(B * rows_out)
    b, q = m // rows_out, m % rows_out
    v = torch.zeros(B * rows_out, c_out, dtype=torch.float64)
    mag = torch.zeros_like(v)
    for t in range(taps):
        xr = x[b * rows_in + q + t]                                # [M, c_in]
        v = v + xr @ w_pack[:, t, :].t()
        mag = mag + xr.abs() @ w_pack[:, t, :].abs().t()
    if bias is not None:
        v = v + bias
        mag = mag + bias.abs()
    act = torch.where(v > 0, v, torch.zeros_like(v)) if relu else v
    out, mag_out = act, mag
    if pos_table is not None:
        ps = src_pos[b, q]
        ok = (ps >= 0) & (ps < pos_table.size(0))
        row = pos_table[ps.clamp(0, pos_table.size(0) - 1)]
        out = torch.where(ok[:, None], act + row, torch.full_like(act, NAN))
        mag_out = mag + row.abs()
    return out, act, mag, mag_out


def relu_bwd_pad_ref(dy, relu_out, B, rows):
    """lamp_conv_relu_bwd_pad: dy * (relu_out > 0) in the xpad layout (pure selection, any dtype)."""
    d = dy.size(-1)
    g = torch.where(relu_out > 0, dy, torch.zeros_like(dy))
    return to_xpad(g.view(B, rows, d))


def conv_pack_ref(w, flip):
    """lamp_conv_pack: flip 0: packed[co][t][ci] = w[co][ci][t]; flip 1: packed[ci][t][co] = w[co][ci][taps - 1 - t]."""
    c_out, c_in, taps = w.shape
    if not flip:
        co, t, ci = torch.meshgrid(torch.arange(c_out), torch.arange(taps), torch.arange(c_in), indexing='ij')
        return w[co, ci, t]
    ci, t, co = torch.meshgrid(torch.arange(c_in), torch.arange(taps), torch.arange(c_out), indexing='ij')
    return w[co, ci, taps - 1 - t]


def conv_input_grad_ref(dy, relu_out, w, B, T2):
    """The fp64 gradient of conv2's input P [B, T2, c_in] from dy [B * T2, c_out], for X = relu(conv2(P)[:, :, :T2]) with
    Conv1d(c_in, c_out, 16, padding 8) weights w [c_out, c_in, 16]: X[q] reads P[q + t - 8] under tap t, so
    dP[b][r][ci] = sum_{t, co, 0 <= r - t + 8 < T2} dZ[b][r - t + 8][co] w[co][ci][t], dZ = dy * (relu_out > 0).
    -> (dP [B * T2, c_in], mag = sum |dZ w|)."""
    c_out, c_in, taps = w.shape
    dz = torch.where(relu_out > 0, dy, torch.zeros_like(dy)).view(B, T2, c_out)
    dP = torch.zeros(B, T2, c_in, dtype=torch.float64)
    mag = torch.zeros_like(dP)
    for t in range(taps):
        for r in range(T2):
            q = r - t + 8
            if 0 <= q < T2:
                dP[:, r] += dz[:, q] @ w[:, :, t]
                mag[:, r] += dz[:, q].abs() @ w[:, :, t].abs()
    return dP.view(B * T2, c_in), mag.view(B * T2, c_in)


# ---------------------------------------------------------------- front end, backward
DT1_ROWS = 256   # rows of one partial sum of the tap-table gradient (csrc/conv.hip)


def front_bwd_ref(seq, t1, b1, dP, keep=None, scale=1):
    """lamp_onehot_front_bwd in fp64 from dP [B, T2, d].  dz [B, T, d]: the pair's winner (the first on a tie) takes dP where
    its activation is > 0, times scale under dropout; everything else, and the last position of an odd T, is 0.
    dt1[v][t][c] = sum over (b, p) with seq[b][p + t - 8] == v of dz[b][p][c].
    -> dict(dz, dt1, dt1_mag = the same sum over |dz|, dt1_n = its number of rows + the number of 256-row chunks,
            unsafe [B, T, d] = the elements whose decision an fp32 rounding may flip (see front_unsafe))."""
    B, T = seq.shape
    V, _, d = t1.shape
    T2 = T // 2
    fp = front_pairs(seq, t1, b1, keep, scale)
    a0, a1 = fp['a0'], fp['a1']
    win0 = ~((a1 > a0) | torch.isnan(a1))
    up = dP * scale if keep is not None else dP
    zero = torch.zeros_like(up)
    dz = torch.zeros(B, T, d, dtype=torch.float64)
    dz[:, 0:2 * T2:2] = torch.where(win0 & (a0 > 0), up, zero)
    dz[:, 1:2 * T2:2] = torch.where(~win0 & (a1 > 0), up, zero)
    win, inside = window_tokens(seq)
    dt1 = torch.zeros(V, TAPS, d, dtype=torch.float64)
    mag = torch.zeros_like(dt1)
    cnt = torch.zeros(V, TAPS)
    for t in range(TAPS):
        for v in range(V):
            hit = win[:, :, t] == v                                  # [B, T]
            dt1[v, t] = dz[hit].sum(0)
            mag[v, t] = dz[hit].abs().sum(0)
            cnt[v, t] = float(hit.sum())
    chunks = (B * T + DT1_ROWS - 1) // DT1_ROWS
    unsafe = torch.zeros(B, T, d, dtype=torch.bool)
    u = front_unsafe(fp)
    unsafe[:, 0:2 * T2:2] = u
    unsafe[:, 1:2 * T2:2] = u
    return dict(dz=dz, dt1=dt1, dt1_mag=mag, dt1_n=(cnt + chunks)[:, :, None], unsafe=unsafe, pairs=fp)


def front_unsafe(fp):
    """Per pair and channel: may fp32 rounding change who takes the gradient?  The margins are |a0 - a1| for the pool and |z| of
    the pair's winner for the ReLU (a loser's gradient is 0 whatever its sign); a margin below twice its a-priori bound leaves
    the pair out.  An exact tie of two equal windows is a tie in any precision and stays in, as does a pair of two dropped
    elements (both exactly 0).  NaN pairs (invalid tokens) give 0 in any precision."""
    z0, z1, a0, a1, e0, e1 = fp['z0'], fp['z1'], fp['a0'], fp['a1'], fp['e0'], fp['e1']
    nan = torch.isnan(z0) | torch.isnan(z1)
    pool_margin = (a0 - a1).abs()
    exact_tie = (fp['same'] & (z0 == z1)) | ((e0 == 0) & (e1 == 0))
    pool_unsafe = (pool_margin < 2 * fp['bound']) & ~exact_tie
    win0 = ~(a1 > a0)
    zw = torch.where(win0, z0, z1)
    ew = torch.where(win0, e0, e1)
    relu_unsafe = zw.abs() < 2 * ew            # ew = 0 (dropped winner): never
    # a pool that could go either way between two values that are both clearly <= 0 still gives 0 to both
    both_off = (z0 <= -2 * e0) & (z1 <= -2 * e1)
    return ~nan & ~both_off & (pool_unsafe | relu_unsafe)


def front_bwd_fp32(seq, t1, b1, dP, keep=None, scale=1):
    """The backward's decisions restated in fp32 torch arithmetic (same tap order as the kernel): shows without a GPU that the
    seeds of the cases below leave the reference's decisions clear of fp32 rounding.  -> dz fp32 [B, T, d]."""
    B, T = seq.shape
    V, _, d = t1.shape
    T2 = T // 2
    t1f, b1f = t1.float(), b1.float()
    win, inside = window_tokens(seq)
    y = b1f.view(1, 1, d).expand(B, T, d).clone()
    bad = torch.zeros(B, T, dtype=torch.bool)
    for t in range(TAPS):
        tok = win[:, :, t]
        live = inside[None, :, t].expand(B, T)
        ok = live & (tok >= 0) & (tok < V)
        bad |= live & ~ok
        y = torch.where(ok[:, :, None], y + t1f[tok.clamp(0, V - 1), t, :], y)
    y = torch.where(bad[:, :, None], torch.full_like(y, NAN), y)
    if keep is not None:
        y = dropped(y, keep, float(scale))
    a = relu_nan(y)
    a0, a1 = a[:, 0:2 * T2:2], a[:, 1:2 * T2:2]
    win0 = ~((a1 > a0) | torch.isnan(a1))
    up = dP.float() * float(scale) if keep is not None else dP.float()
    zero = torch.zeros_like(up)
    dz = torch.zeros(B, T, d, dtype=torch.float32)
    dz[:, 0:2 * T2:2] = torch.where(win0 & (a0 > 0), up, zero)
    dz[:, 1:2 * T2:2] = torch.where(~win0 & (a1 > 0), up, zero)
    return dz


# ---------------------------------------------------------------- inputs
def gen(seed):
    return torch.Generator().manual_seed(seed)


def f32_randn(*shape, seed, scale=1.0):
    """fp32-representable values (what the device gets), returned as fp32."""
    return (torch.randn(*shape, generator=gen(seed)) * scale).float()


def front_weights(V, d, seed):
    """(t1 [V, 16, d], b1 [d]) fp32: tap rows of magnitude ~ 0.25, so that y1 is O(1) with both signs."""
    return f32_randn(V, TAPS, d, seed=seed, scale=0.25), f32_randn(d, seed=seed + 1, scale=0.25)


def tokens(B, T, V, seed):
    """Tokens over the whole range [0, V), 0 included."""
    return torch.randint(0, V, (B, T), generator=gen(seed))


FRONT_AXES = ((2, 3, 15, 16, 17, 33), (1, 4, 9, 16), (4, 36, 64), (1, 3))   # T, n_vocab, d, B


def pairwise_front_cases():
    """A pairwise cover of T x n_vocab x d x B: every (T, n_vocab) pair once, d and B rotated so that every pair of values
    of any two parameters occurs (test_conv_kernels_cpu.py checks it)."""
    Ts, Vs, ds, Bs = FRONT_AXES
    return [(T, V, ds[(i + j) % 3], Bs[(i + j) % 2]) for i, T in enumerate(Ts) for j, V in enumerate(Vs)]


# lamp_onehot_front_bwd: (name, B, T, n_vocab, d, dropout p, seed).  dt1 shapes: B * T = 255, 256, 257, 300, 513; the last three
# put a boundary of the 256-row chunks inside a sample; d = 36 leaves the (t, c) grid's last block partial.
BWD_CASES = [('bt255', 5, 51, 9, 4, 0.0, 11), ('bt255', 5, 51, 9, 36, 0.0, 12),
             ('bt256', 4, 64, 9, 4, 0.0, 13), ('bt256', 4, 64, 9, 36, 0.0, 14),
             ('bt257', 1, 257, 9, 4, 0.0, 15), ('bt257', 1, 257, 9, 36, 0.0, 16),
             ('bt300', 3, 100, 9, 4, 0.0, 17), ('bt300', 3, 100, 9, 36, 0.0, 18),
             ('bt513', 19, 27, 9, 4, 0.0, 19), ('bt513', 19, 27, 9, 36, 0.0, 20),
             ('vocab16', 2, 33, 16, 36, 0.0, 21), ('vocab1', 3, 17, 1, 4, 0.0, 22), ('short', 3, 2, 4, 4, 0.0, 23),
             ('drop', 3, 100, 9, 36, 0.5, 24), ('drop', 19, 27, 9, 4, 0.5, 25)]
DROP_SEED = 4242


def bwd_case_id(c):
    return '%s-B%d-T%d-V%d-d%d-p%g' % c[:6]


def front_bwd_case(case):
    """-> (seq, t1, b1 fp32, dP fp32 [B, T2, d], p, keep or None, scale)."""
    _, B, T, V, d, p, seed = case
    t1, b1 = front_weights(V, d, seed)
    seq = tokens(B, T, V, seed + 100)
    dP = f32_randn(B, T // 2, d, seed=seed + 200)
    return seq, t1, b1, dP, p, front_keep(B, T, d, p), (1.0 / (1.0 - p) if p else 1)


def front_keep(B, T, d, p, seed=DROP_SEED):
    """The keep mask of lamp_onehot_front_fwd / _bwd: lamp_dropout's counter at element (b * T + p) * d + c."""
    if not p:
        return None
    from lamp_amd import _native as N
    return N.dropout_keep_mask(B * T * d, p, seed).view(B, T, d)


def constant_case(V=9, T=40, d=36, seed=31):
    """One sample per token value, each a constant sequence: the windows of positions 8 .. T - 8 are all equal, so the pairs
    q = 4 .. (T - 8) / 2 - 1 tie exactly, in any precision."""
    t1, b1 = front_weights(V, d, seed)
    seq = torch.arange(V)[:, None].expand(V, T).contiguous()
    dP = f32_randn(V, T // 2, d, seed=seed + 200)
    return seq, t1, b1, dP


def invalid_case(V=9, T=40, d=36, seed=41):
    """Tokens -1 and n_vocab at positions 0, T - 1 and mid-sequence of three samples; a fourth sample stays clean."""
    t1, b1 = front_weights(V, d, seed)
    seq = tokens(4, T, V, seed + 100)
    seq[0, 0], seq[0, T - 1] = -1, V
    seq[1, T // 2], seq[1, T // 2 + 5] = V, -1
    seq[2, 0], seq[2, T - 1] = V, -1
    dP = f32_randn(4, T // 2, d, seed=seed + 200)
    return seq, t1, b1, dP
