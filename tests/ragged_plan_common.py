"""Shared pieces of the ragged plan tests (test_ragged_plan_cpu.py, test_ragged_plan_gpu.py, test_graph_replay_gpu.py).

``plan_ref`` restates the sequence plan of a token batch in plain NumPy, from the prose of csrc/lamp_kernels.h (struct SeqPlan)
and of the comment above seq_plan_kernel -- not from the kernels:

  klen[b]   1 + the last position of sample b whose token is not PAD (0 without a token): the sample's keys.
  plen[b]   >= klen[b]: additionally covers every position that carries a non-zero POSITION index (only when the model has a
            position table; without one plen = klen).  The sample's rows in the packed matrix.
  off[b]    the sum of plen before b, off[nb] = n_tok: the sample's first packed row.
  rows      [n_tok, n_tok + 1 when some position is skipped (some plen[b] < T) else n_tok].
  padbits   [nb][(T + 31) / 32] words, bit j % 32 of word j / 32 set = position j holds a PAD token; positions past T count as PAD.

``PATTERNS`` is the named set of length patterns the tests sweep, each built for a given (nb, T).
"""
import numpy as np
import torch

PAD = 0
VOCAB = 11          # tokens 4 .. 10, as lamp_amd.synthetic.make_batch draws them
NBS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 128, 129, 255, 256, 257, 300, 515)   # the batch sweep, at T = T_BATCH
T_BATCH = 5
TS = (1, 2, 31, 32, 33, 63, 64, 65, 511, 512, 513, 577, 1025)                  # the length sweep, at nb = NB_LEN
NB_LEN = 3
T_MAX = max(TS)
SWEEP = [(nb, T_BATCH) for nb in NBS] + [(NB_LEN, T) for T in TS]


def plan_ref(seq, pos=None):
    """(seq [nb, T], pos [nb, T] or None) -> dict(klen, plen, off [nb + 1], rows [2], padbits [nb, words] uint32)."""
    seq = np.asarray(seq)
    nb, T = seq.shape
    tok = seq != PAD
    alive = tok if pos is None else (tok | (np.asarray(pos) != 0))
    klen = np.zeros(nb, dtype=np.int64)
    plen = np.zeros(nb, dtype=np.int64)
    for b in range(nb):
        for j in range(T):
            if tok[b, j]:
                klen[b] = j + 1
            if alive[b, j]:
                plen[b] = j + 1
    off = np.zeros(nb + 1, dtype=np.int64)
    for b in range(nb):
        off[b + 1] = off[b] + plen[b]
    n_tok = int(off[nb])
    rows = np.array([n_tok, n_tok + (1 if (plen < T).any() else 0)], dtype=np.int64)
    words = (T + 31) // 32
    padbits = np.zeros((nb, words), dtype=np.uint32)
    for b in range(nb):
        for j in range(words * 32):
            if j >= T or not tok[b, j]:
                padbits[b, j // 32] |= np.uint32(1) << np.uint32(j % 32)
    return dict(klen=klen, plen=plen, off=off, rows=rows, padbits=padbits)


def _from_lengths(lengths, T, rng):
    """Tokens U{4 .. VOCAB - 1} on [0, n), positions 1 .. n, PAD and 0 behind (the data loader's batches)."""
    nb = len(lengths)
    seq = np.zeros((nb, T), dtype=np.int64)
    pos = np.zeros((nb, T), dtype=np.int64)
    for b, n in enumerate(lengths):
        seq[b, :n] = rng.integers(4, VOCAB, size=n)
        pos[b, :n] = np.arange(1, n + 1)
    return seq, pos


def _random_lengths(nb, T, rng, lo=1):
    return [int(n) for n in rng.integers(lo, T + 1, size=nb)]


def _dense(nb, T, rng):
    return _from_lengths([T] * nb, T, rng)


def _last_short(nb, T, rng):
    return _from_lengths([T] * (nb - 1) + [T // 2], T, rng)


def _first_short(nb, T, rng):
    return _from_lengths([T // 2] + [T] * (nb - 1), T, rng)


def _zero_length(nb, T, rng):
    lengths = _random_lengths(nb, T, rng)
    for b in (0, 63, 64, 65, nb - 1):
        if b < nb:
            lengths[b] = 0
    return _from_lengths(lengths, T, rng)


def _all_pad(nb, T, rng):
    return np.zeros((nb, T), dtype=np.int64), np.zeros((nb, T), dtype=np.int64)


def interior_runs(T):
    """PAD runs [lo, hi) inside a sequence of T positions that cross a 32- and a 64-position boundary where T has one (else one
    short run), always leaving the first and the last position alone."""
    runs = [(lo, hi) for lo, hi in ((30, 34), (62, 66)) if hi < T]
    if not runs and T >= 3:
        runs = [(1, max(2, min(3, T - 1)))]
    return runs


def _interior_pad(nb, T, rng):
    """Full-length samples with PAD runs inside: even samples lose the position indices of the run too (a hole of real PAD
    positions), odd samples keep them (a PAD token at a live position)."""
    seq, pos = _from_lengths([T] * nb, T, rng)
    for b in range(nb):
        for lo, hi in interior_runs(T):
            seq[b, lo:hi] = PAD
            if b % 2 == 0:
                pos[b, lo:hi] = 0
    return seq, pos


def _position_tail(nb, T, rng):
    """Trailing PAD tokens that keep their position indices: plen > klen (with a position table)."""
    lengths = [min(n, T - 1) for n in _random_lengths(nb, T, rng, lo=0)]
    seq, pos = _from_lengths(lengths, T, rng)
    for b, n in enumerate(lengths):
        tail = min(T, n + 1 + b % 3)
        pos[b, n:tail] = np.arange(n + 1, tail + 1)
    return seq, pos


def _last_only(nb, T, rng):
    """Samples 0 and nb / 2 hold one token, at position T - 1, and nothing in front of it."""
    seq, pos = _from_lengths(_random_lengths(nb, T, rng), T, rng)
    for b in {0, nb // 2}:
        seq[b], pos[b] = PAD, 0
        seq[b, T - 1] = 4 + b % (VOCAB - 4)
        pos[b, T - 1] = T
    return seq, pos


PATTERNS = {
    'dense': _dense,
    'last_short': _last_short,
    'first_short': _first_short,
    'zero_length': _zero_length,
    'all_pad': _all_pad,
    'interior_pad': _interior_pad,
    'position_tail': _position_tail,
    'last_only': _last_only,
}
RAGGED = [p for p in PATTERNS if p != 'dense']


def make_pattern(name, nb, T, seed=0):
    """-> (seq, pos) int64 torch tensors [nb, T] of one named pattern."""
    rng = np.random.default_rng([seed, nb, T, sorted(PATTERNS).index(name)])
    seq, pos = PATTERNS[name](nb, T, rng)
    return torch.from_numpy(seq), torch.from_numpy(pos)


# ---- the tiny model of the sweeps: d_model 8, 2 heads of 4, d_inner 8, 3 labels, one encoder and one decoder layer
TINY = dict(V=VOCAB, L=3, d=8, h=2, dff=8)


def tiny_state_dict(pos, n_max_seq=T_MAX, seed=0):
    from oracle import lamp_ref as R
    t = TINY
    return R.make_state_dict(t['V'], t['L'], n_max_seq, t['d'], t['dff'], t['h'], 1, 1, pos_emb=pos, seed=seed)


def tiny_model(sd, pos, n_max_seq=T_MAX, **kw):
    """LAMP on the CPU with the weights of `sd` (the caller moves it to the device)."""
    from lamp_amd.Models import LAMP
    t = TINY
    m = LAMP(t['V'], t['L'], n_max_seq, t['L'], n_layers_enc=1, n_layers_dec=1, n_head=t['h'], n_head2=t['h'], d_word_vec=t['d'],
             d_model=t['d'], d_inner_hid=t['dff'], d_k=t['d'] // t['h'], d_v=t['d'] // t['h'], encoder='graph', decoder='graph',
             no_enc_pos_embedding=not pos, label_adj_matrix=None, label_mask='none', dec_dropout2=False, **kw)
    m.load_state_dict(sd)
    return m


def forward_passes(m, B, T, want_attn=False, opts=None):
    """How many micro-batches LAMP.forward's lamp_forward call makes for a (B, T) batch under m.workspace_limit_bytes, from the
    library's own workspace-bytes query (affine in the micro-batch: fixed + per * mb) and the budget rule of LAMP.forward.
    -> (passes, samples of the last pass)."""
    import ctypes as C
    from lamp_amd import _native as N
    model = m._native_model()[0]
    if opts is not None:
        def q(mb):
            return N.lib().lamp_forward_opts_workspace_bytes(C.byref(model), C.byref(opts), mb, T, int(want_attn))
    else:
        def q(mb):
            return N.lib().lamp_forward_workspace_bytes(C.byref(model), mb, T, int(want_attn))
    one, two = q(1), q(2)
    assert one > 0 and two > one
    per, fixed = two - one, 2 * one - two
    assert q(B) == fixed + per * B
    budget = max(one + 4096, min(fixed + per * B + 4096, m.workspace_limit_bytes))
    mb = min(B, (budget - fixed) // per)
    passes = -(-B // mb)
    return passes, B - (passes - 1) * mb


def limit_for_micro_batch(m, T, mb, want_attn=False, opts=None):
    """A workspace_limit_bytes under which lamp_forward carves micro-batches of exactly `mb` samples (room for mb and a half)."""
    import ctypes as C
    from lamp_amd import _native as N
    model = m._native_model()[0]
    if opts is not None:
        one, two = (N.lib().lamp_forward_opts_workspace_bytes(C.byref(model), C.byref(opts), k, T, int(want_attn)) for k in (1, 2))
    else:
        one, two = (N.lib().lamp_forward_workspace_bytes(C.byref(model), k, T, int(want_attn)) for k in (1, 2))
    per, fixed = two - one, 2 * one - two
    return fixed + per * mb + per // 2


def same_bits(a, b):
    """Bit for bit, except that two NaNs count as equal whatever their payload (a NaN's sign and payload are not part of any
    contract here; which elements are NaN is)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    return torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb])
