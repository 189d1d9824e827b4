"""Data side of the evaluation harness: what reaches the hot path and in which shape
(reference: utils/data_loader.py; on-disk format: utils/preprocess.py:218-232).

Host-side Python on purpose: this is index bookkeeping done once per dataset / per batch on the CPU in
the reference too.  The tensors it emits are exactly the ones ``LAMP.forward`` receives.
"""
import numpy as np
import torch

from . import Constants


def load_dataset(path):
    """The ``train_valid_test.pt`` dict: settings / dict{src,tgt} / train,valid,test{src,tgt} (main.py:23).
    It pickles an argparse.Namespace, hence weights_only=False."""
    return torch.load(path, weights_only=False)


def vocabulary_sizes(data, binary_relevance=True):
    """(src_vocab_size, tgt_vocab_size) as process_data derives them: the label count excludes the four
    special tokens for the graph decoder (utils/data_loader.py:119-124)."""
    n_src = len(data['dict']['src'])
    n_tgt = len(data['dict']['tgt'])
    return n_src, (n_tgt - 4 if binary_relevance else n_tgt)


def prior_adjacency(train_tgt, n_tgt_dict):
    """Label co-occurrence graph of the train split (utils/data_loader.py:37-44): identity, plus an edge
    between every two distinct labels that share a sample.  Targets are [BOS, label ids..., EOS] with ids
    offset by the four special tokens."""
    L = n_tgt_dict - 4
    adj = torch.eye(L)
    for sample in train_tgt:
        labels = [int(v) - 4 for v in sample[1:-1]]
        for i, a in enumerate(labels):
            for b in labels[i + 1:]:
                if a != b:
                    adj[a, b] = 1
                    adj[b, a] = 1
    return adj


def prior_adjacency_device(train_tgt, n_tgt_dict, device):
    """Same matrix as prior_adjacency, built by the HIP kernel (lamp_prior_graph_build): the host only flattens
    the label sets into CSR.  For delicious-sized splits the Python double loop above takes seconds; this does
    not."""
    from . import _native as N
    L = n_tgt_dict - 4
    ids, offsets = _label_csr(train_tgt)
    return N.prior_graph(torch.from_numpy(ids).to(device), torch.from_numpy(offsets).to(device), L)


def _label_csr(train_tgt):
    """The label sets of a split flattened into CSR (ids without the four specials, offsets), as numpy int64."""
    lens = np.fromiter((max(len(s) - 2, 0) for s in train_tgt), dtype=np.int64, count=len(train_tgt))
    offsets = np.zeros(len(train_tgt) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    ids = np.empty(int(offsets[-1]), dtype=np.int64)
    for s, lo in zip(train_tgt, offsets[:-1]):
        n = len(s) - 2
        if n > 0:
            ids[lo:lo + n] = np.asarray(s[1:-1], dtype=np.int64) - 4
    return ids, offsets


def label_cooccurrence(train_tgt, n_tgt_dict, device):
    """(L, L) fp32 co-occurrence counts of the train split on `device`: C[i, j] = samples holding both labels, C[i, i] =
    samples holding label i; a label repeated inside a sample counts once.  The statistics behind the weighted label graph
    (LAMP(label_bias=...)): where prior_adjacency keeps one bit per pair, this keeps how often.  Built on the device from the
    CSR prior_adjacency_device flattens: a multi-hot [L, n] matrix times its own transpose on the library's GEMM (lamp_gemm).
    Sums of 0 / 1 products are exact in fp32 below 2^24 samples, in any order."""
    from . import _native as N
    hot = label_multihot_t(train_tgt, n_tgt_dict, device)
    N.require_device(hot)
    return N.matmul_nt(hot, hot)


def label_multihot_t(train_tgt, n_tgt_dict, device=None):
    """The transposed multi-hot matrix of a split's label sets: fp32 [L, n padded to a multiple of 4], 1 where the sample holds
    the label (a label repeated inside a sample stores its 1 twice).  Host-side index bookkeeping; the product is the
    library's."""
    L = n_tgt_dict - 4
    n = len(train_tgt)
    assert n < 2 ** 24, 'co-occurrence counts are exact in fp32 below 2^24 samples only'
    ids, offsets = _label_csr(train_tgt)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    hot = torch.zeros((L, (max(n, 1) + 3) & ~3), dtype=torch.float32, device=device)
    if ids.size:
        hot[torch.from_numpy(ids).to(hot.device), torch.from_numpy(rows).to(hot.device)] = 1.0
    return hot


def label_bias_from_counts(C, kind, scale=1.0):
    """The (L, L) score bias of LAMP(label_bias=...) from label_cooccurrence's counts.
    'adj':  scale * A, A the prior adjacency with its diagonal (1 where C > 0 or i == j) -- with label_mask='none' the soft
            prior the reference's unused -adj_matrix_lambda points at: a neighbour's score is raised, nobody is blocked.
    'logp': scale * log((C[i, j] + 1) / (C[i, i] + 1)) off the diagonal, 0 on it -- a smoothed log P(j | i), finite
            everywhere and asymmetric; softmax(s + log w) re-weights the attention by w."""
    C = C.to(torch.float32)
    L = C.size(0)
    eye = torch.eye(L, dtype=torch.bool, device=C.device)
    if kind == 'adj':
        return float(scale) * ((C > 0) | eye).to(torch.float32)
    if kind == 'logp':
        logp = torch.log((C + 1.0) / (torch.diagonal(C).unsqueeze(1) + 1.0))
        return float(scale) * logp.masked_fill(eye, 0.0)
    raise ValueError("label bias kind %r: 'adj' or 'logp'" % (kind,))


def build_label_bias(data, kind, scale, device):
    """-label_bias / -label_bias_scale -> the (L, L) bias of LAMP(label_bias=...) from the TRAIN split's co-occurrence counts
    (rebuilt the same way by run_eval, like the prior mask), or None."""
    if kind in (None, 'none'):
        return None
    counts = label_cooccurrence(data['train']['tgt'], len(data['dict']['tgt']), device)
    return label_bias_from_counts(counts, kind, scale).cpu()


def label_pos_weight(train_tgt, n_tgt_dict, device, kind='inv', cap=100.0):
    """The per-label positive weights of -pos_weight (lamp_multilabel_loss_train's pos_weight): a contiguous fp32 (L,) tensor on
    `device`.  With n train samples and c_j of them carrying label j (a label repeated inside a sample counts once):
    'inv':      w_j = min(cap, (n - c_j) / max(c_j, 1)), negatives over positives, torch.nn.BCEWithLogitsLoss's documented recipe;
    'sqrt_inv': w_j = min(cap, sqrt((n - c_j) / max(c_j, 1))).
    A label without a positive gets `cap`.  Host-side counting, once per run."""
    if kind not in ('inv', 'sqrt_inv'):
        raise ValueError("pos_weight kind %r: 'inv' or 'sqrt_inv'" % (kind,))
    cap = float(cap)
    if not cap > 0.0 or cap == float('inf'):
        raise ValueError('pos_weight cap %r: a positive finite number' % (cap,))
    L = n_tgt_dict - 4
    n = len(train_tgt)
    ids, offsets = _label_csr(train_tgt)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    pairs = np.unique(rows * L + ids) if ids.size else ids       # (sample, label) once each
    c = np.bincount(pairs % L, minlength=L).astype(np.float64)
    w = (n - c) / np.maximum(c, 1.0)
    if kind == 'sqrt_inv':
        w = np.sqrt(w)
    w = np.where(c > 0, np.minimum(w, cap), cap)
    return torch.from_numpy(w.astype(np.float32)).to(device).contiguous()


def pad_to_longest(insts):
    """-> (ids int64 (B, T), positions int64 (B, T)); T = longest instance of the batch, PAD = 0, position
    = 1-based index on non-PAD tokens and 0 on PAD (utils/data_loader.py:261-279)."""
    T = max(len(x) for x in insts)
    ids = np.full((len(insts), T), Constants.PAD, dtype=np.int64)
    for i, x in enumerate(insts):
        ids[i, :len(x)] = x
    pos = np.where(ids != Constants.PAD, np.arange(1, T + 1, dtype=np.int64)[None, :], 0)
    return torch.from_numpy(ids), torch.from_numpy(pos)


class _Flat(object):
    """A list of variable-length id lists stored once as ONE int64 array + offsets (CSR), so that padding a batch is a single
    masked store instead of a Python loop over its instances (the reference converts list by list on every batch,
    utils/data_loader.py:261-279; at reuters' size that loop costs more host time than the batch costs the GPU)."""

    def __init__(self, insts):
        import itertools
        self.lens = np.fromiter((len(x) for x in insts), dtype=np.int64, count=len(insts))
        self.offs = np.zeros(len(insts) + 1, dtype=np.int64)
        np.cumsum(self.lens, out=self.offs[1:])
        self.ids = np.fromiter(itertools.chain.from_iterable(insts), dtype=np.int64, count=int(self.offs[-1]))

    def pad(self, lo, hi):
        """pad_to_longest(insts[lo:hi]) -> (ids, positions) as torch int64 (B, T)."""
        lens = self.lens[lo:hi]
        T = int(lens.max())
        live = np.arange(T, dtype=np.int64)[None, :] < lens[:, None]
        ids = np.full((hi - lo, T), Constants.PAD, dtype=np.int64)
        ids[live] = self.ids[self.offs[lo]:self.offs[hi]]     # row-major order of the mask == concatenation order
        pos = np.where(ids != Constants.PAD, np.arange(1, T + 1, dtype=np.int64)[None, :], 0)
        return torch.from_numpy(ids), torch.from_numpy(pos)


class EvalBatcher(object):
    """Sequential (unshuffled) batches in the reference DataLoader's format
    ``((src_seq, src_pos), None, tgt)`` -- utils/data_loader.py:129-312 with shuffle=False, drop_last=False,
    as process_data builds the valid/test loaders.  Tensors are moved to `device` if given.  The instances are flattened
    once at construction (_Flat); every batch is then padded by vectorised numpy, same tensors as pad_to_longest."""

    def __init__(self, src_insts, tgt_insts, batch_size, device=None):
        if not src_insts or len(src_insts) < batch_size:
            raise ValueError('need at least batch_size instances (reference: data_loader.py:139)')
        if tgt_insts is not None and len(tgt_insts) != len(src_insts):
            raise ValueError('src / tgt instance counts differ')
        self._n = len(src_insts)
        self._src = _Flat(src_insts)
        self._tgt = _Flat(tgt_insts) if tgt_insts is not None else None
        self._batch_size = batch_size
        self._n_batch = (len(src_insts) + batch_size - 1) // batch_size
        self.device = device

    def __len__(self):
        return self._n_batch

    @property
    def n_insts(self):
        return self._n

    def __iter__(self):
        return self.iter_range(0, self._n_batch)

    def iter_range(self, b_lo, b_hi):
        """Batches b_lo .. b_hi - 1 only: a rank of a sharded evaluation materialises (pads, uploads) just its own share."""
        for b in range(max(b_lo, 0), min(b_hi, self._n_batch)):
            lo, hi = b * self._batch_size, min((b + 1) * self._batch_size, self._n)
            src_seq, src_pos = self._src.pad(lo, hi)
            tgt = None
            if self._tgt is not None:
                tgt, _ = self._tgt.pad(lo, hi)
            if self.device is not None:
                src_seq, src_pos = src_seq.to(self.device), src_pos.to(self.device)
            yield (src_seq, src_pos), None, tgt


def get_gold_binary(gold, n_labels):
    """(B, n_labels) float 0/1 matrix from padded target rows WITHOUT their leading BOS: drop PADs, drop the
    trailing EOS (the last remaining id of the row), shift ids by the four specials (utils/utils.py:205-216).
    numpy, one fancy-index store instead of the reference's per-row index_fill_ (tiny torch CPU ops pay the
    thread-pool wake-up of a 128-core host: 2 ms per call measured)."""
    g = gold.numpy() if isinstance(gold, torch.Tensor) else np.asarray(gold)
    B, W = g.shape
    out = np.zeros((B, n_labels + 4), dtype=np.float32)
    if W:
        keep = g > 0
        cols = np.arange(W)[None, :]
        last = np.where(keep, cols, -1).max(axis=1, keepdims=True)
        keep &= cols != last
        rows = np.broadcast_to(np.arange(B)[:, None], g.shape)
        out[rows[keep], g[keep]] = 1.0
    return torch.from_numpy(out[:, 4:].copy())
