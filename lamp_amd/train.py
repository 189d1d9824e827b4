"""The training epoch around the step (reference: train.py:15-76, binary-relevance branch).

The reference's loop body pays, per batch: one host-side get_gold_binary and one upload (train.py:34), a `.item()` on the
loss that drains the device (:40), sigmoid + BCE-with-logits and their autograd backward as separate ATen launches (:37-47,
twice as many with -int_preds), and torch's multi-tensor Adam (:48).  Here, symmetric to lamp_amd/evaluate.py:
  * evaluate.py's PRODUCER thread pads the next `prefetch` batches, builds their gold-binary rows and packs them into the
    pinned ring while the device trains on the previous stage; a stage goes up with one asynchronous copy per buffer;
  * per batch: zero_grad, `model.train()` forward (lamp_amd/training.py), ONE lamp_bce_logits_train launch -- the batch's rows
    of the epoch's device prediction matrix, d loss / d logits of the final prediction and of every int_preds intermediate,
    and the per-row loss sums -- then torch.autograd.backward from those gradients and optimizer.step(); with
    `opt.loss_options` (LossOptions: per-label positive weights, focal or asymmetric loss) that launch is
    lamp_multilabel_loss_train, still one; with `opt.rank_loss` (RankLossOptions: LSEP, pairwise hinge or logistic, plus a
    share of the mean BCE) it is lamp_rank_loss_train, still one;
  * the embedding gradient takes lamp_embed_bwd_ordered (one writer per table row instead of the atomic scatter-add; switched
    on for the epoch through training.ORDERED_EMBED_GRAD), so an epoch is reproducible bit for bit;
  * nothing comes back to the host inside the loop: no `.item()`, no copy, no synchronize.  Predictions and row sums come
    back with one copy each after the last batch; the batch means (reduction='mean', train.py:38) and `bce_total` (:40) are
    taken on the host in float64 from the row sums, as evaluate.test_epoch does.
The short last batch is trained on as it is (the reference does not pad it in train_epoch).  The reference's training loader
is built with drop_last=True (utils/data_loader.py:85-95,151-153), which takes one batch off the count whether or not the
last one is short: TrainBatcher reproduces that, and the rows of the batch left out stay zero in the returned matrices, as
they do in the reference.
"""
import queue
import threading
import time

import numpy as np
import torch

from . import Constants
from . import _native as N
from . import evaluate as E
from . import training
from .data import _Flat


class TrainBatcher(object):
    """The reference's training DataLoader (utils/data_loader.py:129-320 as process_data builds it: shuffle=True,
    drop_last=True) in the format ``((src_seq, src_pos), None, tgt)``:
      * the instances are shuffled once at construction and again after every full pass (:181-182, :316-317);
      * n_batch = ceil(n / batch_size), minus one with drop_last (:151-153) -- also when n is a multiple of batch_size;
      * batch b is instances [b * batch_size, (b + 1) * batch_size) of the current order, padded to its longest (:261-312).
    The permutation comes from a torch.Generator seeded from torch's global generator (so `torch.manual_seed` fixes it), where
    the reference uses Python's `random`; `order` (a permutation of range(n)) sets the current order explicitly."""

    def __init__(self, src_insts, tgt_insts, batch_size, shuffle=True, drop_last=True, generator=None, order=None):
        if not src_insts or len(src_insts) < batch_size:
            raise ValueError('need at least batch_size instances (reference: data_loader.py:139)')
        if len(tgt_insts) != len(src_insts):
            raise ValueError('src / tgt instance counts differ')
        self._n = len(src_insts)
        self._src, self._tgt = _Flat(src_insts), _Flat(tgt_insts)
        self._batch_size = batch_size
        self._n_batch = (self._n + batch_size - 1) // batch_size - (1 if drop_last else 0)
        self._need_shuffle = bool(shuffle)
        if generator is None:
            generator = torch.Generator()
            generator.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        self._gen = generator
        self.order = np.arange(self._n, dtype=np.int64)
        if order is not None:
            self.set_order(order)
        elif self._need_shuffle:
            self.shuffle()

    def __len__(self):
        return self._n_batch

    @property
    def n_insts(self):
        return self._n

    def shuffle(self):
        """A fresh permutation of the CURRENT order (the reference shuffles its lists in place, pass after pass)."""
        self.order = self.order[torch.randperm(self._n, generator=self._gen).numpy()]

    def set_order(self, order):
        order = np.asarray(order, dtype=np.int64)
        if sorted(order.tolist()) != list(range(self._n)):
            raise ValueError('order must be a permutation of range(%d)' % self._n)
        self.order = order.copy()

    def _pad(self, flat, idx):
        lens = flat.lens[idx]
        T = int(lens.max())
        ids = np.full((len(idx), T), Constants.PAD, dtype=np.int64)
        for r, (i, n) in enumerate(zip(idx, lens)):
            ids[r, :n] = flat.ids[flat.offs[i]:flat.offs[i] + n]
        pos = np.where(ids != Constants.PAD, np.arange(1, T + 1, dtype=np.int64)[None, :], 0)
        return torch.from_numpy(ids), torch.from_numpy(pos)

    def batch(self, b):
        idx = self.order[b * self._batch_size:min((b + 1) * self._batch_size, self._n)]
        src_seq, src_pos = self._pad(self._src, idx)
        tgt, _ = self._pad(self._tgt, idx)
        return (src_seq, src_pos), None, tgt

    def __iter__(self):
        for b in range(self._n_batch):
            yield self.batch(b)
        if self._need_shuffle:
            self.shuffle()


class LossOptions(object):
    """`opt.loss_options`: the trained objective when it is not plain BCE (lamp_multilabel_loss_train):
    the focusing exponents, the probability margin and the per-label positive weights (a contiguous fp32 (L,) DEVICE tensor or
    None).  Focal loss is gamma_pos = gamma_neg; the published asymmetric loss is (0, 4, 0.05).  Parameters that are not
    served are refused here, not in the first batch."""

    def __init__(self, gamma_pos=0.0, gamma_neg=0.0, clip=0.0, pos_weight=None):
        self.gamma_pos, self.gamma_neg, self.clip = N.check_loss_options(gamma_pos, gamma_neg, clip)
        self.pos_weight = pos_weight


class RankLossOptions(object):
    """`opt.rank_loss`: train on a ranking objective (lamp_rank_loss_train): kind 'lsep', 'hinge' or
    'logistic', the hinge margin (1 by default; the other two have none), and bce_weight x the row's mean BCE mixed in.
    Not to be combined with `opt.loss_options`.  Parameters that are not served are refused here."""

    def __init__(self, kind='lsep', margin=None, bce_weight=0.0):
        if kind not in N.RANK_KINDS:
            raise ValueError('kind = %r: a ranking loss is one of %s' % (kind, ', '.join(sorted(N.RANK_KINDS))))
        if margin is None:
            margin = 1.0 if kind == 'hinge' else 0.0
        _, self.margin, self.bce_weight = N.check_rank_loss_options(kind, margin, bce_weight)
        self.kind = kind


def _loss_weights(n_mats, int_pred_weight):
    return [1.0] + [float(int_pred_weight)] * (n_mats - 1)


def train_batch(model, optimizer, opt, src, adj, gold_d, probs_rows, loss_rows):
    """The loop body (train.py:35-48) for one batch already on the device.  probs_rows (real, L) / loss_rows (n_mats, real):
    this batch's rows of the epoch's prediction matrix and loss-sum matrix.  `opt.loss_options` (a LossOptions, or absent / None
    for the reference's BCE) picks the trained objective: the loss launch is then lamp_multilabel_loss_train and the row sums
    are that loss.  `opt.rank_loss` (a RankLossOptions) picks a ranking objective instead: lamp_rank_loss_train, whose row
    numbers are R_r + bce_weight * bce_row_r / L; both options together are a ValueError.  `opt.weight_average` (an
    optim.WeightAverage, or absent / None) is updated after optimizer.step(): one more launch.  Nothing here waits for the device."""
    optimizer.zero_grad()
    pred, enc_output, *results = model(src, adj, None, gold_d, return_attns=opt.attns_loss, int_preds=opt.int_preds)
    mats = [pred]
    if opt.int_preds and not getattr(opt, 'matching_mlp', False):
        mats += list(results[0])
    if len(mats) != loss_rows.size(0):
        raise RuntimeError('train_epoch sized its loss matrix for %d predictions, the model returned %d' %
                           (loss_rows.size(0), len(mats)))
    weights = _loss_weights(len(mats), getattr(opt, 'int_pred_weight', 0.2))
    grads = []
    M = N.BCE_TRAIN_MAX_MATS
    lo = getattr(opt, 'loss_options', None)
    rl = getattr(opt, 'rank_loss', None)
    if rl is not None and lo is not None:
        raise ValueError('opt.rank_loss and opt.loss_options are both set: a ranking loss does not combine with focal, '
                         'asymmetric or positive-weighted BCE')
    for k in range(0, len(mats), M):   # (more than 8 matrices: 5+ decoder layers with -int_preds)
        if rl is not None:
            _, g, _ = N.rank_loss_train(mats[k:k + M], weights[k:k + M], gold_d, rl.kind, margin=rl.margin,
                                        bce_weight=rl.bce_weight, probs_out=probs_rows if k == 0 else None,
                                        row_loss_out=loss_rows[k:k + M], want_probs=k == 0)
        elif lo is None:
            _, g, _ = N.bce_logits_train(mats[k:k + M], weights[k:k + M], gold_d, probs_out=probs_rows if k == 0 else None,
                                         row_loss_out=loss_rows[k:k + M], want_probs=k == 0)
        else:
            _, g, _ = N.multilabel_loss_train(mats[k:k + M], weights[k:k + M], gold_d, gamma_pos=lo.gamma_pos,
                                              gamma_neg=lo.gamma_neg, clip=lo.clip, pos_weight=lo.pos_weight,
                                              probs_out=probs_rows if k == 0 else None, row_loss_out=loss_rows[k:k + M],
                                              want_probs=k == 0)
        grads += g
    torch.autograd.backward(mats, grads)
    optimizer.step()
    wa = getattr(opt, 'weight_average', None)      # (an optim.WeightAverage, or absent / None: the loop as it has always been)
    if wa is not None:
        wa.update()


def n_loss_matrices(model, opt):
    """1 + the number of int_preds intermediates the model returns (lamp/Decoders.py: one per sub-layer but the last)."""
    if not (opt.int_preds and not getattr(opt, 'matching_mlp', False)):
        return 1
    return sum(2 if hasattr(l, 'slf_attn') else 1 for l in model.decoder.layer_stack)


def train_epoch(model, train_data, optimizer, opt, device=None, prefetch=8, streams=1, timeline=None, device_results=None):
    """-> (all_predictions (n, L) cpu, all_targets (n, L) cpu, bce_total float), as train.py:15-76 returns them.

    `train_data` yields ((src_seq, src_pos), adj, tgt) batches of at most `train_data._batch_size` rows (TrainBatcher, or any
    iterable with `n_insts`, `__len__` and `_batch_size`); `opt` carries what the reference's loop reads: tgt_vocab_size,
    binary_relevance, int_preds, int_pred_weight, attns_loss (only changes return_attns, as in the reference), decoder, and
    optionally `loss_options` (LossOptions) or `rank_loss` (RankLossOptions): the third return value and 'row_loss' are then
    the TRAINED loss, not BCE -- with a ranking loss a per-row number, whose batch mean divides by the rows alone, not by rows * L.
    `prefetch` = batches per stage of the producer thread (evaluate.py); `streams=2` issues the stage uploads on a stream of
    their own instead of in front of the stage's first forward.  Every batch's numbers are the same in every mode, bit for bit.
    `timeline` / `device_results` as in evaluate.test_epoch: 'probs' and 'targets' (n, L) stay on the device for
    lamp_amd.metrics.compute_metrics, and 'row_loss' (n_mats, n) holds every matrix's per-row loss sums."""
    if not opt.binary_relevance:
        raise NotImplementedError("train_epoch covers the binary-relevance branch (train.py:33-50); the '%s' decoder trains "
                                  "through the crit / log-softmax branch (train.py:52-66), which is not ported"
                                  % getattr(opt, 'decoder', 'rnn_m'))
    t_start = time.perf_counter()
    if device is None:
        device = next(model.parameters()).device
    model.train()
    n, n_labels, batch_size = train_data.n_insts, opt.tgt_vocab_size, train_data._batch_size
    n_mats = n_loss_matrices(model, opt)
    pin = torch.cuda.is_available()
    all_targets = torch.zeros(n, n_labels)
    probs_d = torch.zeros((n, n_labels), dtype=torch.float32, device=device)
    targets_d = torch.zeros_like(probs_d) if device_results is not None else None
    row_loss_d = torch.zeros((n_mats, n), dtype=torch.float32, device=device)
    main = torch.cuda.current_stream(device)
    copy_stream = torch.cuda.Stream(device=device) if streams > 1 else None
    if copy_stream is not None:
        copy_stream.wait_stream(main)
    stages, stop = queue.Queue(maxsize=E.STAGE_QUEUE), threading.Event()
    ring = E._borrow_ring()
    seen = []
    it = ((bi, b) for bi, b in enumerate(train_data))
    producer = threading.Thread(target=E._produce, name='lamp-train-producer', daemon=True,
                                args=(it, n_labels, batch_size, max(int(prefetch), 1), all_targets, stages, pin, device, stop,
                                      False, ring))
    producer.start()
    ordered_before = training.ORDERED_EMBED_GRAD
    training.ORDERED_EMBED_GRAD = True      # the embedding gradient in a fixed order: the epoch is reproducible bit for bit
    try:
        while True:
            st = stages.get()
            if st is None:
                break
            if isinstance(st, BaseException):
                raise st
            issue_stage(model, optimizer, opt, st, main, copy_stream, device, probs_d, row_loss_d, targets_d, seen)
    finally:
        training.ORDERED_EMBED_GRAD = ordered_before
        stop.set()
        producer.join()
    t_issued = time.perf_counter()
    if timeline is not None:
        torch.cuda.synchronize(device)
        timeline.update(issued=t_issued - t_start, done=time.perf_counter() - t_start)
    all_predictions = probs_d.cpu()       # (synchronises with the stream the epoch ran on)
    row_loss = row_loss_d[0].cpu().numpy().astype(np.float64)
    E._return_ring(ring)
    bce_total = 0.0
    # a ranking loss is a per-ROW number (lamp_rank_loss_train has divided its BCE share by L already): its mean is over rows
    per_row = 1 if getattr(opt, 'rank_loss', None) is not None else n_labels
    for lo, real in seen:   # the reference adds one python float per batch, the batch's MEAN loss (train.py:38-40)
        bce_total += float(row_loss[lo:lo + real].sum()) / (real * per_row)
    if device_results is not None:
        device_results.update(probs=probs_d, targets=targets_d, rows=(0, n), row_loss=row_loss_d, batches=list(seen))
    return all_predictions, all_targets, bce_total


def issue_stage(model, optimizer, opt, st, main, copy_stream, device, probs_d, row_loss_d, targets_d, seen):
    """Everything the issuing thread does for one stage: its two uploads, then the loop body per batch.  Nothing here waits
    for the device."""
    with (torch.cuda.stream(copy_stream) if copy_stream is not None else E._SAME_STREAM):
        ids_d = st.ids.to(device, non_blocking=True) if st.ids is not None else None
        gold_d = st.gold.to(device, non_blocking=True)
        uploaded = (copy_stream or main).record_event()
    st.slot.uploaded = uploaded
    if copy_stream is not None:
        main.wait_event(uploaded)
        if ids_d is not None:
            ids_d.record_stream(main)
        gold_d.record_stream(main)
    for k, (bi, lo, real, T, off, row, adj) in enumerate(st.items):
        if ids_d is not None:
            cnt = real * T
            src = (ids_d[off:off + cnt].view(real, T), ids_d[off + cnt:off + 2 * cnt].view(real, T))
        else:
            src = st.device_batches[k]
        gold = gold_d[row:row + real]
        if targets_d is not None:
            targets_d[lo:lo + real].copy_(gold, non_blocking=True)
        train_batch(model, optimizer, opt, src, adj, gold, probs_d[lo:lo + real], row_loss_d[:, lo:lo + real])
        seen.append((lo, real))
