"""Training runner: the reference's `main.py` + `runner.run_model` flow (without -test_only) for encoder=graph /
decoder=graph, on the MI355X path.

    python -m lamp_amd.run_train -data data/reuters/train_valid_test.pt -dataset reuters -batch_size 32 \
           -d_model 512 -n_layers_enc 2 -n_head 4 -label_mask prior -epoch 50 -dropout 0.1 -lr 0.0002 [-int_preds] \
           [-enc_self_att] [-attn_type sigmoid] [-lr_decay 0.9 -lr_step_size 10] [-save_mode best] [-load_pretrained] [-name run1] [-results_dir results/]
           [-tune_thresholds f1|youden|balance] [-label_ranking] [-at_k 1,3,5]

Flag names and derived defaults are config_args.py's for everything on this path (n_layers_dec = n_layers_enc :87-88,
test_batch_size = batch_size :93-94, d_k = d_v = d_model / n_head :96-99, dec_dropout = dropout :101-102, no position
embedding for bibtext / delicious / bookmarks / sider :104-105, d_inner_hid = 2 d_model :110-111, n_head2 = n_head :135-136,
-int_preds only with the graph decoder :213-216, the one-hot encoder for the genomics datasets :90-91, and the results
directory name :121-227).  Two deliberate differences: -data names the dataset file itself (as run_eval does; the reference
joins -dataroot and -dataset), and -decoder defaults to 'graph', the decoder this path serves (the reference's default 'sa_m'
exists in its argparse only).

Per epoch, as runner.py:36-92: scheduler.step() first (:38, when -lr_decay > 0), train_epoch (lamp_amd/train.py),
evaluate.test_epoch on valid and test, the metrics of all three splits on the device (lamp_amd/metrics.py), one JSON line, a
row of losses.csv (epoch, train, valid, test loss, each summed batch means / instances as the reference reports them), and the
checkpoint {'model': state_dict, 'settings': opt, 'epoch': i} under utils.save_model's rule (utils/utils.py:228-241).  That
rule's `valid_loss >= min(valid_losses)` is kept as written: the list already holds the current loss, so -save_mode best
rewrites model.chkpt after EVERY epoch -- the reference's behaviour, not a selection of the best epoch.  As in the reference
(runner.py:85) nothing is saved when the results directory's name contains 'test'.  The file loads in
`run_eval -checkpoint` and in the reference's `main.py -load_pretrained`.

-tune_thresholds f1|youden|balance fits one decision threshold per label on every epoch's validation predictions, still on the
device (lamp_amd/metrics.py: tune_thresholds), reports the test epoch's thresholded figures at them as
tuned_ACC .. tuned_maF1 next to the fixed ones in that epoch's record, stores `label_thresholds` (a CPU float32 tensor) and
`tune_criterion` in the checkpoint beside model / settings / epoch (run_eval -tune_thresholds checkpoint reads them) and adds
.thr_<criterion> to the results name.

-label_ranking and -at_k 1,3,5 are reporting only: the per-epoch metrics of all three splits then also carry the label-ranking
figures (LRAP, coverage_error, ranking_loss, one_error, instance_AUC) and P@k / nDCG@k / R@k (section
8.8), computed on the device from the probabilities the epoch left there -- what a ranking -loss_fn optimises, next to the BCE
it is selected on.  They change neither the results name nor the checkpoint (no settings entry, no key) nor losses.csv, and
-save_mode best still looks at the BCE valid loss.

-loss_fn focal|asl and -pos_weight inv|sqrt_inv change the TRAINED objective (focal loss, asymmetric loss, per-label positive
weights from the train split's counts), still in the one loss launch per batch.  The train column of
losses.csv and train_loss are then that objective; the valid and test losses stay plain BCE, so -save_mode best and runs with
different objectives stay comparable.  They add .lossfn_<kind>_<parameters> / .posw_<kind>_<cap> to the results name and
their flags to the checkpoint's settings, and nothing when they are not given.  (-loss is the reference's flag, parsed and,
as there, unused.)

-max_grad_norm F, -weight_decay F, -optim adamw, -momentum F (sgd) and -skip_nonfinite are the training-loop controls of
DESIGN.md section 8.11.  With any of them the optimizer is built over two param groups: parameters with ndim >= 2 decay, 1-D
parameters and decoder.label_bias (whose -inf entries must never meet weight_decay * w) do not.  Both -optim_impl values serve
the first four (torch: clip_grad_norm_ in front of every step, torch.optim.AdamW / Adam(weight_decay=) / SGD(momentum=));
-skip_nonfinite exists with -optim_impl lamp only and adds steps_skipped to each epoch's record, read where the loop already
synchronises.  Each adds .clip_<v> / .wd_<v> / .mom_<v> / .skipnf to the results name and its flag to the checkpoint's settings,
and nothing when it is not given.

-weight_avg ema|swa keeps an average of the weights (lamp_amd.optim.WeightAverage) beside the trained
ones: one lamp_weight_average launch after every optimizer step (-avg_every k: after every k-th) from the first step of epoch
-avg_start_epoch on; ema uses -ema_decay (with -ema_warmup: min(decay, (1 + t) / (10 + t))), swa the running mean.  Once
averaging has begun each epoch's valid and test epochs run with the average swapped in -- thresholds, -at_k, -label_ranking and
the valid loss -save_mode best compares are then the averaged model's, and the epoch's record says "weights": "avg" -- and the
weights are swapped back before the next epoch trains.  The checkpoint keeps 'model' as trained (-load_pretrained resumes
that; the average itself is not resumed and starts again), and gains 'weight_avg' (the average's state without buffers) and,
once an average exists, 'model_avg' (run_eval -weights auto|raw|avg).  The flags add .wavg_<kind>_<decay or 'swa'>[_w][_e<k>]
[_s<epoch>] to the results name and themselves to the checkpoint's settings, and nothing when -weight_avg is not given.
"""
import argparse
import contextlib
import json
import os
import sys
import time
import warnings

import torch

from . import data as D
from .run_eval import ONEHOT_DATASETS


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('-data', required=True, help='train_valid_test.pt in the reference format')
    ap.add_argument('-dataset', type=str, default='reuters')
    ap.add_argument('-results_dir', type=str, default='results/')
    ap.add_argument('-epoch', type=int, default=50)
    ap.add_argument('-batch_size', type=int, default=64)
    ap.add_argument('-test_batch_size', type=int, default=-1)
    ap.add_argument('-d_model', type=int, default=512)
    ap.add_argument('-d_inner_hid', type=int, default=-1)
    ap.add_argument('-d_k', type=int, default=-1)
    ap.add_argument('-d_v', type=int, default=-1)
    ap.add_argument('-n_head', type=int, default=8)
    ap.add_argument('-n_head2', type=int, default=0)
    ap.add_argument('-n_layers_enc', type=int, default=5)
    ap.add_argument('-n_layers_dec', type=int, default=None)
    ap.add_argument('-optim', type=str, choices=['adam', 'sgd', 'adamw'], default='adam')
    ap.add_argument('-lr', type=float, default=0.0002)
    ap.add_argument('-lr_step_size', type=int, default=1)
    ap.add_argument('-lr_decay', type=float, default=0)
    ap.add_argument('-dropout', type=float, default=0.1)
    ap.add_argument('-dec_dropout', type=float, default=-1)
    ap.add_argument('-no_dec_self_att', action='store_true')
    ap.add_argument('-loss', type=str, choices=['ce', 'adv', 'ranking'], default='ce',
                    help="parsed for compatibility with the reference (config_args.py:37) and, as there, ignored: '-loss ranking' "
                         "trains nothing different.  The ranking objectives are -loss_fn lsep | rank_hinge | rank_logistic")
    ap.add_argument('-save_mode', type=str, choices=['all', 'best'], default='best')
    ap.add_argument('-encoder', type=str, choices=['rnn', 'graph', 'emb', 'mlp'], default='graph')
    ap.add_argument('-decoder', type=str, choices=['sa_m', 'rnn_m', 'sa_b', 'graph', 'mlp'], default='graph')
    ap.add_argument('-label_mask', type=str, choices=['none', 'inveye', 'prior'], default='none')
    ap.add_argument('-br_threshold', type=float, default=0.5)
    ap.add_argument('-no_enc_pos_embedding', action='store_true')
    ap.add_argument('-int_preds', action='store_true')
    ap.add_argument('-load_pretrained', action='store_true')
    ap.add_argument('-int_pred_weight', type=float, default=0.2)
    ap.add_argument('-attns_loss', action='store_true')
    ap.add_argument('-name', type=str, default=None)
    # this runner's own
    ap.add_argument('-enc_self_att', action='store_true',
                    help="the encoder's self-attention is live: the paper's feature->feature step, which the reference computes "
                         "and then discards (LAMP(enc_self_attn=True)); stored in the checkpoint's settings for run_eval")
    ap.add_argument('-attn_type', type=str, choices=['softmax', 'sigmoid'], default='softmax',
                    help="the decoder's attention: sigmoid gates every key on its own, no row normalisation (LAMP(dec_attn_type="
                         "'sigmoid')); the reference parses the flag and drops it (config_args.py:49, lamp/Layers.py:23-30), "
                         "here it does what it says; stored in the checkpoint's settings for run_eval")
    ap.add_argument('-label_bias', type=str, choices=['none', 'adj', 'logp'], default='none',
                    help="weighted label graph: an additive bias on the label->label attention scores from the train split's "
                         "co-occurrence counts (LAMP(label_bias=...)): adj = scale on every prior edge (with -label_mask none: "
                         "the soft prior), logp = scale * smoothed log P(j | i); stored in the checkpoint's settings for run_eval")
    ap.add_argument('-label_bias_scale', type=float, default=1.0)
    ap.add_argument('-learn_label_bias', action='store_true',
                    help="train the label graph: the score bias is a parameter (LAMP(learn_label_bias=True)), initialised from "
                         "-label_bias adj|logp or from zeros with none; -label_mask still decides which edges exist at all; "
                         "stored in the checkpoint's settings (and the bias in its weights) for run_eval")
    ap.add_argument('-tune_thresholds', type=str, choices=['f1', 'youden', 'balance'], default=None,
                    help="after each validation epoch fit one decision threshold per label on the valid predictions (lamp_amd/"
                         "metrics.py: tune_thresholds), report the test epoch's tuned_* figures and store label_thresholds / "
                         "tune_criterion in the checkpoint for run_eval -tune_thresholds checkpoint")
    ap.add_argument('-label_ranking', action='store_true',
                    help="reporting only: every epoch's train / valid / test metrics also carry LRAP, coverage_error, "
                         "ranking_loss, one_error and instance_AUC (lamp_amd/metrics.py: label_ranking); no change to the results "
                         "name, the checkpoint or losses.csv")
    ap.add_argument('-at_k', type=str, default='',
                    help="reporting only: comma-separated ranks, e.g. 1,3,5: every epoch's metrics also carry P@k, nDCG@k and R@k "
                         "(lamp_amd/metrics.py: rank_at_k; every k <= min(n_labels, 64)); no change to the results name, the "
                         "checkpoint or losses.csv")
    ap.add_argument('-loss_fn', type=str, choices=['bce', 'focal', 'asl', 'lsep', 'rank_hinge', 'rank_logistic'], default='bce',
                    help="the TRAINED objective (lamp_multilabel_loss_train, DESIGN.md section 8.10): focal = -focal_gamma on both "
                         "branches, asl = the asymmetric loss of -asl_gamma_pos / -asl_gamma_neg / -asl_clip; or a ranking loss "
                         "(lamp_rank_loss_train, section 8.12): lsep, rank_hinge (-rank_margin) or rank_logistic, each plus "
                         "-rank_bce_weight x the mean BCE, the train loss then a mean over samples.  Only the training "
                         "loss changes: the valid and test losses stay plain BCE, so -save_mode best and runs with different "
                         "objectives stay comparable; the train column of losses.csv is the trained loss")
    ap.add_argument('-focal_gamma', type=float, default=2.0, help='focal loss: the focusing exponent (0, or 1 .. 16)')
    ap.add_argument('-asl_gamma_pos', type=float, default=0.0, help='asymmetric loss: the exponent of the positives')
    ap.add_argument('-asl_gamma_neg', type=float, default=4.0, help='asymmetric loss: the exponent of the negatives')
    ap.add_argument('-asl_clip', type=float, default=0.05,
                    help='asymmetric loss: the probability margin in [0, 1); a negative predicted below it is discarded')
    ap.add_argument('-rank_margin', type=float, default=1.0, help='rank_hinge: the margin a positive must lead a negative by (>= 0)')
    ap.add_argument('-rank_bce_weight', type=float, default=0.0,
                    help='lsep / rank_hinge / rank_logistic: the weight of the mean BCE mixed into the ranking loss (>= 0)')
    ap.add_argument('-pos_weight', type=str, choices=['none', 'inv', 'sqrt_inv'], default='none',
                    help="per-label weights of the positives in the TRAINED loss, from the train split's label counts "
                         "(lamp_amd/data.py: label_pos_weight): inv = negatives / positives, sqrt_inv = its square root; "
                         "combines with bce, focal and asl (not with a ranking loss); the valid and test losses stay plain BCE")
    ap.add_argument('-pos_weight_cap', type=float, default=100.0, help='the largest weight, also given to a label without a positive')
    ap.add_argument('-max_grad_norm', type=float, default=None,
                    help='clip the gradient to this GLOBAL L2 norm before every update (DESIGN.md section 8.11): lamp = one '
                         'lamp_grad_norm launch, the factor applied inside the optimizer launch; torch = clip_grad_norm_')
    ap.add_argument('-weight_decay', type=float, default=None,
                    help='weight decay of every parameter with ndim >= 2 but decoder.label_bias (1-D parameters and the label '
                         'bias never decay): L2 with -optim adam / sgd, decoupled with -optim adamw (default there: 0.01)')
    ap.add_argument('-momentum', type=float, default=None, help='-optim sgd only: buf = momentum buf + g; w -= lr buf')
    ap.add_argument('-skip_nonfinite', action='store_true',
                    help='-optim_impl lamp only: a batch whose gradient norm is inf or NaN changes no weight and no moment (the '
                         "decision is taken on the device); the epoch's log line reports steps_skipped")
    ap.add_argument('-weight_avg', type=str, choices=['ema', 'swa'], default=None,
                    help='keep an average of the weights beside them (lamp_amd.optim.WeightAverage, DESIGN.md section 8.14; one '
                         'lamp_weight_average launch after every optimizer step, with either -optim_impl): ema = exponential '
                         'moving average with -ema_decay, swa = the running mean.  Once averaging has begun the valid and test '
                         "epochs run on the average, and the checkpoint holds it as 'model_avg' beside the trained 'model'")
    ap.add_argument('-ema_decay', type=float, default=0.999, help='-weight_avg ema: the decay, in [0, 1)')
    ap.add_argument('-ema_warmup', action='store_true',
                    help='-weight_avg ema: the decay of update t is min(-ema_decay, (1 + t) / (10 + t))')
    ap.add_argument('-avg_every', type=int, default=1, help='-weight_avg: average after every k-th optimizer step only')
    ap.add_argument('-avg_start_epoch', type=int, default=1,
                    help="-weight_avg: the 1-based epoch whose first step begins the average (SWA's usual last quarter of training)")
    ap.add_argument('-optim_impl', choices=['lamp', 'torch'], default=DEFAULT_OPTIM_IMPL,
                    help='lamp = lamp_amd.optim (one lamp_optim_step launch per step); torch = torch.optim (fused=True for adam)')
    ap.add_argument('-streams', type=int, default=4, choices=[1, 2, 3, 4], help='batches in flight in the valid / test epochs')
    ap.add_argument('-prefetch', type=int, default=8, help='batches per stage of the producer thread')
    ap.add_argument('-seed', type=int, default=0, help='torch.manual_seed: weight init, shuffling, dropout seeds')
    ap.add_argument('-gpus', type=int, default=1)
    opt = ap.parse_args(argv)
    try:
        opt.at_k = tuple(int(v) for v in opt.at_k.split(',') if v.strip())
    except ValueError:
        ap.error('-at_k takes comma-separated integers, e.g. 1,3,5')
    if any(k < 1 or k > 64 for k in opt.at_k):
        ap.error('-at_k: every k must lie in 1 .. 64')
    return derive(opt)


# torch's fused Adam: lamp_optim_step has not been shown to beat it same-box (nothing is measured yet; tools/bench_train_epoch.py
# is the tool that would), and without a measured win the default stays torch's.  (With clipping the lamp route is the shorter
# one -- DESIGN.md section 8.11, tools/bench_optim_ext.py -- which does not decide the plain case.)
DEFAULT_OPTIM_IMPL = 'torch'


# -loss_fn -> the flags that parameterise it (they enter the results name and the checkpoint's settings only with it)
LOSS_FN_FLAGS = {'bce': (), 'focal': ('focal_gamma',), 'asl': ('asl_gamma_pos', 'asl_gamma_neg', 'asl_clip'),
                 'lsep': ('rank_bce_weight',), 'rank_hinge': ('rank_margin', 'rank_bce_weight'), 'rank_logistic': ('rank_bce_weight',)}
# -loss_fn -> the kind of train.RankLossOptions (lamp_rank_loss_train)
RANK_LOSS_FNS = {'lsep': 'lsep', 'rank_hinge': 'hinge', 'rank_logistic': 'logistic'}


def loss_parameters(opt):
    """-loss_fn and its flags -> (gamma_pos, gamma_neg, clip) of lamp_multilabel_loss_train; ValueError for what it refuses."""
    from . import _native as N
    if opt.loss_fn in RANK_LOSS_FNS:
        raise ValueError('-loss_fn %s is a ranking loss: rank_loss_parameters' % opt.loss_fn)
    if opt.loss_fn == 'focal':
        return N.check_loss_options(opt.focal_gamma, opt.focal_gamma, 0.0)
    if opt.loss_fn == 'asl':
        return N.check_loss_options(opt.asl_gamma_pos, opt.asl_gamma_neg, opt.asl_clip)
    return N.check_loss_options()


def rank_loss_parameters(opt):
    """A ranking -loss_fn and its flags -> (kind, margin, bce_weight) of train.RankLossOptions; ValueError for what
    lamp_rank_loss_train refuses, and for -pos_weight beside it."""
    from . import _native as N
    kind = RANK_LOSS_FNS[opt.loss_fn]
    if getattr(opt, 'pos_weight', 'none') != 'none':
        raise ValueError('-pos_weight %s with -loss_fn %s: per-label positive weights belong to the BCE family (bce, focal, '
                         'asl); a ranking loss has none' % (opt.pos_weight, opt.loss_fn))
    margin = opt.rank_margin if kind == 'hinge' else 0.0
    N.check_rank_loss_options(kind, margin, opt.rank_bce_weight)
    return kind, margin, opt.rank_bce_weight


def build_rank_loss(opt):
    """-> the train.RankLossOptions of a ranking -loss_fn, or None."""
    if opt.loss_fn not in RANK_LOSS_FNS:
        return None
    from .train import RankLossOptions
    return RankLossOptions(*rank_loss_parameters(opt))


def build_loss_options(opt, data, device):
    """-> the train.LossOptions of -loss_fn / -pos_weight (the weights from the TRAIN split's label counts), or None for plain
    BCE -- train_batch then makes the call it has always made -- and for a ranking loss (build_rank_loss)."""
    if (opt.loss_fn == 'bce' and opt.pos_weight == 'none') or opt.loss_fn in RANK_LOSS_FNS:
        return None
    from .train import LossOptions
    w = None
    if opt.pos_weight != 'none':
        w = D.label_pos_weight(data['train']['tgt'], len(data['dict']['tgt']), device, opt.pos_weight, opt.pos_weight_cap)
    return LossOptions(*loss_parameters(opt), pos_weight=w)


OPTIM_CONTROL_FLAGS = ('max_grad_norm', 'weight_decay', 'momentum', 'skip_nonfinite')


def optimizer_controls(opt):
    """-max_grad_norm, -weight_decay, -momentum and -skip_nonfinite: normalised on `opt` (None / False = not given), what is
    not served refused, -> their part of the results name ('' without them)."""
    name = ''
    for flag, tag in (('max_grad_norm', 'clip'), ('weight_decay', 'wd'), ('momentum', 'mom')):
        v = getattr(opt, flag, None)
        v = None if v is None else float(v)
        setattr(opt, flag, v)
        if v is None:
            continue
        if not 0.0 <= v < float('inf'):
            raise ValueError('-%s %r: a finite number >= 0' % (flag, v))
        name += '.%s_%s' % (tag, v)
    opt.skip_nonfinite = bool(getattr(opt, 'skip_nonfinite', False))
    if opt.momentum is not None and (opt.optim != 'sgd' or opt.momentum >= 1.0):
        raise ValueError('-momentum %r: with -optim sgd only, and in [0, 1)' % (opt.momentum,))
    if opt.skip_nonfinite:
        if getattr(opt, 'optim_impl', DEFAULT_OPTIM_IMPL) != 'lamp':
            raise ValueError('-skip_nonfinite needs -optim_impl lamp: torch.optim has no way to leave a step out without '
                             'reading the gradient norm back')
        name += '.skipnf'
    return name


WEIGHT_AVG_FLAGS = ('weight_avg', 'ema_decay', 'ema_warmup', 'avg_every', 'avg_start_epoch')


def weight_average_controls(opt):
    """-weight_avg and its flags: normalised on `opt` (None = not given), what is not served refused, -> their part of the
    results name ('' without -weight_avg): .wavg_<kind>_<decay or 'swa'>[_w][_e<k>][_s<epoch>]."""
    opt.weight_avg = getattr(opt, 'weight_avg', None) or None
    if opt.weight_avg is None:
        return ''
    if opt.weight_avg not in ('ema', 'swa'):
        raise ValueError('-weight_avg %r: ema or swa' % (opt.weight_avg,))
    opt.ema_decay = float(getattr(opt, 'ema_decay', 0.999))
    opt.ema_warmup = bool(getattr(opt, 'ema_warmup', False))
    opt.avg_every = int(getattr(opt, 'avg_every', 1))
    opt.avg_start_epoch = int(getattr(opt, 'avg_start_epoch', 1))
    if not 0.0 <= opt.ema_decay < 1.0:
        raise ValueError('-ema_decay %r: a decay in [0, 1)' % (opt.ema_decay,))
    if opt.avg_every < 1:
        raise ValueError('-avg_every %r: an integer >= 1' % (opt.avg_every,))
    if opt.avg_start_epoch < 1:
        raise ValueError('-avg_start_epoch %r: epochs count from 1' % (opt.avg_start_epoch,))
    ema = opt.weight_avg == 'ema'
    name = '.wavg_%s_%s' % (opt.weight_avg, opt.ema_decay if ema else 'swa')
    if ema and opt.ema_warmup:
        name += '_w'
    if opt.avg_every != 1:
        name += '_e%d' % opt.avg_every
    if opt.avg_start_epoch != 1:
        name += '_s%d' % opt.avg_start_epoch
    return name


def build_weight_average(optimizer, opt):
    """-> the optim.WeightAverage of -weight_avg over every parameter the optimizer holds, or None without the flag."""
    if getattr(opt, 'weight_avg', None) is None:
        return None
    from . import optim
    params = [p for g in optimizer.param_groups for p in g['params']]
    return optim.WeightAverage(params, kind=opt.weight_avg, decay=opt.ema_decay if opt.weight_avg == 'ema' else 0.0,
                               warmup=opt.ema_warmup and opt.weight_avg == 'ema', update_every=opt.avg_every)


def derive(opt):
    """config_args.py:80-259 for the flags above."""
    if opt.gpus != 1:
        raise NotImplementedError('-gpus %d: multi-GPU training is out of scope here -- no gradient collective exists in this '
                                  'library (run_eval -gpus N shards evaluation, which needs none)' % opt.gpus)
    if opt.n_layers_dec is None:
        opt.n_layers_dec = opt.n_layers_enc
    opt.onehot = opt.dataset in ONEHOT_DATASETS
    if opt.test_batch_size <= 0:
        opt.test_batch_size = opt.batch_size
    if opt.d_v == -1:
        opt.d_v = int(opt.d_model / opt.n_head)
    if opt.d_k == -1:
        opt.d_k = int(opt.d_model / opt.n_head)
    if opt.dec_dropout == -1:
        opt.dec_dropout = opt.dropout
    if opt.dataset in ('bibtext', 'delicious', 'bookmarks', 'sider'):
        opt.no_enc_pos_embedding = True
    if opt.d_inner_hid == -1:
        opt.d_inner_hid = int(opt.d_model * 2)
    if opt.decoder in ('mlp', 'rnn_m'):
        opt.n_head = 1
        opt.d_k = opt.d_model
    name = 'enc_' + opt.encoder + '.dec_' + opt.decoder
    name += '.%s.%s.%s.%s' % (opt.d_model, opt.d_inner_hid, opt.d_k, opt.d_v)
    name += '.nlayers_%s_%s' % (opt.n_layers_enc, opt.n_layers_dec)
    name += '.nheads_' + str(opt.n_head)
    if opt.n_head2 == 0:
        opt.n_head2 = opt.n_head
    else:
        name += '_' + str(opt.n_head2)
    opt.proj_share_weight = opt.decoder != 'mlp'
    if opt.proj_share_weight:
        name += '.proj_share'
    name += '.bsz_' + str(opt.batch_size)
    name += '.loss_' + str(opt.loss)
    name += '.' + str(opt.optim)
    name += '.lr_' + str(opt.lr).split('.')[1]
    if opt.lr_decay > 0:
        name += '.decay_' + str(opt.lr_decay).replace('.', '') + '_' + str(opt.lr_step_size)
    name += '.drop_' + ('%.2f' % opt.dropout).split('.')[1] + '_' + ('%.2f' % opt.dec_dropout).split('.')[1]
    if opt.decoder == 'graph' and opt.no_dec_self_att:
        name += '.no_dec_self_att'
    if opt.decoder == 'graph' and not opt.no_dec_self_att:
        name += '.' + opt.label_mask + 'mask'
    opt.dec_dropout2 = False
    if opt.attns_loss:
        name += '.attns_loss'
    if opt.decoder == 'graph' and opt.int_preds:
        name += '.int_preds_' + str(opt.int_pred_weight).replace('.', '')
    else:
        opt.int_preds = False
    opt.enc_self_att = bool(getattr(opt, 'enc_self_att', False))
    if opt.enc_self_att:
        name += '.enc_self_att'
    opt.attn_type = getattr(opt, 'attn_type', None) or 'softmax'
    if opt.attn_type != 'softmax':
        name += '.attn_' + opt.attn_type
    opt.label_bias = getattr(opt, 'label_bias', None) or 'none'
    opt.label_bias_scale = float(getattr(opt, 'label_bias_scale', 1.0))
    if opt.label_bias != 'none':
        name += '.lbias_%s_%s' % (opt.label_bias, opt.label_bias_scale)
    opt.learn_label_bias = bool(getattr(opt, 'learn_label_bias', False))
    if opt.learn_label_bias:
        name += '.lbias_learn'
    opt.tune_thresholds = getattr(opt, 'tune_thresholds', None) or None
    if opt.tune_thresholds:
        name += '.thr_' + opt.tune_thresholds
    opt.loss_fn = getattr(opt, 'loss_fn', None) or 'bce'
    if opt.loss_fn not in LOSS_FN_FLAGS:
        raise ValueError("-loss_fn %r: one of %s" % (opt.loss_fn, ', '.join(sorted(LOSS_FN_FLAGS))))
    for flag, default in (('focal_gamma', 2.0), ('asl_gamma_pos', 0.0), ('asl_gamma_neg', 4.0), ('asl_clip', 0.05),
                          ('pos_weight_cap', 100.0), ('rank_margin', 1.0), ('rank_bce_weight', 0.0)):
        setattr(opt, flag, float(getattr(opt, flag, default)))
    opt.pos_weight = getattr(opt, 'pos_weight', None) or 'none'
    if opt.pos_weight not in ('none', 'inv', 'sqrt_inv'):
        raise ValueError("-pos_weight %r: none, inv or sqrt_inv" % (opt.pos_weight,))
    if opt.loss_fn in RANK_LOSS_FNS:
        rank_loss_parameters(opt)
    elif opt.loss_fn != 'bce':
        loss_parameters(opt)    # (refuses what the kernel does not serve, here and not in the first batch)
    if opt.loss_fn != 'bce':
        name += '.lossfn_%s_%s' % (opt.loss_fn, '_'.join(str(getattr(opt, f)) for f in LOSS_FN_FLAGS[opt.loss_fn]))
    if opt.pos_weight != 'none':
        if not 0.0 < opt.pos_weight_cap < float('inf'):
            raise ValueError('-pos_weight_cap %r: a positive finite number' % (opt.pos_weight_cap,))
        name += '.posw_%s_%s' % (opt.pos_weight, opt.pos_weight_cap)
    name += optimizer_controls(opt)
    name += weight_average_controls(opt)
    if opt.name:
        name += '.' + str(opt.name)
    opt.model_name = os.path.join(opt.results_dir, opt.dataset, name)
    opt.data_type = opt.dataset
    opt.d_word_vec = opt.d_model
    opt.matching_mlp = False
    if opt.decoder in ('mlp', 'sa_b', 'graph'):
        opt.binary_relevance = True
    elif opt.decoder in ('sa_m', 'rnn_m'):
        opt.binary_relevance = False
    if opt.encoder != 'graph' or opt.decoder != 'graph':
        raise NotImplementedError("run_train trains encoder='graph' with decoder='graph' (the binary-relevance branch, "
                                  "train.py:33-50); the '%s' encoder / '%s' decoder%s not served here" %
                                  (opt.encoder, opt.decoder, ' (crit / log-softmax branch, train.py:52-66) are'
                                   if not opt.binary_relevance else ' are'))
    if opt.d_model % opt.n_head:
        raise ValueError('d_model must be divisible by n_head')
    return opt


def build_model(opt, data, device):
    """main.py:53-88."""
    from .Models import LAMP
    n_src, n_labels = D.vocabulary_sizes(data)
    opt.src_vocab_size, opt.tgt_vocab_size = n_src, n_labels
    opt.max_token_seq_len_e = data['settings'].max_seq_len
    adj = (D.prior_adjacency_device(data['train']['tgt'], len(data['dict']['tgt']), device).cpu()
           if opt.label_mask == 'prior' else None)
    bias = D.build_label_bias(data, opt.label_bias, opt.label_bias_scale, device)
    return LAMP(n_src, n_labels, opt.max_token_seq_len_e, n_labels, proj_share_weight=opt.proj_share_weight,
                embs_share_weight=True, d_k=opt.d_k, d_v=opt.d_v, d_model=opt.d_model, d_word_vec=opt.d_word_vec,
                d_inner_hid=opt.d_inner_hid, n_layers_enc=opt.n_layers_enc, n_layers_dec=opt.n_layers_dec, n_head=opt.n_head,
                n_head2=opt.n_head2, dropout=opt.dropout, dec_dropout=opt.dec_dropout, dec_dropout2=opt.dec_dropout2,
                encoder=opt.encoder, decoder=opt.decoder, onehot=opt.onehot, no_enc_pos_embedding=opt.no_enc_pos_embedding,
                no_dec_self_att=opt.no_dec_self_att, loss=opt.loss, label_adj_matrix=adj, label_mask=opt.label_mask,
                int_preds=opt.int_preds, enc_self_attn=opt.enc_self_att,
                dec_attn_type=None if opt.attn_type == 'softmax' else opt.attn_type, label_bias=bias,
                learn_label_bias=opt.learn_label_bias)


def build_optimizer(model, opt):
    """main.py:99 (the reference builds this Adam whatever -optim says; -optim sgd gets the plain update here)."""
    params = list(model.get_trainable_parameters())
    controls = {f: getattr(opt, f, None) for f in OPTIM_CONTROL_FLAGS}
    if opt.optim != 'adamw' and all(v is None or v is False for v in controls.values()):
        # without the new flags: the optimizers this runner has always built, over one flat parameter list
        if opt.optim_impl == 'lamp':
            from . import optim
            return optim.Adam(params, betas=(0.9, 0.98), lr=opt.lr) if opt.optim == 'adam' else optim.SGD(params, lr=opt.lr)
        if opt.optim == 'adam':
            return torch.optim.Adam(params, betas=(0.9, 0.98), lr=opt.lr, fused=True)
        return torch.optim.SGD(params, lr=opt.lr)
    wd = controls['weight_decay']
    if wd is None:
        wd = 1e-2 if opt.optim == 'adamw' else 0.0       # (torch.optim.AdamW's default)
    groups = decay_param_groups(model, wd)
    clip, momentum = controls['max_grad_norm'], controls['momentum'] or 0.0
    if opt.optim_impl == 'lamp':
        from . import optim
        extra = dict(max_grad_norm=clip, skip_nonfinite=bool(controls['skip_nonfinite']))
        if opt.optim == 'sgd':
            return optim.SGD(groups, lr=opt.lr, momentum=momentum, **extra)
        return (optim.AdamW if opt.optim == 'adamw' else optim.Adam)(groups, betas=(0.9, 0.98), lr=opt.lr, **extra)
    if controls['skip_nonfinite']:
        raise ValueError('-skip_nonfinite needs -optim_impl lamp')
    if opt.optim == 'sgd':
        optimizer = torch.optim.SGD(groups, lr=opt.lr, momentum=momentum)
    else:
        optimizer = (torch.optim.AdamW if opt.optim == 'adamw' else torch.optim.Adam)(groups, betas=(0.9, 0.98), lr=opt.lr, fused=True)
    if clip is not None:      # in front of every step(), where the reference's loop would call it (no read-back: foreach, no check)
        clipped = [p for g in groups for p in g['params']]

        def clip_first(*_):
            torch.nn.utils.clip_grad_norm_(clipped, clip)

        optimizer.register_step_pre_hook(clip_first)
    return optimizer


def decay_param_groups(model, weight_decay):
    """-> [decay group, no-decay group] over model.get_trainable_parameters(): parameters with ndim >= 2 decay; 1-D parameters
    (biases, LayerNorm) and decoder.label_bias do not -- the learnable label graph holds -inf where an edge is blocked, and
    -inf must never meet weight_decay * w."""
    trainable = {id(p) for p in model.get_trainable_parameters()}
    decay, no_decay, seen = [], [], set()
    for name, p in model.named_parameters():
        if id(p) not in trainable or id(p) in seen:
            continue
        seen.add(id(p))
        (no_decay if p.ndim < 2 or name.endswith('label_bias') else decay).append(p)
    return [dict(params=decay, weight_decay=float(weight_decay)), dict(params=no_decay, weight_decay=0.0)]


def checkpoint_settings(opt):
    """The Namespace that travels in the checkpoint: plain values only, so that it unpickles anywhere.  `learn_label_bias`
    and `tune_thresholds` travel only when they are set: without the flags the settings are what they were before they
    existed.  Likewise `loss_fn` with the flags of the chosen objective, and `pos_weight` with its cap."""
    drop = {'loss_options', 'rank_loss', 'weight_average'}      # (the run's own objects, None by default: never a setting)
    if getattr(opt, 'weight_avg', None) is None:      # (-weight_avg's flags travel with it, never without)
        drop.update(WEIGHT_AVG_FLAGS)
    drop.update(('label_ranking', 'at_k'))    # (reporting only: a checkpoint does not depend on what was printed beside it)
    loss_fn = getattr(opt, 'loss_fn', 'bce')
    if loss_fn == 'bce':
        drop.add('loss_fn')
    for fn, flags in LOSS_FN_FLAGS.items():
        if fn != loss_fn:
            drop.update(f for f in flags if f not in LOSS_FN_FLAGS.get(loss_fn, ()))
    if getattr(opt, 'pos_weight', 'none') == 'none':
        drop.update(('pos_weight', 'pos_weight_cap'))
    for f in OPTIM_CONTROL_FLAGS:      # (set flags travel, unset ones never)
        if getattr(opt, f, None) is None or getattr(opt, f) is False:
            drop.add(f)
    return argparse.Namespace(**{k: v for k, v in vars(opt).items() if isinstance(v, (bool, int, float, str, type(None)))
                                 and (k not in ('learn_label_bias', 'tune_thresholds') or v) and k not in drop})


def save_model(opt, epoch_i, model, valid_loss, valid_losses, label_thresholds=None, weight_average=None):
    """utils/utils.py:228-241, `>=` included (see the module docstring).  -> the path written, or None.  With
    -tune_thresholds the epoch's fitted thresholds travel beside the weights.  With -weight_avg (`weight_average`, not
    swapped in): 'weight_avg', the average's state without its buffers, and -- once it holds an average -- 'model_avg', the
    state dict with the averaged weights; 'model' stays what was trained."""
    checkpoint = {'model': model.state_dict(), 'settings': checkpoint_settings(opt), 'epoch': epoch_i}
    if weight_average is not None:
        checkpoint['weight_avg'] = weight_average.state_dict(buffers=False)
        if weight_average.n_averaged > 0:
            checkpoint['model_avg'] = weight_average.averaged_state_dict(model)
    if label_thresholds is not None:
        checkpoint['label_thresholds'] = label_thresholds.detach().to('cpu', torch.float32).contiguous()
        checkpoint['tune_criterion'] = opt.tune_thresholds
    if opt.save_mode == 'all':
        path = opt.model_name + '/accu_{accu:3.3f}.chkpt'.format(accu=100 * valid_loss)
        torch.save(checkpoint, path)
        return path
    if opt.save_mode == 'best':
        path = opt.model_name + '/model.chkpt'
        if valid_loss >= min(valid_losses):
            torch.save(checkpoint, path)
            return path
    return None


def _json_metrics(m):
    return {k: (v.tolist() if hasattr(v, 'tolist') else v) for k, v in m.items() if k not in ('allAUC', 'allAUPR')}


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    opt = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit('lamp_amd.run_train needs an MI355X: no HIP device visible (there is no CPU path)')
    from . import hostcpu
    from .evaluate import test_epoch
    from .metrics import compute_metrics, tune_thresholds
    from .train import TrainBatcher, train_epoch
    hostcpu.fit_intra_op_threads()
    device = torch.device('cuda', torch.cuda.current_device())
    data = D.load_dataset(opt.data)
    torch.manual_seed(opt.seed)
    model = build_model(opt, data, device)
    opt.total_num_parameters = int(sum(p.numel() for p in model.parameters() if p.requires_grad))
    model = model.to(device)       # (before the optimizer: torch's fused Adam wants device parameters at construction)
    optimizer = build_optimizer(model, opt)
    opt.loss_options = build_loss_options(opt, data, device)      # (None for plain BCE; never part of the checkpoint's settings)
    opt.rank_loss = build_rank_loss(opt)                          # (likewise; None unless -loss_fn is a ranking loss)
    wavg = build_weight_average(optimizer, opt)                   # (None without -weight_avg: nothing below then differs)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=opt.lr_step_size, gamma=opt.lr_decay, last_epoch=-1)
    os.makedirs(opt.model_name, exist_ok=True)
    if opt.load_pretrained:   # main.py:117-119
        ckpt = torch.load(opt.model_name + '/model.chkpt', map_location='cpu', weights_only=False)
        model.load_state_dict(ckpt['model'])
    train_data = TrainBatcher(data['train']['src'], data['train']['tgt'], opt.batch_size, shuffle=True, drop_last=True)
    valid_data = D.EvalBatcher(data['valid']['src'], data['valid']['tgt'], opt.test_batch_size)
    test_data = D.EvalBatcher(data['test']['src'], data['test']['tgt'], opt.test_batch_size)
    n_labels = opt.tgt_vocab_size
    valid_losses, history = [], []
    report = {}                    # -label_ranking / -at_k: more keys in the per-epoch metrics, nothing else
    if getattr(opt, 'label_ranking', False):
        report['label_ranking'] = True
    if getattr(opt, 'at_k', ()):
        report['at_k'] = tuple(opt.at_k)
    skipped_before = 0
    with open(os.path.join(opt.model_name, 'losses.csv'), 'w+') as loss_file:
        for epoch_i in range(opt.epoch):
            if scheduler and opt.lr_decay > 0:   # runner.py:38
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    scheduler.step()
            out = {'epoch': epoch_i + 1, 'lr': optimizer.param_groups[0]['lr']}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            on_dev = {}
            if wavg is not None and epoch_i + 1 >= opt.avg_start_epoch:
                opt.weight_average = wavg                         # (train_batch updates it after every optimizer.step())
            _, _, train_loss = train_epoch(model, train_data, optimizer, opt, device=device, prefetch=opt.prefetch,
                                           device_results=on_dev)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            train_loss = train_loss / train_data.n_insts
            metrics = {'train': compute_metrics(on_dev['probs'], on_dev['targets'], train_loss, opt.br_threshold, dt / 60,
                                                **report)}
            out.update(train_loss=train_loss, train_seconds=dt,
                       train_samples_per_s=sum(real for _, real in on_dev['batches']) / dt)
            if opt.skip_nonfinite:      # (the loop has synchronised above: the device counter's first and only read-back)
                skipped = getattr(optimizer, 'skipped_steps', None)
                total = int(skipped.item()) if skipped is not None else 0
                out['steps_skipped'], skipped_before = total - skipped_before, total
            losses = {}
            label_thresholds = None
            # once averaging has begun, valid and test (thresholds, -at_k and -label_ranking with them, and the loss -save_mode
            # best compares) are the averaged model's: swapped in here, swapped back below, also on an exception
            averaged = wavg is not None and wavg.n_averaged > 0
            with (wavg.applied() if averaged else contextlib.nullcontext()):
                for split, batches in (('valid', valid_data), ('test', test_data)):
                    t0 = time.perf_counter()
                    on_dev = {}
                    _, _, loss = test_epoch(model, batches, n_labels, opt.test_batch_size, device, streams=opt.streams,
                                            prefetch=opt.prefetch, int_preds=opt.int_preds, device_results=on_dev)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    losses[split] = loss / batches.n_insts
                    metrics[split] = compute_metrics(on_dev['probs'], on_dev['targets'], losses[split], opt.br_threshold, dt / 60,
                                                     **report)
                    if opt.tune_thresholds and split == 'valid':   # (valid comes first: the test epoch below uses them)
                        fit = tune_thresholds(on_dev['probs'], on_dev['targets'], opt.tune_thresholds, opt.br_threshold)
                        label_thresholds = fit['threshold']
                        out['n_labels_tuned'] = int(fit['tuned'].sum())
                        out['tune_criterion'] = opt.tune_thresholds
                    if label_thresholds is not None and split == 'test':
                        tuned = compute_metrics(on_dev['probs'], on_dev['targets'], losses[split], opt.br_threshold, dt / 60,
                                                all_metrics=False, thresholds=label_thresholds)
                        metrics[split].update({'tuned_' + k: tuned[k] for k in ('ACC', 'HA', 'ebF1', 'miF1', 'maF1')})
                    out['%s_loss' % split] = losses[split]
                    out['%s_samples_per_s' % split] = batches.n_insts / dt
            valid_losses.append(losses['valid'])
            if wavg is not None:
                out['weights'] = 'avg' if averaged else 'raw'
            out['metrics'] = {k: _json_metrics(v) for k, v in metrics.items()}
            out['checkpoint'] = None
            if 'test' not in opt.model_name:   # runner.py:85
                out['checkpoint'] = save_model(opt, epoch_i, model, losses['valid'], valid_losses, label_thresholds, wavg)
            loss_file.write('%d,%s,%s,%s\n' % (epoch_i + 1, train_loss, losses['valid'], losses['test']))
            loss_file.flush()
            history.append(out)
            print(json.dumps(out), flush=True)
    return history


if __name__ == '__main__':
    main()
