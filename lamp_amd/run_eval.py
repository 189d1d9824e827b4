"""Evaluation runner: the `main.py -test_only` flow of the reference for encoder=graph / decoder=graph,
on the MI355X path.

    python -m lamp_amd.run_eval -data data/reuters/train_valid_test.pt -dataset reuters \
           -d_model 512 -d_inner_hid 512 -n_layers_enc 2 -n_head 4 -label_mask prior \
           [-checkpoint results/.../model.chkpt] [-split test] [-batch_size 32] [-streams 2] [-gpus N] [-all_metrics]
           [-at_k 1,3,5] [-label_ranking] [-tune_thresholds f1|youden|balance|checkpoint [-tune_split valid] [-tune_scope label|global]]

-gpus N starts one process per GPU (rendezvous on 127.0.0.1; "nccl" = RCCL for the final gather only); every rank
evaluates its contiguous share of the batches -- the forward path needs no collective (lamp_amd/sharding.py).

Flag names and derived defaults follow the reference's config_args.py (single-dash flags; n_layers_dec =
n_layers_enc :87-88, d_k = d_v = d_model / n_head :96-99, d_inner_hid = 2 d_model :110-111, no position
embedding for bibtext / delicious / bookmarks / sider :104-105, n_head2 = n_head :135-136; -n_head2, -d_k and -d_v
as run_train stored them in the checkpoint's settings take precedence over the flags and the defaults).  The model is
built from the dataset exactly as main.py:53-88 does (vocabulary sizes, max sequence length, prior label
adjacency from the train split).  Metrics are the thresholded multi-label basics the reference prints first
(utils/evals.py:316-372: subset accuracy, Hamming accuracy, example-/micro-/macro-F1 at -br_threshold, with the
reference's conventions for empty samples / labels); with -all_metrics also the ranking metrics the reference computes with
all_metrics=True (:208-298: mean / median AUC, AUPR and recall at FDR <= 0.5 over the labels, and the per-label arrays), on the
device (lamp_amd/metrics.py); with -at_k 1,3,5 precision, nDCG and recall at those ranks, each sample's labels ranked on
the device in the order include/lamp_hip.h defines (the figures are printed on stderr and join the JSON result line); with
-label_ranking the label-ranking metrics of whole rows (lamp_amd/metrics.py: label_ranking; DESIGN.md section 8.13: LRAP,
coverage_error, ranking_loss, one_error, instance_AUC and the row counts n_with_gold, n_with_both, n_rows_with_nan), printed
and joined to the JSON line in the same way, with label_ranking_seconds.
With -tune_thresholds f1|youden|balance the -tune_split (valid) is evaluated first and one decision threshold per label is
fitted on it on the device (lamp_amd/metrics.py: tune_thresholds), then -split is evaluated as always and
the five thresholded figures at the fitted thresholds join the JSON line as tuned_ACC, tuned_HA, tuned_ebF1, tuned_miF1 and
tuned_maF1, with tune_criterion, tune_split, n_labels_tuned, thresholds (a list; Infinity = the label is never predicted) and
tune_seconds; the figures at -br_threshold stay.  -tune_thresholds checkpoint takes the thresholds run_train -tune_thresholds
stored in the checkpoint.
-weights auto|raw|avg picks between the trained weights ('model') and the EMA / SWA average ('model_avg') of a
run_train -weight_avg checkpoint; auto, the default, takes the average when the checkpoint has one, and the JSON line then
carries "weights": "avg".  A checkpoint without the key loads as it always has.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch

from . import data as D
from . import sharding
from .evaluate import test_epoch
from .Models import LAMP


ONEHOT_DATASETS = ('deepsea', 'gm12878', 'gm12878_unique2', 'gm12878_unique', 'tcell')


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('-data', required=True, help='train_valid_test.pt in the reference format')
    ap.add_argument('-dataset', default='', help='dataset name (used for the no-position-embedding and one-hot rules)')
    ap.add_argument('-checkpoint', default=None, help="reference checkpoint: {'model': state_dict, ...}")
    ap.add_argument('-split', default='test', choices=['train', 'valid', 'test'])
    ap.add_argument('-batch_size', type=int, default=32)
    ap.add_argument('-d_model', type=int, default=512)
    ap.add_argument('-d_inner_hid', type=int, default=-1)
    ap.add_argument('-n_layers_enc', type=int, default=5)
    ap.add_argument('-n_layers_dec', type=int, default=None)
    ap.add_argument('-n_head', type=int, default=4)
    ap.add_argument('-n_head2', type=int, default=0)
    ap.add_argument('-d_k', type=int, default=-1,
                    help="width of a query / key head (default d_model / n_head); a run_train checkpoint brings -d_k, -d_v and "
                         "-n_head2 in its settings, the flags are for bare state dicts")
    ap.add_argument('-d_v', type=int, default=-1, help='width of a value head (default d_model / n_head)')
    ap.add_argument('-label_mask', default='none', choices=['none', 'inveye', 'prior'])
    ap.add_argument('-no_dec_self_att', action='store_true')
    ap.add_argument('-no_enc_pos_embedding', action='store_true')
    ap.add_argument('-br_threshold', type=float, default=0.5)
    ap.add_argument('-enc_self_att', action='store_true',
                    help="the encoder's self-attention is live (LAMP(enc_self_attn=True)); a run_train checkpoint brings the flag "
                         "in its settings, this is for bare state dicts")
    ap.add_argument('-attn_type', type=str, choices=['softmax', 'sigmoid'], default='softmax',
                    help="the decoder's attention (LAMP(dec_attn_type=...)); a run_train checkpoint brings the setting, this is for "
                         "bare state dicts")
    ap.add_argument('-label_bias', type=str, choices=['none', 'adj', 'logp'], default='none',
                    help="weighted label graph (LAMP(label_bias=...)), rebuilt from the train split as the prior mask is; a "
                         "run_train checkpoint brings the setting, this is for bare state dicts")
    ap.add_argument('-label_bias_scale', type=float, default=1.0)
    ap.add_argument('-matmul_precision', type=str, choices=['highest', 'high', 'bf16x6'], default='highest',
                    help="LAMP.matmul_precision: the forward's nn.Linear-class GEMMs on the fp32 matrix pipe ('highest'), as three "
                         "bf16 products per fp32 product ('high') or as six ('bf16x6'); attention, the chain launch and the "
                         "read-out stay fp32")
    ap.add_argument('-streams', type=int, default=4, choices=[1, 2, 3, 4],
                    help='batches in flight (HIP streams); 4 measured best: 36.6 k / 43.3 k / 46.2 k samples/s with 1 / 2 / 4 on a '
                         'reuters-sized split (tools/bench_eval_epoch.py)')
    ap.add_argument('-prefetch', type=int, default=8, help='batches per stage of the evaluation epoch (padded by the producer thread while the device runs the previous stage)')
    ap.add_argument('-merge_stages', action='store_true',
                    help='one forward per stage instead of one per batch (same predictions, targets and losses bit for bit)')
    ap.add_argument('-all_metrics', action='store_true',
                    help='also report meanAUC / medianAUC / meanAUPR / medianAUPR / meanFDR / medianFDR and the per-label allAUC / '
                         'allAUPR (computed on the device; with -gpus N by rank 0 after the combine)')
    ap.add_argument('-at_k', type=str, default='',
                    help='comma-separated ranks, e.g. 1,3,5: also report precision (P@k), nDCG@k and recall (R@k) at those k, each '
                         "sample's labels ranked on the device (lamp_amd/metrics.py: rank_at_k; every k <= min(n_labels, 64)); "
                         'independent of -all_metrics; with -gpus N by rank 0 after the combine')
    ap.add_argument('-label_ranking', action='store_true',
                    help='also report LRAP, coverage_error, ranking_loss, one_error and instance_AUC, from the rank of every gold '
                         "label among all labels of its sample, on the device (lamp_amd/metrics.py: label_ranking); independent "
                         'of -all_metrics and -at_k; with -gpus N by rank 0 after the combine')
    ap.add_argument('-tune_thresholds', type=str, choices=['f1', 'youden', 'balance', 'checkpoint'], default=None,
                    help='fit one decision threshold per label on -tune_split under this criterion (lamp_amd/metrics.py: '
                         "tune_thresholds) and also report the thresholded figures of -split at them (tuned_*); 'checkpoint' takes "
                         'the thresholds run_train -tune_thresholds stored in -checkpoint; with -gpus N rank 0 tunes on what it '
                         'gathered')
    ap.add_argument('-tune_split', default='valid', choices=['train', 'valid', 'test'], help='the split the thresholds are fitted on')
    ap.add_argument('-tune_scope', default='label', choices=['label', 'global'],
                    help='label = one threshold per label; global = one threshold for all labels, fitted on the flattened matrix')
    ap.add_argument('-weights', type=str, choices=['auto', 'raw', 'avg'], default='auto',
                    help="which weights of a run_train -weight_avg checkpoint to evaluate: avg = 'model_avg' (the EMA / SWA "
                         "average), raw = 'model' (as trained), auto = model_avg when the checkpoint has it, model otherwise -- "
                         'every checkpoint without the key loads as it always has')
    ap.add_argument('-seed', type=int, default=0, help='weight init seed when no checkpoint is given')
    ap.add_argument('-gpus', type=int, default=1, help='processes (one per GPU) the batches are sharded over')
    opt = ap.parse_args(argv)
    if opt.n_layers_dec is None:
        opt.n_layers_dec = opt.n_layers_enc
    if opt.d_inner_hid == -1:
        opt.d_inner_hid = 2 * opt.d_model
    if opt.n_head2 == 0:
        opt.n_head2 = opt.n_head
    if opt.d_k == -1:
        opt.d_k = opt.d_model // opt.n_head
    if opt.d_v == -1:
        opt.d_v = opt.d_model // opt.n_head
    if opt.dataset in ('bibtext', 'delicious', 'bookmarks', 'sider'):
        opt.no_enc_pos_embedding = True
    try:
        opt.at_k = tuple(int(v) for v in opt.at_k.split(',') if v.strip())
    except ValueError:
        ap.error('-at_k takes comma-separated integers, e.g. 1,3,5')
    if any(k < 1 or k > 64 for k in opt.at_k):
        ap.error('-at_k: every k must lie in 1 .. 64')
    # config_args.py:90-91: the genomics datasets read DNA through the one-hot / Conv1d encoder
    opt.onehot = opt.dataset in ONEHOT_DATASETS
    if opt.onehot and opt.merge_stages:
        ap.error('-merge_stages changes the padded length, hence the results, of a one-hot model')
    if opt.d_model % opt.n_head:
        ap.error('d_model must be divisible by n_head')
    return opt


def multilabel_metrics(pred, target, threshold):
    """Thresholded metrics on (n, L) cpu tensors, with the conventions of the reference's utils/evals.py:
    example-based F1 averages only over samples with at least one gold or predicted label (example_f1_score
    :105-123 deletes zero denominators), macro-F1 only over labels with tp + fp + fn > 0 (f1_score_from_stats
    :141-147 drops the non-finite ratios).  Rows with NaN predictions are counted as all-negative."""
    p = (torch.nan_to_num(pred, nan=0.0) >= threshold).double()
    t = target.double()
    tp = (p * t).sum(0)
    fp = (p * (1 - t)).sum(0)
    fn = ((1 - p) * t).sum(0)
    ex_tp = (p * t).sum(1)
    ex_den = p.sum(1) + t.sum(1)
    ex_ok = ex_den > 0
    lab_den = 2 * tp + fp + fn
    lab_ok = lab_den > 0
    nan = float('nan')
    return {
        'subset_accuracy': (p == t).all(dim=1).double().mean().item(),
        'hamming_accuracy': (p == t).double().mean().item(),
        'example_f1': (2 * ex_tp[ex_ok] / ex_den[ex_ok]).mean().item() if ex_ok.any() else nan,
        'micro_f1': (2 * tp.sum() / lab_den.sum()).item() if lab_den.sum() > 0 else nan,
        'macro_f1': (2 * tp[lab_ok] / lab_den[lab_ok]).mean().item() if lab_ok.any() else nan,
    }


def load_checkpoint_state(path):
    """state_dict of a reference checkpoint ({'model': state_dict, ...} or a bare state_dict).  Hosts with more than
    one GPU save from inside nn.DataParallel (main.py:106-108 before utils.save_model): `module.`-prefixed keys, which
    LAMP.load_state_dict strips."""
    return load_checkpoint(path)[0]


def load_checkpoint(path):
    """(state_dict, enc_self_att) of a checkpoint: the flag is run_train's `-enc_self_att` as stored in the checkpoint's
    'settings'; a checkpoint without the setting (the reference's, a bare state_dict) has it off."""
    return load_checkpoint_settings(path)[:2]


def load_checkpoint_settings(path):
    """(state_dict, enc_self_att, attn_type) of a checkpoint: run_train's `-enc_self_att` and `-attn_type` as stored in the
    checkpoint's 'settings'; a checkpoint without a field (an earlier run_train's, the reference's, a bare state_dict) has the
    encoder's self-attention off and a softmax decoder."""
    return checkpoint_settings(load_checkpoint_object(path))


def load_checkpoint_object(path):
    """The checkpoint file as saved: read once, then handed to checkpoint_settings and load_checkpoint_label_bias."""
    return torch.load(path, map_location='cpu', weights_only=False)


def checkpoint_settings(ckpt):
    """load_checkpoint_settings of an already loaded checkpoint."""
    if isinstance(ckpt, dict) and 'model' in ckpt:
        settings = ckpt.get('settings')
        return (ckpt['model'], bool(getattr(settings, 'enc_self_att', False)),
                getattr(settings, 'attn_type', None) or 'softmax')
    return ckpt, False, 'softmax'


def checkpoint_weights(ckpt, which='auto'):
    """(state_dict, averaged) of a LOADED checkpoint under -weights: 'raw' = ckpt['model'] (or a bare state dict itself), 'avg'
    = ckpt['model_avg'], the average run_train -weight_avg stored -- a ValueError naming the key where it is absent -- and
    'auto' = the average when there is one."""
    if which not in ('auto', 'raw', 'avg'):
        raise ValueError("-weights %r: auto, raw or avg" % (which,))
    wrapped = isinstance(ckpt, dict) and 'model' in ckpt
    has_avg = wrapped and ckpt.get('model_avg') is not None
    if which == 'avg' and not has_avg:
        raise ValueError("-weights avg: the checkpoint holds no 'model_avg' (run_train -weight_avg ema|swa stores it once "
                         "averaging has begun)")
    if has_avg and which != 'raw':
        return ckpt['model_avg'], True
    return (ckpt['model'] if wrapped else ckpt), False


def load_checkpoint_label_bias(ckpt):
    """(kind, scale) of run_train's `-label_bias` / `-label_bias_scale` as stored in the 'settings' of a LOADED checkpoint
    (load_checkpoint_object), or None for one that says nothing about it (an earlier run_train's, the reference's, a bare
    state_dict)."""
    settings = ckpt.get('settings') if isinstance(ckpt, dict) and 'model' in ckpt else None
    kind = getattr(settings, 'label_bias', None)
    if kind is None:
        return None
    return kind, float(getattr(settings, 'label_bias_scale', 1.0))


def load_checkpoint_learn_label_bias(ckpt):
    """Whether a LOADED checkpoint (load_checkpoint_object) holds a trained label graph (run_train -learn_label_bias): its
    'settings' say so, or -- a bare state_dict, saved from an nn.DataParallel wrapper or not -- its weights hold
    `decoder.label_bias`.  The bias then comes from the weights and is not rebuilt from the train split."""
    if isinstance(ckpt, dict) and 'model' in ckpt:
        if bool(getattr(ckpt.get('settings'), 'learn_label_bias', False)):
            return True
        ckpt = ckpt['model']
    return isinstance(ckpt, dict) and ('decoder.label_bias' in ckpt or 'module.decoder.label_bias' in ckpt)


def load_checkpoint_head_geometry(ckpt):
    """{'n_head2' / 'd_k' / 'd_v': value} for each of run_train's `-n_head2`, `-d_k` and `-d_v` that the 'settings' of a LOADED
    checkpoint (load_checkpoint_object) carry as a positive integer; empty for one that says nothing about them (a bare
    state_dict).  run_train and the reference store all three, derived defaults included."""
    settings = ckpt.get('settings') if isinstance(ckpt, dict) and 'model' in ckpt else None
    out = {}
    for key in ('n_head2', 'd_k', 'd_v'):
        value = getattr(settings, key, None)
        if isinstance(value, int) and not isinstance(value, bool) and value > 0:
            out[key] = value
    return out


def spawn_ranks(n, argv):
    """One process per GPU, each re-running this module with RANK / WORLD_SIZE set; rank 0 prints the result."""
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, '-m', 'lamp_amd.run_eval'] + list(argv), env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    alive = list(procs)
    while alive:
        time.sleep(0.05)
        for p in list(alive):
            code = p.poll()
            if code is None:
                continue
            alive.remove(p)
            if code != 0:
                rc = rc or code
                for q in alive:   # a dead rank leaves the others in a collective: stop exactly the ones we started
                    q.terminate()
    return rc


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    opt = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit('lamp_amd.run_eval needs an MI355X: no HIP device visible (there is no CPU path)')
    if opt.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        rc = spawn_ranks(opt.gpus, argv)
        if rc:
            raise SystemExit(rc)
        return None
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    dev_index = int(os.environ.get('LOCAL_RANK', '0')) % torch.cuda.device_count() if world > 1 else torch.cuda.current_device()
    torch.cuda.set_device(dev_index)
    device = torch.device('cuda', dev_index)
    if world > 1:   # this rank's issue loop and host threads on the cores next to its device (sharding.pin_rank_to_device_cpus)
        sharding.pin_rank_to_device_cpus(int(os.environ.get('LOCAL_RANK', '0')), int(os.environ.get('LOCAL_WORLD_SIZE', world)))
    # gloo rendezvous + an RCCL group for the final gather when RCCL comes up (probed; falls back to gloo and says so);
    # LAMP_EVAL_BACKEND=gloo lets several ranks share one GPU (tests)
    plane = sharding.ControlPlane(rank, world, device, os.environ.get('LAMP_EVAL_BACKEND', 'nccl'))
    data = D.load_dataset(opt.data)
    n_src, n_labels = D.vocabulary_sizes(data)
    adj = (D.prior_adjacency_device(data['train']['tgt'], len(data['dict']['tgt']), device).cpu()
           if opt.label_mask == 'prior' else None)
    d, h = opt.d_model, opt.n_head
    torch.manual_seed(opt.seed)
    ckpt = load_checkpoint_object(opt.checkpoint) if opt.checkpoint else None
    state, live, attn_type = checkpoint_settings(ckpt) if ckpt is not None else (None, False, 'softmax')
    averaged = False
    if ckpt is not None or opt.weights == 'avg':
        try:
            state, averaged = checkpoint_weights(ckpt, opt.weights)
        except ValueError as e:
            raise SystemExit('%s: %s' % (opt.checkpoint or 'no -checkpoint was given', e))
    live = live or opt.enc_self_att
    if opt.attn_type != 'softmax':
        attn_type = opt.attn_type
    bias_kind, bias_scale = opt.label_bias, opt.label_bias_scale
    stored = load_checkpoint_label_bias(ckpt)
    geometry = dict(n_head2=opt.n_head2, d_k=opt.d_k, d_v=opt.d_v)
    geometry.update(load_checkpoint_head_geometry(ckpt))   # the checkpoint's settings override the flags
    learn = load_checkpoint_learn_label_bias(ckpt)
    stored_thresholds = ckpt.get('label_thresholds') if isinstance(ckpt, dict) and 'model' in ckpt else None
    stored_criterion = ckpt.get('tune_criterion') if isinstance(ckpt, dict) and 'model' in ckpt else None
    del ckpt
    if opt.tune_thresholds == 'checkpoint' and stored_thresholds is None:
        raise SystemExit('-tune_thresholds checkpoint: %s holds no label_thresholds (run_train -tune_thresholds f1|youden|balance '
                         'stores them)' % (opt.checkpoint or 'no -checkpoint was given, and a run without one'))
    if stored is not None:   # the checkpoint's settings override the flags
        bias_kind, bias_scale = stored
    # a trained label graph is among the weights (decoder.label_bias): nothing to rebuild but the mask above
    bias = None if learn else D.build_label_bias(data, bias_kind, bias_scale, device)
    model = LAMP(n_src, n_labels, data['settings'].max_seq_len, n_labels, n_layers_enc=opt.n_layers_enc,
                 n_layers_dec=opt.n_layers_dec, n_head=h, n_head2=geometry['n_head2'], d_word_vec=d, d_model=d,
                 d_inner_hid=opt.d_inner_hid, d_k=geometry['d_k'], d_v=geometry['d_v'], encoder='graph', decoder='graph',
                 no_enc_pos_embedding=opt.no_enc_pos_embedding, no_dec_self_att=opt.no_dec_self_att,
                 label_adj_matrix=adj, label_mask=opt.label_mask, dec_dropout2=False, onehot=opt.onehot, enc_self_attn=live,
                 dec_attn_type=None if attn_type == 'softmax' else attn_type, label_bias=bias,
                 learn_label_bias=learn)
    if state is not None:
        model.load_state_dict(state)
    model = model.to(device).eval()
    model.matmul_precision = opt.matmul_precision
    tuned = None
    if opt.tune_thresholds == 'checkpoint':
        thresholds = torch.as_tensor(stored_thresholds, dtype=torch.float32).reshape(-1)
        if thresholds.numel() != n_labels:
            raise SystemExit('-tune_thresholds checkpoint: %d stored thresholds for %d labels' % (thresholds.numel(), n_labels))
        tuned = {'thresholds': thresholds.to(device), 'tune_criterion': stored_criterion, 'tune_split': None,
                 'n_labels_tuned': None, 'tune_seconds': 0.0}
    elif opt.tune_thresholds:
        from .metrics import tune_thresholds
        t1 = time.perf_counter()
        tune_batches = D.EvalBatcher(data[opt.tune_split]['src'], data[opt.tune_split]['tgt'], opt.batch_size)
        tune_dev = {} if world == 1 else None
        tune_preds, tune_targets, _ = test_epoch(model, tune_batches, n_labels, opt.batch_size, device, streams=opt.streams,
                                                 prefetch=opt.prefetch, merge_stage=opt.merge_stages, world_size=world,
                                                 rank=rank, group=plane.group, device_results=tune_dev)
        if rank == 0:
            fit = (tune_thresholds(tune_dev['probs'], tune_dev['targets'], opt.tune_thresholds, opt.br_threshold, opt.tune_scope)
                   if tune_dev else tune_thresholds(tune_preds.to(device), tune_targets.to(device), opt.tune_thresholds,
                                                    opt.br_threshold, opt.tune_scope))
            tuned = {'thresholds': fit['threshold'].contiguous(), 'tune_criterion': opt.tune_thresholds,
                     'tune_split': opt.tune_split, 'n_labels_tuned': int(fit['tuned'].sum()),
                     'tune_seconds': time.perf_counter() - t1}
        del tune_preds, tune_targets, tune_dev
    split = data[opt.split]
    batches = D.EvalBatcher(split['src'], split['tgt'], opt.batch_size)
    torch.cuda.synchronize()
    # one rank holds the whole split: nothing goes back up
    on_device = {} if (opt.all_metrics or opt.at_k or opt.label_ranking or opt.tune_thresholds) and world == 1 else None
    t0 = time.perf_counter()
    preds, targets, bce_total = test_epoch(model, batches, n_labels, opt.batch_size, device, streams=opt.streams,
                                           prefetch=opt.prefetch, merge_stage=opt.merge_stages,
                                           world_size=world, rank=rank, group=plane.group,
                                           device_results=on_device)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {'split': opt.split, 'n_samples': batches.n_insts, 'n_labels': n_labels, 'n_batches': len(batches),
           'bce_total': bce_total, 'seconds': dt, 'samples_per_s': batches.n_insts / dt,
           'checkpoint': opt.checkpoint, 'onehot': opt.onehot, 'matmul_precision': model.matmul_precision, 'n_gpus': world, 'backend': plane.backend, 'backend_note': plane.note}
    if averaged:
        out['weights'] = 'avg'
    out.update(multilabel_metrics(preds, targets, opt.br_threshold))
    if opt.all_metrics and rank == 0:
        from .metrics import RANKING_KEYS, compute_metrics
        t1 = time.perf_counter()
        m = (compute_metrics(on_device['probs'], on_device['targets'], bce_total, opt.br_threshold) if on_device else
             compute_metrics(preds, targets, bce_total, opt.br_threshold, device=device))
        out.update({k: (m[k].tolist() if hasattr(m[k], 'tolist') else m[k]) for k in RANKING_KEYS})
        out['metrics_seconds'] = time.perf_counter() - t1
    if opt.at_k and rank == 0:
        from .metrics import rank_at_k
        t1 = time.perf_counter()
        at_k = (rank_at_k(on_device['probs'], on_device['targets'], opt.at_k) if on_device else
                rank_at_k(preds.to(device), targets.to(device), opt.at_k))
        out.update(at_k)
        out['at_k_seconds'] = time.perf_counter() - t1
        print('  '.join('%s %.6f' % (key, at_k[key]) for key in at_k if key != 'n_with_gold') +
              '  n_with_gold %d' % at_k['n_with_gold'], file=sys.stderr, flush=True)
    if opt.label_ranking and rank == 0:
        from .metrics import label_ranking
        t1 = time.perf_counter()
        lr = (label_ranking(on_device['probs'], on_device['targets']) if on_device else
              label_ranking(preds.to(device), targets.to(device)))
        out.update(lr)
        out['label_ranking_seconds'] = time.perf_counter() - t1
        print('  '.join(('%s %d' if key.startswith('n_') else '%s %.6f') % (key, lr[key]) for key in lr), file=sys.stderr,
              flush=True)
    if tuned is not None and rank == 0:
        from .metrics import compute_metrics
        t1 = time.perf_counter()
        m = (compute_metrics(on_device['probs'], on_device['targets'], bce_total, opt.br_threshold, all_metrics=False,
                             thresholds=tuned['thresholds']) if on_device else
             compute_metrics(preds, targets, bce_total, opt.br_threshold, all_metrics=False, device=device,
                             thresholds=tuned['thresholds']))
        out.update({'tuned_' + k: m[k] for k in ('ACC', 'HA', 'ebF1', 'miF1', 'maF1')})
        out.update(tune_criterion=tuned['tune_criterion'], tune_split=tuned['tune_split'],
                   n_labels_tuned=tuned['n_labels_tuned'], thresholds=tuned['thresholds'].cpu().tolist(),
                   tune_seconds=tuned['tune_seconds'] + time.perf_counter() - t1)
        print('  '.join('tuned_%s %.6f' % (k, out['tuned_' + k]) for k in ('ACC', 'HA', 'ebF1', 'miF1', 'maF1')),
              file=sys.stderr, flush=True)
    if rank == 0:
        print(json.dumps(out), flush=True)
    plane.close()
    return out


if __name__ == '__main__':
    main()
