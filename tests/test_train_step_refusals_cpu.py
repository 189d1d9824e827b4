"""What the entry points of csrc/train_step.hip answer to calls they refuse: every single violation of their argument rules
and every pair of violations, for lamp_bce_logits_train, lamp_multilabel_loss_train, lamp_rank_loss_train, lamp_optim_step,
lamp_optim_step_ext, lamp_grad_norm and lamp_grad_norm_workspace_bytes, plus the calls that succeed without a launch (n == 0,
a table of only empty tensors).  A call that breaks two rules is answered in an order that differs from entry to entry; that
order is behaviour, and this pins it.

The expected statuses are RECORDED, not derived:  python tests/test_train_step_refusals_cpu.py --record  writes
tests/train_step_refusals.json (key: entry, then the sorted violation names) from the library as built.  The record is taken
once from a library whose answers are the wanted ones; a later change of the unit has to pass against the file as it stands.

No call here reaches a launch: every address is a fake one that is never dereferenced, no call of the sweep is fully valid,
and a case is only called when the record holds it with a refusal (or, for the no-launch cases, with LAMP_OK).  Nothing here
needs a GPU."""
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lamp_amd import _native as N  # noqa: E402

RECORD = os.path.join(ROOT, 'tests', 'train_step_refusals.json')
OK, E_DIMS, E_ALIGN, E_WORKSPACE, E_UNSUPPORTED, E_NULL = 0, -1, -2, -3, -4, -5
REFUSALS = (E_DIMS, E_ALIGN, E_WORKSPACE, E_UNSUPPORTED, E_NULL)


def fake(i):
    """A 16-byte aligned address that is never dereferenced."""
    return 0x100000 * (i + 1)


# ------------------------------------------------------------------ the loss entries
# base call (valid, hence never made): 2 matrices of 5 x 8, probs and row_loss given, dlogits given
def loss_base(entry):
    a = dict(n_mats=2, n_rows=5, L=8, ld_probs=8, ld_row_loss=5, logits=[fake(i) for i in range(9)], logits_null=False,
             weights_null=False, targets=fake(20), probs=fake(21), row_loss=fake(22))
    if entry == 'multilabel':
        a.update(opts_null=False, gamma_pos=2.0, gamma_neg=0.0, clip=0.0, reserved=0)
    if entry == 'rank':
        a.update(opts_null=False, kind=N.LAMP_RANK_HINGE, margin=1.0, bce_weight=0.5, reserved=0)
    return a


def _set(**kw):
    return lambda a: a.update(kw)


def _null_matrix(a):
    a['logits'][1] = None


# (name, group, apply): two violations of one group set the same argument and are never paired.  Applied in this order: the
# two leading-dimension rules read the sizes the earlier ones have set.
LOSS_VIOLATIONS = [
    ('n_mats_0', 'n_mats', _set(n_mats=0)),
    ('n_mats_9', 'n_mats', _set(n_mats=9)),
    ('null_matrix', None, _null_matrix),
    ('n_rows_0', 'n_rows', _set(n_rows=0)),
    ('n_rows_2p33', 'n_rows', _set(n_rows=1 << 33, ld_row_loss=1 << 33)),
    ('L_0', 'L', _set(L=0)),
    ('L_5000', 'L', _set(L=5000, ld_probs=5000)),                    # the pair kinds of the rank entry only
    ('ld_probs_short', None, lambda a: a.update(ld_probs=a['L'] - 1)),
    ('ld_row_loss_short', None, lambda a: a.update(ld_row_loss=a['n_rows'] - 1)),
    ('null_logits', None, _set(logits_null=True)),
    ('null_weights', None, _set(weights_null=True)),
    ('null_targets', None, _set(targets=None)),
    ('option_unserved', 'opts', None),                               # (per entry, below)
    ('null_opts', 'opts', _set(opts_null=True)),
    ('reserved', 'opts_reserved', _set(reserved=1)),
]
LOSS_SERVES = {
    'bce': {'L_5000', 'option_unserved', 'null_opts', 'reserved'},   # what is NO violation of the entry
    'multilabel': {'L_5000', 'null_opts'},                           # (NULL opts: plain BCE)
    'rank': set(),
}
LOSS_NEVER_PAIRED = {frozenset(('null_opts', 'reserved'))}


def loss_apply(entry, a, name, fn):
    if name == 'option_unserved':
        a.update(gamma_pos=0.5) if entry == 'multilabel' else a.update(kind=7)
    else:
        fn(a)


def loss_call(entry, a):
    lib = N.lib()
    xp = (C.c_void_p * 9)(*a['logits'])
    gp = (C.c_void_p * 9)(*[fake(30 + i) for i in range(9)])
    wp = (C.c_float * 9)(*([1.0] * 9))
    args = (None if a['logits_null'] else xp, None if a['weights_null'] else wp, gp, a['n_mats'], a['targets'], a['n_rows'],
            a['L'], a['probs'], a['ld_probs'], a['row_loss'], a['ld_row_loss'])
    if entry == 'bce':
        return lib.lamp_bce_logits_train(*args, None)
    if entry == 'multilabel':
        o = N.LossOptions(a['gamma_pos'], a['gamma_neg'], a['clip'], a['reserved'], None)
        return lib.lamp_multilabel_loss_train(*args, None if a['opts_null'] else C.byref(o), None)
    o = N.RankLossOptions(a['kind'], a['margin'], a['bce_weight'], a['reserved'])
    return lib.lamp_rank_loss_train(*args, None if a['opts_null'] else C.byref(o), None)


# ------------------------------------------------------------------ the optimizer entries
# base table: 8 elements, an empty tensor, 4097 elements (two chunks).  The NULLs and the 2^31 chunks go to entry 0 (a launch
# is cut in front of an entry that would take it to 2^31 chunks, so only the FIRST entry of a launch is refused before anything
# is launched), the negative numel to entry 1, the misaligned address to entry 2.
TABLE_SIZES = (8, 0, 4097)
TABLE_CHUNKS = 3
WD = (0.1, 0.0, 0.05)


def optim_base(entry, variant):
    a = dict(n=3, entries_null=False, numel=list(TABLE_SIZES), param=[fake(3 * i) for i in range(3)],
             grad=[fake(3 * i + 1) for i in range(3)], exp_avg=[fake(3 * i + 2) for i in range(3)],
             exp_avg_sq=[fake(40 + i) for i in range(3)], step=1)
    a['kind'] = N.LAMP_OPTIM_ADAM if variant == 'adam' else N.LAMP_OPTIM_SGD
    if variant == 'sgd':
        a['exp_avg'] = [None] * 3
    if variant != 'adam':
        a['exp_avg_sq'] = [None] * 3
    if entry == 'optim_step_ext':      # decay and a clip record: the extended kernels, not the forward to lamp_optim_step
        a.update(wd=list(WD), grad_state=fake(50), momentum=0.9 if variant == 'sgd_momentum' else 0.0, reserved=0,
                 flags=N.LAMP_OPTIM_DECOUPLED_DECAY if variant == 'adam' else 0)
    if entry == 'grad_norm':
        a.update(max_norm=1.0, workspace=fake(51), workspace_bytes=8 * TABLE_CHUNKS, grad_state=fake(50), skipped=fake(52))
    return a


def _item(key, i, value):
    return lambda a: a[key].__setitem__(i, value)


def _or_flags(bits, **kw):
    return lambda a: a.update(flags=a['flags'] | bits, **kw)


# (name, group, apply, entries it is a rule of, variants it is a rule of or None for all)
STEP = ('optim_step', 'optim_step_ext')
TABLE = STEP + ('grad_norm', 'grad_norm_workspace_bytes')
OPTIM_VIOLATIONS = [
    ('n_negative', 'n', _set(n=-1), TABLE, None),
    ('null_entries', None, _set(entries_null=True), TABLE, None),
    ('numel_negative', 'numel1', _item('numel', 1, -1), TABLE, None),
    ('chunks_2p31', 'numel0', _item('numel', 0, (1 << 31) * 4096), TABLE, None),
    ('kind_unknown', None, _set(kind=7), STEP, None),
    ('adam_step_0', None, _set(step=0), STEP, ('adam',)),
    ('null_param', None, _item('param', 0, None), STEP, None),
    ('null_grad', None, _item('grad', 0, None), STEP + ('grad_norm',), None),
    ('null_moment', None, _item('exp_avg', 0, None), STEP, ('adam', 'sgd_momentum')),
    ('param_misaligned', None, _item('param', 2, fake(6) + 2), STEP, None),
    ('grad_misaligned', None, _item('grad', 2, fake(7) + 2), ('grad_norm',), None),
    # lamp_optim_ext's rules (test_optim_ext_cpu.py)
    ('flag_unknown', None, _or_flags(4), ('optim_step_ext',), None),
    ('reserved', None, _set(reserved=1), ('optim_step_ext',), None),
    ('decay_negative', None, _item('wd', 0, -0.1), ('optim_step_ext',), None),
    ('momentum_1', 'momentum', _set(momentum=1.0), ('optim_step_ext',), None),
    ('momentum_with_adam', 'momentum', _set(momentum=0.9), ('optim_step_ext',), ('adam',)),
    ('skip_without_grad_state', 'grad_state', _or_flags(N.LAMP_OPTIM_SKIP_NONFINITE, grad_state=None), ('optim_step_ext',), None),
    ('decoupled_with_sgd', None, _or_flags(N.LAMP_OPTIM_DECOUPLED_DECAY), ('optim_step_ext',), ('sgd', 'sgd_momentum')),
    ('grad_state_misaligned', 'grad_state', _set(grad_state=fake(50) + 2), ('optim_step_ext', 'grad_norm'), None),
    # lamp_grad_norm's own
    ('null_grad_state', 'grad_state', _set(grad_state=None), ('grad_norm',), None),
    ('null_workspace', 'workspace', _set(workspace=None), ('grad_norm',), None),
    ('workspace_misaligned', 'workspace', _set(workspace=fake(51) + 4), ('grad_norm',), None),
    ('workspace_short', None, _set(workspace_bytes=8 * TABLE_CHUNKS - 1), ('grad_norm',), None),
    ('skipped_misaligned', None, _set(skipped=fake(52) + 2), ('grad_norm',), None),
    ('max_norm_nan', None, _set(max_norm=float('nan')), ('grad_norm',), None),
]
# The calls without a launch.  lamp_optim_step(_ext) launch nothing for them whatever else the call holds, so they are swept
# alone and with every violation, and may answer LAMP_OK.  lamp_grad_norm still launches its closing kernel for an empty
# table, so there they only accompany the violations that do not depend on the table, and LAMP_OK is never accepted.
NO_LAUNCH = [
    ('n_0', 'n', _set(n=0)),
    ('all_empty', ('numel0', 'numel1'), _set(numel=[0, 0, 0])),
]
TABLE_FREE = {'grad_state_misaligned', 'null_grad_state', 'workspace_misaligned', 'skipped_misaligned', 'max_norm_nan'}
OPTIM_VARIANTS = {'optim_step': ('adam', 'sgd'), 'optim_step_ext': ('adam', 'sgd_momentum'), 'grad_norm': ('sgd',),
                  'grad_norm_workspace_bytes': ('sgd',)}


def optim_call(entry, a):
    lib = N.lib()
    arr = (N.OptimEntry * 3)()
    for i in range(3):
        arr[i].param, arr[i].grad, arr[i].exp_avg, arr[i].exp_avg_sq = a['param'][i], a['grad'][i], a['exp_avg'][i], a['exp_avg_sq'][i]
        arr[i].numel = a['numel'][i]
    table = None if a['entries_null'] else arr
    if entry == 'grad_norm_workspace_bytes':
        return lib.lamp_grad_norm_workspace_bytes(table, a['n'])
    if entry == 'grad_norm':
        return lib.lamp_grad_norm(table, a['n'], a['max_norm'], a['workspace'], a['workspace_bytes'], a['grad_state'], a['skipped'],
                                  None)
    scalars = (a['n'], a['kind'], a['step'], 1e-3, 0.9, 0.98, 1e-8)
    if entry == 'optim_step':
        return lib.lamp_optim_step(table, *scalars, None)
    ext = N.OptimExt((C.c_float * 3)(*a['wd']), a['grad_state'], a['momentum'], a['flags'], a['reserved'])
    return lib.lamp_optim_step_ext(table, *scalars, C.byref(ext), None)


# ------------------------------------------------------------------ the sweep
def _groups(g):
    return set(g) if isinstance(g, tuple) else {g} if g else set()


def _combos(violations, never_paired=()):
    """Every single violation and every pair whose groups differ, in list order."""
    for v in violations:
        yield (v,)
    for v, w in itertools.combinations(violations, 2):
        if not (_groups(v[1]) & _groups(w[1])) and frozenset((v[0], w[0])) not in never_paired:
            yield (v, w)


def cases():
    """-> [(key, entry, may answer LAMP_OK, thunk)]; key = 'entry|violation+violation', names sorted."""
    out = []
    for entry in ('bce', 'multilabel', 'rank'):
        mine = [v for v in LOSS_VIOLATIONS if v[0] not in LOSS_SERVES[entry]]
        for combo in _combos(mine, LOSS_NEVER_PAIRED):
            def thunk(entry=entry, combo=combo):
                a = loss_base(entry)
                for name, _, fn in combo:
                    loss_apply(entry, a, name, fn)
                return loss_call(entry, a)
            out.append(('%s|%s' % (entry, '+'.join(sorted(v[0] for v in combo))), entry, False, thunk))
    for entry, variants in OPTIM_VARIANTS.items():
        for variant in variants:
            mine = [v[:3] for v in OPTIM_VIOLATIONS if entry in v[3] and (v[4] is None or variant in v[4])]
            combos = [(c, False) for c in _combos(mine)]
            for nl in NO_LAUNCH:
                launches = entry == 'grad_norm'
                if not launches:
                    combos.append(((nl,), True))
                combos += [((nl, v), not launches) for v in mine
                           if not (_groups(nl[1]) & _groups(v[1])) and (not launches or v[0] in TABLE_FREE)]
            for combo, may_ok in combos:
                def thunk(entry=entry, variant=variant, combo=combo):
                    a = optim_base(entry, variant)
                    for _, _, fn in combo:
                        fn(a)
                    return optim_call(entry, a)
                name = entry if len(variants) == 1 else '%s/%s' % (entry, variant)
                out.append(('%s|%s' % (name, '+'.join(sorted(v[0] for v in combo))), entry, may_ok, thunk))
    # the size query launches nothing: its answer for the valid table belongs to the record as well
    out.append(('grad_norm_workspace_bytes|', 'grad_norm_workspace_bytes', True,
                lambda: optim_call('grad_norm_workspace_bytes', optim_base('grad_norm_workspace_bytes', 'sgd'))))
    return out


def _admissible(entry, may_ok, status):
    if entry == 'grad_norm_workspace_bytes':
        return status >= 0                   # a byte count
    return status in REFUSALS or (may_ok and status == OK)


def test_the_record_holds_the_sweep_and_nothing_that_launches():
    rec = json.load(open(RECORD))
    swept = cases()
    assert len({k for k, *_ in swept}) == len(swept)
    assert set(rec) == {k for k, *_ in swept}
    bad = [k for k, entry, may_ok, _ in swept if not _admissible(entry, may_ok, rec[k])]
    assert not bad, bad
    # the sizes the issue quotes: the loss sweep alone is a few hundred calls
    assert sum(1 for k in rec if k.split('|')[0] in ('bce', 'multilabel', 'rank')) >= 250
    # the no-launch calls are there and succeed
    for k in ('optim_step/adam|n_0', 'optim_step/sgd|all_empty', 'optim_step_ext/adam|n_0', 'optim_step_ext/sgd_momentum|all_empty'):
        assert rec[k] == OK, k
    assert rec['grad_norm_workspace_bytes|'] == 8 * TABLE_CHUNKS and rec['grad_norm_workspace_bytes|all_empty'] == 0


def test_two_violations_are_answered_in_each_entrys_own_order():
    """The orders that differ today, spelled out (they are in the record as well): n_mats = 9 with a NULL target, and
    ld_probs < L with a NULL target."""
    rec = json.load(open(RECORD))
    assert rec['bce|n_mats_9+null_targets'] == E_UNSUPPORTED
    assert rec['multilabel|n_mats_9+null_targets'] == rec['rank|n_mats_9+null_targets'] == E_NULL
    assert rec['bce|ld_probs_short+null_targets'] == E_NULL
    assert rec['multilabel|ld_probs_short+null_targets'] == rec['rank|ld_probs_short+null_targets'] == E_DIMS
    # one violation: everyone agrees
    for v, want in (('n_mats_9', E_UNSUPPORTED), ('null_targets', E_NULL), ('ld_probs_short', E_DIMS), ('n_rows_2p33', E_UNSUPPORTED),
                    ('null_matrix', E_NULL), ('L_0', E_DIMS)):
        assert [rec['%s|%s' % (e, v)] for e in ('bce', 'multilabel', 'rank')] == [want] * 3, v


def test_every_refusal_is_the_recorded_one():
    rec = json.load(open(RECORD))
    wrong = []
    for key, entry, may_ok, thunk in cases():
        want = rec.get(key)
        if want is None or not _admissible(entry, may_ok, want):
            wrong.append((key, 'not called: the record has no refusal for it'))       # (reported by the test above, too)
            continue
        got = thunk()
        if got != want:
            wrong.append((key, got, want))
    assert not wrong, wrong


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        sys.exit('usage: python tests/test_train_step_refusals_cpu.py --record')
    rec = {}
    for key, entry, may_ok, thunk in cases():
        rec[key] = thunk()
        assert _admissible(entry, may_ok, rec[key]), ('this call was not refused', key, rec[key])
    with open(RECORD, 'w') as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d cases -> %s' % (len(rec), RECORD))
