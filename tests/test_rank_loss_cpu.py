"""CPU-side checks of the ranking losses (lamp_rank_loss_train): the ABI bookkeeping, the wrapper's
refusals raised without a device, the fp64 reference the GPU tests compare against held to a brute-force double loop over the
pairs, and run_train's flags, results name and checkpoint settings.  Nothing here needs a GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

from lamp_amd import _native as N
from lamp_amd import run_train as RT
from lamp_amd import train as T

import rank_loss_common as RC
import train_common as TC


# ------------------------------------------------------------------ ABI bookkeeping
def test_header_ctypes_and_library_carry_the_entry_point():
    raw = open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    m = re.search(r'\bint\s+lamp_rank_loss_train\s*\(([^)]*)\)', text)
    base = re.search(r'\bint\s+lamp_bce_logits_train\s*\(([^)]*)\)', text)
    assert m and base
    n_args, n_base = len(m.group(1).split(',')), len(base.group(1).split(','))
    assert n_args == n_base + 1 and 'const lamp_rank_loss_options* opts' in m.group(1)
    restype, argtypes = N.PROTOTYPES['lamp_rank_loss_train']
    assert restype is ctypes.c_int and len(argtypes) == n_args
    assert argtypes[:-2] == N.PROTOTYPES['lamp_bce_logits_train'][1][:-1] and argtypes[-2] == ctypes.POINTER(N.RankLossOptions)
    assert 'lamp_rank_loss_train' in N.LATE_ENTRY_POINTS                    # added without an ABI bump
    body = re.search(r'typedef struct lamp_rank_loss_options \{(.*?)\} lamp_rank_loss_options;', text, flags=re.S).group(1)
    assert re.findall(r'(\w+)\s*;', body) == [f[0] for f in N.RankLossOptions._fields_] == ['kind', 'margin', 'bce_weight', 'reserved']
    assert ctypes.sizeof(N.RankLossOptions) == 16
    assert re.search(r'#define LAMP_HIP_ABI_VERSION 5\b', raw)
    assert N.lib().lamp_version() == N.ABI_VERSION == 5
    assert re.search(r'LAMP_RANK_LSEP = 1, LAMP_RANK_HINGE = 2, LAMP_RANK_LOGISTIC = 3', text)
    assert (N.LAMP_RANK_LSEP, N.LAMP_RANK_HINGE, N.LAMP_RANK_LOGISTIC) == (1, 2, 3)
    assert hasattr(ctypes.CDLL(N.LIB_PATH), 'lamp_rank_loss_train')
    flat = ' '.join(raw.split())
    for rule in ('difference FIRST', 'A pair is active iff', 'L <= 4096', 'empty class'):     # the header states the rules
        assert rule in flat, rule
    from lamp_amd import build as B
    kernels = B.kernel_resources('train_step.hip')
    mine = {k: r for k, r in kernels.items() if 'rank_lsep_train_kernel' in k or 'rank_pair_train_kernel' in k}
    assert len(mine) == 3, sorted(kernels)              # LSEP, and the pair kernel for HINGE and for LOGISTIC
    for name, r in mine.items():
        assert r.get('scratch', 0) == 0 and r.get('agpr', 0) == 0 and r.get('lds', 0) <= 64 * 1024, (name, r)


# ------------------------------------------------------------------ refusals, without a device
@pytest.mark.parametrize('args', [
    ('warp',), (0,), (4,), (None,), (True,), (1.0,),
    ('hinge', -1.0), ('hinge', float('nan')), ('hinge', float('inf')), ('hinge', 1e39),
    ('lsep', 1.0), ('logistic', 0.5),
    ('lsep', 0.0, -0.5), ('hinge', 1.0, float('nan')), ('logistic', 0.0, float('inf')),
])
def test_check_rank_loss_options_refuses(args):
    with pytest.raises(ValueError):
        N.check_rank_loss_options(*args)


def test_check_rank_loss_options_accepts_and_normalises():
    assert N.check_rank_loss_options('lsep') == (1, 0.0, 0.0)
    assert N.check_rank_loss_options('hinge', 1, 2) == (2, 1.0, 2.0)
    assert N.check_rank_loss_options(3, 0, 0.5) == (3, 0.0, 0.5)
    assert N.check_rank_loss_options('hinge', 0.0) == (2, 0.0, 0.0)                 # a zero margin is served
    assert N.check_rank_loss_options('hinge', 0.05)[1] == float(torch.tensor(0.05, dtype=torch.float32))   # as the library gets it


@pytest.mark.parametrize('kw', [dict(kind='warp'), dict(kind='hinge', margin=-1.0), dict(kind='lsep', margin=1.0),
                                dict(kind='logistic', bce_weight=-1.0), dict(kind='lsep', bce_weight=float('nan'))])
def test_wrapper_refuses_parameters_before_it_looks_for_a_device(kw, monkeypatch):
    def no_library():
        raise AssertionError('the library was called')
    monkeypatch.setattr(N, 'lib', no_library)
    x, t = torch.zeros(3, 5), torch.zeros(3, 5)
    with pytest.raises(ValueError):
        N.rank_loss_train([x], [1.0], t, **kw)
    with pytest.raises(ValueError):
        T.RankLossOptions(**kw)


def test_wrapper_signature_width_and_matrix_limits(monkeypatch):
    sig = inspect.signature(N.rank_loss_train)
    assert list(sig.parameters) == ['logits', 'weights', 'targets', 'kind', 'margin', 'bce_weight', 'probs_out', 'row_loss_out',
                                    'want_grads', 'want_probs']
    assert [sig.parameters[k].default for k in ('margin', 'bce_weight', 'probs_out', 'want_grads')] == [0.0, 0.0, None, True]
    monkeypatch.setattr(N, 'lib', lambda: (_ for _ in ()).throw(AssertionError('the library was called')))
    x = torch.zeros(3, 5)
    with pytest.raises(ValueError):
        N.rank_loss_train([x] * 9, [1.0] * 9, x, 'lsep')       # the entry point takes 8
    with pytest.raises(ValueError):
        N.rank_loss_train([x] * 2, [1.0], x, 'lsep')
    wide = torch.zeros(1, 4097)
    for kind in ('hinge', 'logistic'):
        with pytest.raises(ValueError, match='4096'):
            N.rank_loss_train([wide], [1.0], wide, kind)


def test_rank_loss_options_defaults_and_the_two_objects_together_raise():
    assert (T.RankLossOptions().kind, T.RankLossOptions().margin, T.RankLossOptions().bce_weight) == ('lsep', 0.0, 0.0)
    assert T.RankLossOptions('hinge').margin == 1.0 and T.RankLossOptions('hinge', 0.25).margin == 0.25
    assert T.RankLossOptions('logistic', bce_weight=2).bce_weight == 2.0

    class Model(torch.nn.Module):
        def forward(self, src, adj, a, gold, return_attns=False, int_preds=False):
            return torch.zeros(2, 3, requires_grad=True), None

    opt = TC.train_opt(3)
    opt.rank_loss, opt.loss_options = T.RankLossOptions('lsep'), T.LossOptions(2.0, 2.0)
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.0)
    with pytest.raises(ValueError, match='rank_loss and opt.loss_options'):      # at the first batch, before any launch
        T.train_batch(Model(), sgd, opt, None, None, torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(1, 2))


# ------------------------------------------------------------------ the reference's own checks
def _moderate(B=5, L=23, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, generator=g, dtype=torch.float64) * 3.0
    t = (torch.rand(B, L, generator=g) < 0.25).float()
    t[0] = 0.0
    t[B - 1] = 1.0
    t[1] = 0.0
    t[1, 0] = 1.0
    return x, t


@pytest.mark.parametrize('kind', RC.KINDS)
def test_fp64_reference_equals_the_double_loop_over_pairs(kind):
    x, t = _moderate()
    B, L = x.shape
    margin = 0.75 if kind == 'hinge' else 0.0
    _, (g,), rows = RC.rank_reference([x], [1.0], t, kind, margin, 0.0, torch.float64)
    for r in range(B):
        R, gr = RC.brute_force_row(x[r].tolist(), (t[r] > 0.5).tolist(), kind, margin)      # (LSEP: the naive log1p(sum sum exp))
        assert abs(float(rows[0, r]) - R) <= 1e-12 * max(1.0, abs(R)), (kind, r)
        assert float((g[r] * B - torch.tensor(gr, dtype=torch.float64)).abs().max()) <= 1e-12, (kind, r)
    assert float(rows[0, 0]) == 0.0 and float(rows[0, B - 1]) == 0.0                        # an empty class: R = 0 ...
    assert not g[0].any() and not g[B - 1].any()                                            # ... and no gradient
    assert float(rows[0, 1]) > 0.0


@pytest.mark.parametrize('kind', RC.KINDS)
def test_reference_mixes_the_mean_bce_in(kind):
    x, t = _moderate(seed=1)
    B, L = x.shape
    margin = 1.0 if kind == 'hinge' else 0.0
    _, (g0,), r0 = RC.rank_reference([x], [0.5], t, kind, margin, 0.0)
    _, (g2,), r2 = RC.rank_reference([x], [0.5], t, kind, margin, 2.0)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(x, t.double(), reduction='none')
    assert float((r2 - r0 - 2.0 * bce.sum(1) / L).abs().max()) <= 1e-12
    assert float((g2 - g0 - 0.5 * 2.0 * (torch.sigmoid(x) - t.double()) / (B * L)).abs().max()) <= 1e-14
    assert float(r2[0, 0]) > 0.0 and g2[0].any()                # the all-zero row: BCE alone


@pytest.mark.parametrize('kind', RC.KINDS)
def test_autograd_reference_equals_the_headers_closed_forms_on_the_kernel_cases(kind):
    """On the cases the kernels are held to -- equal logits (x_n - x_p = 0 exactly), x = 0 and +-1e4 planted -- the fp64
    reference's autograd gradients are the header's formulas: no subgradient of a clamp or an abs stands in for a derivative."""
    for B, L, n_mats in ((4, 63, 1), (7, 65, 3)):
        logits, weights, targets, margin = RC.rank_case(B, L, n_mats, kind, seed=B * 1000 + L)
        assert any(bool((x == 0).any()) for x in logits)
        _, grads, rows = RC.rank_reference(logits, weights, targets, kind, margin, 1.0, torch.float64)
        t, pos = targets.double(), targets > 0.5
        for k, x in enumerate(logits):
            x = x.double()
            for r in range(B):
                R, g = RC.closed_form_row(x[r], pos[r], kind, margin)
                bce = torch.clamp(x[r], min=0) - x[r] * t[r] + torch.log1p(torch.exp(-x[r].abs()))
                want_row = R + bce.sum() / L
                want_g = (g + (torch.sigmoid(x[r]) - t[r]) / L) * weights[k] / B
                assert abs(float(rows[k, r] - want_row)) <= 1e-12 * max(1.0, abs(float(want_row))), (kind, k, r)
                assert float((grads[k][r] - want_g).abs().max()) <= 1e-15, (kind, k, r)


def test_the_hinge_kink_is_inactive_in_the_reference():
    x = torch.tensor([[2.0, 1.0, 1.0, 0.5]], dtype=torch.float64)       # x_n - x_p = -1 twice: a = 0 with margin 1
    t = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    _, (g,), rows = RC.rank_reference([x], [1.0], t, 'hinge', 1.0, 0.0)
    assert float(rows[0, 0]) == 0.0 and not g.any()
    _, (g,), rows = RC.rank_reference([x], [1.0], t, 'hinge', 1.5, 0.0)
    assert float(rows[0, 0]) == (0.5 + 0.5 + 0.0) / 3 and g[0].tolist() == [-2.0 / 3, 1.0 / 3, 1.0 / 3, 0.0]


def test_cases_carry_their_planted_rows_and_the_hinge_grid():
    for B, L, n_mats in RC.SHAPES:
        for kind in ('lsep', 'hinge'):
            logits, weights, targets, margin = RC.rank_case(B, L, n_mats, kind, seed=B * 1000 + L)
            assert len(logits) == len(weights) == n_mats and targets.shape == (B, L)
            assert not targets[0].any()
            if B >= 2:
                assert bool(targets[B - 1].all())
            if B >= 3:
                assert targets[1].nonzero().view(-1).tolist() == [0]
            if B >= 4:
                assert targets[2].nonzero().view(-1).tolist() == [L - 1]
            if L == 4096:
                assert int(targets[3].sum()) == 2048
            if B * L >= 9:
                assert float(max(x.max() for x in logits)) == 1e4 and float(min(x.min() for x in logits)) == -1e4
            assert margin == (RC.HINGE_MARGIN if kind == 'hinge' else 0.0)      # (rank_case asserted the grid property itself)


# ------------------------------------------------------------------ run_train's flags
BASE = ['-data', 'x.pt', '-dataset', 'syn', '-d_model', '32', '-n_head', '2', '-name', 'n1']
NEW_KEYS = ('rank_margin', 'rank_bce_weight', 'rank_loss', 'loss_fn', 'loss_options')


def test_name_and_settings_are_unchanged_without_the_flags():
    opt = RT.parse(BASE)
    assert opt.loss_fn == 'bce' and 'lossfn' not in opt.model_name and opt.model_name.endswith('.n1')
    st = RT.checkpoint_settings(opt)
    assert not any(hasattr(st, k) for k in NEW_KEYS)
    opt.loss_options, opt.rank_loss = None, None            # as run_train.main leaves them for plain BCE
    assert vars(RT.checkpoint_settings(opt)) == vars(st)
    assert RT.build_rank_loss(opt) is None and RT.build_loss_options(opt, None, 'cpu') is None
    ranking = RT.parse(BASE + ['-loss', 'ranking'])         # the reference's flag: parsed, named, ignored
    assert ranking.loss_fn == 'bce' and RT.build_rank_loss(ranking) is None
    assert ranking.model_name == opt.model_name.replace('.loss_ce.', '.loss_ranking.')
    assert 'ignored' in _help() and 'rank_hinge' in _help()


def _help():
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        RT.parse(['-h'])
    return ' '.join(buf.getvalue().split())


def test_suffixes_settings_and_objects_with_the_flags():
    plain = RT.parse(BASE).model_name
    opt = RT.parse(BASE + ['-loss_fn', 'lsep', '-rank_bce_weight', '1'])
    assert opt.model_name == plain[:-len('.n1')] + '.lossfn_lsep_1.0.n1'
    st = RT.checkpoint_settings(opt)
    assert (st.loss_fn, st.rank_bce_weight) == ('lsep', 1.0)
    assert not any(hasattr(st, k) for k in ('rank_margin', 'rank_loss', 'loss_options', 'focal_gamma', 'asl_clip', 'pos_weight'))
    rl = RT.build_rank_loss(opt)
    assert isinstance(rl, T.RankLossOptions) and (rl.kind, rl.margin, rl.bce_weight) == ('lsep', 0.0, 1.0)
    assert RT.build_loss_options(opt, None, 'cpu') is None
    opt.rank_loss, opt.loss_options = rl, None              # as run_train.main leaves them: never settings
    assert vars(RT.checkpoint_settings(opt)) == vars(st)
    assert all(isinstance(v, (bool, int, float, str, type(None))) for v in vars(st).values())
    opt = RT.parse(BASE + ['-loss_fn', 'rank_hinge'])
    assert opt.model_name == plain[:-len('.n1')] + '.lossfn_rank_hinge_1.0_0.0.n1'
    st = RT.checkpoint_settings(opt)
    assert (st.loss_fn, st.rank_margin, st.rank_bce_weight) == ('rank_hinge', 1.0, 0.0)
    rl = RT.build_rank_loss(opt)
    assert (rl.kind, rl.margin, rl.bce_weight) == ('hinge', 1.0, 0.0)
    opt = RT.parse(BASE + ['-loss_fn', 'rank_logistic', '-rank_bce_weight', '0.5', '-rank_margin', '3'])   # (no margin: not read)
    assert opt.model_name == plain[:-len('.n1')] + '.lossfn_rank_logistic_0.5.n1'
    st = RT.checkpoint_settings(opt)
    assert (st.loss_fn, st.rank_bce_weight) == ('rank_logistic', 0.5) and not hasattr(st, 'rank_margin')
    rl = RT.build_rank_loss(opt)
    assert (rl.kind, rl.margin, rl.bce_weight) == ('logistic', 0.0, 0.5)
    focal = RT.checkpoint_settings(RT.parse(BASE + ['-loss_fn', 'focal']))      # the other objectives' settings gain nothing
    assert not hasattr(focal, 'rank_margin') and not hasattr(focal, 'rank_bce_weight')


@pytest.mark.parametrize('argv', [
    ['-loss_fn', 'lsep', '-pos_weight', 'inv'], ['-loss_fn', 'rank_hinge', '-pos_weight', 'sqrt_inv'],
    ['-loss_fn', 'rank_hinge', '-rank_margin', '-1'], ['-loss_fn', 'rank_hinge', '-rank_margin', 'nan'],
    ['-loss_fn', 'lsep', '-rank_bce_weight', '-0.1'], ['-loss_fn', 'rank_logistic', '-rank_bce_weight', 'inf'],
    ['-loss_fn', 'warp'],
])
def test_flag_validation(argv):
    with pytest.raises((ValueError, SystemExit)):
        RT.parse(BASE + argv)


def test_pos_weight_with_a_rank_loss_is_refused_with_a_clear_message():
    with pytest.raises(ValueError, match='-pos_weight inv with -loss_fn lsep'):
        RT.parse(BASE + ['-pos_weight', 'inv', '-loss_fn', 'lsep'])
