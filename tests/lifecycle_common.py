"""Shared pieces of the life-cycle tests (tests/test_model_lifecycle_cpu.py, tests/test_model_lifecycle_gpu.py): the eval
forward reads tables derived from the weights (LAMP._native_model: hoisted query, chain packs, GEMM and K / V packs, folded
embedding, one-hot tables; GraphDecoder.current_label_bias: the folded bias buffer), kept under a hand-written key.  These tests
change a model in every supported way and ask one thing: is the next forward the forward of a freshly loaded model?

* ``FAMILIES``: the models, each at the smallest shape at which the library really reads the tables named beside it (the
  stale-table control of the GPU file is what proves that):
    tokpos   head_geometry_common.GEOMS['G5a'], B = 6: 540 decoder rows at d = 512 -- the decoder chain launch (from 512 rows, d = 512
             only: chain.hip::chain_applies) and with it the chain packs; every projection has N a multiple of 16 and K of 32, so
             the tile GEMMs read the fragment-major packs (gemm.hip::gemm_packed_ok) and the K / V projection its own; token +
             position rows, so both folded tables exist; hoisted query
    tok      d = 64, no position rows: b1 sits inside the folded token table
    live     G5a with enc_self_attn=True at T = 88, B = 6: 528 encoder rows -- the live encoder's tails run as the chain launch too,
             from its own packs; nothing is folded
    onehot   d = 64, the one-hot front end: tap table, conv pack, contiguous bias copies
    lbias    d = 64, learn_label_bias=True on a 'prior' mask: the folded bias buffer
    bias     d = 64, a constant bias: the buffer is read live, no table of its own
* ``fresh``: the truth.  A second model of the same construction and route switches that has just loaded the first one's
  state_dict -- load_state_dict invalidates wholesale, so it never depends on the keys under test.
* ``fp64_check``: both stay inside the project's bars against the fp64 restatement of the CURRENT state dict.
* ``perturb``: p.add_(N(0, (0.25 max(std(p), 0.1))^2)) from a generator seeded by the parameter's name.

Importable without a GPU."""
import collections
import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import combo_common as CC  # noqa: E402
import head_geometry_common as HG  # noqa: E402
from conftest import max_abs_diff  # noqa: E402
from oracle import lamp_ref as R  # noqa: E402

# the route switches a twin model must share (class attributes of LAMP; an instance may override them)
FLAGS = ('cache_layer0_query', 'use_chain_packs', 'use_gemm_packs', 'use_kv_gemm_packs', 'fold_embedding', 'matmul_precision',
         'use_packed_live_encoder', 'use_label_tiles', 'use_sparse_label_attention', 'use_mask_bits', 'workspace_limit_bytes')

Case = collections.namedtuple('Case', 'family model seq pos ref live')     # ref(state dict, dtype) -> (logits, enc)

LIVE_T, LIVE_LENGTHS = 88, [88, 51, 88, 7, 64, 30]     # 6 x 88 = 528 encoder rows


def _combo_cfg(front, score):
    return CC._c('lifecycle', front, 'dead', score, 'std', 'on', '2x2', 'plain', 'whole', 'highest')


_COMBO = {'tok': _combo_cfg('tok', 'prior'), 'onehot': _combo_cfg('onehot', 'prior'), 'lbias': _combo_cfg('tokpos', 'lbias'),
          'bias': _combo_cfg('tokpos', 'bias')}
FAMILIES = ('tokpos', 'tok', 'live', 'onehot', 'lbias', 'bias')
# the tables each family keeps alive, by the names of stale_built / table_weights
TABLES = {'tokpos': ('hoist', 'chain', 'gemm', 'kv', 'fold'), 'tok': ('fold',), 'live': ('enc_chain', 'chain'),
          'onehot': ('onehot',), 'lbias': ('lbias',), 'bias': ()}


def make(family):
    """-> Case with a new LAMP on the CPU (eval mode); every call of one family builds the same model."""
    if family in ('tokpos', 'live'):
        live = family == 'live'
        if live:
            m, sd, blocked, seq, pos, g = HG.build('G5a', lengths=LIVE_LENGTHS, T=LIVE_T, enc_self_attn=True)
        else:
            m, sd, blocked, seq, pos, g = HG.build('G5a', lengths=HG.chain_lengths(6))

        def ref(sd_now, dtype):
            sdx = R.to_dtype(sd_now, dtype)
            with torch.no_grad():
                if live:
                    return HG.live_forward_ref(sdx, seq, pos, g, blocked)[:2]
                return R.forward(sdx, seq, pos, g['h'], blocked, n_head2=g['h2'])[:2]
        return Case(family, m.eval(), seq, pos, ref, live)
    cfg = _COMBO[family]
    b = CC.combo_build(cfg)

    def ref(sd_now, dtype):
        bias = b.bias
        if family == 'lbias':     # the restatement adds the raw (L, L) parameter on top of the mask
            bias = sd_now['decoder.label_bias']
        sdx = R.to_dtype({k: v for k, v in sd_now.items() if k != 'decoder.label_bias'}, dtype)
        with torch.no_grad():
            return CC.combo_forward_ref(sdx, b.seq, b.pos, cfg, b.blocked, None, bias.to(dtype) if bias is not None else None)[:2]
    return Case(family, b.model.eval(), b.seq, b.pos, ref, False)


def flags_of(m):
    return {k: m.__dict__['_matmul_precision' if k == 'matmul_precision' else k] for k in FLAGS
            if ('_matmul_precision' if k == 'matmul_precision' else k) in m.__dict__}


def fresh(case, m, dev, into=None):
    """The truth for ``m``: a model of the same construction (``into``: reuse that twin) and route switches that has just loaded
    m's state_dict."""
    f = into if into is not None else make(case.family).model.to(dev).eval()
    for k in FLAGS:
        if k in f.__dict__ or (k == 'matmul_precision' and '_matmul_precision' in f.__dict__):
            delattr(f, k)
    for k, v in flags_of(m).items():
        setattr(f, k, v)
    f.load_state_dict(m.state_dict())
    return f


def run(case, m, dev):
    with torch.no_grad():
        logits, enc, _ = m((case.seq.to(dev), case.pos.to(dev)), None, None, None)
    return logits, enc


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def cpu_state_dict(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def fp64_fractions(case, m, out):
    """``out`` = (logits, enc) of a forward of ``m`` against the fp64 restatement of m's current state dict -> {quantity: error /
    bar}; each bar is max(the project's bar, 4 x the fp32 CPU restatement's own gap to fp64) -- the rule of tests/fuzz_parity.py."""
    sd = cpu_state_dict(m)
    r64, r32 = case.ref(sd, torch.float64), case.ref(sd, torch.float32)
    high = getattr(m, 'matmul_precision', 'highest') != 'highest'
    base = (CC.TOL_LOGIT, CC.TOL_ENC_LIVE if case.live or high else CC.TOL_ENC)
    return {name: max_abs_diff(got, want) / max(bar, 4 * max_abs_diff(low, want))
            for name, got, want, low, bar in zip(('logits', 'enc'), out, r64, r32, base)}


def noise_for(name, p):
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    finite = p.detach().float()
    finite = finite[torch.isfinite(finite)]     # (a learned label bias holds -inf where its prior blocks)
    std = float(finite.std().item()) if finite.numel() > 1 else 0.0
    return (torch.randn(p.shape, generator=gen) * (0.25 * max(std, 0.1))).to(device=p.device, dtype=p.dtype)


def perturb(name, p):
    """In place, under no_grad: the version counter moves, the address does not."""
    with torch.no_grad():
        p.add_(noise_for(name, p))


def names_of(m, tensors):
    by_id = {id(p): n for n, p in m.named_parameters()}
    return {by_id[id(t)] for t in tensors if t is not None}


def table_weights(m, table):
    """The tensors a table is built from: the code's own lists."""
    if table == 'hoist':
        return [m.decoder.tgt_word_emb.weight, m.decoder.layer_stack[0].enc_attn.w_qs.weight]
    if table == 'chain':
        return m._chain_weights()
    if table == 'enc_chain':
        return m._enc_chain_weights()
    if table == 'gemm':
        enc, dec, _ = m._gemm_pack_weights()
        return [w for group in (enc, dec) for ws in group for w in ws if w is not None]
    if table == 'kv':
        return [w for ws in m._gemm_pack_weights()[2] for w in ws]
    if table == 'fold':
        return [w for w in m._fold_weights() if w is not None]
    if table == 'onehot':
        return list(m._onehot_weights())
    if table == 'lbias':
        return [m.decoder.label_bias]
    raise KeyError(table)


def feeding_names(m, family):
    """Every parameter that feeds a table this family keeps (what the per-parameter sweep must see move the output)."""
    out = set()
    for table in TABLES[family]:
        out |= names_of(m, table_weights(m, table))
    return out


def stale_built(fresh_built, old_built, table):
    """``fresh_built`` (LAMP._native_cache[1]) with ONE table taken from ``old_built`` -- what a key that forgot the table's weights
    would leave behind.  Both tuples must stay alive while the result is used."""
    from lamp_amd import _native as N
    out = list(fresh_built)
    if table in ('hoist', 'chain', 'fold'):
        model = N.Model.from_buffer_copy(fresh_built[0])
        old = old_built[0]
        if table == 'hoist':
            model.dec0_query = old.dec0_query
        elif table == 'chain':
            model.chain_packs = old.chain_packs
        else:
            model.enc0_emb_w1, model.enc0_pos_w1 = old.enc0_emb_w1, old.enc0_pos_w1
        out[0] = model
    elif table == 'enc_chain':
        out[8] = old_built[8]
    elif table == 'gemm':
        out[9] = tuple(old_built[9][:4]) + (fresh_built[9][4],)
    elif table == 'kv':
        out[9] = tuple(fresh_built[9][:4]) + (old_built[9][4],)
    elif table == 'onehot':
        out[7] = old_built[7]
    else:
        raise KeyError(table)
    return tuple(out)
