"""-m gpu: a captured eval forward replayed over batches whose lengths change between replays.

A ragged batch's SeqPlan is counted on the device so that a captured forward stays valid for any lengths, and the plan hand-off
of embed_plan_kernel tags its granules with a host-side epoch that a captured launch repeats at every replay: the replay is safe
only because the forward's last encoder LayerNorm (layernorm_kernel<.., RG == 2>; on the live packed route scatter_rows_kernel)
returns the granules to "no epoch" (csrc/lamp_kernels.h: launch_embed_plan).  A length decision on the host, or a lost zeroing,
leaves every eager test green and hands a replay rows placed by the previous batch's plan.

One forward is captured into static seq / pos buffers after an eager run on the same stream (the model's native cache and the
grow-only workspace of that stream exist before the capture), then five batches of the same (B, T) are copied into the buffers and
replayed: every replay must give the eager forward's bits, and the eager forward meets the oracle bars of
tests/test_ragged_plan_gpu.py.  The capture is one stream without a parallel branch."""
import numpy as np
import pytest
import torch

import enc_live_common as EC
import ragged_plan_common as RP
from conftest import max_abs_diff
from oracle import lamp_ref as R
from test_enc_self_attn_gpu import TOL as TOL_LIVE
from test_gpu_parity import TOL_ACT, TOL_LOGIT

pytestmark = pytest.mark.gpu

T = 40


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from lamp_amd import _native as N
    N.lib()
    return torch.device('cuda:0')


def batches(B):
    """Five (B, T) batches: ragged, dense, ragged with zero-length samples, all PAD, interior PADs with position-only tails."""
    rng = np.random.default_rng(B)
    ragged = RP._from_lengths([T, 3, 17, 29, 8, 33, 21][:B], T, rng)
    dense = RP._from_lengths([T] * B, T, rng)
    zero = RP._from_lengths([12, 0, T, 5, 0, 22, 0][:B], T, rng)
    allpad = RP._all_pad(B, T, rng)
    lengths = [37, 20, 36, 38, 9, 35, 1][:B]
    seq, pos = RP._from_lengths(lengths, T, rng)
    for b, n in enumerate(lengths):
        if n > 34:
            seq[b, 30:34] = 0              # crosses the 32-position boundary
            if b % 2 == 0:
                pos[b, 30:34] = 0
        pos[b, n:min(T, n + 2)] = np.arange(n + 1, min(T, n + 2) + 1)   # trailing PAD tokens that keep position indices
    out = [ragged, dense, zero, allpad, (seq, pos)]
    return [(torch.from_numpy(s), torch.from_numpy(p)) for s, p in out]


def _fwd(m, src, **kw):
    with torch.no_grad():
        return m(src, None, None, None, **kw)


def _tiny_route(dev):
    sd = RP.tiny_state_dict(True, n_max_seq=T)
    m = RP.tiny_model(sd, True, n_max_seq=T).to(dev).eval()
    sd64 = R.to_dtype(sd, torch.float64)

    def oracle(seq, pos):
        with torch.no_grad():
            ref_logits, ref_enc, _ = R.forward(sd, seq, pos, RP.TINY['h'], None)
            ref64, _, _ = R.forward(sd64, seq, pos, RP.TINY['h'], None)
        return ref_logits, ref_enc, ref64, TOL_ACT
    return m, oracle


def _live_route(dev):
    """Built like tests/enc_live_common.py: build -- the live packed encoder needs a head width its ragged attention serves."""
    shape = dict(V=50, L=24, d=128, h=2, dff=256, T=T, lengths=[T])
    m, sd, blocked, _, _, h = EC.build(shape, 'prior', True)
    m = m.to(dev).eval()
    m.use_packed_live_encoder = True
    sd64 = R.to_dtype(sd, torch.float64)

    def oracle(seq, pos):
        with torch.no_grad():
            ref = EC.live_forward_ref(sd, seq, pos, h, blocked)
            ref64 = EC.live_forward_ref(sd64, seq, pos, h, blocked)
        return ref[0], ref[1], ref64[0], TOL_LIVE
    return m, oracle


ROUTES = {
    'packed': (6, {}),                       # the default packed encoder
    'packed_three_passes': (7, {}),          # ... in micro-batches of 3 + 3 + 1: three plan launches share the granule words
    'live_packed': (6, {}),                  # scatter_rows_kernel does the zeroing
    'padded_with_maps': (6, dict(return_attns=True)),   # seq_plan_kernel, no granules
}


@pytest.mark.parametrize('order', ['back_to_back', 'interleaved_with_eager'])
@pytest.mark.parametrize('route', sorted(ROUTES))
def test_replayed_forward_follows_the_lengths_of_each_batch(dev, route, order):
    B, kw = ROUTES[route]
    m, oracle = _live_route(dev) if route == 'live_packed' else _tiny_route(dev)
    if route == 'packed_three_passes':
        # six samples cannot make three passes with a short last one (micro-batches of 2 give 2 + 2 + 2): seven do, 3 + 3 + 1
        m.workspace_limit_bytes = RP.limit_for_micro_batch(m, T, 3)
        passes, last = RP.forward_passes(m, B, T)
        assert passes >= 3 and last < -(-B // passes), (passes, last)
    elif route != 'live_packed':
        assert RP.forward_passes(m, B, T, want_attn=bool(kw)) == (1, B)
    data = [(s.to(dev), p.to(dev)) for s, p in batches(B)]
    stream = torch.cuda.Stream()
    sseq = torch.zeros((B, T), dtype=torch.int64, device=dev)
    spos = torch.zeros((B, T), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        sseq.copy_(data[0][0])
        spos.copy_(data[0][1])
        _fwd(m, (sseq, spos), **kw)           # eager first: the native model cache and this stream's workspace exist
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = _fwd(m, (sseq, spos), **kw)

    replayed, eager = {}, {}
    with torch.cuda.stream(stream):
        for i, (seq, pos) in enumerate(data):
            sseq.copy_(seq)
            spos.copy_(pos)
            graph.replay()
            replayed[i] = (out[0].clone(), out[1].clone())
            if order == 'interleaved_with_eager':
                # an eager forward of ANOTHER batch in between: same stream, same workspace, a fresh epoch
                j = (i + 2) % len(data)
                eager[j] = _fwd(m, data[j], **kw)[:2]
        for i, src in enumerate(data):
            if i not in eager:
                eager[i] = _fwd(m, src, **kw)[:2]
    stream.synchronize()
    torch.cuda.synchronize()
    for i in range(len(data)):
        assert RP.same_bits(replayed[i][0], eager[i][0]), (route, order, i, 'logits')
        assert RP.same_bits(replayed[i][1], eager[i][1]), (route, order, i, 'enc_output')
    for i, (seq, pos) in enumerate(batches(B)):
        ref_logits, ref_enc, ref64, tol_enc = oracle(seq, pos)
        logits, enc = eager[i]
        assert max_abs_diff(enc, ref_enc) < tol_enc, (route, i)
        gap = max_abs_diff(ref_logits, ref64)
        assert torch.equal(torch.isnan(logits).cpu(), torch.isnan(ref_logits)), (route, i)
        assert max_abs_diff(logits, ref64) < max(TOL_LOGIT, 4 * gap), (route, i, gap)
