"""CPU half of the ragged plan tests: the NumPy restatement of the sequence plan (ragged_plan_common.plan_ref) is tied to the
oracle's own masking, the named length patterns hold what their names say, and the hook that forces the plan hand-off's fall-back
routes exists in the tuning library only."""
import ctypes

import numpy as np
import pytest
import torch

import ragged_plan_common as RP
from oracle import lamp_ref as R


def test_plan_restatement_on_a_worked_example():
    """Counted by hand.  Sample 0: tokens at 0 .. 2.  Sample 1: nothing.  Sample 2: a token at 1 only, position indices up to 3.
    Sample 3: full."""
    seq = np.array([[5, 6, 7, 0, 0], [0, 0, 0, 0, 0], [0, 9, 0, 0, 0], [4, 4, 4, 4, 4]])
    pos = np.array([[1, 2, 3, 0, 0], [0, 0, 0, 0, 0], [1, 2, 3, 4, 0], [1, 2, 3, 4, 5]])
    p = RP.plan_ref(seq, pos)
    assert p['klen'].tolist() == [3, 0, 2, 5] and p['plen'].tolist() == [3, 0, 4, 5]
    assert p['off'].tolist() == [0, 3, 3, 7, 12] and p['rows'].tolist() == [12, 13]
    assert p['padbits'].shape == (4, 1)
    assert p['padbits'][:, 0].tolist() == [0xfffffff8, 0xffffffff, 0xfffffffd, 0xffffffe0]
    q = RP.plan_ref(seq, None)            # no position table: rows stop at the last token
    assert q['plen'].tolist() == q['klen'].tolist() == [3, 0, 2, 5] and q['rows'].tolist() == [10, 11]
    assert np.array_equal(q['padbits'], p['padbits'])
    d = RP.plan_ref(seq[3:], pos[3:])     # nothing skipped: no PAD row
    assert d['rows'].tolist() == [5, 5]
    w = RP.plan_ref(np.ones((1, 33), dtype=np.int64))   # the last, partial word: positions past T count as PAD
    assert w['padbits'].tolist() == [[0, 0xfffffffe]]


def test_patterns_hold_what_their_names_say():
    for nb, T in RP.SWEEP:
        plans = {}
        for name in RP.PATTERNS:
            seq, pos = RP.make_pattern(name, nb, T)
            assert seq.shape == pos.shape == (nb, T) and seq.dtype == pos.dtype == torch.int64
            assert int(seq.min()) >= 0 and int(seq.max()) < RP.VOCAB and int(pos.min()) >= 0 and int(pos.max()) <= T
            assert torch.equal(seq, RP.make_pattern(name, nb, T)[0])          # reproducible
            plans[name] = (seq.numpy(), pos.numpy(), RP.plan_ref(seq.numpy(), pos.numpy()))
        p = plans['dense'][2]
        assert (p['plen'] == T).all() and p['rows'][0] == p['rows'][1] == nb * T
        p = plans['last_short'][2]
        assert p['plen'][-1] == T // 2 and (p['plen'][:-1] == T).all() and p['rows'][1] == p['rows'][0] + 1
        p = plans['first_short'][2]
        assert p['plen'][0] == T // 2 and (p['plen'][1:] == T).all()
        p = plans['zero_length'][2]
        for b in (0, 63, 64, 65, nb - 1):
            if b < nb:
                assert p['plen'][b] == 0 and p['off'][b + 1] == p['off'][b]
        assert nb < 3 or (p['plen'] > 0).any()
        p = plans['all_pad'][2]
        assert (p['plen'] == 0).all() and p['rows'].tolist() == [0, 1] and (p['padbits'] == 0xffffffff).all()
        seq, pos, p = plans['interior_pad']
        assert (p['klen'] == T).all()                                          # the runs are inside
        if T >= 3:
            assert (seq == 0).any() and ((seq == 0) & (pos != 0)).any() == (nb > 1)
        if T > 34:
            assert (seq[:, 31:33] == 0).all() and p['padbits'][0, 0] >> 30 == 3 and p['padbits'][0, 1] & 3 == 3
        if T > 66:
            assert (seq[:, 63:65] == 0).all() and p['padbits'][0, 1] >> 30 == 3 and p['padbits'][0, 2] & 3 == 3
        p = plans['position_tail'][2]
        assert (p['plen'] > p['klen']).all()
        seq, pos, p = plans['last_only']
        for b in {0, nb // 2}:
            assert p['klen'][b] == T and (seq[b] != 0).sum() == 1 and (pos[b] != 0).sum() == 1


@pytest.mark.parametrize('with_pos', [True, False])
@pytest.mark.parametrize('name', sorted(RP.PATTERNS))
def test_plan_restatement_agrees_with_the_oracles_masks(name, with_pos):
    """Derived from oracle.lamp_ref on the tiny model, in fp64.  Blocked keys: the oracle's enc-dec attention gives a blocked key
    the weight 0 exactly and every other key a positive one (all NaN for a sample without a token: every key blocked) -- they are
    the PAD bits.  plen: the oracle's encoder rows at every position >= plen[b] are its shared PAD row (the row of a PAD token
    with position index 0), and the row at plen[b] - 1 is not."""
    sd = R.to_dtype(RP.tiny_state_dict(with_pos), torch.float64)
    h = RP.TINY['h']
    zero = torch.zeros((1, 1), dtype=torch.int64)
    with torch.no_grad():
        pad_row = R.encoder_forward(sd, zero, zero, h)[0][0, 0]
    for nb, T in RP.SWEEP:
        seq, pos = RP.make_pattern(name, nb, T)
        plan = RP.plan_ref(seq.numpy(), pos.numpy() if with_pos else None)
        with torch.no_grad():
            enc, _ = R.encoder_forward(sd, seq, pos, h)
            _, _, enc_attns, _ = R.decoder_forward(sd, seq, enc, None, h)
        a = enc_attns[0].view(h, nb, RP.TINY['L'], T)
        blocked = ((a == 0) | torch.isnan(a))
        assert torch.equal(blocked.all(dim=2).all(dim=0), blocked.any(dim=2).any(dim=0)), (name, nb, T)   # a key's verdict is one
        blocked = blocked[0, :, 0, :].numpy()
        bits = plan['padbits']
        from_bits = np.array([[(int(bits[b, j // 32]) >> (j % 32)) & 1 for j in range(T)] for b in range(nb)], dtype=bool)
        assert np.array_equal(from_bits, blocked), (name, nb, T)
        for b in range(nb):   # the bits past T in the last word are PAD
            for j in range(T, bits.shape[1] * 32):
                assert (int(bits[b, j // 32]) >> (j % 32)) & 1
        is_pad_row = ((enc - pad_row).abs().amax(dim=2) < 1e-9).numpy()
        for b in range(nb):
            pl, kl = int(plan['plen'][b]), int(plan['klen'][b])
            assert is_pad_row[b, pl:].all(), (name, nb, T, b)
            assert pl == 0 or not is_pad_row[b, pl - 1], (name, nb, T, b)
            assert kl <= pl and (kl == 0 or not blocked[b, kl - 1]) and blocked[b, kl:].all(), (name, nb, T, b)
        assert plan['off'][nb] == plan['plen'].sum() == plan['rows'][0]
        assert plan['rows'][1] - plan['rows'][0] == int((plan['plen'] < T).any())


def test_the_plan_mode_hook_is_in_the_tuning_library_only():
    from lamp_amd import _native as N
    product, tuning = ctypes.CDLL(N.LIB_PATH), ctypes.CDLL(N.TUNING_LIB_PATH)
    assert hasattr(tuning, 'lamp_debug_embed_plan_mode')
    assert not hasattr(product, 'lamp_debug_embed_plan_mode')
    assert hasattr(product, 'lamp_forward') and hasattr(tuning, 'lamp_forward')
