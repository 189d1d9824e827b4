"""What the life-cycle of a model needs no device for (tests/lifecycle_common.py): a model that has run an eval forward holds
ctypes structures full of device addresses in ``_native_cache``; copy.deepcopy, pickle and torch.save must leave them -- and
``_param_list``, and the decoder's ``_label_bias_key`` -- behind, and the copy's buffers must be its own.  And the host-only half
of LAMP._native_model, ``_native_key``: it must change when a Parameter or a submodule is replaced and for a version bump of every
tensor a weights-only table is built from."""
import copy
import io
import pickle

import pytest
import torch
import torch.nn as nn

import lifecycle_common as LC


def _with_cache(family):
    """A CPU model in the state an eval forward leaves behind: a stand-in cache holding real N.Model / array instances."""
    from lamp_amd import _native as N
    m = LC.make(family).model
    m._native_cache = (('k',), (N.Model(), (N.EncLayer * 1)(), (N.DecLayer * 1)(), None, (N.ChainPack * 2)()))
    m._param_list = (m._weight_tensors(), -1)
    m.decoder._label_bias_key = (1, 2, 3, 4)
    return m


def _deepcopy(m):
    return copy.deepcopy(m)


def _pickle(m):
    return pickle.loads(pickle.dumps(m))


def _torch_save(m):
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def _averaged(m):
    return torch.optim.swa_utils.AveragedModel(m).module


@pytest.mark.parametrize('how', [_deepcopy, _pickle, _torch_save, _averaged], ids=lambda f: f.__name__.strip('_'))
@pytest.mark.parametrize('family', ['tok', 'onehot', 'lbias'])
def test_a_model_with_filled_caches_copies(family, how):
    m = _with_cache(family)
    c = how(m)
    assert c is not m and type(c) is type(m)
    # the copy starts empty; the original keeps what it had
    assert c._native_cache is None and c._param_list is None and c.decoder._label_bias_key is None
    assert m._native_cache is not None and m._param_list is not None and m.decoder._label_bias_key == (1, 2, 3, 4)
    # same weights, same buffers, none of them shared
    sd_m, sd_c = m.state_dict(), c.state_dict()
    assert sd_m.keys() == sd_c.keys()
    for k in sd_m:
        assert torch.equal(sd_m[k], sd_c[k]) and sd_m[k].data_ptr() != sd_c[k].data_ptr(), k
    bufs_m, bufs_c = dict(m.named_buffers()), dict(c.named_buffers())
    assert bufs_m.keys() == bufs_c.keys() and 'decoder.label_mask_u8' in bufs_m
    for k in bufs_m:
        assert torch.equal(bufs_m[k], bufs_c[k], ) and bufs_m[k].data_ptr() != bufs_c[k].data_ptr(), k
    assert (c.decoder.label_bias_f32 is not None) == (family == 'lbias')
    assert c.tgt_word_proj.weight is c.decoder.tgt_word_emb.weight     # the reference's tie survives
    for flag in LC.FLAGS:
        assert getattr(c, flag) == getattr(m, flag)


def test_route_switches_set_on_the_instance_travel_with_the_copy():
    m = _with_cache('tok')
    m.matmul_precision = 'high'
    m.fold_embedding = False
    for how in (_deepcopy, _torch_save):
        c = how(m)
        assert c.matmul_precision == 'high' and c.fold_embedding is False and c.use_chain_packs is True


# ------------------------------------------------------------------ the key (host integers only: it exists on the CPU too)
def _key(m):
    return m._native_key()[0]


@pytest.mark.parametrize('family', ['tokpos', 'tok', 'live', 'onehot'])
def test_key_moves_with_the_version_of_every_table_feeding_tensor(family):
    m = LC.make(family).model
    assert _key(m) == _key(m)
    feeding = LC.feeding_names(m, family)
    assert feeding
    params = dict(m.named_parameters())
    for name in sorted(feeding):
        before = _key(m)
        LC.perturb(name, params[name])
        assert _key(m) != before, name
    # ... and not with a tensor that only is read through its address
    before = _key(m)
    LC.perturb('tgt_word_proj.linear.weight', m.tgt_word_proj.linear.weight)
    assert _key(m) == before


def test_key_moves_with_an_optimizer_step_that_moves_no_version():
    """torch's fused optimizers write the parameters without moving Parameter._version: the step itself is counted."""
    m = LC.make('tok').model
    p = m.decoder.layer_stack[0].pos_ffn1.w_1.weight
    try:
        optimizer = torch.optim.SGD([p], lr=0.1, fused=True)
    except (RuntimeError, ValueError, TypeError) as e:
        pytest.skip('torch.optim.SGD(fused=True): %s' % e)
    before, was = _key(m), p.detach().clone()
    p.grad = torch.ones_like(p)
    optimizer.step()
    assert not torch.equal(p.detach(), was) and _key(m) != before
    assert _key(m) == _key(m)


def test_key_moves_when_a_parameter_or_a_submodule_is_replaced():
    m = LC.make('tok').model
    seen = [_key(m)]

    def moved():
        seen.append(_key(m))
        return seen[-1] != seen[-2] and seen[-1] == _key(m)
    lin = m.decoder.layer_stack[1].pos_ffn2.w_2
    lin.weight = nn.Parameter(lin.weight.detach().clone())
    assert moved()
    ln = m.decoder.layer_stack[0].slf_attn.layer_norm
    ln.bias = nn.Parameter(torch.zeros_like(ln.bias))
    assert moved()
    m.encoder.src_word_emb = nn.Embedding.from_pretrained(m.encoder.src_word_emb.weight.detach().clone(), freeze=False)
    assert moved()
    m.decoder.tgt_word_emb = nn.Embedding.from_pretrained(m.decoder.tgt_word_emb.weight.detach().clone(), freeze=False)
    assert moved()
    m.decoder.layer_stack[0] = copy.deepcopy(m.decoder.layer_stack[1])
    assert moved()
    a, b = m.decoder.layer_stack[0].enc_attn.w_ks, m.decoder.layer_stack[1].enc_attn.w_ks
    a.weight = b.weight     # tied
    assert moved()
    assert sum(p is b.weight for p in m._native_key()[1]) == 2
    # a model built elsewhere makes this one walk its modules again, and find what it had
    before = _key(m)
    held = m._param_list[0]
    LC.make('tok')
    assert _key(m) == before and m._param_list[0] is not held
    assert all(x is y for x, y in zip(m._param_list[0], held))
    # nothing registered: the walk is not repeated
    held = m._param_list[0]
    assert _key(m) == before and m._param_list[0] is held
