"""LAMP model facade (reference: lamp/Models.py:18-137) for encoder='graph', decoder='graph'.

``forward`` in eval mode on a HIP device is ONE call into liblamp_hip.so (``lamp_forward``): 18
kernel launches for a 2+2-layer model instead of the reference's ~140 ATen ops, no
per-forward mask materialisation, no head split/merge copies, and the discarded encoder
self-attention (lamp/Layers.py:16-18) is simply not computed unless its maps are requested.

``enc_self_attn=True`` switches the encoder's self-attention ON: the feature->feature message passing of the published
model, which the reference's code computes and then overwrites -- its ``w_qs / w_ks / w_vs / fc / layer_norm`` never train
there.  It is this project's own switch (last keyword, default off: every reference call constructs the reference's model),
served by ``lamp_forward_opts`` in eval and by lamp_amd/training.py in training; parameters and ``state_dict`` are the same in
both modes.

``dec_attn_type='sigmoid'`` makes both attention blocks of every decoder layer sigmoid attention (lamp/SubLayers.py:17-25):
the reference accepts ``attn_type`` and never hands it to its layers (lamp/Layers.py:23-30), so ``attn_type`` stays accepted
and ignored here too, and this second project-own keyword (keyword-only in practice: it sits behind the reference's last argument, in front of
``enc_self_attn``) is the opt-in that does what the flag says (``lamp_forward_opts``
with LAMP_FWD_DEC_SIGMOID in eval, lamp_amd/training.py in training).  The encoder stays softmax; ``state_dict`` is unchanged.

``LAMP.matmul_precision`` ('highest' | 'high' | 'bf16x6', default 'highest') is this chip's reading of
``torch.set_float32_matmul_precision``: 'high' runs the nn.Linear-class GEMM launches of the FUSED EVAL forward as three bf16
products per fp32 product on the bf16 matrix pipe (csrc/gemm_split.hip; gfx950 has no TF32), 'bf16x6' as six.  Only that route
takes it: the module-by-module route (baseline encoders / decoders, per-sample input graphs with maps), ``nn.DataParallel``
replicas and ``model.train()`` stay fp32, and so do the chain launch, attention, conv2, the read-out and the weights-only
precomputations inside the fused forward (include/lamp_hip.h: LAMP_FWD_MATMUL_BF16X3).
"""
import ctypes as C

import collections

import torch
import torch.nn as nn

from . import _native as N
from .Decoders import GraphDecoder, MLPDecoder, RNNDecoder, _optimizer_steps
from .Encoders import GraphEncoder, MLPEncoder, RNNEncoder
from .SubLayers import XavierLinear


# Registrations of a Parameter or a submodule anywhere in the process (nn.Module.__setattr__, register_parameter, add_module,
# ModuleList.__setitem__ ... all run torch's global registration hooks).  LAMP._native_model() keeps the Parameter OBJECTS of its
# first walk; it walks again once this count has moved, so `lin.weight = nn.Parameter(...)`, `encoder.src_word_emb =
# nn.Embedding.from_pretrained(...)` and weight tying are seen by the next forward -- at the price of one integer comparison per
# cache hit.  (Writes into a module's `_parameters` / `_modules` dicts behind nn.Module's back are not seen.)
_registrations = [0]


def _count_registration(module, name, value):
    _registrations[0] += 1


torch.nn.modules.module.register_module_parameter_registration_hook(_count_registration)
torch.nn.modules.module.register_module_module_registration_hook(_count_registration)


def _chain_pack(fc, w1, w2, keep):
    """lamp_chain_pack of one sub-chain's (fc, w_1, w_2) in both formats; the packed tensors are appended to `keep`."""
    ptrs = []
    for fmt in (0, 1):
        trio = [N.weight_pack(w, fmt) for w in (fc, w1, w2)]
        if any(t is None for t in trio):
            trio = [None] * 3
        keep.append(trio)
        ptrs += [N.ptr(t) for t in trio]
    return N.ChainPack(*ptrs)


class _MatmulPrecision:
    """LAMP.matmul_precision: reads 'highest' on the class and on a model that never set it; setting it on a model validates the
    name (ValueError) and touches no other attribute's assignment."""

    def __get__(self, obj, owner=None):
        return 'highest' if obj is None else obj.__dict__.get('_matmul_precision', 'highest')

    def __set__(self, obj, value):
        N.matmul_precision(value)   # ValueError for anything but 'highest' / 'high' / 'bf16x6'
        obj.__dict__['_matmul_precision'] = value

    def __delete__(self, obj):
        obj.__dict__.pop('_matmul_precision', None)


class LAMP(nn.Module):
    def __init__(self, n_src_vocab, n_tgt_vocab, n_max_seq_e, n_max_seq_d, n_layers_enc=6, n_layers_dec=6,
                 n_head=8, n_head2=8, d_word_vec=512, d_model=512, d_inner_hid=1024, d_k=64, d_v=64,
                 dropout=0.1, dec_dropout=0.1, dec_dropout2=0.1, proj_share_weight=True,
                 embs_share_weight=True, encoder='selfatt', decoder='sa_m', enc_transform='', onehot=False,
                 no_enc_pos_embedding=False, no_dec_self_att=False, loss='ce', label_adj_matrix=None,
                 label_mask=None, matching_mlp=False, graph_conv=False, attn_type='softmax', int_preds=False,
                 dec_attn_type=None, label_bias=None, learn_label_bias=False, enc_self_attn=False):
        super().__init__()
        if (label_bias is not None or learn_label_bias) and decoder != 'graph':
            raise NotImplementedError('label_bias belongs to the graph decoder, not to decoder=%r' % (decoder,))
        if dec_attn_type is not None and decoder != 'graph':
            raise NotImplementedError('dec_attn_type belongs to the graph decoder, not to decoder=%r' % (decoder,))
        if dec_attn_type is not None and dec_attn_type not in N.ATTN_TYPES:
            raise NotImplementedError("dec_attn_type=%r: None, 'softmax' or 'sigmoid'" % (dec_attn_type,))
        self.dec_attn_type = dec_attn_type
        if enc_self_attn and encoder != 'graph':
            raise NotImplementedError('enc_self_attn=True belongs to the graph encoder, not to encoder=%r' % (encoder,))
        self.enc_self_attn = bool(enc_self_attn)
        if d_model != d_word_vec:
            raise ValueError('d_model must equal d_word_vec (residual connections)')
        self.decoder_type = decoder
        self.onehot = onehot
        self.loss = loss
        self.enc_vec = encoder == 'mlp' or enc_transform != ''

        if encoder == 'graph':
            self.encoder = GraphEncoder(
                n_src_vocab, n_max_seq_e, n_layers=n_layers_enc, n_head=n_head, d_word_vec=d_word_vec,
                d_model=d_model, d_k=d_k, d_v=d_v, d_inner_hid=d_inner_hid, onehot=onehot, dropout=dropout,
                no_enc_pos_embedding=no_enc_pos_embedding, enc_transform=enc_transform, enc_self_attn=enc_self_attn)
        elif encoder == 'mlp':
            self.encoder = MLPEncoder(
                n_src_vocab, n_max_seq_e, n_layers=n_layers_enc, n_head=n_head, d_word_vec=d_word_vec, d_model=d_model,
                d_k=d_k, d_v=d_v, d_inner_hid=d_inner_hid, onehot=onehot, dropout=dropout)
        elif encoder == 'rnn':
            self.encoder = RNNEncoder(
                n_src_vocab, n_max_seq_e, n_layers=n_layers_enc, n_head=n_head, d_word_vec=d_word_vec, d_model=d_model,
                d_k=d_k, d_v=d_v, d_inner_hid=d_inner_hid, onehot=onehot, dropout=dropout)
        else:
            raise NotImplementedError(encoder)

        if decoder == 'graph':
            self.decoder = GraphDecoder(
                n_tgt_vocab, n_max_seq_d, n_layers=n_layers_dec, n_head=n_head, n_head2=n_head2,
                d_word_vec=d_word_vec, d_model=d_model, d_k=d_k, d_v=d_v, d_inner_hid=d_inner_hid,
                dropout=dec_dropout, dropout2=dec_dropout2, no_dec_self_att=no_dec_self_att,
                label_adj_matrix=label_adj_matrix, label_mask=label_mask, enc_vec=self.enc_vec,
                graph_conv=graph_conv, attn_type=attn_type, dec_attn_type=dec_attn_type, label_bias=label_bias,
                learn_label_bias=bool(learn_label_bias))
        elif decoder == 'mlp':
            self.decoder = MLPDecoder(
                n_tgt_vocab, n_max_seq_e, n_max_seq_d, n_layers=n_layers_dec, n_head=n_head, d_word_vec=d_word_vec,
                d_model=d_model, d_k=d_k, d_v=d_v, d_inner_hid=d_inner_hid, dropout=dec_dropout,
                enc_transform=enc_transform)
        elif decoder == 'rnn_m':
            self.decoder = RNNDecoder(
                n_tgt_vocab, n_max_seq_d, n_layers=n_layers_dec, n_head=n_head, d_word_vec=d_word_vec, d_model=d_model,
                d_k=d_k, d_v=d_v, d_inner_hid=d_inner_hid, dropout=dec_dropout)
        else:
            raise NotImplementedError(decoder)   # 'sa_m' & co. exist in the reference's argparse only (lamp/Models.py:76-77)

        # Read-out.  Assigning the embedding Parameter to `tgt_word_proj.weight` registers a second
        # key on the XavierLinear wrapper but does NOT tie `tgt_word_proj.linear.weight`, which stays
        # the matrix the forward uses -- exactly the reference's (accidental) behaviour; both keys
        # are needed for checkpoint compatibility (lamp/Models.py:87-94).
        bias = self.decoder_type in ('mlp', 'graph', 'star') and not proj_share_weight
        if self.decoder_type != 'mlp':   # lamp/Models.py:86-94: the mlp decoder carries its own output layer
            if proj_share_weight:
                self.tgt_word_proj = XavierLinear(d_model, n_tgt_vocab, bias=bias)
                self.tgt_word_proj.weight = self.decoder.tgt_word_emb.weight
            else:
                self.tgt_word_proj = XavierLinear(d_model, 1, bias=bias)
            if int_preds:
                self.tgt_word_proj_copy = XavierLinear(d_model, n_tgt_vocab, bias=bias)
        # the fused lamp_forward launcher takes the graph model with per-token encoder states; everything else runs
        # module by module (graph parts on the HIP kernels, the baseline parts in plain PyTorch)
        self._fused = (encoder == 'graph' and decoder == 'graph' and not self.enc_vec)

        self.d_model, self.d_inner, self.d_k, self.d_v = d_model, d_inner_hid, d_k, d_v
        self.n_labels = n_tgt_vocab
        self._native_cache = None
        self._param_list = None

    def __getstate__(self):
        """copy.deepcopy, pickle and torch.save(model): the cached descriptor (ctypes structures full of device addresses) and the
        cached Parameter list stay behind -- a copy builds its own tables on its first forward."""
        state = self.__dict__.copy()
        state['_native_cache'] = state['_param_list'] = None
        return state

    def get_trainable_parameters(self):
        """Everything but the frozen sinusoid table, and the one-hot encoder's identity table (reference: lamp/Models.py:97-107)."""
        frozen = set()
        if hasattr(self.encoder, 'position_enc'):
            frozen |= {id(p) for p in self.encoder.position_enc.parameters()}
        if self.onehot:
            frozen |= {id(p) for p in self.encoder.src_word_emb.parameters()}
        return (p for p in self.parameters() if id(p) not in frozen)

    # ------------------------------------------------------------------ native model descriptor
    def invalidate_native_cache(self):
        """Drop the cached lamp_model descriptor and the hoisted layer-0 query projection.  Called by load_state_dict,
        train() / eval() and _apply (.to / .cuda); call it yourself after modifying weights through ``.data`` (in-place
        updates via ``p.data`` do not bump ``p._version``, which is what the cache otherwise watches) or after writing into a
        module's ``_parameters`` / ``_modules`` dicts directly (replacing a Parameter or a submodule by assignment is seen without
        it: _native_key)."""
        self._native_cache = None
        self._param_list = None
        if getattr(getattr(self, 'decoder', None), '_label_bias_key', None) is not None:
            self.decoder._label_bias_key = None   # a learnable label bias is folded into its buffer again on the next forward

    def load_state_dict(self, state_dict, *args, **kwargs):
        """nn.Module.load_state_dict; additionally accepts checkpoints saved from an nn.DataParallel wrapper
        (main.py:106-108 wraps the model BEFORE utils.save_model, so multi-GPU hosts write ``module.``-prefixed keys)."""
        if state_dict and all(k.startswith('module.') for k in state_dict):
            stripped = collections.OrderedDict((k[len('module.'):], v) for k, v in state_dict.items())
            meta = getattr(state_dict, '_metadata', None)
            if meta is not None:   # per-module version records, keyed by module path
                stripped._metadata = collections.OrderedDict(
                    (k[len('module.'):] if k.startswith('module.') else ('' if k == 'module' else k), v) for k, v in meta.items())
            state_dict = stripped
        self.invalidate_native_cache()
        return super().load_state_dict(state_dict, *args, **kwargs)

    def train(self, mode=True):
        self.invalidate_native_cache()   # an optimiser may have stepped through .data; eval recomputes the hoisted query
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_native_cache()
        return super()._apply(fn, *args, **kwargs)

    def _weight_tensors(self):
        """Every weight tensor the descriptor points to, in a fixed order, fetched by ATTRIBUTE: a DataParallel
        replica (torch/nn/parallel/replicate.py) has an empty ``_parameters`` -- ``self.parameters()`` yields nothing
        there -- but carries its device's copies as plain attributes."""
        if not self._fused:
            raise NotImplementedError('the lamp_model descriptor exists for the graph encoder + graph decoder only')
        enc, dec = self.encoder, self.decoder
        out = [enc.src_word_emb.weight, dec.tgt_word_emb.weight, self.tgt_word_proj.linear.weight]
        if hasattr(enc, 'position_enc'):
            out.append(enc.position_enc.weight)

        def mha(m):
            out.extend((m.w_qs.weight, m.w_ks.weight, m.w_vs.weight, m.layer_norm.weight, m.layer_norm.bias))
            if getattr(m, 'fc', None) is not None:
                out.append(m.fc.weight)

        def ffn(m):
            out.extend((m.w_1.weight, m.w_1.bias, m.w_2.weight, m.w_2.bias, m.layer_norm.weight, m.layer_norm.bias))
        for l in enc.layer_stack:
            mha(l.slf_attn)
            ffn(l.pos_ffn)
        for l in dec.layer_stack:
            mha(l.enc_attn)
            ffn(l.pos_ffn1)
            if hasattr(l, 'slf_attn'):
                mha(l.slf_attn)
            ffn(l.pos_ffn2)
        return out

    def _fold_weights(self):
        """(token table, position table or None, W1, b1) of the encoder's first layer."""
        enc = self.encoder
        ff = enc.layer_stack[0].pos_ffn
        return (enc.src_word_emb.weight, enc.position_enc.weight if hasattr(enc, 'position_enc') else None,
                ff.w_1.weight, ff.w_1.bias)

    def _onehot_weights(self):
        enc = self.encoder
        return (enc.src_word_emb.weight, enc.conv1.weight, enc.conv1.bias, enc.conv2.weight, enc.conv2.bias)

    def _chain_weights(self):
        out = []
        for l in self.decoder.layer_stack:
            for att, ff in ((l.enc_attn, l.pos_ffn1), (getattr(l, 'slf_attn', None), l.pos_ffn2)):
                if att is not None and getattr(att, 'fc', None) is not None:
                    out += [att.fc.weight, ff.w_1.weight, ff.w_2.weight]
        return out

    def _enc_chain_weights(self):
        out = []
        for l in self.encoder.layer_stack:
            if getattr(l.slf_attn, 'fc', None) is not None:
                out += [l.slf_attn.fc.weight, l.pos_ffn.w_1.weight, l.pos_ffn.w_2.weight]
        return out

    def _gemm_pack_weights(self):
        """The matrices lamp_gemm_packs covers: every encoder layer's pos_ffn (w_1, w_2), every decoder layer's enc_attn.w_qs and
        slf_attn (w_qs, w_ks, w_vs); and lamp_kv_gemm_pack: every decoder layer's enc_attn (w_ks, w_vs), the K / V projection of the
        encoder rows.  -> (encoder pairs, decoder quads, decoder K / V pairs; None where a block does not exist)"""
        enc = [(l.pos_ffn.w_1.weight, l.pos_ffn.w_2.weight) for l in self.encoder.layer_stack]
        dec = []
        for l in self.decoder.layer_stack:
            slf = getattr(l, 'slf_attn', None)
            dec.append((l.enc_attn.w_qs.weight,) + (tuple(getattr(slf, n).weight for n in ('w_qs', 'w_ks', 'w_vs')) if slf is not None
                                                     else (None, None, None)))
        kv = [(l.enc_attn.w_ks.weight, l.enc_attn.w_vs.weight) for l in self.decoder.layer_stack]
        return enc, dec, kv

    def _native_key(self):
        """What decides whether the cached descriptor is current -- host integers only, nothing is launched or read back (but a
        learnable label bias that changed is folded again on the way: GraphDecoder.current_label_bias).  The key holds data_ptr()
        of every weight, the route switches, and _version of exactly the weights each weights-only table reads.
        -> (key, the weight tensors, what _native_model builds from)"""
        replica = getattr(self, '_is_replica', False)
        # the Parameter objects of the original module are stable (load_state_dict / .to() replace their data, not
        # them) until somebody registers a Parameter or a submodule (_registrations): keep the list until then.  A
        # DataParallel replica is rebuilt on every forward with fresh tensors: no caching.
        params = None
        if not replica and self._param_list is not None and self._param_list[1] == _registrations[0]:
            params = self._param_list[0]
        if params is None:
            epoch = _registrations[0]
            params = self._weight_tensors()
            if not replica:
                self._param_list = (params, epoch)
        mask = self.decoder.label_mask_u8
        tiles = self.decoder.label_tiles
        bits = self.decoder.label_mask_bits
        bias = self.decoder.current_label_bias()   # (a learnable bias: folded again here when the parameter changed)
        if bias is not None:   # LAMP_FWD_LABEL_BIAS: the bias rides in the label_mask slot, its companions stay empty
            mask, tiles, bits = bias, None, None
        hoist = self.cache_layer0_query and not replica   # the hoisted projection needs a one-off stream sync
        packs = self.use_chain_packs and not replica      # weights-only repacks: same one-off cost, same staleness rule
        onehot = bool(getattr(self.encoder, 'onehot', False))
        live = self.enc_self_attn
        # fragment-major copies for the tile GEMM launches (lamp_forward_packs; the one-hot forward has no such entry point)
        gpacks = bool(self.use_gemm_packs and not replica and not onehot and getattr(N.lib(), 'lamp_forward_packs', None))
        kvpacks = bool(gpacks and self.use_kv_gemm_packs and getattr(N.lib(), 'lamp_forward_packs_kv', None))
        # weights-only tables, likewise; a live layer 0 starts with the attention, not with W1: nothing to fold into
        fold = self.fold_embedding and not replica and len(self.encoder.layer_stack) > 0 and not onehot and not live
        sparse = bool(self.use_sparse_label_attention and self.use_mask_bits and self.decoder.label_rows_sparse and bias is None)
        key = tuple(p.data_ptr() for p in params) + (N.ptr(mask), N.ptr(bits), N.ptr(tiles), self.use_label_tiles,
                                                      hoist, self.use_mask_bits, packs, fold, sparse, live, bias is not None, gpacks, kvpacks,
                                                      _optimizer_steps[0])   # (fused torch optimizers move no _version)
        if hoist:  # the hoisted projection below is stale once either operand changes
            l0 = self.decoder.layer_stack[0].enc_attn
            key += (self.decoder.tgt_word_emb.weight._version, l0.w_qs.weight._version)
        if packs:
            key += tuple(w._version for w in self._chain_weights())
            if live:
                key += tuple(w._version for w in self._enc_chain_weights())
        if gpacks:
            key += tuple(w._version for group in self._gemm_pack_weights() for ws in group for w in ws if w is not None)
        if fold:
            key += tuple(w._version for w in self._fold_weights() if w is not None)
        if onehot:   # the tap table and W2's repack are weights-only: rebuilt per weight version
            key += tuple((w.data_ptr(), w._version) for w in self._onehot_weights())
        return key, params, (replica, mask, tiles, bits, hoist, packs, onehot, live, gpacks, kvpacks, fold, sparse)

    def _native_model(self):
        """Build (and cache under _native_key) the lamp_model struct and the weights-only tables that go with it."""
        key, params, flags = self._native_key()
        replica = flags[0]
        cache = None if replica else self._native_cache
        if cache is not None and cache[0] == key:
            return cache[1]
        replica, mask, tiles, bits, hoist, packs, onehot, live, gpacks, kvpacks, fold, sparse = flags
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError('lamp_amd expects contiguous fp32 parameters')
        N.require_device(*params)
        enc, dec = self.encoder, self.decoder
        enc_arr = (N.EncLayer * max(1, len(enc.layer_stack)))()
        for i, l in enumerate(enc.layer_stack):
            enc_arr[i] = N.EncLayer(N.mha_weights(l.slf_attn), N.ffn_weights(l.pos_ffn))
        dec_arr = (N.DecLayer * max(1, len(dec.layer_stack)))()
        for i, l in enumerate(dec.layer_stack):
            slf = N.mha_weights(l.slf_attn) if hasattr(l, 'slf_attn') else N.MhaWeights()
            dec_arr[i] = N.DecLayer(N.mha_weights(l.enc_attn), N.ffn_weights(l.pos_ffn1), slf,
                                    N.ffn_weights(l.pos_ffn2))
        pos = enc.position_enc.weight if hasattr(enc, 'position_enc') else None
        w_out = self.tgt_word_proj.linear.weight
        if w_out.size(0) != self.n_labels:
            raise NotImplementedError('proj_share_weight=False read-out is not on the graph path')
        m = N.Model(enc.src_word_emb.weight.size(0), pos.size(0) if pos is not None else 0, self.n_labels,
                    self.d_model, self.d_inner, self.d_k, self.d_v, len(enc.layer_stack), len(dec.layer_stack),
                    N.LAMP_MASK_SPARSE_ROWS if sparse else 0, N.ptr(enc.src_word_emb.weight), N.ptr(pos), N.ptr(dec.tgt_word_emb.weight),
                    N.ptr(w_out), N.ptr(mask), N.ptr(bits) if self.use_mask_bits else 0,
                    N.ptr(tiles) if self.use_label_tiles else 0, enc_arr, dec_arr, 0)
        m.label_mask_allowed = self.decoder.label_allowed_pairs if sparse else 0
        q0 = None
        if hoist and len(dec.layer_stack) > 0:
            # decoder layer 0's query = label table x W_q: weights only, so it is projected here once per
            # weight version (lamp_linear_fwd) instead of on every forward
            q0 = N.linear(dec.tgt_word_emb.weight.detach(), dec.layer_stack[0].enc_attn.w_qs.weight.detach())
            m.dec0_query = q0.data_ptr()
            # forwards may be issued from several streams (evaluate.test_epoch(streams=2)); the cached
            # projection must be complete before any of them reads it -- a one-off sync per weight version
            torch.cuda.current_stream().synchronize()
        pack_arr = pack_keep = None
        if packs and len(dec.layer_stack) > 0:
            # the decoder sub-chains' weights in the order the fused chain launch streams them (lamp_pack_weight): weights
            # only, rebuilt once per weight version like the hoisted query above; same bits with and without
            pack_arr = (N.ChainPack * (2 * len(dec.layer_stack)))()
            pack_keep = []
            for i, l in enumerate(dec.layer_stack):
                for j, (att, ff) in enumerate(((l.enc_attn, l.pos_ffn1), (getattr(l, 'slf_attn', None), l.pos_ffn2))):
                    if att is None or getattr(att, 'fc', None) is None:
                        continue
                    pack_arr[2 * i + j] = _chain_pack(att.fc.weight, ff.w_1.weight, ff.w_2.weight, pack_keep)
            m.chain_packs = pack_arr
            torch.cuda.current_stream().synchronize()
        enc_pack_arr = None
        if packs and live and len(enc.layer_stack) > 0:
            # the live encoder layers' row-local tails are the same sub-chain (lamp_fwd_options.enc_chain_packs)
            enc_pack_arr = (N.ChainPack * len(enc.layer_stack))()
            pack_keep = pack_keep if pack_keep is not None else []
            for i, l in enumerate(enc.layer_stack):
                if getattr(l.slf_attn, 'fc', None) is None:
                    continue
                enc_pack_arr[i] = _chain_pack(l.slf_attn.fc.weight, l.pos_ffn.w_1.weight, l.pos_ffn.w_2.weight, pack_keep)
            torch.cuda.current_stream().synchronize()
        gemm_keep = None
        if gpacks:
            # the same format-0 copies for the projections and encoder FFN matrices that run as tile-GEMM launches
            # (lamp_gemm_packs): weights only, rebuilt once per weight version like the chain packs; same bits with and without
            enc_ws, dec_ws, kv_ws = self._gemm_pack_weights()
            tensors = []

            def pk(w):
                t = N.weight_pack(w, 0) if w is not None else None
                tensors.append(t)
                return N.ptr(t)
            enc_gp = (N.EncGemmPack * max(1, len(enc_ws)))(*[N.EncGemmPack(*[pk(w) for w in ws]) for ws in enc_ws])
            dec_gp = (N.DecGemmPack * max(1, len(dec_ws)))(*[N.DecGemmPack(*[pk(w) for w in ws]) for ws in dec_ws])
            kv_gp = None   # the K / V projection's packs have an entry point of their own: a library without it is never handed them
            if kvpacks:
                kv_gp = (N.KvGemmPack * max(1, len(kv_ws)))(*[N.KvGemmPack(*[pk(w) for w in ws]) for ws in kv_ws])
            gemm_keep = (N.GemmPacks(enc_gp, dec_gp), enc_gp, dec_gp, tensors, kv_gp)
            torch.cuda.current_stream().synchronize()
        fold_keep = None
        if fold:
            # encoder layer 0's W1 folded into the embedding tables (lamp_model.enc0_emb_w1 / enc0_pos_w1, include/lamp_hip.h):
            # the gather is a one-hot product, so relu((Emb[tok] + Pos[p]) W1^T + b1) = relu((Emb W1^T)[tok] + (Pos W1^T + b1)[p]).
            # Weights only -- built with lamp_linear_fwd once per weight version, like the hoisted query above.
            emb_w, pos_w, w1, b1 = self._fold_weights()
            w1 = w1.detach().reshape(w1.size(0), -1)
            e1 = N.linear(emb_w.detach(), w1, None if pos_w is not None else b1.detach())
            p1 = N.linear(pos_w.detach(), w1, b1.detach()) if pos_w is not None else None
            m.enc0_emb_w1, m.enc0_pos_w1 = e1.data_ptr(), N.ptr(p1)
            fold_keep = (e1, p1)
            torch.cuda.current_stream().synchronize()
        onehot_keep = None
        if onehot:
            # lamp_onehot_frontend: conv1 as a gather from t1 = E . W1 (a pure repack for the reference's identity E), W2 repacked
            # [co][t][ci] for the implicit-GEMM conv2; built once per weight version like the tables above
            e_w, w1, b1, w2, b2 = (w.detach() for w in self._onehot_weights())
            t1 = N.onehot_tap_table(e_w, w1)
            w2c, b1c, b2c = N.f32c(w2), N.f32c(b1), N.f32c(b2)
            w2p = N.conv_pack(w2c)
            fe = N.onehot_frontend(t1, b1c, w2c, b2c, w2p)
            onehot_keep = (fe, t1, w2c, b1c, b2c, w2p)
            torch.cuda.current_stream().synchronize()
        built = (m, enc_arr, dec_arr, q0, pack_arr, pack_keep, fold_keep, onehot_keep, enc_pack_arr, gemm_keep)
        if not replica:
            self._native_cache = (key, built)
        return built

    def _forward_composite(self, src, adj, tgt_seq, return_attns, int_preds):
        """lamp/Models.py:110-137 module by module, for the model combinations outside the fused launcher: the mlp /
        rnn baselines (plain PyTorch) and the graph decoder fed by a vector encoder (mlp, or graph + enc_transform)."""
        src_seq, src_pos = src
        batch_size = src_seq.size(0)
        if self.decoder_type in ('sa_m', 'rnn_m'):
            tgt_seq = tgt_seq[:, :-1]
        enc_output, *enc_self_attns = self.encoder(src_seq, adj, src_pos, return_attns=return_attns)
        dec_output, *dec_output2 = self.decoder(tgt_seq, src_seq, enc_output, return_attns=return_attns,
                                                int_preds=int_preds)
        if self.decoder_type in ('rnn_m', 'mlp'):
            seq_logit = dec_output
        else:
            w = self.tgt_word_proj.linear.weight
            if self.decoder_type == 'graph' and w.size(0) == dec_output.size(1) and self.tgt_word_proj.linear.bias is None:
                if self.training:
                    from . import training
                    seq_logit = training._ReadoutFn.apply(dec_output, w)
                else:
                    seq_logit = N.diag_logits(dec_output, w)   # diag(y W^T) without the (B, L, L) product
            else:
                seq_logit = self.tgt_word_proj(dec_output)
                if self.decoder_type == 'graph':
                    seq_logit = torch.diagonal(seq_logit, 0, 1, 2)
        if int_preds:
            w = self.tgt_word_proj.linear.weight.detach()
            if self.training:
                from . import training
                preds = [training._ReadoutFn.apply(o, w) for o in dec_output2[0][:-1]]
            else:
                preds = [N.diag_logits(o, w) for o in dec_output2[0][:-1]]
            return seq_logit.reshape(-1, seq_logit.size(-1)), enc_output, preds
        if return_attns:
            return seq_logit.reshape(-1, seq_logit.size(-1)), enc_output, enc_self_attns, dec_output2
        return seq_logit.reshape(-1, seq_logit.size(-1)), enc_output, None

    def forward(self, src, adj, tgt_seq, binary_tgt, return_attns=False, int_preds=False):
        if self.onehot and adj:
            raise NotImplementedError('per-sample input graphs (adj) are not served with the one-hot encoder')
        if not self._fused:
            return self._forward_composite(src, adj, tgt_seq, return_attns, int_preds)
        if adj and return_attns and not int_preds and not self.training and not self.enc_self_attn:
            # per-sample input graphs only shape the encoder's attention MAPS (its output is dead compute): the maps come
            # from the module-by-module route, everything else from the fused launcher below, which may ignore `adj`
            return self._forward_composite(src, adj, tgt_seq, return_attns, int_preds)
        src_seq, src_pos = src
        if src_seq.is_cuda and src_seq.device.index != torch.cuda.current_device():
            # every launch goes to the CURRENT device's stream: make the tensors' device current for the call
            with torch.cuda.device(src_seq.device):
                return self.forward(src, adj, tgt_seq, binary_tgt, return_attns=return_attns, int_preds=int_preds)
        N.require_device(src_seq, src_pos)
        if self.training:
            # train.py:36: the autograd-recording path (HIP kernels forward and backward, lamp_amd/training.py)
            from . import training
            return training.forward_train(self, src_seq, src_pos, return_attns=bool(return_attns and not int_preds),
                                          int_preds=bool(int_preds), adj=adj if self.enc_self_attn else None)
        dev = src_seq.device
        seq = src_seq.long().contiguous()
        pos = src_pos.long().contiguous()
        B, T = seq.shape
        L, d = self.n_labels, self.d_model
        built = self._native_model()
        model, enc_arr, dec_arr = built[:3]
        fe = built[7][0] if self.onehot else None
        gp = built[9][0] if built[9] is not None else None
        T_in = T
        if fe is not None:
            T = T_in // 2   # lamp/Encoders.py:69-73: the encoder sees T / 2 rows
        Ne, Nd = model.n_layers_enc, model.n_layers_dec

        logits = torch.empty((B, L), dtype=torch.float32, device=dev)
        enc_output = torch.empty((B, T, d), dtype=torch.float32, device=dev)

        aux, keep = None, []
        want_attn = bool(return_attns and not int_preds)
        enc_attns = slf_attns = encdec_attns = ipreds = None
        if int_preds:
            n_int = sum(2 if hasattr(l, 'slf_attn') else 1 for l in self.decoder.layer_stack) - 1
            ipreds = [torch.empty((B, L), dtype=torch.float32, device=dev) for _ in range(n_int)]
            arr = (C.c_void_p * max(1, n_int))(*[t.data_ptr() for t in ipreds])
            keep.append(arr)
            aux = N.Aux(None, None, None, arr, n_int, 0)
        elif want_attn:
            def alloc(h, lq, lk):
                return torch.empty((h * B, lq, lk), dtype=torch.float32, device=dev)
            enc_attns = [alloc(l.slf_attn.n_head, T, T) for l in self.encoder.layer_stack]
            slf_attns = [alloc(l.slf_attn.n_head, L, L) if hasattr(l, 'slf_attn') else None
                         for l in self.decoder.layer_stack]
            encdec_attns = [alloc(l.enc_attn.n_head, L, T) for l in self.decoder.layer_stack]
            a0 = (C.c_void_p * max(1, Ne))(*[t.data_ptr() for t in enc_attns])
            a1 = (C.c_void_p * max(1, Nd))(*[N.ptr(t) for t in slf_attns])
            a2 = (C.c_void_p * max(1, Nd))(*[t.data_ptr() for t in encdec_attns])
            keep += [a0, a1, a2]
            aux = N.Aux(a0, a1, a2, None, 0, 0)

        lib = N.lib()
        opts = None
        if self.enc_self_attn:
            # the live encoder self-attention (lamp_fwd_options): per-sample input graphs ride along as one byte mask
            opts = N.FwdOptions(1, N.LAMP_FWD_PACKED_ENCODER if self.use_packed_live_encoder else 0, None, built[8])
            if adj:
                from .Encoders import adj_attn_mask
                m8 = adj_attn_mask(seq, adj)
                mstruct = N.Mask(N.LAMP_MASK_U8, 0, m8.data_ptr(), T * T, T, None, 0, 0)
                keep += [m8, mstruct]
                opts.enc_mask = C.pointer(mstruct)
        if self.dec_attn_type == 'sigmoid':   # both decoder attention blocks: sigmoid attention (LAMP_FWD_DEC_SIGMOID)
            if opts is None:
                opts = N.FwdOptions(0, 0, None, None)
            opts.flags |= N.LAMP_FWD_DEC_SIGMOID
        if getattr(self.decoder, 'label_bias_f32', None) is not None:   # the label_mask slot holds the score bias
            if opts is None:
                opts = N.FwdOptions(0, 0, None, None)
            opts.flags |= N.LAMP_FWD_LABEL_BIAS
        prec_flag = N.matmul_precision(self.matmul_precision)[1]
        if prec_flag and not getattr(self, '_is_replica', False):   # the nn.Linear-class GEMMs as bf16 split products (LAMP_FWD_MATMUL_*)
            if opts is None:
                opts = N.FwdOptions(0, 0, None, None)
            opts.flags |= prec_flag
        if opts is not None and fe is not None:
            def ws_bytes(mb):
                return lib.lamp_onehot_forward_opts_workspace_bytes(C.byref(model), C.byref(fe), C.byref(opts), mb, T_in,
                                                                    int(want_attn))
        elif opts is not None:
            def ws_bytes(mb):
                return lib.lamp_forward_opts_workspace_bytes(C.byref(model), C.byref(opts), mb, T, int(want_attn))
        elif fe is not None:
            def ws_bytes(mb):
                return lib.lamp_onehot_forward_workspace_bytes(C.byref(model), C.byref(fe), mb, T_in, int(want_attn))
        else:
            def ws_bytes(mb):
                return lib.lamp_forward_workspace_bytes(C.byref(model), mb, T, int(want_attn))
        per_sample = ws_bytes(1)
        fixed = 2 * per_sample - ws_bytes(2)
        # enough for the whole batch in one pass unless that exceeds the cap (then it micro-batches)
        whole = fixed + (per_sample - fixed) * B + 4096
        budget = max(per_sample + 4096, min(whole, self.workspace_limit_bytes))
        ws = N.workspace(budget, dev)
        # the grow-only buffer may be larger than this call's budget (an earlier, larger call): hand over the budget, so that
        # workspace_limit_bytes decides the micro-batch split whatever ran before
        ws_given = min(ws.numel(), budget)
        if opts is not None and fe is not None:
            N.check(lib.lamp_onehot_forward_opts(C.byref(model), C.byref(fe), C.byref(opts), seq.data_ptr(), pos.data_ptr(), B,
                                                 T_in, logits.data_ptr(), enc_output.data_ptr(),
                                                 C.byref(aux) if aux is not None else None, ws.data_ptr(), ws_given,
                                                 N.stream()), 'lamp_onehot_forward_opts')
        elif gp is not None and fe is None and built[9][4] is not None:
            N.check(lib.lamp_forward_packs_kv(C.byref(model), C.byref(opts) if opts is not None else None, C.byref(gp), built[9][4],
                                              seq.data_ptr(), pos.data_ptr(), B, T, logits.data_ptr(), enc_output.data_ptr(),
                                              C.byref(aux) if aux is not None else None, ws.data_ptr(), ws_given, N.stream()),
                    'lamp_forward_packs_kv')
        elif gp is not None and fe is None:
            N.check(lib.lamp_forward_packs(C.byref(model), C.byref(opts) if opts is not None else None, C.byref(gp), seq.data_ptr(),
                                           pos.data_ptr(), B, T, logits.data_ptr(), enc_output.data_ptr(),
                                           C.byref(aux) if aux is not None else None, ws.data_ptr(), ws_given, N.stream()),
                    'lamp_forward_packs')
        elif opts is not None:
            N.check(lib.lamp_forward_opts(C.byref(model), C.byref(opts), seq.data_ptr(), pos.data_ptr(), B, T,
                                          logits.data_ptr(), enc_output.data_ptr(), C.byref(aux) if aux is not None else None,
                                          ws.data_ptr(), ws_given, N.stream()), 'lamp_forward_opts')
        elif fe is not None:
            N.check(lib.lamp_onehot_forward(C.byref(model), C.byref(fe), seq.data_ptr(), pos.data_ptr(), B, T_in,
                                            logits.data_ptr(), enc_output.data_ptr(), C.byref(aux) if aux is not None else None,
                                            ws.data_ptr(), ws_given, N.stream()), 'lamp_onehot_forward')
        else:
            N.check(lib.lamp_forward(C.byref(model), seq.data_ptr(), pos.data_ptr(), B, T, logits.data_ptr(),
                                     enc_output.data_ptr(), C.byref(aux) if aux is not None else None,
                                     ws.data_ptr(), ws_given, N.stream()), 'lamp_forward')
        del keep
        if int_preds:
            return logits, enc_output, ipreds
        if want_attn:
            return logits, enc_output, [enc_attns], [slf_attns, encdec_attns]
        return logits, enc_output, None

    def predict_topk(self, src, k, adj=None):
        """The k most likely labels of every sample: an eval forward under no_grad, the LOGITS ranked on the device in the
        order include/lamp_hip.h defines (lamp_topk_labels: larger first, the lower column on a tie) -- the sigmoid is monotone
        but saturates in fp32 and would turn distinct logits into index-ordered ties -- and the sigmoid applied to the (B, k)
        winners only.  -> (probs float32 (B, k), labels int64 (B, k)), labels being columns of the logit matrix.  Works on the
        fused and on the module-by-module route; there is no CPU path."""
        from . import metrics
        if not src[0].is_cuda:
            N.require_device(src[0])   # raises: HIP device only
        was_training = self.training
        if was_training:
            self.eval()
        try:
            with torch.no_grad(), torch.cuda.device(src[0].device):
                logits = self.forward(src, adj, None, None)[0]
                idx, val = metrics.topk_labels(logits, k, values=True)
                return torch.sigmoid(val), idx.long()
        finally:
            if was_training:
                self.train(True)

    def predict_labels(self, src, thresholds=0.5, adj=None):
        """The predicted label set of every sample: an eval forward under no_grad, then the rule of lamp_threshold_counts --
        sigmoid(logit), a NaN read as 0, >= threshold.  `thresholds` is a float for all labels or a tensor of length L (one per
        label, e.g. metrics.tune_thresholds(...)['threshold'] fitted on the validation split; +inf or NaN predicts nothing).
        -> bool (B, L).  Works on the fused and on the module-by-module route; there is no CPU path."""
        if not src[0].is_cuda:
            N.require_device(src[0])   # raises: HIP device only
        was_training = self.training
        if was_training:
            self.eval()
        try:
            with torch.no_grad(), torch.cuda.device(src[0].device):
                probs = torch.nan_to_num(torch.sigmoid(self.forward(src, adj, None, None)[0]), nan=0.0)
                if torch.is_tensor(thresholds):
                    thresholds = thresholds.detach().to(device=probs.device, dtype=torch.float32)
                    if thresholds.dim() != 1 or thresholds.numel() != probs.size(1):
                        raise ValueError('thresholds: expected a tensor of length %d, got shape %s' %
                                         (probs.size(1), tuple(thresholds.shape)))
                    return probs >= thresholds.unsqueeze(0)
                return probs >= torch.tensor(float(thresholds), dtype=torch.float32, device=probs.device)   # rounded as the C ABI's float
        finally:
            if was_training:
                self.train(True)

    # Upper bound on the scratch a forward may claim; larger batches are processed in micro-batches
    # inside lamp_forward.  8 GiB of 288 GB keeps even the 4096-label configuration at >= 64 samples.
    workspace_limit_bytes = 8 << 30
    # Hoist decoder layer 0's (weights-only) query projection out of the per-batch path.
    cache_layer0_query = True
    # Keep fragment-major copies of the decoder sub-chains' weight matrices (lamp_pack_weight) for the fused chain launch.
    use_chain_packs = True
    # Keep fragment-major copies of the encoder FFN matrices and of the decoder's query / label self-attention projections
    # (lamp_gemm_packs): the tile GEMM's one-wave-row tile reads its weight fragments straight from them.  Same bits; one extra copy
    # of each packed matrix in device memory.
    use_gemm_packs = True
    # ... and of the decoder's enc_attn K / V matrices (lamp_kv_gemm_pack): the K / V projection of the encoder rows, the largest
    # launch of a forward, on the tall packed tile.  Needs use_gemm_packs.  Same bits; 4 MiB more for reuters (2 layers, d 512).
    use_kv_gemm_packs = True
    # Fold encoder layer 0's first FFN matrix into the embedding tables (weights-only: Emb . W1^T and Pos . W1^T + b1, one
    # GEMM fewer per forward; results move in the last bits, a re-association).  False = the unfolded route.
    fold_embedding = True
    # Matmul precision of the fused eval forward's nn.Linear-class GEMMs: 'highest' (fp32 matrix pipe), 'high' (bf16x3: each fp32
    # product as three bf16 products of split operands -- torch.set_float32_matmul_precision('high') on a chip without TF32) or
    # 'bf16x6' (six products, fp32-class error).  The module-by-module route, nn.DataParallel replicas and model.train() stay
    # fp32.  Anything else raises ValueError when set on a model or used.
    matmul_precision = _MatmulPrecision()
    # Live encoder (enc_self_attn=True) on the packed token rows (csrc/attention_ragged.hip) instead of the padded layout.  Off:
    # it measured slower than the padded route on the ragged reuters batch, so it ships behind this switch.
    use_packed_live_encoder = False
    # Skip fully blocked 32x32 tiles of the label graph in the label->label attention.
    use_label_tiles = True
    # Compute only the allowed (query, key) pairs of a sparse, unstructured label graph (csrc/attention_sparse.hip; the
    # decoder flags such graphs, GraphDecoder.label_rows_sparse).  False = the dense tile kernels.
    use_sparse_label_attention = True
    # Read the label mask bit-packed (one 32-bit word per 32-key tile and row) instead of as bytes.
    use_mask_bits = True
