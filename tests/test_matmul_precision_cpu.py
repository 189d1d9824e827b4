"""LAMP.matmul_precision / LAMP_PREC_* / LAMP_FWD_MATMUL_* without a GPU: the ABI's three views agree, argument errors come back
as status codes before any launch, the Python attribute rejects unknown names, and no kernel of gemm_split.hip spills."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from lamp_amd import _native as N
from lamp_amd import build
from lamp_amd.Models import LAMP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -4


def test_new_symbols_and_constants_in_header_exports_and_ctypes_table():
    text = open(os.path.join(ROOT, 'include', 'lamp_hip.h')).read()
    for name, value in (('LAMP_PREC_FP32', 0), ('LAMP_PREC_BF16X3', 1), ('LAMP_PREC_BF16X6', 2), ('LAMP_FWD_MATMUL_BF16X3', 4),
                        ('LAMP_FWD_MATMUL_BF16X6', 8)):
        assert re.search(r'#define %s %d\b' % (name, value), text), name
        assert getattr(N, name) == value
    assert re.search(r'\bint lamp_linear_prec_fwd\s*\(', re.sub(r'/\*.*?\*/', '', text, flags=re.S))
    exported = subprocess.run(['nm', '-D', '--defined-only', N.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r' T lamp_linear_prec_fwd$', exported, flags=re.M)
    # lamp_linear_fwd's arguments with int32 precision in front of the stream
    restype, args = N.PROTOTYPES['lamp_linear_prec_fwd']
    base = N.PROTOTYPES['lamp_linear_fwd'][1]
    assert restype is ctypes.c_int and args == base[:-1] + [ctypes.c_int32] + base[-1:]
    assert N.lib().lamp_version() == N.ABI_VERSION == 5
    assert N.MATMUL_PRECISIONS == {'highest': (0, 0), 'high': (1, 4), 'bf16x6': (2, 8)}


def test_argument_errors_come_back_as_status_codes_without_a_gpu():
    lib = N.lib()
    # validation happens before any launch, so these are safe on a GPU-less host
    for bad in (3, -1, 6):
        assert lib.lamp_linear_prec_fwd(16, 4, 8, 8, 16, 4, 8, None, None, 0, 0, 16, 4, bad, None) == UNSUPPORTED
    for prec in (0, 1, 2):   # the precision is accepted, the shape checks of lamp_linear_fwd follow
        assert lib.lamp_linear_prec_fwd(None, 4, 8, 8, None, 4, 8, None, None, 0, 0, None, 4, prec, None) == -5
        assert lib.lamp_linear_prec_fwd(16, 4, 6, 6, 16, 4, 6, None, None, 0, 0, 16, 4, prec, None) == -2   # K % 4
        assert lib.lamp_linear_prec_fwd(16, 0, 8, 8, 16, 4, 8, None, None, 0, 0, 16, 4, prec, None) == -1
    # both matmul flags: refused in front of every other check of the forward, with otherwise valid-looking arguments
    h, d = 2, 64
    enc = (N.EncLayer * 2)(*[N.EncLayer(N.MhaWeights(16, 16, 16, 16, 16, 16, h, 1)) for _ in range(2)])
    dec = (N.DecLayer * 2)(*[N.DecLayer(N.MhaWeights(16, 16, 16, 16, 16, 16, h, 1), N.FfnWeights(),
                                        N.MhaWeights(16, 16, 16, 16, 16, 16, h, 1)) for _ in range(2)])
    m = N.Model(50, 51, 10, d, 2 * d, d // h, d // h, 2, 2, 0, 16, 16, 16, 16, 0, 0, 0, enc, dec)
    both = N.FwdOptions(0, N.LAMP_FWD_MATMUL_BF16X3 | N.LAMP_FWD_MATMUL_BF16X6, None, None)
    assert lib.lamp_forward_opts(ctypes.byref(m), ctypes.byref(both), 16, 16, 3, 12, 16, 16, None, 16, 1 << 30, None) == UNSUPPORTED
    fe = N.OnehotFrontend(16, 16, 16, 16, 16, 9, 16)
    m.n_src_vocab = 9
    assert lib.lamp_onehot_forward_opts(ctypes.byref(m), ctypes.byref(fe), ctypes.byref(both), 16, 16, 3, 12, 16, 16, None, 16,
                                        1 << 30, None) == UNSUPPORTED
    # the workspace functions return what they return without the flags
    for flag in (N.LAMP_FWD_MATMUL_BF16X3, N.LAMP_FWD_MATMUL_BF16X6):
        o = N.FwdOptions(0, flag, None, None)
        for mb in (1, 7):
            assert lib.lamp_forward_opts_workspace_bytes(ctypes.byref(m), ctypes.byref(o), mb, 12, 0) == \
                lib.lamp_forward_workspace_bytes(ctypes.byref(m), mb, 12, 0) > 0


def _tiny():
    return LAMP(50, 10, 16, 10, n_layers_enc=2, n_layers_dec=2, n_head=2, n_head2=2, d_word_vec=64, d_model=64, d_inner_hid=128,
                d_k=32, d_v=32, encoder='graph', decoder='graph', label_mask='none', dec_dropout2=False)


def test_unknown_precision_names_raise_value_error():
    assert LAMP.matmul_precision == 'highest'
    m = _tiny()
    for ok in ('high', 'bf16x6', 'highest'):
        m.matmul_precision = ok
        assert m.matmul_precision == ok
    for bad in ('medium', 'bf16', None, 3):
        with pytest.raises(ValueError):
            m.matmul_precision = bad
        with pytest.raises(ValueError):
            N.matmul_precision(bad)
    assert m.matmul_precision == 'highest' and LAMP.matmul_precision == 'highest'
    with pytest.raises(ValueError):   # the wrapper checks the name in front of the device
        N.linear(torch.zeros(2, 4), torch.zeros(4, 4), precision='medium')


def test_no_kernel_of_the_split_unit_uses_scratch():
    assert 'gemm_split.hip' in build.SOURCES
    rows = build.kernel_resources('gemm_split.hip', False)
    kernels = {k: r for k, r in rows.items() if 'gemm_split_kernel' in k}
    # three tiles x (two planes | three planes) x (16-byte, 16-byte + gathered residual, scalar epilogue)
    assert len(kernels) == 18, sorted(rows)
    for name, r in rows.items():
        assert r.get('scratch', 0) == 0, (name, r)
