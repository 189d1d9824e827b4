"""CPU: what the packed-W tile of the forward GEMM (csrc/gemm.hip, WPACK) owes its speed to, read from the compiler's output.

The instantiation's k loop is written as straight-line code so that hipcc's own wait counts stay exact: one conditional request
inside it and the loop is back to `s_waitcnt vmcnt(0)` in front of every LDS store, i.e. to a prefetch distance of one k-step
(profiles/gemm_packed_w_ab.txt: that form measured slower than the staged kernel).  Nothing on the GPU fails when that
happens -- the bits stay right -- so the ISA is checked here."""
import ctypes
import os
import re
import sys

from conftest import ROOT

from lamp_amd import build as B

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import count_loop_valu as CLV  # noqa: E402

PACKED = ('lamp::gemm_nt_kernel<32, 64, 32, 1, 4, false, 16, true, true, false, true>',
          'lamp::gemm_nt_kernel<32, 64, 32, 1, 4, false, 16, true, true, true, true>')   # ... with the gathered residual


def test_packed_k_loop_is_straight_line_with_counted_waits():
    asm = CLV.device_asm(os.path.join(ROOT, 'lamp_amd', 'csrc', 'gemm.hip'))
    found = {n.split('(')[0].replace('void ', ''): l for n, l in CLV.kernels(asm).items() if 'gemm_nt_kernel<' in n}
    for name in PACKED:
        lines = found[name]
        first, last, count = CLV.mfma_loops(lines)[0]
        body = lines[first:last + 1]
        # two k-steps per trip: 2 steps x 2 chunks x 2 row blocks x 4 MFMAs; no vector-ALU instruction among them
        assert count['mfma'] == 32 and count['valu'] == 0 and count['trans'] == 0, (name, dict(count))
        # the only branch is the back edge; three requests and one LDS store per step
        assert sum(bool(re.match(r'\s*s_c?branch', l)) for l in body) == 1, name
        assert sum('buffer_load_dwordx4' in l for l in body) == 6 and sum('ds_write_b128' in l for l in body) == 2, name
        # and no wait in the loop drains the vector-memory queue: every one leaves at least three requests in flight
        waits = [int(m.group(1)) for l in body for m in [re.search(r's_waitcnt.*vmcnt\((\d+)\)', l)] if m]
        assert waits and min(waits) >= 3, (name, waits)


def test_packed_instantiations_keep_five_workgroups_per_cu():
    """Registers leave room for more (no scratch, no AGPR parking); the launch's LDS request is what holds five."""
    res = B.kernel_resources('gemm.hip')
    for name in PACKED:
        r = res[name]
        assert r['scratch'] == 0 and r.get('agpr', 0) == 0 and r['vgpr'] <= 96 and r['occupancy'] >= 5, (name, r)


def test_the_packs_ride_beside_the_model():
    """No struct of the ABI changed: the packs have their own (lamp_gemm_packs) and their own entry points."""
    from lamp_amd import _native as N
    assert ctypes.sizeof(N.GemmPacks) == 16 and ctypes.sizeof(N.EncGemmPack) == 16 and ctypes.sizeof(N.DecGemmPack) == 32
    lib = N.lib()
    for name in N.LATE_ENTRY_POINTS:
        assert name in N.PROTOTYPES and getattr(lib, name).argtypes == N.PROTOTYPES[name][1]
    from lamp_amd.Models import LAMP
    assert LAMP.use_gemm_packs is True
