"""CPU: the ctypes mirrors of the weight-pack structs against include/lamp_hip.h, and the registers of the tall packed tiles
(csrc/gemm.hip: 64x64x32, one wave row) as the compiler reports them for the product build."""
import ctypes
import os
import re

from conftest import ROOT


def test_pack_structs_mirror_the_header():
    """Every pack struct of include/lamp_hip.h holds pointers only: member i sits at 8 i.  The ctypes mirrors must have the same
    members in the same order at those offsets, and the same size."""
    from lamp_amd import _native as N
    with open(os.path.join(ROOT, 'include', 'lamp_hip.h')) as f:
        header = f.read()
    for cname, mirror in (('lamp_dec_gemm_pack', N.DecGemmPack), ('lamp_enc_gemm_pack', N.EncGemmPack), ('lamp_gemm_packs', N.GemmPacks),
                          ('lamp_kv_gemm_pack', N.KvGemmPack)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), header, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        decls = [d.strip() for d in body.split(';') if d.strip()]
        assert decls and all('*' in d for d in decls), (cname, decls)
        names = [re.search(r'(\w+)$', d).group(1) for d in decls]
        assert [n for n, _ in mirror._fields_] == names, cname
        assert ctypes.sizeof(mirror) == 8 * len(names), cname
        for i, n in enumerate(names):
            assert getattr(mirror, n).offset == 8 * i and getattr(mirror, n).size == 8, (cname, n)
    assert 'lamp_forward_packs_kv' in N.PROTOTYPES and 'lamp_forward_packs_kv' in N.LATE_ENTRY_POINTS
    assert N.PROTOTYPES['lamp_forward_packs_kv'][1][3] == ctypes.POINTER(N.KvGemmPack)


def test_tall_packed_instantiations_keep_five_waves_per_simd():
    """64x64x32 with one wave row: 16 accumulators, two A sets, two W fragment sets and the prefetched epilogue operands within 96
    registers, no scratch -- five workgroups per CU, the residency its tile rule counts rounds with (launch_gemm)."""
    from lamp_amd import build as B
    for tuning, gathered in ((False, 'false'), (True, 'false'), (True, 'true')):   # the gathered one: tuning build only (forced tile 19)
        r = B.kernel_resources('gemm.hip', tuning)['lamp::gemm_nt_kernel<64, 64, 32, 1, 4, false, 16, true, true, %s, true>' % gathered]
        assert r['scratch'] == 0 and r.get('agpr', 0) == 0 and r['vgpr'] <= 96 and r['occupancy'] >= 5, (tuning, gathered, r)
