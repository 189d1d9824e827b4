#!/usr/bin/env python3
"""Machine-code comparison of one translation unit between a git revision and the working tree: the check a refactor of the
hand-scheduled kernels (chain.hip: inline-assembly loads, hand-counted waits) has to pass -- "the tests pass" does not show
that no wait, load or MFMA moved.

    python tools/chain_isa_diff.py [REV] [--unit lamp_amd/csrc/chain.hip] [-DLAMP_TUNING ...]     exit 1 on a difference

Both sides are compiled as lamp_amd/isa_guard.py: device_asm does (hipcc --offload-arch=gfx950 -O3 -std=c++17 -S
--cuda-device-only, plus -Rpass-analysis=kernel-resource-usage).  Per kernel of the REVISION (default HEAD) the instruction
stream between the symbol's label and its last s_endpgm is compared: comments, blank lines and directives dropped, local
labels (.LBBn_m) renamed by order of appearance; and the lines of the resource report (registers, scratch, occupancy, LDS).
Kernels only one side has are listed, not failed on the working tree's side (a refactor may retire instantiations).
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get('HIPCC') or '/opt/rocm/bin/hipcc'
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
REPORT_KEYS = ('SGPRs', 'VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy', 'SGPRs Spill', 'VGPRs Spill', 'LDS Size', 'Dynamic Stack')


def compile_unit(path, flags):
    with tempfile.NamedTemporaryFile(suffix='.s') as f:
        r = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                            '-Rpass-analysis=kernel-resource-usage', '-o', f.name, path, *flags], capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr[-4000:])
        return open(f.name).read(), r.stderr


def demangle(names):
    out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return dict(zip(names, out))


def kernels_of(asm):
    """-> {mangled name: [normalised instruction lines]}"""
    out, cur, labels = {}, None, {}
    for line in asm.split('\n'):
        m = re.match(r'^(_Z\w+):', line)
        if m:
            cur, labels = [], {}
            out[m.group(1)] = cur
            continue
        if cur is None:
            continue
        t = line.split(';')[0].strip()
        if t.startswith('.Lfunc_end'):
            while cur and not cur[-1].startswith('s_endpgm'):
                cur.pop()
            cur = None
            continue
        if not t or (t.startswith('.') and not re.match(r'^\.LBB\d+_\d+:', t)):
            continue
        t = re.sub(r'\.LBB\d+_\d+', lambda k: labels.setdefault(k.group(0), 'L%d' % len(labels)), t)
        cur.append(re.sub(r'\s+', ' ', t))
    return out


def reports_of(stderr):
    """-> {mangled name: [report lines]}"""
    out, cur = {}, None
    for line in stderr.split('\n'):
        m = re.search(r'remark: (?:[^:]*:\d+:\d+: )?(.*)$', line)
        text = m.group(1).strip() if m else line.strip()
        m = re.search(r'Function Name: (\S+)', text)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and any(k in text for k in REPORT_KEYS):
            cur.append(re.sub(r'^.*?remark:\s*', '', text))
    return out


def show(a, b, limit=40):
    d = [l for l in difflib.unified_diff(a, b, 'revision', 'working tree', lineterm='', n=2)]
    for l in d[:limit]:
        print('      ' + l)
    if len(d) > limit:
        print('      ... %d more diff lines' % (len(d) - limit))


def main():
    args = sys.argv[1:]
    unit = 'lamp_amd/csrc/chain.hip'
    if '--unit' in args:
        unit = args[args.index('--unit') + 1]
        del args[args.index('--unit'):args.index('--unit') + 2]
    flags = [a for a in args if a.startswith('-')]
    rev = ([a for a in args if not a.startswith('-')] or ['HEAD'])[0]
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(['git', '-C', ROOT, 'archive', rev, 'lamp_amd/csrc', 'include'], capture_output=True, check=True).stdout
        subprocess.run(['tar', '-x', '-C', tmp], input=tar, check=True)
        with ThreadPoolExecutor(2) as pool:   # the two compilations side by side
            jobs = [pool.submit(compile_unit, os.path.join(d, unit), flags) for d in (tmp, ROOT)]
            (old_asm, old_err), (new_asm, new_err) = [j.result() for j in jobs]
    old, new, old_r, new_r = kernels_of(old_asm), kernels_of(new_asm), reports_of(old_err), reports_of(new_err)
    pretty = demangle(sorted(set(old) | set(new)))
    same = differ = 0
    for k in sorted(old, key=lambda k: pretty[k]):
        if k not in new:
            print('retired    %s' % pretty[k])
            continue
        ok_r = old_r.get(k) == new_r.get(k) and old_r.get(k)
        ok = old[k] == new[k]
        what = '%d instructions' % len(old[k])
        same += bool(ok and ok_r)
        differ += not (ok and ok_r)
        print('%s  %s  (%s; report %s)' % ('identical' if ok else 'DIFFERENT', pretty[k], what, 'identical' if ok_r else 'DIFFERENT'))
        if not ok_r:
            show(old_r.get(k) or [], new_r.get(k) or [])
        if not ok:
            show(old[k], new[k])
    for k in sorted(set(new) - set(old), key=lambda k: pretty[k]):
        print('new        %s' % pretty[k])
    print('%d kernels identical, %d different, %d retired, %d new' % (same, differ, len(set(old) - set(new)), len(set(new) - set(old))))
    sys.exit(1 if differ else 0)


if __name__ == '__main__':
    main()
