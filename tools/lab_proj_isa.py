#!/usr/bin/env python3
"""Did adding the HG_PROJ_LAB instantiations leave the existing histogram kernels alone?  No GPU needed.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S -I include histogan_amd/csrc/hg_hist.hip -o X.s
        once in a checkout of the parent (parent.s) and once in the change (change.s), and in the change
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Rpass-analysis=kernel-resource-usage -I include \
        -c histogan_amd/csrc/hg_hist.hip -o /dev/null 2> res.txt
    python tools/lab_proj_isa.py parent.s change.s res.txt PARENT_COMMIT profiles/lab_proj_isa.json

Every kernel's assembly (its function body, kernel descriptor and resource symbols) is hashed with its own symbol name and
the function ordinal of its local labels replaced by placeholders -- a defaulted template parameter changes the mangled name
and new instantiations change the order, nothing else may differ.  Every parent kernel must have a change kernel with the
same hash; the rest of the change's kernels are the additions, listed with the compiler's resource remarks."""
import collections
import hashlib
import json
import re
import subprocess
import sys


def kernels(path):
    lines = open(path).read().split('\n')
    names = [m.group(1) for ln in lines if (m := re.match(r'\t\.amdhsa_kernel (\S+)', ln))]
    start = {m.group(1): i for i, ln in enumerate(lines) if (m := re.match(r'\t\.globl\t(\S+)', ln))}
    out = {}
    for name in names:
        i = start[name]
        tail = f'\t.set {name}.has_indirect_call'
        j = next(k for k in range(i, len(lines)) if lines[k].startswith(tail))
        body = '\n'.join(ln for ln in lines[i:j + 1] if '__hip_cuid_' not in ln).replace(name, 'K')
        body = re.sub(r'\.L(func_begin|func_end|tmp|JTI)\d+', r'.L\1', body)
        body = re.sub(r'BB\d+_(\d+)', r'BB_\1', body)          # labels (.LBB12_3) and the loop comments that name them (BB12_3)
        body = re.sub(r'[ \t]+;', ' ;', body)                  # comments are padded to a column that moves with the label's width
        out[name] = hashlib.sha256(body.encode()).hexdigest()
    return out


def demangle(names):
    dem = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return {n: d.replace('(anonymous namespace)::', '').replace('void ', '') for n, d in zip(names, dem)}


def resources(path):
    blocks = re.split(r'remark: [^\n]*Function Name: ', open(path).read())[1:]
    res = {}
    for b in blocks:
        g = lambda k: int(m.group(1)) if (m := re.search(k + r': (\d+)', b)) else -1   # noqa: E731
        res[b.split('\n')[0].split()[0]] = {'vgpr': g('VGPRs'), 'agpr': g('AGPRs'), 'sgpr': g('SGPRs'),
                                            'scratch_bytes_per_lane': g(r'ScratchSize \[bytes/lane\]'),
                                            'occupancy_waves_per_simd': g(r'Occupancy \[waves/SIMD\]'),
                                            'lds_bytes_per_block': g(r'LDS Size \[bytes/block\]')}
    return res


def main(parent_s, change_s, res_txt, parent_commit, out_path):
    kp, kc = kernels(parent_s), kernels(change_s)
    pool = collections.Counter(kc.values())
    missing = []
    for name, h in kp.items():
        if pool[h] > 0:
            pool[h] -= 1
        else:
            missing.append(name)
    parent_hashes = collections.Counter(kp.values())
    new = []
    for name, h in kc.items():
        if parent_hashes[h] > 0:
            parent_hashes[h] -= 1
        else:
            new.append(name)
    dem, res = demangle(list(kc) + missing), resources(res_txt)
    table = {dem[n]: res.get(n, {}) for n in sorted(new, key=lambda n: dem[n])}
    with_scratch = [k for k, v in table.items() if v.get('scratch_bytes_per_lane', -1) != 0]
    json.dump({
        'command': 'hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S -I include '
                   'histogan_amd/csrc/hg_hist.hip -o hg_hist.s (parent and change); resources: -Rpass-analysis=kernel-resource-usage',
        'normalisation': "per kernel: .globl line through its last .set resource symbol; lines containing __hip_cuid_ dropped; the kernel's "
                         'own symbol name and the function ordinal of the BBn_m / .Lfunc / .Ltmp / .LJTI labels (and of the comments naming them) replaced by placeholders; blanks in front of a comment collapsed',
        'parent': parent_commit,
        'kernels_parent': len(kp), 'kernels_change': len(kc),
        'parent_kernels_with_an_identical_change_kernel': len(kp) - len(missing),
        'parent_kernels_without': [dem[n] for n in missing],
        'new_kernels': len(new), 'new_kernels_with_scratch': with_scratch,
        'new_kernel_resources': table,
        'verdict': ('every kernel of the parent object is in the new object with the same normalised assembly; '
                    f'{len(new)} kernels are additions, ' + ('none uses scratch' if not with_scratch else f'{len(with_scratch)} use scratch'))
                   if not missing else f'{len(missing)} parent kernels changed',
    }, open(out_path, 'w'), indent=1)
    print(f'parent {len(kp)} kernels, change {len(kc)}; identical {len(kp) - len(missing)}; new {len(new)}; with scratch {len(with_scratch)}')
    return 1 if missing or with_scratch else 0


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:6]))
