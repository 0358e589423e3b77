"""Did the device code move?  Compares the -O3 assembly of hg_conv.hip, hg_hist.hip and hg_wino.hip of two trees
(profiles/conv_route_isa.json has the command and the result of the convolution host-side refactor):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S -I include histogan_amd/csrc/F.hip -o DIR/F.s     (each tree)
    python tools/conv_route_isa.py PARENT_DIR CHANGE_DIR

Whole file: sha256 without the __hip_cuid_ lines.  Per kernel: the text from its label to its .Lfunc_end plus its .amdhsa_kernel
descriptor, without assembler comments and with the function number taken out of local labels (that number is the kernel's
position in the file, so it moves when the order of instantiation does)."""
import hashlib
import json
import re
import sys


def load(path):
    lines = [ln for ln in open(path) if '__hip_cuid_' not in ln]
    text = ''.join(lines)
    norm = lambda ln: re.sub(r'\.(LBB|Lfunc_end|Lfunc_begin|LJTI|Ltmp)\d+', r'.\1N', re.sub(r'\s*;.*$', '', ln))
    names = set(re.findall(r'\.amdhsa_kernel (\S+)', text))
    desc = {m.group(1): m.group(2) for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', text, re.S)}
    body, cur = {}, None
    for ln in lines:
        m = re.match(r'^(_Z\w+):', ln)
        if m and cur is None and m.group(1) in names:
            cur = m.group(1)
            body[cur] = []
        if cur:
            body[cur].append(norm(ln))
            if ln.startswith('.Lfunc_end'):
                cur = None
    assert set(body) == names, 'a kernel without a body'
    return hashlib.sha256(text.encode()).hexdigest(), {k: hashlib.sha256((''.join(v) + desc[k]).encode()).hexdigest() for k, v in body.items()}


if __name__ == '__main__':
    res = {}
    for f in ('hg_conv', 'hg_hist', 'hg_wino'):
        (wp, kp), (wc, kc) = (load('%s/%s.s' % (d, f)) for d in sys.argv[1:3])
        res[f + '.hip'] = {'sha256_parent': wp, 'sha256_change': wc, 'whole_file_identical': wp == wc, 'kernels_parent': len(kp), 'kernels_change': len(kc),
                           'same_kernel_names': set(kp) == set(kc), 'kernels_with_identical_text': sum(kp[k] == kc.get(k) for k in kp),
                           'only_parent': sorted(set(kp) - set(kc)), 'only_change': sorted(set(kc) - set(kp)), 'differ': sorted(k for k in kp if k in kc and kp[k] != kc[k])}
    print(json.dumps(res, indent=1))
