#!/usr/bin/env python3
"""What does the fused sRGB -> Lab projection cost?  HIP events, un-profiled, one process, alternating rounds.

    python tools/lab_probe.py OUT.json [rounds] [iterations per round]

At 32 x 3 x 256 x 256, h = 64, inverse-quadratic, module defaults otherwise (insz = 150, bilinear), forward + backward:
  (a) LabHistBlock(from_rgb=True)(x)                       the conversion inside the histogram kernels, 150 x 150 pixels / image
  (b) LabHistBlock()(lab), lab converted beforehand        the `direct` projection, the kernels as they were
  (c) post.srgb_to_lab(x) alone                            the stand-alone conversion of the 256 x 256 input
The expectation is (a) <= (b) + (c); the spread of (b) over the rounds is the noise measure."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main(out_path, rounds=7, iters=20):
    from histogan_amd import post
    from histogram_classes.LabHistBlock import LabHistBlock
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(32, 3, 256, 256, generator=gen).to(dev)
    go = torch.rand(32, 1, 64, 64, generator=gen).to(dev)
    lab = post.srgb_to_lab(x)
    fused, direct = LabHistBlock(h=64, from_rgb=True), LabHistBlock(h=64)

    def fwd_bwd(block, inp):
        t = inp.detach().requires_grad_(True)
        block(t).backward(go)

    work = {'a_from_rgb_fwd_bwd': lambda: fwd_bwd(fused, x), 'b_direct_fwd_bwd': lambda: fwd_bwd(direct, lab),
            'c_srgb_to_lab': lambda: post.srgb_to_lab(x)}
    for f in work.values():                       # warm-up: module load, allocator, clocks
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in work}
    for _ in range(rounds):
        for k, f in work.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / iters)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    spread_b = max(ms['b_direct_fwd_bwd']) - min(ms['b_direct_fwd_bwd'])
    excess = med['a_from_rgb_fwd_bwd'] - (med['b_direct_fwd_bwd'] + med['c_srgb_to_lab'])
    res = {'shape': '32x3x256x256, h=64, inverse-quadratic, insz=150 bilinear, forward + backward', 'device': torch.cuda.get_device_name(0),
           'rounds': rounds, 'iterations_per_round': iters, 'ms_per_call_by_round': ms, 'median_ms': med,
           'spread_of_b_ms': spread_b, 'a_minus_b_plus_c_ms': excess, 'a_within_b_plus_c': excess <= spread_b}
    json.dump(res, open(out_path, 'w'), indent=1)
    print(json.dumps({k: res[k] for k in ('median_ms', 'spread_of_b_ms', 'a_minus_b_plus_c_ms', 'a_within_b_plus_c')}))


if __name__ == '__main__':
    main(sys.argv[1], *(int(a) for a in sys.argv[2:4]))
