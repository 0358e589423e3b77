#!/usr/bin/env python3
"""Device time of bilateral guided upsampling (hg_bgu_normal, hg_bgu_slice, histogan_amd/post.py) at the sizes a user runs.

    python tools/bgu_probe.py [--H 4000 --W 6000 --low 256 --reps 20]

A seeded synthetic uint8 photo (H x W) and a low x low recoloured image.  From HIP events, one pair per call after three
warm-up calls, reported as min / median over --reps: the normal-equation kernels alone, the whole fit (normal
equations, smoothness terms, block-tridiagonal Cholesky), the slice to uint8 with its fraction of the 8 TB/s HBM peak on
6 bytes per pixel (3 read, 3 written), and, for comparison, pyramid_upsampling at the same photo size.  The calls that
read the photo rotate over enough copies of it to exceed the 256 MB last-level cache, so no call finds its input there;
outputs are fresh allocations.  Prints one JSON line at the end.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8.0e12


LLC = 256 << 20


def dev_time(fn, reps):
    """(min, median) seconds of fn(k), k the call number, each call between its own pair of events."""
    for k in range(3):
        fn(k)
    torch.cuda.synchronize()
    ts = []
    for k in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(3 + k)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.min(ts)), float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--H', type=int, default=4000)
    ap.add_argument('--W', type=int, default=6000)
    ap.add_argument('--low', type=int, default=256)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    from histogan_amd import build
    build.build()
    from histogan_amd import post as P
    if not torch.cuda.is_available():
        raise SystemExit('bgu_probe: no GPU; nothing is measured')
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(a.H) / a.H, torch.arange(a.W) / a.W, indexing='ij')
    ph = torch.stack([0.5 + 0.3 * torch.sin(6.28 * (k + 1.3) * yy) * torch.cos(6.28 * (2.1 - 0.4 * k) * xx)
                      for k in range(3)], -1) + 0.05 * torch.randn(a.H, a.W, 3, generator=g)
    ph = (ph.clamp(0, 1) * 255).round().to(torch.uint8).to(dev)
    in_ds = P.imresize(P.u8_hwc_to_float(ph), output_shape=(a.low, a.low))
    out_ds = (in_ds.clamp(0, 1) ** 0.8 * 0.9 + 0.05).contiguous()
    gamma = P.bgu_fit(in_ds, out_ds)
    copies = LLC // ph.numel() + 2
    phs = [ph] + [ph.clone() for _ in range(copies - 1)]
    res = dict(H=a.H, W=a.W, low=a.low, grid=list(gamma.shape[:3]), photo_copies=copies)

    def put(name, fn, reps):
        lo, med = dev_time(fn, reps)
        res[name + '_ms_min'], res[name + '_ms_median'] = lo * 1e3, med * 1e3
        return lo, med
    put('normal', lambda k: P.bgu_normal(in_ds, out_ds), a.reps)
    put('fit', lambda k: P.bgu_fit(in_ds, out_ds), max(5, a.reps // 2))
    lo, med = put('slice', lambda k: P.bgu_slice(gamma, phs[k % copies]), a.reps)
    res['slice_frac_hbm_peak_min'], res['slice_frac_hbm_peak_median'] = (6.0 * a.H * a.W / t / HBM for t in (lo, med))
    put('bgu_upsampling', lambda k: P.bgu_upsampling(out_ds, phs[k % copies], quantize=True), max(5, a.reps // 2))
    put('pyramid_upsampling', lambda k: P.float_to_u8_hwc(P.pyramid_upsampling(out_ds, phs[k % copies])[0]),
        max(5, a.reps // 2))
    for k, v in res.items():
        print(f'{k:<24s} {v}')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
