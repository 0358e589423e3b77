"""Times the 3D LUT kernels (hg_lut_*, include/hg_lut.h) on one GPU with HIP events, un-profiled: post.lut_apply on an H x W
synthetic photo (default 4096 x 6144) -- fp32 -> fp32, fp32 -> uint8 and uint8 -> uint8, N = 17 and 33, both interpolations --
and post.lut_fit on a 256 x 256 pair with its splat and its solve timed separately.  Rates are against the bytes each pass must
move: 12 or 3 B in and 12 or 3 B out per pixel for the apply, 24 B per pixel for the splat; the solve moves no image and is
reported in ms alone.  Prints one JSON line at the end and, with --out, writes it to a file.

    python tools/lut_probe.py [--H 4096 --W 6144 --reps 10 --out profiles/lut_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def photo(rng, H, W):
    """A smooth, textured (H, W, 3) fp32 image in [0, 1]."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32) / np.float32(max(H, W))
    img = np.stack([0.5 + 0.4 * np.sin(9 * yy) * np.cos(7 * xx), 0.45 + 0.4 * np.cos(5 * xx + 1), 0.2 + 0.7 * yy * xx], axis=-1)
    return np.clip(img + rng.normal(0, 0.03, img.shape).astype(np.float32), 0, 1).astype(np.float32)


def graded(x):
    """A smooth, non-affine recolouring of an (H, W, 3) image: what a fit is given as its target."""
    y = x ** torch.tensor([0.8, 1.1, 1.35], device=x.device)
    return y @ torch.tensor([[0.90, 0.10, 0.00], [0.05, 0.85, 0.10], [0.00, 0.15, 0.85]], device=x.device).t()


def dev_time(fn, reps):
    """Mean seconds of fn() over reps calls, HIP events, after two warm-up calls."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--H', type=int, default=4096)
    ap.add_argument('--W', type=int, default=6144)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lut_probe: no GPU (a timing taken anywhere else says nothing)')
    from histogan_amd import post as P
    dev = torch.device('cuda', 0)
    rng = np.random.RandomState(0)
    rows = []

    def row(name, seconds, nbytes=None):
        rows.append(dict(name=name, ms=seconds * 1e3, mbytes=None if nbytes is None else nbytes / 1e6,
                         gbs=None if nbytes is None else nbytes / seconds / 1e9))
        rate = '' if nbytes is None else f'  {nbytes / 1e6:9.1f} MB  {nbytes / seconds / 1e9:8.0f} GB/s'
        print(f'{name:64s} {seconds * 1e3:9.3f} ms{rate}', flush=True)

    # the fit, at the size ReHistoGAN works at
    small = torch.from_numpy(photo(rng, 256, 256)).to(dev)
    target = graded(small)
    luts = {}
    for n in (17, 33):
        luts[n] = P.lut_fit(small, target, n=n)
        sums = P.lut_splat(small, target, n=n)
        row(f'lut_fit(n={n}), 256x256', dev_time(lambda: P.lut_fit(small, target, n=n), a.reps))
        row(f'  splat, N={n}', dev_time(lambda: P.lut_splat(small, target, n=n, sums=sums), a.reps), 256 * 256 * 24)
        for sweeps in (P.LUT_SWEEPS, 2 * P.LUT_SWEEPS):
            t = dev_time(lambda: P.lut_solve(sums, iterations=sweeps), a.reps)
            row(f'  solve, N={n}, {sweeps} sweeps ({t / sweeps * 1e6:.2f} us per sweep)', t)
    # the apply, on the photo
    H, W = a.H, a.W
    n_pix = H * W
    img = torch.from_numpy(photo(rng, H, W)).to(dev)
    img_u8 = (img * 255).to(torch.uint8)
    for n in (17, 33):
        for interpolation in ('tetrahedral', 'trilinear'):
            for src, q, name, nbytes in ((img, False, 'fp32 -> fp32', 24), (img, True, 'fp32 -> uint8', 15), (img_u8, True, 'uint8 -> uint8', 6)):
                t = dev_time(lambda: P.lut_apply(src, luts[n], interpolation, quantize=q), a.reps)
                row(f'lut_apply N={n} {interpolation} {name}, {H}x{W}', t, n_pix * nbytes)
    record = dict(H=H, W=W, reps=a.reps, lambda_smooth=P.LUT_LAMBDA, sweeps=P.LUT_SWEEPS, device=torch.cuda.get_device_name(0), rows=rows)
    line = json.dumps(record)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(record, indent=1) + '\n')


if __name__ == '__main__':
    main()
