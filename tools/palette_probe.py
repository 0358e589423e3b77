"""Times the palette kernels (hg_palette_*, include/hg_post.h) on one GPU with HIP events, un-profiled: post.palette(k, iterations)
and post.color_transfer_palette on a 256 x 256 image and on an H x W synthetic photo (default 4096 x 6144), and the per-point
kernels on the photo from the stage entry points.  Rates are against the bytes each pass must move: 12 B in + 8 B out per pixel
for the quantisation, 8 B per pixel for the cells and for a Lloyd step, 12 B in + 12 or 3 B out for the transfer.  Prints one JSON
line at the end.

    python tools/palette_probe.py [--H 4096 --W 6144 --k 8 --iterations 16 --reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def photo(rng, H, W):
    """A smooth, textured (3, H, W) fp32 image in [0, 1]."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32) / np.float32(max(H, W))
    img = np.stack([0.5 + 0.4 * np.sin(9 * yy) * np.cos(7 * xx), 0.45 + 0.4 * np.cos(5 * xx + 1), 0.2 + 0.7 * yy * xx])
    return np.clip(img + rng.normal(0, 0.03, img.shape).astype(np.float32), 0, 1).astype(np.float32)


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
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--iterations', type=int, default=16)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('palette_probe: no GPU (a timing taken anywhere else says nothing)')
    from histogan_amd import post as P
    lib, dev = P.lib, torch.device('cuda', 0)
    rng = np.random.RandomState(0)
    rows = []

    def row(name, seconds, nbytes):
        rows.append(dict(name=name, ms=seconds * 1e3, mbytes=nbytes / 1e6, gbs=nbytes / seconds / 1e9))
        print(f'{name:64s} {seconds * 1e3:9.3f} ms  {nbytes / 1e6:9.1f} MB  {nbytes / seconds / 1e9:8.0f} GB/s', flush=True)

    for H, W in ((256, 256), (a.H, a.W)):
        n = H * W
        img = torch.from_numpy(photo(rng, H, W)).to(dev)
        hwc = img.permute(1, 2, 0).contiguous()
        tag = f'{H}x{W}'
        t = dev_time(lambda: P.palette(img, k=a.k, iterations=a.iterations), a.reps)
        row(f'palette(k={a.k}, iterations={a.iterations}), {tag}', t, n * (20 + 8 + 8 * (a.iterations + 1)))
        src, dst = P.paired_palette(img, img.flip(0), k=a.k, iterations=a.iterations)
        for q in (False, True):
            t = dev_time(lambda: P.color_transfer_palette(hwc, src, dst, quantize=q), a.reps)
            row(f'color_transfer_palette(K={a.k}) -> {"uint8" if q else "fp32"}, {tag}', t, n * (12 + (3 if q else 12)))
        one = P.Palette(src.rgb[:1], src.lab[:1], src.weight[:1]), P.Palette(dst.rgb[:1], dst.lab[:1], dst.weight[:1])
        t = dev_time(lambda: P.color_transfer_palette(hwc, *one, quantize=True), a.reps)
        row(f'color_transfer_palette(K=1) -> uint8, {tag}', t, n * 15)
        if n < 10 ** 6:
            continue
        # the per-point kernels on the photo, from the stage entry points
        st = P.raw_stream(dev)
        stride = lib.hg_palette_point_stride(n)
        pts = torch.empty((1, stride, 4), dtype=torch.int16, device=dev)
        cells = torch.zeros((1, 4096, 4), dtype=torch.int64, device=dev)
        centres = torch.round(src.lab * 128).to(torch.int32).reshape(1, a.k, 3).contiguous()
        sums = torch.zeros((1, a.k, 4), dtype=torch.int64, device=dev)
        x4 = img.unsqueeze(0)
        row(f'quantise, {tag}', dev_time(lambda: P.check(lib.hg_palette_quantize(x4.data_ptr(), *x4.stride(), None, 0, 0, 0, pts.data_ptr(),
                                                                                1, H, W, st), 'quantize'), a.reps), 20 * n)
        row(f'cells, {tag}', dev_time(lambda: P.check(lib.hg_palette_bins(pts.data_ptr(), 1, n, cells.data_ptr(), 0, st), 'bins'), a.reps), 8 * n)
        row(f'seeds (K={a.k})', dev_time(lambda: P.check(lib.hg_palette_seeds(cells.data_ptr(), 1, a.k, centres.data_ptr(), st), 'seeds'),
                                        a.reps), 4096 * 32)
        row(f'Lloyd step (K={a.k}), {tag}', dev_time(lambda: P.check(lib.hg_palette_step(pts.data_ptr(), pts.data_ptr(), 1, n, centres.data_ptr(), a.k,
                                                                                      sums.data_ptr(), None, 0, st), 'step'), a.reps), 8 * n)
    print(json.dumps(dict(k=a.k, iterations=a.iterations, rows=rows)))


if __name__ == '__main__':
    main()
