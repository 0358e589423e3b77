"""Times regrain (hg_regrain_*, include/hg_regrain.h; post.regrain) on one GPU with HIP events, un-profiled, at 3000 x 4000 and
256 x 256: the whole call with one sweep per launch (fused = 1) and with the plan (fused = 0), alternating; then per level the
stages -- begin, the resizes, the coefficients, the level's n sweeps at fused = 1, 2, 4 and 8, finish -- and the same sweeps
written in torch operations on the same planes, the comparison point (the project had no regrain before).  Every figure is the
median of --reps timed calls after two warm-up calls.  The sweep's rate is against the bytes one sweep per launch must move,
52 B per pixel and sweep (D in and out and E for three channels, four coefficient planes), and the 8 TB/s HBM peak the other
probes use; a fused launch moves fewer, so its "rate" on the same bytes is a speed-up figure, not a bandwidth.  Prints one JSON
line at the end and, with --out, writes it to a file.

    python tools/regrain_probe.py [--sizes 3000x4000,256x256 --reps 7 --out profiles/regrain.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8e12
SWEEP_BYTES = 52


def pair(rng, H, W):
    """(original, transferred), (H, W, 3) fp32 in [0, 1]: a smooth textured photo with an edge, and an affine colour map of it
    quantised to 24 levels plus grain."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32) / np.float32(max(H, W))
    img = np.stack([0.5 + 0.4 * np.sin(9 * yy) * np.cos(7 * xx), 0.45 + 0.4 * np.cos(5 * xx + 1), 0.2 + 0.7 * yy * xx], axis=-1)
    img[H // 4:H // 2, W // 3:2 * W // 3] *= 0.5
    img = np.clip(img + rng.normal(0, 0.01, img.shape).astype(np.float32), 0, 1).astype(np.float32)
    t = img @ np.array([[0.8, 0.15, 0.0], [0.05, 0.7, 0.2], [0.1, 0.0, 0.85]], dtype=np.float32).T + np.float32(0.05)
    t = np.round(t * 24) / 24 + rng.normal(0, 0.01, t.shape)
    return img, np.clip(t, 0, 1).astype(np.float32)


def dev_time(fn, reps):
    """Median seconds of fn() over reps separately timed calls, HIP events, after two warm-up calls."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) / 1e3)
    return float(np.median(times))


def torch_sweeps(D, E, C, n, rho):
    """n sweeps of the definition in torch operations (each a launch or several over the planes)."""
    psi, wr, wd, s = C
    for _ in range(n):
        a = psi * E
        a[:, :, :-1] += wr[:, :-1] * D[:, :, 1:]
        a[:, :, 1:] += wr[:, :-1] * D[:, :, :-1]
        a[:, :-1, :] += wd[:-1, :] * D[:, 1:, :]
        a[:, 1:, :] += wd[:-1, :] * D[:, :-1, :]
        D = s * a + rho * D
    return D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='3000x4000,256x256')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('regrain_probe: no GPU (a timing taken anywhere else says nothing)')
    from histogan_amd import post as P
    lib = P.lib
    dev = torch.device('cuda', 0)
    st = P.raw_stream(dev)
    rng = np.random.RandomState(0)
    rows = []

    def row(name, seconds, **extra):
        rows.append(dict(name=name, ms=seconds * 1e3, **extra))
        print(f'{name:72s} {seconds * 1e3:10.3f} ms  ' + '  '.join(f'{k} {v:.3g}' if isinstance(v, float) else f'{k} {v}'
                                                                    for k, v in extra.items()), flush=True)

    for size in a.sizes.split(','):
        H, W = (int(v) for v in size.split('x'))
        o, t = (torch.from_numpy(v).to(dev) for v in pair(rng, H, W))
        sizes = P.regrain_levels(H, W)
        its = P.REGRAIN_ITERATIONS
        base = P.regrain(o, t, fused=1)
        assert torch.equal(P.regrain(o, t, fused=0), base)
        # the whole call, the two settings alternating
        whole = {1: [], 0: []}
        for _ in range(3):
            for f in (1, 0):
                whole[f].append(dev_time(lambda: P.regrain(o, t, fused=f), a.reps))
        for f in (1, 0):
            row(f'regrain {H}x{W}, {len(sizes)} levels, fused={f}', float(np.median(whole[f])), runs_ms=[round(v * 1e3, 3) for v in whole[f]])
        # the stages, level by level, on the planes the call itself works on
        lv = P._regrain_carve(torch.empty(lib.hg_regrain_workspace_bytes(H, W, len(sizes)) // 4, dtype=torch.float32, device=dev), sizes)
        src, _, ps, cs = P._pixels(o, 'original', 'regrain')
        tgt, _, pt, ct = P._pixels(t, 'transferred', 'regrain')
        begin = lambda: P.check(lib.hg_regrain_begin(src.data_ptr(), ps, cs, tgt.data_ptr(), pt, ct, H, W, lv[0]['I'].data_ptr(),  # noqa: E731
                                                     lv[0]['E'].data_ptr(), st), 'begin')
        row(f'  begin {H}x{W}', dev_time(begin, a.reps))
        for l, (h, w) in enumerate(sizes):
            v = lv[l]
            if l:
                row(f'  level {l} {h}x{w}: resize of I and E from level {l - 1}',
                    dev_time(lambda: (P._resize_planes_into(lv[l - 1]['I'], v['I']), P._resize_planes_into(lv[l - 1]['E'], v['E'])), a.reps))
            coef = lambda: P.check(lib.hg_regrain_coef(v['I'].data_ptr(), h, w, l, 1.0, v['coef'].data_ptr(),  # noqa: E731
                                                       v['scratch'].data_ptr(), st), 'coef')
            row(f'  level {l} {h}x{w}: coef', dev_time(coef, a.reps))
        for l, (h, w) in enumerate(sizes):
            v, n = lv[l], its[l]
            v['a'].copy_(v['E'])
            nbytes = SWEEP_BYTES * h * w * n
            for f in (1, 2, 4, 8, 1, 2, 4, 8):       # every setting twice, alternating: the spread
                s = dev_time(lambda: P.regrain_sweep(v['a'], v['b'], v['E'], v['coef'], n, f), a.reps)
                row(f'  level {l} {h}x{w}: {n} sweeps, fused={f}', s, us_per_sweep=s / n * 1e6, tbs_on_unfused_bytes=nbytes / s / 1e12,
                    share_of_hbm_peak=nbytes / s / HBM_PEAK, plan=lib.hg_regrain_plan_fused(h, w, n))
            C = tuple(v['coef'])
            s = dev_time(lambda: torch_sweeps(v['a'], v['E'], C, n, P.REGRAIN_RHO), max(3, a.reps // 2))
            row(f'  level {l} {h}x{w}: {n} sweeps in torch operations', s, us_per_sweep=s / n * 1e6)
            if l:
                row(f'  level {l} {h}x{w}: resize of D to level {l - 1}', dev_time(lambda: P._resize_planes_into(v['a'], lv[l - 1]['a']), a.reps))
        out = torch.empty(H, W, 3, device=dev)
        row(f'  finish {H}x{W}', dev_time(lambda: P.check(lib.hg_regrain_finish(lv[0]['I'].data_ptr(), lv[0]['a'].data_ptr(), H, W,
                                                                                out.data_ptr(), 0, st), 'finish'), a.reps))
    record = dict(sizes=a.sizes, reps=a.reps, iterations=list(P.REGRAIN_ITERATIONS), min_side=P.REGRAIN_MIN_SIDE,
                  tile=[lib.hg_regrain_tile_h(), lib.hg_regrain_tile_w()], device=torch.cuda.get_device_name(0), rows=rows)
    print(json.dumps(record))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(record, indent=1) + '\n')


if __name__ == '__main__':
    main()
