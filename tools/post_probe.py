#!/usr/bin/env python3
"""Device time of the full-resolution post-processing (include/hg_post.h, histogan_amd/post.py) at a phone-photo size.

    python tools/post_probe.py [--H 3024 --W 4032 --levels 6 --reps 20] [--cpu-ref]

A seeded synthetic uint8 photo (H x W) and a 256x256 generated image.  Per stage: device time from HIP events after
warm-up (mean over --reps), the algorithmic bytes counted from the shapes (every input element read once, every output
element written once), and the achieved fraction of the 8 TB/s HBM peak.  Then the whole pyramid_upsampling and
color_transfer_mkl calls as evaluate runs them, from the H2D upload of the photo to the uint8 array the writer gets
(host clock around synchronised work).  --cpu-ref also times tests/post_ref.py, the fp64 numpy restatement, on this
host's CPU for the same two calls.  The `idt` rows time the iterative distribution transfer (hg_idt_*): each per-pixel
kernel on the photo from its stage entry point, the table kernel, the target's one-off tables, and the whole
color_transfer_idt call at --idt-iterations rotations from device-resident inputs (HIP events).  Prints one JSON line at the
end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8.0e12


def photo(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32) / max(H, W)
    ch = [0.5 + 0.3 * np.sin(2 * np.pi * rng.uniform(1, 6) * yy + rng.uniform(0, 6)) *
          np.cos(2 * np.pi * rng.uniform(1, 6) * xx + rng.uniform(0, 6)) for _ in range(3)]
    img = np.stack(ch, -1) + rng.normal(0, 0.06, (H, W, 3)).astype(np.float32)
    return np.clip(np.round(img * 255), 0, 255).astype(np.uint8)


def dev_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def host_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def resize_bytes(C, hw_in, hw_out, scale, esz):
    """Two passes, smaller scale first: each reads its input once and writes its output once."""
    order = [0, 1] if scale[0] <= scale[1] else [1, 0]
    cur, total = list(hw_in), 0
    for ax in order:
        n_in = cur[0] * cur[1]
        cur[ax] = hw_out[ax]
        total += C * (n_in + cur[0] * cur[1]) * esz
    return total


def idt_rows(P, a, dev, src, gen_d, stage, rows):
    """The `idt` rows: every kernel of hg_idt_run on the photo (src, (H, W, 3) fp32) and the 256x256 target, from the stage
    entry points on slots of their own, then the whole transfer.  Bytes: 12 per pixel and plane pass (range: strided read +
    planes written; histogram: planes read; apply: planes read and written, or read + 3 bytes of uint8 out on the last)."""
    lib, st = P.lib, P.raw_stream(dev)
    H, W = src.shape[:2]
    n0, n1, iters, bins = H * W, 256 * 256, a.idt_iterations, a.idt_bins
    tgt = gen_d.permute(1, 2, 0)                                   # a CHW image's view: pix_stride 1, chan_stride 65536
    rot = torch.from_numpy(P.idt_rotations(iters).astype(np.float32)).to(dev)
    stride = lib.hg_idt_plane_stride(n0)
    planes = torch.empty((3, stride), device=dev)
    s_rng = torch.empty(12, dtype=torch.int32, device=dev)
    s_hist = torch.empty(3 * bins, dtype=torch.int64, device=dev)
    t_rng = torch.empty(iters * 6, dtype=torch.int32, device=dev)
    t_hist = torch.empty(iters * 3 * bins, dtype=torch.int64, device=dev)
    m = torch.empty(3 * bins, device=dev)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    ck = P.check

    def clear():
        ck(lib.hg_idt_clear(s_rng.data_ptr(), 2, s_hist.data_ptr(), 3 * bins, st), 'hg_idt_clear')

    def target():
        ck(lib.hg_idt_target_tables(tgt.data_ptr(), n1, 1, n1, rot.data_ptr(), iters, bins, t_rng.data_ptr(), t_hist.data_ptr(), st),
           'hg_idt_target_tables')

    def rng():
        ck(lib.hg_idt_range(src.data_ptr(), n0, 3, 1, rot.data_ptr(), 1, s_rng.data_ptr(), planes.data_ptr(), st), 'hg_idt_range')

    def hist():
        ck(lib.hg_idt_hist(planes.data_ptr(), n0, 1, stride, rot.data_ptr(), 1, bins, s_rng.data_ptr(), s_hist.data_ptr(), 0, st),
           'hg_idt_hist')

    def table():                                                   # keeps the counters, so that it can be repeated
        ck(lib.hg_idt_table(s_hist.data_ptr(), t_hist.data_ptr(), t_rng.data_ptr(), bins, m.data_ptr(), s_rng[6:].data_ptr(), 0, st),
           'hg_idt_table')

    def apply_mid():                                               # rho = 0.5: repeated in place, the pixels stay in the range
        ck(lib.hg_idt_apply(planes.data_ptr(), n0, rot.data_ptr(), rot[1].data_ptr(), bins, s_rng.data_ptr(), m.data_ptr(), 0.5,
                            s_rng[6:].data_ptr(), None, 0, st), 'hg_idt_apply')

    def apply_last():
        ck(lib.hg_idt_apply(planes.data_ptr(), n0, rot.data_ptr(), None, bins, s_rng.data_ptr(), m.data_ptr(), 1.0, None,
                            out.data_ptr(), 1, st), 'hg_idt_apply')

    clear()
    target()
    rng()
    hist()
    table()
    stage(f'idt target tables ({iters} rotations, 256x256)', target, 2 * 12 * n1)
    stage('idt range + planar copy (photo)', rng, 24 * n0)
    stage(f'idt histogram ({bins} nodes, photo)', hist, 12 * n0)
    stage('idt table (one workgroup per axis)', table, 2 * 3 * bins * 8 + 3 * bins * 4)
    # the worst case for the LDS counters: a two-colour image, every pixel of an axis on the same two nodes
    flat = torch.empty((3, stride), device=dev)
    flat[:, 0::2], flat[:, 1::2] = 0.25, 0.75
    f_rng = P.idt_range_tensor(P.idt_encode_range([0.25] * 3, [0.75] * 3), dev)

    def hist_flat():
        ck(lib.hg_idt_hist(flat.data_ptr(), n0, 1, stride, rot.data_ptr(), 1, bins, f_rng.data_ptr(), s_hist.data_ptr(), 0, st),
           'hg_idt_hist')
    stage(f'idt histogram ({bins} nodes, two-colour image)', hist_flat, 12 * n0)
    stage('idt apply, middle rotation (photo)', apply_mid, 24 * n0)
    stage('idt apply, last rotation -> uint8 (photo)', apply_last, 15 * n0)
    nbytes = 2 * 12 * n1 + 24 * n0 + iters * 12 * n0 + (iters - 1) * 24 * n0 + 15 * n0
    t = dev_time(lambda: P.color_transfer_idt(src, tgt, iterations=iters, bins=bins, quantize=True), max(3, a.reps // 4))
    return dict(iterations=iters, bins=bins, transfer_ms=t * 1e3, transfer_bytes=int(nbytes), transfer_gbs=nbytes / t / 1e9,
                hist_blocks=lib.hg_idt_blocks(n0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--H', type=int, default=3024)
    ap.add_argument('--W', type=int, default=4032)
    ap.add_argument('--levels', type=int, default=6)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--cpu-ref', action='store_true')
    ap.add_argument('--idt-iterations', type=int, default=20)
    ap.add_argument('--idt-bins', type=int, default=256)
    a = ap.parse_args()
    from histogan_amd import build
    build.build()
    from histogan_amd import post as P
    if not torch.cuda.is_available():
        raise SystemExit('post_probe: no GPU; nothing is measured')
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    H, W, L = a.H, a.W, a.levels
    ph = photo(rng, H, W)
    gen = (rng.random((3, 256, 256)) * 1.2 - 0.1).astype(np.float32)
    ph_d, gen_d = torch.from_numpy(ph).to(dev), torch.from_numpy(gen).to(dev)
    ref_f = P.u8_hwc_to_float(ph_d)
    Hp, Wp = P.padded_size(H, W, L)
    f4 = 4
    rows = []

    def stage(name, fn, nbytes):
        t = dev_time(fn, a.reps)
        rows.append(dict(stage=name, ms=t * 1e3, bytes=int(nbytes), frac_hbm_peak=nbytes / t / HBM))

    stage('u8 photo -> fp32 planar', lambda: P.u8_hwc_to_float(ph_d), 3 * H * W * (1 + f4))
    stage(f'resize reference {H}x{W} -> {Hp}x{Wp}', lambda: P.imresize(ref_f, output_shape=(Hp, Wp)),
          resize_bytes(3, (H, W), (Hp, Wp), (Hp / H, Wp / W), f4))
    ref_p = P.imresize(ref_f, output_shape=(Hp, Wp)) if (Hp, Wp) != (H, W) else ref_f
    stage(f'resize target 256x256 -> {Hp}x{Wp}', lambda: P.imresize(gen_d, output_shape=(Hp, Wp), clamp=True),
          resize_bytes(3, (256, 256), (Hp, Wp), (Hp / 256, Wp / 256), f4))
    tgt = P.imresize(gen_d, output_shape=(Hp, Wp), clamp=True)

    def pyramids():
        ga, gb = [tgt], [ref_p]
        for _ in range(L - 1):
            ga.append(P.pyr_down(ga[-1]))
            gb.append(P.pyr_down(gb[-1]))
        return ga, gb
    ga, gb = pyramids()
    pb = sum(3 * (g.shape[1] * g.shape[2] + P.pyr_down(g).shape[1] * P.pyr_down(g).shape[2]) * f4 for g in ga[:-1])
    stage(f'both Gaussian pyramids ({L - 1} pyrDown each)', pyramids, 2 * pb)

    ab = P.level_weights(L, 1, False)

    def recon():
        out = ga[L - 1]
        for k in range(1, L):
            wa, wb = ab[k]
            f, c = L - 1 - k, L - k
            out = P.pyr_up_add(out, ga[f] if wa else None, ga[c] if wa else None, wa, gb[f] if wb else None,
                               gb[c] if wb else None, wb)
        return out
    rb = 0
    for k in range(1, L):
        n_f, n_c = ga[L - 1 - k].shape[1] * ga[L - 1 - k].shape[2], ga[L - k].shape[1] * ga[L - k].shape[2]
        rb += 3 * f4 * (n_c + n_f + n_c + n_f)          # prev, one fine + coarse pair, out
    stage(f'reconstruction ({L - 1} fused pyrUp+Laplacian launches)', recon, rb)

    src = torch.from_numpy((ph / 255).astype(np.float32)).to(dev)
    stage('colour moments (photo + generated)', lambda: (P.color_moments(src), P.color_moments(gen_d.permute(1, 2, 0))),
          (3 * H * W + 3 * 256 * 256) * f4)
    m0, A = P.color_moments(src)
    m1, B = P.color_moments(gen_d.permute(1, 2, 0))
    T = P.MKL(A, B)
    coef = np.concatenate([m0, T.reshape(-1), m1]).astype(np.float32)
    import ctypes
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)

    def affine():
        P.check(P.lib.hg_color_affine(src.data_ptr(), H * W, 3, 1, coef.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                      out.data_ptr(), 1, P.raw_stream(dev)), 'hg_color_affine')
    stage('affine -> uint8', affine, 3 * H * W * (f4 + 1))

    idt = idt_rows(P, a, dev, src, gen_d, stage, rows)

    def full_pyr():
        r = torch.from_numpy(ph).to(dev)
        o = P.pyramid_upsampling(gen_d, r, levels=L, swapping_levels=1)
        return P.float_to_u8_hwc(o[0]).cpu()

    def full_mkl():
        s = torch.from_numpy((ph / 255).astype(np.float32)).to(dev)
        o, _ = P.color_transfer_mkl(s, gen_d.permute(1, 2, 0), quantize=True)
        return o.cpu()
    reps = max(3, a.reps // 4)
    res = dict(H=H, W=W, levels=L, padded=[Hp, Wp], stages=rows,
               pyramid_upsampling_call_ms=host_time(full_pyr, reps) * 1e3,
               color_transfer_mkl_call_ms=host_time(full_mkl, reps) * 1e3, idt=idt,
               note='call times include the H2D upload of the photo and the D2H copy of the uint8 result; for MKL '
                    'the photo is converted to fp32 on the host first (as evaluate receives it as a float64 array)')
    for r in rows:
        print(f"{r['stage']:<55s} {r['ms']:8.3f} ms  {r['bytes'] / 1e6:9.1f} MB  {100 * r['frac_hbm_peak']:5.1f}% of HBM peak")
    print(f"pyramid_upsampling, upload -> writer input: {res['pyramid_upsampling_call_ms']:.2f} ms")
    print(f"color_transfer_mkl, upload -> writer input: {res['color_transfer_mkl_call_ms']:.2f} ms")
    print(f"color_transfer_idt, {idt['iterations']} rotations, {idt['bins']} bins, device-resident: {idt['transfer_ms']:.3f} ms, "
          f"{idt['transfer_bytes'] / 1e6:.1f} MB, {idt['transfer_gbs']:.0f} GB/s")
    if a.cpu_ref:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import post_ref as R
        t = time.perf_counter()
        R.pyramid_upsampling(gen, ph.transpose(2, 0, 1).astype(np.float32) / np.float32(255), L, 1)
        res['post_ref_cpu_pyramid_s'] = time.perf_counter() - t
        t = time.perf_counter()
        R.color_transfer(ph / 255, gen.transpose(1, 2, 0))
        res['post_ref_cpu_mkl_s'] = time.perf_counter() - t
        print(f"tests/post_ref.py on this host's CPU: pyramid {res['post_ref_cpu_pyramid_s']:.2f} s, "
              f"MKL {res['post_ref_cpu_mkl_s']:.2f} s")
    print(json.dumps(res))


if __name__ == '__main__':
    main()
