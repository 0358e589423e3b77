#!/usr/bin/env python3
"""What do the fused SSIM / MS-SSIM cost against what a user would write today?  HIP events, un-profiled, alternating rounds;
each case is timed in a child process of its own under a time limit, so that one that hangs ends there.

    python tools/ssim_probe.py OUT.json [rounds] [iterations per round]

At 32 x 3 x 256 x 256, forward alone and forward + backward of mean_b(value) with respect to the first image, for
post.ssim 'L', post.ssim 'rgb' and post.ms_ssim 'L':
  (a) the fused fp64 kernels (hg_ssim_fwd + its finish, hg_ssim_bwd; five of each for MS-SSIM)
  (b) the same formula composed from aten ops in fp32 (depthwise separable F.conv2d) with autograd, on the same GPU
The requirement is (a) < (b) for every case.  Also reported: the share of the three-image HBM floor (two images read, one
gradient written: 3 x 25.2 MB) that (a)'s forward + backward reaches at the chip's nominal 8 TB/s."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMIT_S = 240
CASES = ('ssim-L', 'ssim-rgb', 'ms-ssim-L')
HBM_BYTES_PER_S = 8.0e12
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def aten_planes(x, channels):
    import torch
    c = x.clamp(0, 1)
    if channels == 'rgb':
        return c
    M = torch.tensor([0.212671, 0.715160, 0.072169], dtype=x.dtype, device=x.device)
    one = torch.ones((), dtype=x.dtype, device=x.device)
    hi = c > 0.04045
    lin = torch.where(hi, ((torch.where(hi, c, one) + 0.055) / 1.055) ** 2.4, c / 12.92)
    Y = torch.einsum('j,bjhw->bhw', M / M.sum(), lin)[:, None]
    d = 6.0 / 29.0
    up = Y > d ** 3
    f = torch.where(up, torch.where(up, Y, one) ** (1.0 / 3.0), Y / (3 * d * d) + 4.0 / 29.0)
    return (116 * f - 16) / 100


def aten_level(x, y, g):
    """(mean ssim, mean cs), each (B,), of (B, P, H, W) planes: the definition of include/hg_post.h in the tensors' precision."""
    import torch.nn.functional as F
    P = x.shape[1]
    gh, gv = g.view(1, 1, 1, -1).repeat(P, 1, 1, 1), g.view(1, 1, -1, 1).repeat(P, 1, 1, 1)
    blur = lambda p: F.conv2d(F.conv2d(p, gh, groups=P), gv, groups=P)      # noqa: E731
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    cs = (2 * sxy + 9e-4) / (sxx + syy + 9e-4)
    s = (2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4) * cs
    return s.mean(dim=(1, 2, 3)), cs.mean(dim=(1, 2, 3))


def aten_value(pred, target, case):
    import torch
    import torch.nn.functional as F
    channels = case.rsplit('-', 1)[1]
    k = torch.arange(11, dtype=pred.dtype, device=pred.device)
    g = torch.exp(-((k - 5) ** 2) / 4.5)
    g = g / g.sum()
    x, y = aten_planes(pred, channels), aten_planes(target, channels)
    if not case.startswith('ms-'):
        return aten_level(x, y, g)[0]
    ms = None
    for s, w in enumerate(WEIGHTS):
        ss, cs = aten_level(x, y, g)
        term = (ss if s == len(WEIGHTS) - 1 else cs).clamp(min=0) ** w
        ms = term if ms is None else ms * term
        if s + 1 < len(WEIGHTS):
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    return ms


def measure(case, rounds, iters):
    import torch
    from histogan_amd import post
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(0)
    t = (0.05 + 0.9 * torch.rand(32, 3, 256, 256, generator=gen)).to(dev)
    u = (0.05 + 0.9 * torch.rand(32, 3, 256, 256, generator=gen)).to(dev)
    pred = 0.85 * t + 0.15 * u
    channels = case.rsplit('-', 1)[1]
    fused = (lambda p: post.ms_ssim(p, t, channels)) if case.startswith('ms-') else (lambda p: post.ssim(p, t, channels))
    aten = lambda p: aten_value(p, t, case)      # noqa: E731

    def fwd(fn):
        with torch.no_grad():
            return fn(pred)

    def fwd_bwd(fn):
        p = pred.detach().requires_grad_(True)
        fn(p).mean().backward()
        return p.grad

    work = {'fwd_fused': lambda: fwd(fused), 'fwd_aten_fp32': lambda: fwd(aten),
            'fwdbwd_fused': lambda: fwd_bwd(fused), 'fwdbwd_aten_fp32': lambda: fwd_bwd(aten)}
    ga, gb = work['fwdbwd_fused'](), work['fwdbwd_aten_fp32']()
    agree = float((ga - gb).abs().max() / gb.abs().max())     # fp32 composition against the fp64 kernel: a sanity figure only
    value = float((work['fwd_fused']() - work['fwd_aten_fp32']()).abs().max())
    for f in work.values():                                   # warm-up: module load, allocator, clocks
        for _ in range(3):
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
    floor_ms = 3 * pred.numel() * 4 / HBM_BYTES_PER_S * 1e3
    return {'case': case, 'ms_per_call_by_round': ms, 'median_ms': med,
            'ratio_aten_over_fused': {'fwd': med['fwd_aten_fp32'] / med['fwd_fused'],
                                      'fwdbwd': med['fwdbwd_aten_fp32'] / med['fwdbwd_fused']},
            'fused_is_faster': {'fwd': max(ms['fwd_fused']) < min(ms['fwd_aten_fp32']),
                                'fwdbwd': max(ms['fwdbwd_fused']) < min(ms['fwdbwd_aten_fp32'])},
            'hbm_floor_ms': floor_ms, 'share_of_hbm_floor_fwdbwd': floor_ms / med['fwdbwd_fused'],
            'value_absmax_fused_vs_aten': value, 'gradient_relmax_fused_vs_aten': agree, 'device': torch.cuda.get_device_name(0)}


def main(out_path, rounds=5, iters=10):
    res = {'shape': '32x3x256x256; forward, and forward + backward of mean_b(value) with respect to the first image', 'rounds': rounds,
           'iterations_per_round': iters, 'cases': {}}
    for case in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), '--child', case, str(rounds), str(iters)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            res['cases'][case] = {'error': f'no result within {STEP_LIMIT_S} s'}
            break                                             # nothing more on the GPU after a step that hung
        if out.returncode != 0:
            res['cases'][case] = {'error': f'exit status {out.returncode}', 'stderr': out.stderr[-2000:]}
            break
        res['cases'][case] = json.loads(out.stdout.strip().splitlines()[-1])
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {n: v.get(n) for n in ('median_ms', 'ratio_aten_over_fused', 'fused_is_faster', 'share_of_hbm_floor_fwdbwd', 'error')}
                      for k, v in res['cases'].items()}))
    return 0 if all('error' not in v for v in res['cases'].values()) else 1


if __name__ == '__main__':
    if sys.argv[1] == '--child':
        print(json.dumps(measure(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))))
    else:
        sys.exit(main(sys.argv[1], *(int(a) for a in sys.argv[2:4])))
