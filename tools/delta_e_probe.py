#!/usr/bin/env python3
"""What does the fused colour difference cost against what a user would write today?  HIP events, un-profiled, alternating
rounds; each kind is timed in a child process of its own under a time limit, so that one that hangs ends there.

    python tools/delta_e_probe.py OUT.json [rounds] [iterations per round]

At 32 x 3 x 256 x 256, forward + backward of mean_b(dE) with respect to the first image, for kind 76 and 2000:
  (a) post.delta_e(pred, target, kind)                    one fused fp64 launch (+ its finish) and the autograd scaling
  (b) the same formula composed from aten ops in fp32     with autograd, on the same GPU: the yardstick
The expectation is (a) <= (b); the margin is the spread of (b) over the rounds."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMIT_S = 240


def aten_delta_e(pred, target, kind):
    """The definition of include/hg_post.h written with aten ops in the tensors' own precision (fp32 here), roots and atan2
    guarded so that the gradient is finite: (B,) means."""
    import torch
    M = torch.tensor([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]],
                     dtype=pred.dtype, device=pred.device)
    M = M / M.sum(dim=1, keepdim=True)
    one = torch.ones((), dtype=pred.dtype, device=pred.device)

    def root(x):
        pos = x > 0
        return torch.where(pos, torch.sqrt(torch.where(pos, x, one)), 0 * x)

    def lab(x):
        c = x.clamp(0, 1)
        hi = c > 0.04045
        lin = torch.where(hi, ((torch.where(hi, c, one) + 0.055) / 1.055) ** 2.4, c / 12.92)
        xyz = torch.einsum('ij,bjhw->bihw', M, lin)
        d = 6.0 / 29.0
        up = xyz > d ** 3
        f = torch.where(up, torch.where(up, xyz, one) ** (1.0 / 3.0), xyz / (3 * d * d) + 4.0 / 29.0)
        return 116 * f[:, 1] - 16, 500 * (f[:, 0] - f[:, 1]), 200 * (f[:, 1] - f[:, 2])

    L1, a1, b1 = lab(pred)
    L2, a2, b2 = lab(target)
    if kind == 76:
        return root((L1 - L2) ** 2 + (a1 - a2) ** 2 + (b1 - b2) ** 2).mean(dim=(1, 2))

    def hue(y, x):
        o = (x == 0) & (y == 0)
        h = torch.rad2deg(torch.atan2(torch.where(o, 0 * y, y), torch.where(o, one, x)))
        return torch.where(h < 0, h + 360, h)

    cosd = lambda v: torch.cos(torch.deg2rad(v))      # noqa: E731
    sind = lambda v: torch.sin(torch.deg2rad(v))      # noqa: E731
    C1, C2 = root(a1 * a1 + b1 * b1), root(a2 * a2 + b2 * b2)
    Cm7 = ((C1 + C2) / 2) ** 7
    G = 0.5 * (1 - root(Cm7 / (Cm7 + 25.0 ** 7)))
    a1p, a2p = (1 + G) * a1, (1 + G) * a2
    C1p, C2p = root(a1p * a1p + b1 * b1), root(a2p * a2p + b2 * b2)
    h1, h2 = hue(b1, a1p), hue(b2, a2p)
    grey = C1p * C2p == 0
    dh = h2 - h1
    dh = torch.where(dh > 180, dh - 360, torch.where(dh < -180, dh + 360, dh))
    dh = torch.where(grey, 0 * dh, dh)
    dH = 2 * root(C1p * C2p) * sind(dh / 2)
    Lm, Cmp, hs = (L1 + L2) / 2, (C1p + C2p) / 2, h1 + h2
    hm = torch.where((h1 - h2).abs() <= 180, hs / 2, torch.where(hs < 360, (hs + 360) / 2, (hs - 360) / 2))
    hm = torch.where(grey, hs, hm)
    T = 1 - 0.17 * cosd(hm - 30) + 0.24 * cosd(2 * hm) + 0.32 * cosd(3 * hm + 6) - 0.20 * cosd(4 * hm - 63)
    dtheta = 30 * torch.exp(-(((hm - 275) / 25) ** 2))
    Cmp7 = Cmp ** 7
    RC = 2 * root(Cmp7 / (Cmp7 + 25.0 ** 7))
    SL = 1 + 0.015 * (Lm - 50) ** 2 / torch.sqrt(20 + (Lm - 50) ** 2)
    SC, SH = 1 + 0.045 * Cmp, 1 + 0.015 * Cmp * T
    RT = -sind(2 * dtheta) * RC
    tL, tC, tH = (L2 - L1) / SL, (C2p - C1p) / SC, dH / SH
    return root(tL * tL + tC * tC + tH * tH + RT * tC * tH).mean(dim=(1, 2))


def measure(kind, rounds, iters):
    import torch
    from histogan_amd import post
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(0)
    t = (0.05 + 0.9 * torch.rand(32, 3, 256, 256, generator=gen)).to(dev)
    u = (0.05 + 0.9 * torch.rand(32, 3, 256, 256, generator=gen)).to(dev)
    pred = 0.85 * t + 0.15 * u

    def fwd_bwd(fn):
        p = pred.detach().requires_grad_(True)
        fn(p).mean().backward()
        return p.grad

    work = {'a_fused': lambda: fwd_bwd(lambda p: post.delta_e(p, t, kind)),
            'b_aten_fp32': lambda: fwd_bwd(lambda p: aten_delta_e(p, t, kind))}
    ga, gb = work['a_fused'](), work['b_aten_fp32']()
    agree = float((ga - gb).abs().max() / gb.abs().max())     # fp32 composition against the fp64 kernel: a sanity figure only
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
    spread = max(ms['b_aten_fp32']) - min(ms['b_aten_fp32'])
    return {'kind': kind, 'ms_per_call_by_round': ms, 'median_ms': med, 'spread_of_b_ms': spread,
            'a_minus_b_ms': med['a_fused'] - med['b_aten_fp32'], 'a_not_slower_than_b': med['a_fused'] <= med['b_aten_fp32'] + spread,
            'gradient_relmax_a_vs_b': agree, 'device': torch.cuda.get_device_name(0)}


def main(out_path, rounds=5, iters=10):
    res = {'shape': '32x3x256x256, forward + backward of mean_b(dE) with respect to the first image', 'rounds': rounds,
           'iterations_per_round': iters, 'kinds': {}}
    for kind in (76, 2000):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', str(kind), str(rounds), str(iters)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            res['kinds'][str(kind)] = {'error': f'no result within {STEP_LIMIT_S} s'}
            break                                             # nothing more on the GPU after a step that hung
        if out.returncode != 0:
            res['kinds'][str(kind)] = {'error': f'exit status {out.returncode}', 'stderr': out.stderr[-2000:]}
            break
        res['kinds'][str(kind)] = json.loads(out.stdout.strip().splitlines()[-1])
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {n: v.get(n) for n in ('median_ms', 'spread_of_b_ms', 'a_minus_b_ms', 'a_not_slower_than_b', 'error')}
                      for k, v in res['kinds'].items()}))
    return 0 if all('error' not in v for v in res['kinds'].values()) else 1


if __name__ == '__main__':
    if sys.argv[1] == '--child':
        print(json.dumps(measure(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))))
    else:
        sys.exit(main(sys.argv[1], *(int(a) for a in sys.argv[2:4])))
