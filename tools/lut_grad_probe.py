"""Times the differentiable side of the 3D LUTs (hg_lut_apply_bwd, hg_lut_adam_step, post.lut_refine) on one GPU with HIP
events, un-profiled, and measures what the refine is for.

  backward   hg_lut_apply_bwd (both gradients, and the LUT's alone) at N = 17 and 33, both interpolations, on a 256 x 256 and on a
             3000 x 4000 image; next to each the forward on the same input and the LUT's gradient computed by torch eager
             (gather, mask, index_add_) on the same GPU.
  refine     seconds per post.lut_refine step at the block's working size, and the same step launch by launch.
  hellinger  for one 3000 x 4000 synthetic photo: the Hellinger distance between the target histogram and the histogram of the
             full-size output (the block reduces LUT(photo) itself) before and after the refine, next to the loss the refine sees
             (the histogram of LUT(reduced photo)).

    python tools/lut_grad_probe.py [--H 3000 --W 4000 --reps 10 --out profiles/lut_grad.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lut_probe import dev_time, graded, photo  # noqa: E402


def eager_glut(x, lut, g, interpolation):
    """The LUT's gradient from torch ops alone: the yardstick (fp32 index_add_, so its sums depend on their order)."""
    n = lut.shape[0]
    xc = torch.nan_to_num(x.reshape(-1, 3)).clamp(0, 1)
    t = xc * (n - 1)
    i = t.floor().clamp(max=n - 2).long()
    f = t - i
    L, g = lut.reshape(-1, 3), g.reshape(-1, 3)
    step = torch.tensor([1, n, n * n], device=x.device)
    base = (i * step).sum(1)
    if interpolation == 'trilinear':
        nodes, weights = [], []
        for j in range(8):
            bit = torch.tensor([j & 1, (j >> 1) & 1, j >> 2], device=x.device)
            nodes.append(base + (bit * step).sum())
            weights.append(torch.where(bit.bool(), f, 1 - f).prod(1))
    else:
        fs, order = f.sort(dim=1, descending=True)
        inc = step[order].cumsum(1)
        nodes = [base, base + inc[:, 0], base + inc[:, 1], base + inc[:, 2]]
        weights = [1 - fs[:, 0], fs[:, 0] - fs[:, 1], fs[:, 1] - fs[:, 2], fs[:, 2]]
    out = sum(w[:, None] * L[k] for k, w in zip(nodes, weights))
    gm = torch.where((out >= 0) & (out <= 1) & torch.isfinite(g), g, torch.zeros_like(g))
    glut = torch.zeros_like(L)
    for k, w in zip(nodes, weights):
        glut.index_add_(0, k, w[:, None] * gm)
    return glut.view(n, n, n, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--H', type=int, default=3000)
    ap.add_argument('--W', type=int, default=4000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lut_grad_probe: no GPU (a timing taken anywhere else says nothing)')
    from histogan_amd import post as P
    from histogan_amd.hist import hellinger_loss
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    dev = torch.device('cuda', 0)
    rng = np.random.RandomState(0)
    rows = []

    def row(name, seconds, **extra):
        rows.append(dict(name=name, ms=seconds * 1e3, **extra))
        print(f'{name:86s} {seconds * 1e3:9.3f} ms', flush=True)

    big = torch.from_numpy(photo(rng, a.H, a.W)).to(dev)
    small = torch.from_numpy(photo(rng, 256, 256)).to(dev)
    luts = {n: P.lut_fit(small, graded(small), n=n) for n in (17, 33)}
    # ---- the backward against its two yardsticks
    for img in (small, big):
        H, W = img.shape[:2]
        g = torch.randn(H, W, 3, device=dev)
        for n in (17, 33):
            for interpolation in ('tetrahedral', 'trilinear'):
                tag = f'N={n} {interpolation} {H}x{W}'
                fwd = dev_time(lambda: P.lut_apply(img, luts[n], interpolation), a.reps)
                both = dev_time(lambda: P.lut_apply_backward(img, luts[n], g, interpolation), a.reps)
                only = dev_time(lambda: P.lut_apply_backward(img, luts[n], g, interpolation, want_image=False), a.reps)
                gx = dev_time(lambda: P.lut_apply_backward(img, luts[n], g, interpolation, want_lut=False), a.reps)
                eager = dev_time(lambda: eager_glut(img, luts[n], g, interpolation), max(2, a.reps // 3))
                row(f'lut_apply forward {tag}', fwd)
                row(f'hg_lut_apply_bwd gx + glut {tag}', both, over_forward=both / fwd)
                row(f'hg_lut_apply_bwd glut only {tag}', only, over_forward=only / fwd, eager_over_this=eager / only)
                row(f'hg_lut_apply_bwd gx only {tag}', gx, over_forward=gx / fwd)
                row(f'torch eager glut (index_add_) {tag}', eager)
                ref = eager_glut(img, luts[n], g, interpolation)
                got = P.lut_apply_backward(img, luts[n], g, interpolation, want_image=False)[1]
                rows[-1]['max_abs_difference_to_hip'] = float((ref - got).abs().max())
    # ---- one refine step and its parts, at the working size of the default block
    block = RGBuvHistBlock(h=64, insz=150, device=dev)
    target = block(graded(graded(small)).permute(2, 0, 1).unsqueeze(0)).detach()
    work, _ = P.lut_working_copy(big, block)
    n = 33
    steps = 50
    t_refine = dev_time(lambda: P.lut_refine(luts[n], big, target, block, steps=steps), 3)
    t_copy = dev_time(lambda: P.lut_working_copy(big, block), a.reps)
    row(f'lut_refine N={n}, {steps} steps, {a.H}x{a.W} photo, whole call', t_refine, per_step_ms=(t_refine - t_copy) / steps * 1e3)
    row(f'  working copy ({work.shape[0]}x{work.shape[1]}), once', t_copy)
    table = luts[n].clone().requires_grad_(True)
    out = P.lut_apply(work, table, differentiable=True)
    x4 = out.detach().permute(2, 0, 1).unsqueeze(0).requires_grad_(True)
    hist = block(x4)
    hleaf = hist.detach().requires_grad_(True)
    gh, gout = torch.randn_like(hist), torch.randn_like(out)
    m, v, nxt = torch.zeros_like(luts[n]), torch.zeros_like(luts[n]), torch.empty_like(luts[n])
    parts = (('lut_apply forward', lambda: P.lut_apply(work, luts[n], differentiable=True)),
             ('histogram forward', lambda: block(x4)),
             ('Hellinger forward + backward', lambda: torch.autograd.grad(hellinger_loss(target, hleaf, global_batch=False), hleaf)),
             ('histogram backward', lambda: torch.autograd.grad(hist, x4, gh, retain_graph=True)),
             ('hg_lut_apply_bwd (glut)', lambda: P.lut_apply_backward(work, luts[n], gout, want_image=False)),
             ('hg_lut_adam_step', lambda: P.lut_adam_step(luts[n], gout.new_zeros(luts[n].shape), m, v, 1, out=nxt)))
    for name, fn in parts:
        row(f'  step part: {name}', dev_time(fn, 5 * a.reps))
    # ---- what the refine is for: the histogram of the full-size output
    def full_size(lut):
        out = P.lut_apply(big, lut)
        return float(hellinger_loss(target, block(out.permute(2, 0, 1).unsqueeze(0)), global_batch=False))

    hell = {}
    for start, lut0 in (('fitted', P.lut_fit(small, graded(small), n=n)), ('identity', P.lut_identity(n, dev))):
        refined, losses = P.lut_refine(lut0, big, target, block, return_losses=True)
        hell[start] = dict(full_size_before=full_size(lut0), full_size_after=full_size(refined),
                           working_copy_before=float(losses[0]), working_copy_after=float(losses[-1]),
                           smoothness_after=float(P.lut_smoothness(refined)))
        print(f'Hellinger to the target, LUT from {start}: full size {hell[start]["full_size_before"]:.4f} -> '
              f'{hell[start]["full_size_after"]:.4f}; working copy {losses[0]:.4f} -> {losses[-1]:.4f}', flush=True)
    record = dict(H=a.H, W=a.W, reps=a.reps, steps=P.LUT_REFINE_STEPS, lr=P.LUT_REFINE_LR, lambda_smooth=P.LUT_REFINE_LAMBDA,
                  device=torch.cuda.get_device_name(0), rows=rows, hellinger=hell)
    print(json.dumps(record))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(record, indent=1) + '\n')


if __name__ == '__main__':
    main()
