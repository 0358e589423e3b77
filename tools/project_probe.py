#!/usr/bin/env python3
"""Cost of the projection path, un-profiled (HIP events, as tools/phase_probe.py):

  kernel   hg_noise_grad stand-alone at the 14 stage shapes of Generator(256, 512, 16), B = 1: us per launch and the
           fraction of the 8 TB/s HBM peak its read of gconv reaches (back-to-back launches over rotating inputs);
  step     one projection step at 256^2 / capacity 16 / B = 1 against frozen weights, forward + backward of an L1 pixel
           loss: styles only, and styles + noise image.

    python tools/project_probe.py [--iters 200] [--steps 30] [--out project_probe.json]

The step part uses nothing but Generator.forward, so it also runs on a tree without hg_noise_grad (styles only: the
figure the frozen-weight gating is compared against)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=200)
ap.add_argument('--steps', type=int, default=30)
ap.add_argument('--out', default='')
a = ap.parse_args()
from histogan_amd._lib import lib  # noqa: E402
from histogan_amd.nets import Generator  # noqa: E402

dev = torch.device('cuda:0')
med = lambda v: sorted(v)[len(v) // 2]
HBM_PEAK = 8e12
out = {'kernel': [], 'step': {}}


_blk = torch.randn(8192, 8192, device=dev)


def timed(fn, n, ahead=False):
    """Median GPU time of fn() in ms over n calls, each between its own pair of events.  ahead: a ~10 ms matrix product
    is enqueued in front of the first event, so that the host has enqueued all of fn()'s launches before the GPU starts on
    them (short kernels: the GPU's time, not the host's launch rate)."""
    for _ in range(3):
        fn()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if ahead:
            torch.mm(_blk, _blk)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return med(ts)


if hasattr(lib, 'hg_noise_grad'):
    from histogan_amd.launch import noise_grad
    filters = [64] + [16 * 2 ** (i + 1) for i in range(7)][::-1]
    S = 256
    gnz = torch.zeros(1, S, S, device=dev)
    shapes = [(filters[i + 1], 4 << i) for i in range(7) for _ in range(2)]
    total_us = 0.0
    for O, H in shapes:
        nbytes = O * H * H * 4
        # Rotate over enough copies of gconv that a launch does not find its input in the 256 MB last-level cache from the
        # previous one (the small maps stay cache-resident either way -- as they are in the backward, where the stage kernel
        # has just written them); `window` back-to-back launches between two events, enqueued while the GPU is still busy with earlier work; median of 7 windows.
        rot = max(2, min(64, (512 << 20) // nbytes))
        gcs = [torch.randn(1, O, H, H, device=dev) for _ in range(rot)]
        d, wn = torch.rand(1, O, device=dev) + 0.5, torch.randn(O, device=dev)
        window = max(rot, a.iters)
        it = [0]

        def burst():
            for _ in range(window):
                noise_grad(gcs[it[0] % rot], d, wn, gnz, True)
                it[0] += 1

        us = timed(burst, 7, ahead=True) * 1e3 / window
        out['kernel'].append({'O': O, 'H': H, 'us': round(us, 2), 'gconv_bytes': nbytes,
                              'hbm_fraction': round(nbytes / (us * 1e-6) / HBM_PEAK, 4)})
        total_us += us
        del gcs
    out['kernel_total_us'] = round(total_us, 1)
    out['kernel_total_bytes'] = sum(r['gconv_bytes'] for r in out['kernel'])

torch.manual_seed(0)
G = Generator(256, 512, 16).to(dev)
with torch.no_grad():
    for b in G.blocks:
        for m in (b.to_noise1, b.to_noise2):
            m.weight.normal_(std=0.3)
            m.bias.normal_(std=0.1)
for p in G.parameters():
    p.requires_grad_(False)
L = G.num_layers
image = torch.rand(1, 3, 256, 256, device=dev)
for name, with_noise in (('styles_only', False), ('styles_and_noise', True)):
    styles = torch.randn(1, L - 2, 512, device=dev, requires_grad=True)
    hists = torch.randn(1, 2, 512, device=dev, requires_grad=True)
    noise = torch.rand(1, 256, 256, 1, device=dev, requires_grad=with_noise)

    def step():
        styles.grad = hists.grad = noise.grad = None
        (image - G(styles, hists, noise)).abs().mean().backward()

    ms = timed(step, a.steps)
    if with_noise and noise.grad is None:
        out['step'][name] = None          # (a tree without the noise gradient)
        continue
    out['step'][name] = round(ms, 3)
torch.cuda.synchronize()
print(json.dumps(out))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
