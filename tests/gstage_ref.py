"""Test helper (NOT a test module): the fp64 autograd reference of hg_gstage_bwd (include/hg_nets.h), shared by
tests/test_gstage_gpu.py (small shapes) and tests/test_c3_fused_gpu.py (every stage of the C3 generator).

The chain the kernel replaces (GeneratorBlock.forward / Conv2DMod / RGBBlock, histoGAN/histoGAN.py:461-479, 420-440,
380-390): out = lrelu_0.2(conv d + wn nz + bn), consumed by the next modulated convolution (same resolution, or behind the
bilinear x2 of the next block) and by the block's to-RGB convolution."""
import torch
import torch.nn.functional as F


def gstage_inputs(B, Cc, H, S, up, rgb, g):
    """fp64 inputs of one stage drawn from generator `g` (on g's device).  up: True (next block's conv1 behind the x2),
    False (conv2 of the same block), None (no next convolution: the last block's to-RGB only).  Scales as in the live
    network: styles ~ N(0, 0.5^2), d in [0.5, 1.5], noise weights / biases non-zero, ~half the pre-activations negative."""
    dev = g.device
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64, device=dev)
    conv, d = rnd(B, Cc, H, H), torch.rand(B, Cc, generator=g, dtype=torch.float64, device=dev) + 0.5
    nzt = torch.rand(B, S, S, generator=g, dtype=torch.float64, device=dev)
    wn, bn = rnd(Cc) * 0.5, rnd(Cc) * 0.2
    sa, srgb, w = rnd(B, Cc) * 0.5, rnd(B, Cc) * 0.5, rnd(3, Cc)
    has_a = up is not None
    ga = rnd(B, Cc, 2 * H, 2 * H) if up else (rnd(B, Cc, H, H) if has_a else None)
    g_rgb = rnd(B, 3, H, H) if rgb else None
    return dict(conv=conv, d=d, nzt=nzt, wn=wn, bn=bn, sa=sa, srgb=srgb, w=w, ga=ga, g_rgb=g_rgb)


def gstage_fp64(inp, up, rgb):
    """fp64 autograd of the replaced chain -> (out, (gconv, gd, gwn, gbn, gs_a, gs_rgb, gw_rgb)); entries of consumers the
    stage does not have are None."""
    H = inp['conv'].shape[-1]
    leaves = [inp[k].detach().clone().requires_grad_(True) for k in ('conv', 'd', 'wn', 'bn', 'sa', 'srgb', 'w')]
    conv, d, wn, bn, sa, srgb, w = leaves
    nzt, ga, g_rgb = inp['nzt'], inp['ga'], inp['g_rgb']
    pre = conv * d[:, :, None, None] + wn[None, :, None, None] * nzt[:, None, :H, :H] + bn[None, :, None, None]
    out = F.leaky_relu(pre, 0.2)
    loss = 0.0
    if up is not None:
        xa = F.interpolate(out, scale_factor=2, mode='bilinear', align_corners=False) if up else out
        loss = loss + (xa * (sa + 1)[:, :, None, None] * ga).sum()
    if rgb:
        loss = loss + (torch.einsum('kc,bcij->bkij', w, out * (srgb + 1)[:, :, None, None]) * g_rgb).sum()
    want = torch.autograd.grad(loss, leaves, allow_unused=True)
    return out.detach(), want


def run_gstage(out, inp, up, rgb, dev):
    """hg_gstage_bwd on the fp32 roundings of `out` and the inputs -> (gconv, gs_a, gs_rgb, gw_rgb, gd, gwn, gbn)."""
    from histogan_amd.gfused import gstage_bwd
    has_a = up is not None
    f = lambda t: None if t is None else t.detach().float().to(dev).contiguous()
    return gstage_bwd(f(out), f(inp['ga']), f(inp['sa']) if has_a else None, bool(up), f(inp['g_rgb']),
                      f(inp['w']) if rgb else None, f(inp['srgb']) if rgb else None, f(inp['d']), f(inp['nzt']),
                      f(inp['wn']), f(inp['bn']))
