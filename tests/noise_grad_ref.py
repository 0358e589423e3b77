"""Test helper (NOT a test module): fp64 references for the noise image's gradient (hg_noise_grad, include/hg_nets.h;
tests/test_noise_grad_gpu.py).

A generator stage is out = lrelu_0.2(d conv + wn nzt + bn) (GeneratorBlock.forward, histoGAN/histoGAN.py:461-479); with
gconv = g lrelu'(out) d the gradient of the transposed noise image is sum_o (wn[o] / d[b,o]) gconv[b,o] on the stage's
H x H window."""
import torch
import torch.nn.functional as F


def noise_grad_inputs(B, O, H, demod, seed):
    """fp32 inputs of one hg_noise_grad call (CPU): gconv (B,O,H,H), d (B,O) in [0.5, 1.5] or None, wn (O)."""
    g = torch.Generator().manual_seed(seed)
    gconv = torch.randn(B, O, H, H, generator=g)
    d = torch.rand(B, O, generator=g) + 0.5 if demod else None
    wn = torch.randn(O, generator=g) * 0.5
    return gconv, d, wn


def noise_grad_fp64(gconv, d, wn):
    """sum_o (wn[o] / d[b,o]) gconv[b,o,i,j] in fp64 on the fp32 inputs -> (B,H,H)."""
    sc = wn.double()[None, :] / d.double() if d is not None else wn.double()[None, :].expand(gconv.shape[0], -1)
    return torch.einsum('bo,boij->bij', sc, gconv.double())


def stage_nzt_grad_fp64(conv, d, nzt, wn, bn, gout, mask):
    """fp64 autograd of the written-out stage with respect to nzt (B,S,S), on the LeakyReLU branches `mask` (= out > 0 of
    the run under test): out = where(mask, pre, 0.2 pre), pre = conv d + wn nzt[:, :H, :H] + bn."""
    H = conv.shape[-1]
    n = nzt.detach().double().clone().requires_grad_(True)
    pre = conv.double() * (d.double()[:, :, None, None] if d is not None else 1.0) \
        + wn.double().reshape(1, -1, 1, 1) * n[:, None, :H, :H] + bn.double().reshape(1, -1, 1, 1)
    out = torch.where(mask, pre, 0.2 * pre)
    return torch.autograd.grad(out, n, gout.double())[0]


def demod_fp64(style, w):
    """Conv2DMod's demodulation coefficient (histoGAN/histoGAN.py:427-429) in fp64: (B,N)."""
    s1 = style.double() + 1
    return torch.rsqrt((s1 * s1) @ w.double().pow(2).sum(dim=(2, 3)).t() + 1e-8)


def modconv_fp64(x, style, w, upsample):
    """conv(up?(x) (style + 1), w) in fp64 (the shared-weight form of Conv2DMod, without demodulation)."""
    x = x.double()
    if upsample:
        x = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
    return F.conv2d(x * (style.double() + 1)[:, :, None, None], w.double(), padding=w.shape[-1] // 2)


_ORACLE = {}


def projection_oracle(sd, image, hist, seed, pixel_loss, steps, lr, noise_reg_weight, style_reg_weight, dtype):
    """The reference's projection loop (projection_gaussian.py:407-504: one latent repeated over the style rows and a
    noise image, Adam on both against fixed SE / HE / GE) on oracle.histogan_nets on the CPU in `dtype`; the draws are
    histogan_amd.project.project's (randn(B, latent) then rand(B, S, S, 1) from a CPU generator seeded `seed`).
    sd: state dict with 'SE.', 'HE.', 'GE.' prefixes.  Returns the list of per-step losses.  Cached per argument set."""
    from oracle import histogan_nets as N
    key = (seed, pixel_loss, steps, lr, noise_reg_weight, style_reg_weight, dtype)
    if key in _ORACLE:
        return _ORACLE[key]
    sub = lambda p: {k[len(p) + 1:]: v.detach().cpu().to(dtype) for k, v in sd.items() if k.startswith(p + '.')}
    sG, sS, sH = sub('GE'), sub('SE'), sub('HE')
    L = sum(1 for k in sG if k.endswith('.conv1.weight'))
    B, S = image.shape[0], image.shape[-1]
    LAT = sG['blocks.0.to_style1.weight'].shape[1]
    g = torch.Generator().manual_seed(seed)
    styles = torch.randn(B, LAT, generator=g)[:, None, :].repeat(1, L - 2, 1).to(dtype).requires_grad_()
    noise = torch.rand(B, S, S, 1, generator=g).to(dtype).requires_grad_()
    img = image.detach().cpu().to(dtype)
    hw = N.vectorizer(sH, hist.detach().cpu().to(dtype), 'fcs')
    opt = torch.optim.Adam([styles, noise], lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        w = torch.stack([N.vectorizer(sS, styles[:, i, :], 'net') for i in range(L - 2)], dim=1)
        rgb = N.generator(sG, w, torch.stack((hw, hw), dim=1), noise, L)
        rec = (img - rgb).abs().mean() if pixel_loss == 'L1' else F.mse_loss(img, rgb)
        loss = rec + noise_reg_weight * noise.mean() ** 2 + style_reg_weight * styles.mean() ** 2 / styles.shape[1]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    _ORACLE[key] = losses
    return losses
