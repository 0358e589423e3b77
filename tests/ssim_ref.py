"""Test helper (NOT a test module): SSIM and MS-SSIM as include/hg_post.h (hg_ssim_fwd, hg_ssim_bwd) define them, restated in
torch fp64 on the CPU from the published formulas (Wang, Bovik, Sheikh, Simoncelli 2004; Wang, Simoncelli, Bovik 2003) and not
from the code under test, on top of tests/lab_ref.srgb_to_lab.  Gradients come from autograd; `analytic_plane_grad` is the
three-map form of the definition as a second, independent function (adjoint blur = conv_transpose2d).

Nothing needs excluding: denominators are at least C1 and C2, the CIE f is C1 in lab_ref's form, and seeded_pair keeps every
component inside (0.05, 0.95), away from the clamp and from the sRGB knee at 0.04045."""
import torch
import torch.nn.functional as F

import lab_ref

C1, C2 = 1e-4, 9e-4
TAPS = 11
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
CHANNELS = ('L', 'rgb')


def window():
    """The 11 taps g_k = exp(-(k - 5)^2 / 4.5) / sum, fp64."""
    k = torch.arange(TAPS, dtype=torch.float64)
    g = torch.exp(-((k - 5.0) ** 2) / 4.5)
    return g / g.sum()


def planes(x, channels):
    """(B, 3, H, W) sRGB of any float type -> (B, P, H, W) fp64 planes of the pixels clamped to [0, 1]: P = 1, L* / 100 ('L'), or
    P = 3, the components ('rgb').  Differentiable (torch.clamp's mask is inclusive)."""
    B, _, H, W = x.shape
    c = x.double().clamp(0.0, 1.0)
    if channels == 'rgb':
        return c
    assert channels == 'L'
    return lab_ref.srgb_to_lab(c.reshape(B, 3, H * W))[:, 0].reshape(B, 1, H, W)


def blur(p):
    """Valid separable Gaussian of (B, P, H, W): (B, P, H - 10, W - 10)."""
    B, P, H, W = p.shape
    g = window()
    q = F.conv2d(p.reshape(B * P, 1, H, W), g.view(1, 1, 1, TAPS))
    return F.conv2d(q, g.view(1, 1, TAPS, 1)).reshape(B, P, H - TAPS + 1, W - TAPS + 1)


def plane_maps(x, y):
    """(ssim, cs) maps, each (B, P, H - 10, W - 10), of fp64 planes."""
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    l = (2 * mx * my + C1) / (mx * mx + my * my + C1)
    cs = (2 * sxy + C2) / (sxx + syy + C2)
    return l * cs, cs


def plane_means(x, y):
    """(mean ssim, mean cs), each (B,), over positions and planes."""
    s, cs = plane_maps(x, y)
    return s.mean(dim=(1, 2, 3)), cs.mean(dim=(1, 2, 3))


def ssim_map(pred, target, channels='L'):
    """(B, H - 10, W - 10) fp64: the ssim map, averaged over the planes."""
    return plane_maps(planes(pred, channels), planes(target, channels))[0].mean(dim=1)


def ssim_means(pred, target, channels='L'):
    return plane_means(planes(pred, channels), planes(target, channels))


def _clamped_pow(v, w):
    """max(v, 0)^w with value 0 and slope 0 for v <= 0 (the discarded branch is evaluated at 1)."""
    pos = v > 0
    return torch.where(pos, torch.where(pos, v, torch.ones_like(v)) ** w, torch.zeros_like(v))


def ms_ssim_levels(pred, target, channels='L'):
    """[(mean ssim, mean cs, (h, w))] of the five levels; the PLANES are pooled (F.avg_pool2d(., 2) drops an odd row / column)."""
    x, y = planes(pred, channels), planes(target, channels)
    out = []
    for s in range(len(WEIGHTS)):
        out.append(plane_means(x, y) + (tuple(x.shape[-2:]),))
        if s + 1 < len(WEIGHTS):
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    return out


def ms_ssim(pred, target, channels='L'):
    """(B,) fp64: prod_{s<5} max(mean cs_s, 0)^w_s * max(mean ssim_5, 0)^w_5."""
    lv = ms_ssim_levels(pred, target, channels)
    ms = _clamped_pow(lv[-1][0], WEIGHTS[-1])
    for (_, cs, _), w in zip(lv[:-1], WEIGHTS[:-1]):
        ms = ms * _clamped_pow(cs, w)
    return ms


def fwd_bwd(pred, target, channels, upstream=None, kind='ssim'):
    """(value (B,), grad (B, 3, H, W)) in fp64: grad = d (sum_b upstream[b] value[b]) / d pred, upstream = ones by default;
    kind 'ssim' (the mean of the map), 'cs' (the mean of cs) or 'ms-ssim'."""
    p = pred.detach().double().requires_grad_(True)       # an fp64 leaf: the gradient of an fp32 leaf would be rounded to fp32
    if kind == 'ms-ssim':
        v = ms_ssim(p, target, channels)
    else:
        v = ssim_means(p, target, channels)[0 if kind == 'ssim' else 1]
    up = torch.ones_like(v) if upstream is None else upstream.double()
    grad, = torch.autograd.grad((v * up).sum(), p)
    return v.detach(), grad


def analytic_plane_grad(x, y, a, c):
    """The definition's three-map gradient of sum_b (a_b mean_ssim[b] + c_b mean_cs[b]) with respect to the planes x, written
    out by hand (no autograd): dP = adj(M) + 2 x adj(Exx) + y adj(Exy), adj the zero-padded full correlation with g."""
    B, P, H, W = x.shape
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    A2, B2 = mx * mx + my * my + C1, sxx + syy + C2
    l, cs = (2 * mx * my + C1) / A2, (2 * sxy + C2) / B2
    n = float(P * (H - TAPS + 1) * (W - TAPS + 1))
    a, c = a.double().view(B, 1, 1, 1) / n, c.double().view(B, 1, 1, 1) / n
    Exx = -(a * l + c) * (2 * sxy + C2) / (B2 * B2)
    Exy = 2 * (a * l + c) / B2
    M = a * cs * 2 * (my - l * mx) / A2 - 2 * mx * Exx - my * Exy
    g = window()

    def adj(m):
        q = F.conv_transpose2d(m.reshape(B * P, 1, H - TAPS + 1, W - TAPS + 1), g.view(1, 1, TAPS, 1))
        return F.conv_transpose2d(q, g.view(1, 1, 1, TAPS)).reshape(B, P, H, W)

    return adj(M) + 2 * x * adj(Exx) + y * adj(Exy)


def seeded_pair(seed, shape):
    """The test images: t, u = 0.05 + 0.9 rand from one CPU generator, target = t, pred = 0.85 t + 0.15 u (both inside (0, 1))."""
    g = torch.Generator().manual_seed(seed)
    t = 0.05 + 0.9 * torch.rand(*shape, generator=g)
    u = 0.05 + 0.9 * torch.rand(*shape, generator=g)
    return 0.85 * t + 0.15 * u, t


def near_flat_pair(seed, shape):
    """The pair on which an fp32 composition loses E[x^2] - mu^2: both images 0.9 + 0.001 rand."""
    g = torch.Generator().manual_seed(seed)
    return 0.9 + 0.001 * torch.rand(*shape, generator=g), 0.9 + 0.001 * torch.rand(*shape, generator=g)


_ORACLE = {}


def projection_oracle(sd, image, hist, seed, pixel_loss, steps, lr, noise_reg_weight, style_reg_weight, ssim_weight, dtype):
    """tests/noise_grad_ref.projection_oracle with the structure term: the same Adam loop on oracle.histogan_nets on the CPU in
    `dtype`, the per-step loss gaining ssim_weight * mean_b(1 - mean ssim(rgb, image)) of the L* plane.  SSIM itself is
    evaluated in fp64 on the `dtype` pixels (as the kernel evaluates it in fp64 on fp32 pixels) and cast back to `dtype`.
    Returns the per-step losses.  Cached per argument set."""
    from oracle import histogan_nets as N
    key = (seed, pixel_loss, steps, lr, noise_reg_weight, style_reg_weight, ssim_weight, dtype)
    if key in _ORACLE:
        return _ORACLE[key]
    sub = lambda p: {k[len(p) + 1:]: v.detach().cpu().to(dtype) for k, v in sd.items() if k.startswith(p + '.')}  # noqa: E731
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
        loss = rec + ssim_weight * (1.0 - ssim_means(rgb, img, 'L')[0].to(dtype)).mean()
        loss = loss + noise_reg_weight * noise.mean() ** 2 + style_reg_weight * styles.mean() ** 2 / styles.shape[1]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    _ORACLE[key] = losses
    return losses
