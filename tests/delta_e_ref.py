"""Test helper (NOT a test module): the colour differences of include/hg_post.h (hg_delta_e) restated in torch fp64 on the CPU,
from the published formula (Sharma, Wu, Dalal 2005) and not from the code under test, on top of tests/lab_ref.srgb_to_lab.

Every root and atan2 is `where`-guarded (the discarded branch is evaluated at a harmless point), so that autograd returns the
conventions of the definition -- slope 0 where a root's argument is 0 and for atan2 at the origin -- instead of NaN.

SHARMA: the published test pairs, (L, a, b), (L, a, b), dE00 to four decimals.  The bar for the helper is 1e-4 (the table's own
rounding is 5e-5)."""
import torch
import torch.nn.functional as F

import lab_ref

SHARMA = (
    ((50.0, 2.6772, -79.7751), (50.0, 0.0, -82.7485), 2.0425),
    ((50.0, 3.1571, -77.2803), (50.0, 0.0, -82.7485), 2.8615),
    ((50.0, 2.8361, -74.0200), (50.0, 0.0, -82.7485), 3.4412),
    ((50.0, -1.3802, -84.2814), (50.0, 0.0, -82.7485), 1.0000),
    ((50.0, -1.1848, -84.8006), (50.0, 0.0, -82.7485), 1.0000),
    ((50.0, -0.9009, -85.5211), (50.0, 0.0, -82.7485), 1.0000),
    ((50.0, 0.0, 0.0), (50.0, -1.0, 2.0), 2.3669),
    ((50.0, -1.0, 2.0), (50.0, 0.0, 0.0), 2.3669),
    ((50.0, 2.49, -0.001), (50.0, -2.49, 0.0009), 7.1792),
    ((50.0, 2.49, -0.001), (50.0, -2.49, 0.0010), 7.1792),
    ((50.0, 2.49, -0.001), (50.0, -2.49, 0.0011), 7.2195),
    ((50.0, 2.49, -0.001), (50.0, -2.49, 0.0012), 7.2195),
    ((50.0, -0.001, 2.49), (50.0, 0.0009, -2.49), 4.8045),
    ((50.0, -0.001, 2.49), (50.0, 0.0010, -2.49), 4.8045),
    ((50.0, -0.001, 2.49), (50.0, 0.0011, -2.49), 4.7461),
    ((50.0, 2.5, 0.0), (50.0, 0.0, -2.5), 4.3065),
    ((50.0, 2.5, 0.0), (73.0, 25.0, -18.0), 27.1492),
    ((50.0, 2.5, 0.0), (61.0, -5.0, 29.0), 22.8977),
    ((50.0, 2.5, 0.0), (56.0, -27.0, -3.0), 31.9030),
    ((50.0, 2.5, 0.0), (58.0, 24.0, 15.0), 19.4535),
    ((50.0, 2.5, 0.0), (50.0, 3.1736, 0.5854), 1.0000),
    ((50.0, 2.5, 0.0), (50.0, 3.2972, 0.0), 1.0000),
    ((50.0, 2.5, 0.0), (50.0, 1.8634, 0.5757), 1.0000),
    ((50.0, 2.5, 0.0), (50.0, 3.2592, 0.3350), 1.0000),
    ((60.2574, -34.0099, 36.2677), (60.4626, -34.1751, 39.4387), 1.2644),
)
SHARMA_TOL = 1e-4
KINDS = (76, 2000)


def _root(x):
    """sqrt with value 0 and slope 0 where the argument is not positive."""
    pos = x > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, x, torch.ones_like(x))), torch.zeros_like(x))


def _hue(y, x):
    """atan2(y, x) in degrees in [0, 360); value 0 and slope 0 at the origin."""
    origin = (x == 0) & (y == 0)
    h = torch.rad2deg(torch.atan2(torch.where(origin, torch.zeros_like(y), y), torch.where(origin, torch.ones_like(x), x)))
    return torch.where(h < 0, h + 360.0, h)


def _cosd(x):
    return torch.cos(torch.deg2rad(x))


def _sind(x):
    return torch.sin(torch.deg2rad(x))


def ciede2000_terms(lab1, lab2):
    """dE00 and the quantities the tests' condition is stated on: (dE, C'_1, C'_2, h'_1, h'_2), each (...,) fp64, from
    (..., 3) Lab triples in Lab units."""
    L1, a1, b1 = lab1[..., 0], lab1[..., 1], lab1[..., 2]
    L2, a2, b2 = lab2[..., 0], lab2[..., 1], lab2[..., 2]
    C1, C2 = _root(a1 * a1 + b1 * b1), _root(a2 * a2 + b2 * b2)
    Cm7 = ((C1 + C2) / 2) ** 7
    G = 0.5 * (1 - _root(Cm7 / (Cm7 + 25.0 ** 7)))
    a1p, a2p = (1 + G) * a1, (1 + G) * a2
    C1p, C2p = _root(a1p * a1p + b1 * b1), _root(a2p * a2p + b2 * b2)
    h1, h2 = _hue(b1, a1p), _hue(b2, a2p)
    grey = C1p * C2p == 0
    dh = h2 - h1
    dh = torch.where(dh > 180, dh - 360, torch.where(dh < -180, dh + 360, dh))
    dh = torch.where(grey, torch.zeros_like(dh), dh)
    dLp, dCp = L2 - L1, C2p - C1p
    dHp = 2 * _root(C1p * C2p) * _sind(dh / 2)
    Lm, Cmp = (L1 + L2) / 2, (C1p + C2p) / 2
    hs = h1 + h2
    hm = torch.where((h1 - h2).abs() <= 180, hs / 2, torch.where(hs < 360, (hs + 360) / 2, (hs - 360) / 2))
    hm = torch.where(grey, hs, hm)
    T = 1 - 0.17 * _cosd(hm - 30) + 0.24 * _cosd(2 * hm) + 0.32 * _cosd(3 * hm + 6) - 0.20 * _cosd(4 * hm - 63)
    dtheta = 30 * torch.exp(-(((hm - 275) / 25) ** 2))
    Cmp7 = Cmp ** 7
    RC = 2 * _root(Cmp7 / (Cmp7 + 25.0 ** 7))
    SL = 1 + 0.015 * (Lm - 50) ** 2 / torch.sqrt(20 + (Lm - 50) ** 2)
    SC, SH = 1 + 0.045 * Cmp, 1 + 0.015 * Cmp * T
    RT = -_sind(2 * dtheta) * RC
    tL, tC, tH = dLp / SL, dCp / SC, dHp / SH
    return _root(tL * tL + tC * tC + tH * tH + RT * tC * tH), C1p, C2p, h1, h2


def delta_e_lab(lab1, lab2, kind):
    """dE of (..., 3) fp64 Lab triples; kind 76 or 2000."""
    if kind == 76:
        d = lab1 - lab2
        return _root((d * d).sum(dim=-1))
    return ciede2000_terms(lab1, lab2)[0]


def check_sharma():
    """Largest deviation of the helper from the published dE00 values."""
    p1 = torch.tensor([p[0] for p in SHARMA], dtype=torch.float64)
    p2 = torch.tensor([p[1] for p in SHARMA], dtype=torch.float64)
    want = torch.tensor([p[2] for p in SHARMA], dtype=torch.float64)
    return float((delta_e_lab(p1, p2, 2000) - want).abs().max())


def image_lab(x):
    """(B, 3, H, W) sRGB of any float type -> (B, H, W, 3) fp64 Lab in Lab units of the pixels clamped to [0, 1]; differentiable
    (torch.clamp's mask is inclusive)."""
    B, _, H, W = x.shape
    n = lab_ref.srgb_to_lab(x.double().clamp(0.0, 1.0).reshape(B, 3, H * W))
    lab = torch.stack([100.0 * n[:, 0], 255.0 * n[:, 1] - 128.0, 255.0 * n[:, 2] - 128.0], dim=-1)
    return lab.reshape(B, H, W, 3)


def delta_e_map(pred, target, kind):
    """(B, H, W) fp64 dE of two (B, 3, H, W) sRGB images."""
    return delta_e_lab(image_lab(pred), image_lab(target), kind)


def delta_e_mean(pred, target, kind, weight=None):
    """(B,) fp64: sum w dE / sum w per sample (w clamped to [0, 1]; 0 when sum w = 0); weight (B, H, W) or None."""
    de = delta_e_map(pred, target, kind)
    if weight is None:
        return de.mean(dim=(1, 2))
    w = weight.double().clamp(0.0, 1.0)
    sw = w.sum(dim=(1, 2))
    ok = sw > 0
    return torch.where(ok, (w * de).sum(dim=(1, 2)) / torch.where(ok, sw, torch.ones_like(sw)), torch.zeros_like(sw))


def fwd_bwd(pred, target, kind, weight=None, upstream=None):
    """(map, mean, grad) in fp64: grad = d (sum_b upstream[b] mean[b]) / d pred, upstream = ones by default."""
    p = pred.detach().double().requires_grad_(True)       # an fp64 leaf: the gradient of an fp32 leaf would be rounded to fp32
    mean = delta_e_mean(p, target, kind, weight)
    up = torch.ones_like(mean) if upstream is None else upstream.double()
    grad, = torch.autograd.grad((mean * up).sum(), p)
    return delta_e_map(pred, target, kind).detach(), mean.detach(), grad.double()


def condition(pred, target):
    """What a comparison of two correct fp64 evaluations needs (the quantities are discontinuous or have unbounded slopes at
    these places): (smallest dE00, smallest dE76, smallest C' of either pixel, smallest | 180 - |h'_2 - h'_1| | in degrees)."""
    l1, l2 = image_lab(pred), image_lab(target)
    de, c1, c2, h1, h2 = ciede2000_terms(l1, l2)
    return (float(de.min()), float(delta_e_lab(l1, l2, 76).min()), float(torch.minimum(c1, c2).min()),
            float((180 - (h2 - h1).abs()).abs().min()))


def excluded_share(pred, target, mask=None):
    """Share of the (selected) pixels with dE < 1e-2, min(C'_1, C'_2) < 1e-2 or a hue difference within 1e-2 degrees of 180."""
    l1, l2 = image_lab(pred), image_lab(target)
    de, c1, c2, h1, h2 = ciede2000_terms(l1, l2)
    bad = (de < 1e-2) | (delta_e_lab(l1, l2, 76) < 1e-2) | (torch.minimum(c1, c2) < 1e-2) | ((180 - (h2 - h1).abs()).abs() < 1e-2)
    if mask is not None:
        bad = bad & mask
        return float(bad.sum()) / max(float(mask.sum()), 1.0)
    return float(bad.double().mean())


def seeded_pair(seed, shape):
    """The test images: t, u = 0.05 + 0.9 rand from one CPU generator, pred = 0.85 t + 0.15 u (both inside (0, 1))."""
    g = torch.Generator().manual_seed(seed)
    t = 0.05 + 0.9 * torch.rand(*shape, generator=g)
    u = 0.05 + 0.9 * torch.rand(*shape, generator=g)
    return 0.85 * t + 0.15 * u, t


_ORACLE = {}


def projection_oracle(sd, image, hist, seed, pixel_loss, steps, lr, noise_reg_weight, style_reg_weight, delta_e_weight,
                      delta_e_kind, dtype):
    """tests/noise_grad_ref.projection_oracle with the colour term: the same Adam loop on oracle.histogan_nets on the CPU in
    `dtype`, the per-step loss gaining delta_e_weight * mean_b(delta_e_mean(rgb, image)).  dE itself is evaluated in fp64 on
    the `dtype` pixels (as the kernel evaluates it in fp64 on fp32 pixels) and its mean is cast back to `dtype`.  Returns
    (losses, renders): the per-step losses and the image rendered at every step (detached).  Cached per argument set."""
    from oracle import histogan_nets as N
    key = (seed, pixel_loss, steps, lr, noise_reg_weight, style_reg_weight, delta_e_weight, delta_e_kind, dtype)
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
    losses, renders = [], []
    for _ in range(steps):
        opt.zero_grad()
        w = torch.stack([N.vectorizer(sS, styles[:, i, :], 'net') for i in range(L - 2)], dim=1)
        rgb = N.generator(sG, w, torch.stack((hw, hw), dim=1), noise, L)
        rec = (img - rgb).abs().mean() if pixel_loss == 'L1' else F.mse_loss(img, rgb)
        loss = rec + delta_e_weight * delta_e_mean(rgb, img, delta_e_kind).to(dtype).mean()
        loss = loss + noise_reg_weight * noise.mean() ** 2 + style_reg_weight * styles.mean() ** 2 / styles.shape[1]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        renders.append(rgb.detach().clone())
    _ORACLE[key] = (losses, renders)
    return _ORACLE[key]

