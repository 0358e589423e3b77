"""Shared reference of the `LabHistBlock(from_rgb=True)` tests (tests/test_lab_from_rgb_cpu.py, tests/test_lab_from_rgb_gpu.py):
the HG_PROJ_LAB definition of include/hg_hist.h restated in torch fp64 on the CPU, from the formulas and not from the code
under test.

  clamp -> resize (fp32: aten's bilinear taps are part of the definition, see tests/hist_weight_ref.py) -> per pixel, in fp64:
  c_lin = c/12.92 (c <= 0.04045) else ((c+0.055)/1.055)^2.4;  XYZ = M c_lin, every row of M divided by its sum;
  f(t) = cbrt(t) (t > (6/29)^3) else t/(3 (6/29)^2) + 4/29;  L = 116 f(Y) - 16, a = 500 (f(X)-f(Y)), b = 200 (f(Y)-f(Z));
  (Ln, an, bn) = (L/100, (a+128)/255, (b+128)/255), rounded ONCE to fp32 (a straight-through identity for autograd);
  then a `direct` pixel: (u, v) = (an, bn), weight Ln (1 without intensity_scale) times the map; fp64 kernels, contraction
  and normalisation.

Bars: those of tests/test_hist_planes_gpu.py, max-norm relative."""
import numpy as np
import torch
import torch.nn.functional as F

from hist_weight_ref import BWD_TOL, EPS, FWD_TOL, _sampling_indices  # noqa: F401

M = torch.tensor([[0.412453, 0.357580, 0.180423],
                  [0.212671, 0.715160, 0.072169],
                  [0.019334, 0.119193, 0.950227]], dtype=torch.float64)
MN = M / M.sum(dim=1, keepdim=True)
D = 6.0 / 29.0

# literals that do not come from this repository's code: sRGB -> CIE Lab (D65), to 1e-3 in Lab units
ANCHORS = (((1.0, 1.0, 1.0), (100.0, 0.0, 0.0)),
           ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
           ((1.0, 0.0, 0.0), (53.2406, 80.0942, 67.2015)),
           ((0.0, 1.0, 0.0), (87.7351, -86.1813, 83.1775)),
           ((0.0, 0.0, 1.0), (32.2957, 79.1870, -107.8617)),
           ((0.5, 0.5, 0.5), (53.3890, 0.0, 0.0)))


def srgb_to_lab(c):
    """(..., 3, N) fp64 sRGB -> (..., 3, N) fp64 normalised Lab, differentiable.  The branch a `where` discards is
    evaluated at 1 instead of at the pixel, so that its slope (infinite at 0 for the cube root) never meets the 0 of the mask."""
    c = c.double()
    hi = c > 0.04045
    lin = torch.where(hi, ((torch.where(hi, c, torch.ones_like(c)) + 0.055) / 1.055) ** 2.4, c / 12.92)
    xyz = torch.matmul(MN, lin)
    up = xyz > D ** 3
    f = torch.where(up, torch.where(up, xyz, torch.ones_like(xyz)) ** (1.0 / 3.0), xyz / (3 * D * D) + 4.0 / 29.0)
    fx, fy, fz = f[..., 0, :], f[..., 1, :], f[..., 2, :]
    L, a, b = 116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)
    return torch.stack([L / 100.0, (a + 128.0) / 255.0, (b + 128.0) / 255.0], dim=-2)


def lab_to_srgb(lab):
    """The exact inverse, clipped to [0, 1]: (..., 3, N) normalised Lab -> fp64 sRGB."""
    lab = lab.double()
    L, a, b = 100.0 * lab[..., 0, :], 255.0 * lab[..., 1, :] - 128.0, 255.0 * lab[..., 2, :] - 128.0
    fy = (L + 16.0) / 116.0
    f = torch.stack([fy + a / 500.0, fy, fy - b / 200.0], dim=-2)
    xyz = torch.where(f > D, f ** 3, 3 * D * D * (f - 4.0 / 29.0))
    lin = torch.matmul(torch.linalg.inv(MN), xyz)
    hi = lin > 0.04045 / 12.92
    c = torch.where(hi, 1.055 * torch.where(hi, lin, torch.ones_like(lin)) ** (1.0 / 2.4) - 0.055, 12.92 * lin)
    return c.clamp(0.0, 1.0)


def check_anchors():
    """The helper against the literals above; returns the largest deviation in Lab units."""
    worst = 0.0
    for rgb, lab in ANCHORS:
        n = srgb_to_lab(torch.tensor(rgb, dtype=torch.float64).reshape(3, 1)).reshape(3)
        got = (100.0 * n[0], 255.0 * n[1] - 128.0, 255.0 * n[2] - 128.0)
        worst = max(worst, max(abs(float(g) - e) for g, e in zip(got, lab)))
    return worst


def convert_image(x, inverse=False):
    """The stand-alone conversions on an image (B, 3, H, W) or (3, H, W): fp64 result (srgb_to_lab clamps its input)."""
    shp = x.shape
    flat = x.double().reshape(*shp[:-2], -1)
    out = lab_to_srgb(flat) if inverse else srgb_to_lab(flat.clamp(0.0, 1.0))
    return out.reshape(shp)


def stage0(x, w, h, insz, resizing):
    """clamp + resize of the image (and of the map, like one more colour channel), fp32: (B, 3, N) and (B, N) or None."""
    x = x.float()
    planes = [torch.clamp(x[:, :3], 0, 1)]
    if w is not None:
        w = w.float()
        planes.append(torch.clamp(w if w.dim() == 4 else w.unsqueeze(1), 0, 1))
    xw = torch.cat(planes, dim=1)
    if xw.shape[2] > insz or xw.shape[3] > insz:
        if resizing == 'interpolation':
            xw = F.interpolate(xw, size=(insz, insz), mode='bilinear', align_corners=False)
        else:
            xw = xw.index_select(2, _sampling_indices(xw.shape[2], h)).index_select(3, _sampling_indices(xw.shape[3], h))
    B = xw.shape[0]
    return xw[:, :3].reshape(B, 3, -1), (None if w is None else xw[:, 3].reshape(B, -1))


def rounded_lab(I):
    """(B, 3, N) fp32 sRGB -> fp64 tensor holding the fp32-rounded (Ln, an, bn); autograd sees the unrounded chain."""
    lab = srgb_to_lab(I)
    return lab + (lab.detach().float().double() - lab.detach())


def coordinates(x, h=64, insz=150, resizing='interpolation', **_):
    """The fp32 (an, bn) coordinates of every histogram pixel: (B, 2, N) fp64 tensor of fp32 values."""
    I, _w = stage0(x, None, h, insz, resizing)
    return rounded_lab(I)[:, 1:].detach()


def definition(x, w=None, h=64, insz=150, resizing='interpolation', method='inverse-quadratic', sigma=0.02,
               intensity_scale=False, hist_boundary=None):
    lo, hi = sorted(hist_boundary if hist_boundary is not None else [0, 1])
    I, wn = stage0(x, w, h, insz, resizing)
    lab = rounded_lab(I)
    weight = lab[:, 0] if intensity_scale else torch.ones_like(lab[:, 0])
    if wn is not None:
        weight = weight * wn.double()
    bins = torch.from_numpy(np.linspace(lo, hi, num=h))

    def kern(c):
        d = (c.unsqueeze(-1) - bins).abs()
        if method == 'thresholding':
            return (d <= (abs(lo) + abs(hi)) / h / 2).double()
        if method == 'RBF':
            return torch.exp(-(d * d) / sigma ** 2)
        return 1 / (1 + (d * d) / sigma ** 2)

    hist = torch.bmm((kern(lab[:, 1]) * weight.unsqueeze(-1)).transpose(1, 2), kern(lab[:, 2])).unsqueeze(1)
    return hist / (hist.sum(dim=(1, 2, 3)).view(-1, 1, 1, 1) + EPS)


def fwd_bwd(x, grad_out, w=None, weight_grad=False, **kw):
    """(hist, grad_x, grad_weight or None) of `definition` by fp64 autograd, as numpy fp64."""
    xr = x.detach().clone().requires_grad_(True)
    wr = None if w is None else w.detach().clone().requires_grad_(weight_grad)
    hist = definition(xr, wr, **kw)
    if hist.requires_grad:
        hist.backward(grad_out.double())
    gx = xr.grad if xr.grad is not None else torch.zeros_like(xr)
    gw = None
    if weight_grad:
        gw = (wr.grad if wr.grad is not None else torch.zeros_like(wr)).double().numpy()
    return hist.detach().numpy(), gx.double().numpy(), gw


def edge_image():
    """1x3x2x4: the six anchor colours, the knee of the transfer curve, and a pixel with components below 0 and above 1."""
    px = [rgb for rgb, _ in ANCHORS] + [(0.04045, 0.04045, 0.04045), (-0.1, 0.5, 1.2)]
    return torch.tensor(px, dtype=torch.float32).t().reshape(1, 3, 2, 4).contiguous()
