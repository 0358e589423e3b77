"""Shared pieces of the weighted-histogram tests (tests/test_hist_weight_cpu.py, tests/test_hist_weight_gpu.py): the
blocks under test, the binary-mask gather that pins a weighted histogram to the oracle, and a double-precision statement
of the definition of include/hg_hist.h (`weight`) for what the reference has no counterpart of.

Bars: the ones tests/test_hist_gpu.py and tests/test_hist_cpu_path.py apply to the unweighted kernels, max-norm relative."""
import numpy as np
import torch
import torch.nn.functional as F

FWD_TOL, BWD_TOL = 1e-5, 1e-4
EPS = 1e-6


def make_block(projection, device, **kw):
    from histogram_classes.LabHistBlock import LabHistBlock
    from histogram_classes.RGBuvHistBlock import RGBuvHistBlock
    from histogram_classes.rgChromaHistBlock import rgChromaHistBlock
    kw = dict(kw)
    if kw.get('hist_boundary') is not None:
        kw['hist_boundary'] = list(kw['hist_boundary'])
    cls = {'rgbuv': RGBuvHistBlock, 'rgchroma': rgChromaHistBlock, 'direct': LabHistBlock}[projection]
    return cls(device=device, **kw)


def oracle_hist(x, projection, **kw):
    """The oracle (the reference's arithmetic) of the block `make_block(projection, ...)`."""
    from oracle import rgbuv_hist as O
    if projection == 'rgbuv':
        return O.rgbuv_hist(x, **kw)
    return O.plane_hist(x, projection, **kw)


def random_mask(B, H, W, K, gen):
    """(B, H, W) float 0/1 masks with exactly K ones each, a different one per image."""
    m = torch.zeros(B, H * W)
    for b in range(B):
        m[b, torch.randperm(H * W, generator=gen)[:K]] = 1.0
    return m.reshape(B, H, W)


def gather_selected(t, mask, a, b):
    """t (B, C, H, W), mask (B, H, W) with a*b ones per image -> (B, C, a, b): the selected pixels in raster order."""
    B, C = t.shape[:2]
    sel = mask.reshape(B, -1) > 0
    return torch.stack([t[i].reshape(C, -1)[:, sel[i]] for i in range(B)]).reshape(B, C, a, b)


def _sampling_indices(size, h):
    return torch.from_numpy(np.linspace(0, size, h, endpoint=False).astype(np.int64))


def definition(x, w, projection='rgbuv', h=64, insz=150, resizing='interpolation', method='inverse-quadratic', sigma=0.02,
               intensity_scale=True, hist_boundary=None, green_only=False, pre_relu=False, proj_dtype=torch.float64):
    """The weighted histogram as include/hg_hist.h defines it, differentiable with respect to x by autograd; returns fp64.

    x (B, C>=3, H, W), w (B, H, W).  Stage 0 clamps x and w and resizes w like a colour channel; pixel n enters plane
    (u, v) with the weight w_n * I_y,n (w_n alone without intensity_scale, w_n * channel 0 for 'direct'); normalisation
    hist / (sum + 1e-6).  Kernel values, the accumulation and the normalisation are always double precision.
    Stage 0 is fp32: the definition names its arithmetic (aten's fp32 bilinear taps and fma form, which is what
    F.interpolate evaluates here); the taps' lambdas carry ~4e-6 of fp32 rounding, so a double-precision resize is
    another image at the 1e-4 level of the histogram, not a more exact evaluation of the same one.
    proj_dtype: precision of the projection (u, v, I_y).  float64 for the smooth kernels.  float32 for 'thresholding':
    there the definition is discontinuous in u -- the 0/1 window decision |u - b_i| <= eps/2 is taken on the fp32 value
    of u the reference computes (fp32 log - fp32 log), and a double-precision u (~1e-7 away) puts about one pixel in
    10^5 into another bin, which is a change of the definition, not a rounding error."""
    if hist_boundary is None:
        hist_boundary = [-3, 3] if projection == 'rgbuv' else [0, 1]
    lo, hi = sorted(hist_boundary)
    x = x.float()
    if pre_relu:
        x = F.relu(x)
    xw = torch.cat([torch.clamp(x[:, :3], 0, 1), torch.clamp(w.float(), 0, 1).unsqueeze(1)], dim=1)
    if xw.shape[2] > insz or xw.shape[3] > insz:
        if resizing == 'interpolation':
            xw = F.interpolate(xw, size=(insz, insz), mode='bilinear', align_corners=False)
        else:
            xw = xw.index_select(2, _sampling_indices(xw.shape[2], h)).index_select(3, _sampling_indices(xw.shape[3], h))
    xw = xw.to(proj_dtype)
    B = xw.shape[0]
    I, wn = xw[:, :3].reshape(B, 3, -1), xw[:, 3].reshape(B, -1)
    if projection == 'rgbuv':
        L = torch.log(I + EPS)
        r, g, b = L[:, 0], L[:, 1], L[:, 2]
        green = (g - r, g - b)
        planes = [green] if green_only else [(r - g, r - b), green, (b - r, b - g)]
        iy = torch.sqrt((I * I).sum(dim=1) + EPS) if intensity_scale else None
    elif projection == 'rgchroma':
        s = I.sum(dim=1) + EPS
        planes = [(I[:, 0] / s, I[:, 1] / s)]
        iy = torch.sqrt((I * I).sum(dim=1) + EPS) if intensity_scale else None
    else:
        planes = [(I[:, 1], I[:, 2])]
        iy = I[:, 0] if intensity_scale else None
    weight = (wn if iy is None else wn * iy).double()
    bins = torch.from_numpy(np.linspace(lo, hi, num=h))

    def kern(c):
        d = (c.double().unsqueeze(-1) - bins).abs()
        if method == 'thresholding':
            return (d <= (abs(lo) + abs(hi)) / h / 2).double()
        if method == 'RBF':
            return torch.exp(-(d * d) / sigma ** 2)
        return 1 / (1 + (d * d) / sigma ** 2)

    hs = [torch.bmm((kern(u) * weight.unsqueeze(-1)).transpose(1, 2), kern(v)) for u, v in planes]
    hist = torch.stack(hs, dim=1)
    return hist / (hist.sum(dim=(1, 2, 3)).view(-1, 1, 1, 1) + EPS)


def definition_fwd_bwd(x, w, grad_out, **kw):
    """(hist, grad_x) of `definition`, fp64 numpy; thresholding takes the fp32 projection (see `definition`)."""
    dt = torch.float32 if kw.get('method') == 'thresholding' else torch.float64
    xr = x.detach().clone().requires_grad_(True)
    hist = definition(xr, w, proj_dtype=dt, **kw)
    if hist.requires_grad:
        hist.backward(grad_out.double())
    gx = xr.grad if xr.grad is not None else torch.zeros_like(xr)
    return hist.detach().numpy(), gx.detach().double().numpy()


def sample_image(B, C, H, W, gen):
    """Generator-like input: values below 0 and above 1, exact zeros and ones."""
    x = torch.rand(B, C, H, W, generator=gen) * 1.2 - 0.1
    x[0, :, :3] = 0.0
    x[-1, :, 5:8, 5:8] = 1.0
    return x

