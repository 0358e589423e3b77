"""Full-resolution output of ReHistoGAN on the MI355X kernels of include/hg_post.h.

The reference's `rehistoGAN.py --generate` offers two ways to carry its 256x256 result back to the photo
(ReHistoGAN/rehistoGAN.py:1135-1165): the Laplacian-pyramid detail swap of utils/pyramid_upsampling.py on top of the
MATLAB-bicubic utils/imresize.py, and the Monge-Kantorovich linear colour transfer of utils/color_transfer_MKL.py.  Both
are numpy / OpenCV in float64 there; here every pass over the image is a HIP kernel on the caller's stream, and only the
host-built resize tables (fp64, passed as fp32) and the 3x3 algebra of MKL stay on the host.

Device layouts: float images are (C, H, W) -- any strides -- and come back contiguous; uint8 images are (H, W, C), as
PIL and the reference's uint8 path hold them.  The drop-ins at the reference's import paths (utils/imresize.py,
utils/pyramid_upsampling.py, utils/color_transfer_MKL.py) convert to and from the reference's host types around these.

Also here, with no counterpart in the reference: the sRGB <-> CIE Lab conversions, and the CIE colour difference between
two sRGB images (delta_e, delta_e_map: dE76 and CIEDE2000) as a differentiable loss and as the metric reported for
recolourings; SSIM / MS-SSIM of the lightness plane or of the components (ssim, ssim_map, ms_ssim), the structure term
and the number reported for "structure preserved under recolouring"; and the iterative distribution transfer
(color_transfer_idt, idt_rotations), the nonlinear colour transfer that reaches the target distributions -- bimodal, skewed,
saturated -- an affine map cannot; and palettes (palette, paired_palette, palette_labels, match_palettes, palette_histogram):
an image described by K colours, and color_transfer_palette, the third transfer, between the two -- every pixel moves by a
smooth blend of per-cluster shifts, so colour regions move independently and flat regions stay flat; and 3D colour LUTs
(include/hg_lut.h: lut_fit, lut_apply, lut_identity, lut_bake, lut_compose, save_cube, load_cube), the object people who
grade colour exchange: the recolouring as a function of colour alone, fitted once on the 256x256 pair, applied to a photo, a
clip or a folder in one memory-bound pass, and written as a .cube file every grading tool reads -- differentiable on request
(lut_apply(differentiable=True), lut_smoothness), so that lut_refine can pull a LUT towards a target histogram; and regrain
(include/hg_regrain.h: regrain, regrain_levels), the second half of the method color_transfer_idt comes from: the colours of a
transferred picture on the gradient field of the original photo, a multi-level damped Jacobi solve at the photo's full size
that removes the grain a distribution transfer leaves on flat regions.
"""
import ctypes
from collections import namedtuple
from functools import lru_cache
from math import ceil

import numpy as np
import torch

from ._lib import check, lib, need_gpu, on_device, ptr, raw_stream, workspace

EPS = 2.2204e-16          # utils/color_transfer_MKL.py:3


# ---- host: the resize tables (utils/imresize.py:21-55) ----------------------------------------------------------------
def cubic(x):
    """Keys' cubic with a = -0.5, MATLAB's bicubic kernel."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    a2, a3 = a * a, a * a * a
    return (1.5 * a3 - 2.5 * a2 + 1) * (a <= 1) + (-0.5 * a3 + 2.5 * a2 - 4 * a + 2) * ((a > 1) & (a <= 2))


def triangle(x):
    """The bilinear ('triangle') kernel, 1 - |x| on [-1, 1]."""
    x = np.asarray(x, dtype=np.float64)
    return (x + 1) * ((x >= -1) & (x < 0)) + (1 - x) * ((x >= 0) & (x <= 1))


KERNELS = {'bicubic': cubic, 'bilinear': triangle}
KERNEL_WIDTH = 4.0        # the reference widens every kernel to 4 taps, the triangle included


def contributions(in_length, out_length, scale, kernel, k_width):
    """(weights, indices), each (out_length, taps): output sample i is sum_t weights[i, t] * x[indices[i, t]].
    Output centre i (1-based) maps to u = i/scale + (1 - 1/scale)/2 in the input; P = ceil(width) + 2 taps start at
    floor(u - width/2); down-scaling (scale < 1) stretches the kernel by 1/scale.  Rows are normalised, indices outside
    [0, in_length) fold with period 2*in_length repeating the edge sample, and taps that are zero for every output
    are dropped.  fp64 throughout."""
    if scale < 1:
        width = k_width / scale
        h = lambda t: scale * kernel(scale * t)  # noqa: E731
    else:
        width, h = k_width, kernel
    u = np.arange(1, out_length + 1, dtype=np.float64) / scale + 0.5 * (1 - 1 / scale)
    first = np.floor(u - width / 2)
    taps = int(ceil(width)) + 2
    idx = (first[:, None] + np.arange(taps) - 1).astype(np.int32)
    w = h(u[:, None] - idx - 1)
    w = w / w.sum(axis=1, keepdims=True)
    fold = np.concatenate([np.arange(in_length), np.arange(in_length - 1, -1, -1)]).astype(np.int32)
    idx = fold[np.mod(idx, fold.size)]
    keep = np.any(w != 0, axis=0)
    return w[:, keep], idx[:, keep]


def resize_plan(in_hw, output_shape=None, scalar_scale=None):
    """(out_hw, scale): the reference's deriveSizeFromScale / deriveScaleFromSize (utils/imresize.py:8-19)."""
    if scalar_scale is not None:
        s = float(scalar_scale)
        return [int(ceil(s * in_hw[k])) for k in range(2)], [s, s]
    if output_shape is None:
        raise ValueError('imresize: give output_shape or scalar_scale')
    out = [int(output_shape[0]), int(output_shape[1])]
    return out, [1.0 * out[k] / in_hw[k] for k in range(2)]


@lru_cache(maxsize=64)
def _tables(n_in, n_out, scale, method, device):
    w, i = contributions(n_in, n_out, scale, KERNELS[method], KERNEL_WIDTH)
    dev = torch.device(device)
    return (torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(i, dtype=np.int32)).to(dev), w.shape[1])


_FOUND = 'expects a tensor on the GPU'     # need_gpu's wording here


# ---- the argument rules of the conversions, the colour difference and SSIM (no HIP call is made) ----------------------------
# A function that refuses an input for more than one reason raises what needs no device (ValueError) first, then need_gpu.
def _rgb_batch(t, what, name=None):
    """The rule "a float RGB image or batch": (single, t as (B, 3, H, W)).  name: 'pred' / 'target', for the message."""
    if not torch.is_tensor(t) or t.dim() not in (3, 4) or t.shape[-3] != 3 or not t.is_floating_point():
        got = f'{t.dtype} {tuple(t.shape)}' if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f'{what}: {"expected" if name is None else name + " must be"} a float (B, 3, H, W) or (3, H, W) tensor, '
                         f'got {got}')
    single = t.dim() == 3
    return single, (t.unsqueeze(0) if single else t)


def _rgb_pair(pred, target, what):
    """The rule "pred and target: two such images of one shape and device": (single, pred (B, 3, H, W), target)."""
    single, p4 = _rgb_batch(pred, what, 'pred')
    _, t4 = _rgb_batch(target, what, 'target')
    if p4.shape != t4.shape or p4.device != t4.device:
        raise ValueError(f'{what}: pred and target must have one shape and device, got {tuple(p4.shape)} on {p4.device} and '
                         f'{tuple(t4.shape)} on {t4.device}')
    return single, p4, t4


def _detached_f32(t):
    """`t` as the kernels read it here: detached, fp32 (the same storage when it already is), any strides."""
    t = t.detach()
    return t if t.dtype == torch.float32 else t.float()


# ---- device: resize ---------------------------------------------------------------------------------------------------
def _resize_axis(x, x_u8, xs, C, H, W, axis, out, out_u8, os_, n_out, scale, method, clamp):
    wt, ind, taps = _tables(H if axis == 0 else W, n_out, scale, method, str(x.device))
    check(lib.hg_resize_axis(x.data_ptr(), int(x_u8), xs[0], xs[1], xs[2], int(clamp), out.data_ptr(), int(out_u8),
                             os_[0], os_[1], os_[2], C, H, W, axis, wt.data_ptr(), ind.data_ptr(), n_out, taps,
                             raw_stream(x.device)), 'hg_resize_axis')


def imresize(x, output_shape=None, scalar_scale=None, method='bicubic', clamp=False):
    """MATLAB imresize (utils/imresize.py:98-136) on the GPU.  x: float (C, H, W) / (H, W), any strides, or uint8
    (H, W, C) / (H, W).  Returns fp32 (C, H', W') / (H', W') contiguous, or uint8 (H', W', C) / (H', W') with the
    reference's clip + round-half-to-even after EACH pass (its uint8 path rounds the intermediate too).  The axis with
    the smaller scale is resized first (the reference's argsort).  clamp: clamp the input to [0, 1] as it is read."""
    need_gpu(x, 'imresize', _FOUND)
    if method not in KERNELS:
        raise ValueError(f"imresize: method must be 'bicubic' or 'bilinear', not {method!r}")
    u8 = x.dtype == torch.uint8
    if not u8 and x.dtype != torch.float32:
        x = x.float()
    if x.dim() not in (2, 3):
        raise ValueError(f'imresize: expects a 2-D or 3-D image, got shape {tuple(x.shape)}')
    flat = x.dim() == 2
    if u8:
        v = x.unsqueeze(2) if flat else x
        H, W, C = v.shape
        xs = (v.stride(2), v.stride(0), v.stride(1))
    else:
        v = x.unsqueeze(0) if flat else x
        C, H, W = v.shape
        xs = (v.stride(0), v.stride(1), v.stride(2))
    (Ho, Wo), scale = resize_plan((H, W), output_shape, scalar_scale)
    order = [0, 1] if scale[0] <= scale[1] else [1, 0]
    cur = [H, W]
    src, src_s = v, xs
    with on_device(x.device):
        for step, axis in enumerate(order):
            ih, iw = cur
            cur[axis] = (Ho, Wo)[axis]
            h, w = cur
            if u8:
                dst = torch.empty((h, w, C), dtype=torch.uint8, device=x.device)
                ds = (1, w * C, C)
            else:
                dst = torch.empty((C, h, w), dtype=torch.float32, device=x.device)
                ds = (h * w, w, 1)
            _resize_axis(src, u8, src_s, C, ih, iw, axis, dst, u8, ds, cur[axis], scale[axis], method,
                         clamp and step == 0)
            src, src_s = dst, ds
    if flat:
        return src[:, :, 0] if u8 else src[0]
    return src


# ---- device: layout conversions -----------------------------------------------------------------------------------------
def u8_hwc_to_float(x):
    """uint8 (H, W, C) -> fp32 (C, H, W) = x / 255 (torchvision ToTensor)."""
    need_gpu(x, 'u8_hwc_to_float', _FOUND)
    x = x.contiguous()
    H, W, C = x.shape
    out = torch.empty((C, H, W), dtype=torch.float32, device=x.device)
    with on_device(x.device):
        check(lib.hg_u8_hwc_to_f32(x.data_ptr(), out.data_ptr(), C, H * W, raw_stream(x.device)), 'hg_u8_hwc_to_f32')
    return out


def float_to_u8_hwc(x):
    """fp32 (C, H, W) -> uint8 (H, W, C) = clamp(x*255 + 0.5, 0, 255) truncated (torchvision save_image)."""
    need_gpu(x, 'float_to_u8_hwc', _FOUND)
    x = x.float().contiguous()
    C, H, W = x.shape
    out = torch.empty((H, W, C), dtype=torch.uint8, device=x.device)
    with on_device(x.device):
        check(lib.hg_f32_to_u8_hwc(x.data_ptr(), out.data_ptr(), C, H * W, raw_stream(x.device)), 'hg_f32_to_u8_hwc')
    return out


# ---- device: sRGB <-> normalised CIE Lab ------------------------------------------------------------------------------
def _lab_convert(x, fn, what):
    if torch.is_tensor(x) and x.requires_grad:      # before any HIP call
        raise ValueError(f'{what} is not differentiable (a data-side tool): the input requires grad.  For a Lab histogram of '
                         f'an sRGB image with a gradient use histogram_classes.LabHistBlock(from_rgb=True)')
    single, x4 = _rgb_batch(x, what)
    need_gpu(x4, what, _FOUND)
    x4 = _detached_f32(x4)
    B, _, H, W = x4.shape
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=x.device)
    with on_device(x.device):
        check(fn(x4.data_ptr(), *x4.stride(), out.data_ptr(), B, H, W, raw_stream(x.device)), what)
    return out[0] if single else out


def srgb_to_lab(x):
    """sRGB float (B, 3, H, W) or (3, H, W), any strides -> fp32 contiguous normalised CIE Lab (L/100, (a+128)/255,
    (b+128)/255): what LabHistBlock() bins and what LabHistBlock(from_rgb=True) computes per pixel (include/hg_post.h,
    hg_srgb_to_lab: the input is clamped to [0, 1]; fp64, rounded once).  Not differentiable: a tensor that requires grad
    raises ValueError."""
    return _lab_convert(x, lib.hg_srgb_to_lab, 'srgb_to_lab')


def lab_to_srgb(x):
    """The exact inverse of srgb_to_lab, clipped to [0, 1] (hg_lab_to_srgb): normalised Lab -> sRGB, e.g. to save what a
    network trained on Lab images generates.  Not differentiable."""
    return _lab_convert(x, lib.hg_lab_to_srgb, 'lab_to_srgb')


# ---- device: CIE colour difference (hg_delta_e) -----------------------------------------------------------------------
_DE_KINDS = {'76': 76, '2000': 2000, 76: 76, 2000: 2000}


def delta_e_kind(kind, what='delta_e'):
    """'76' | '2000' | 76 | 2000 -> the C ABI's integer; anything else raises ValueError (no HIP call is made)."""
    try:
        if isinstance(kind, bool):
            raise KeyError(kind)
        return _DE_KINDS[kind]
    except (KeyError, TypeError):
        raise ValueError(f"{what}: kind must be '76' or '2000' (dE76, CIEDE2000), not {kind!r}") from None


def _delta_e_launch(pred, target, weight, kind, want_map, want_grad, what):
    """One hg_delta_e call on a (B, 3, H, W) pair on the GPU (_de_batched's): (mean (B,), map (B, H, W) or None, grad
    (B, 3, H, W) or None), fp32."""
    x1, x2 = _detached_f32(pred), _detached_f32(target)
    B, _, H, W = x1.shape
    w, wstr = None, (0, 0, 0)
    if weight is not None:
        need_gpu(weight, what, _FOUND)
        w = weight
        if w.dim() == 4 and w.shape[1] == 1:
            w = w[:, 0]
        if tuple(w.shape) != (B, H, W) or not w.is_floating_point() or w.device != x1.device:
            raise ValueError(f'{what}: weight must be a float (B, H, W) or (B, 1, H, W) map = {(B, H, W)} on {x1.device}, got '
                             f'{weight.dtype} {tuple(weight.shape)} on {weight.device}')
        w = _detached_f32(w)
        wstr = w.stride()
    dev = x1.device
    with on_device(dev):
        mean = torch.empty((B,), dtype=torch.float32, device=dev)
        dmap = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_map else None
        grad = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if want_grad else None
        nb = lib.hg_delta_e_workspace_bytes(B, H, W)
        ws = workspace(nb, dev)
        check(lib.hg_delta_e(x1.data_ptr(), *x1.stride(), x2.data_ptr(), *x2.stride(), ptr(w), *wstr, kind, mean.data_ptr(),
                             ptr(dmap), ptr(grad), B, H, W, ws.data_ptr(), nb, raw_stream(dev)), 'hg_delta_e')
    return mean, dmap, grad


class DeltaEFunction(torch.autograd.Function):
    """mean dE per sample; the gradient for `pred` is computed in the forward (one fused launch, as HellingerFunction) and
    saved, the backward scales it by the upstream vector.  target and weight get no gradient."""

    @staticmethod
    def forward(ctx, pred, target, weight, kind):
        want = ctx.needs_input_grad[0]
        mean, _, grad = _delta_e_launch(pred, target, weight, kind, False, want, 'delta_e')
        ctx.dtype = pred.dtype
        if want:
            ctx.save_for_backward(grad)
        return mean

    @staticmethod
    def backward(ctx, up):
        (grad,) = ctx.saved_tensors
        return (grad * up[:, None, None, None]).to(ctx.dtype), None, None, None


def _de_batched(pred, target, what):
    """Every refusal of the images of delta_e / delta_e_map: (single, pred (B, 3, H, W), target), on the GPU."""
    single, p4, t4 = _rgb_pair(pred, target, what)
    need_gpu(p4, what, _FOUND)
    return single, p4, t4


def delta_e(pred, target, kind='2000', weight=None):
    """The CIE colour difference between two sRGB images as a loss: fp32 (B,) per-sample means of dE over the pixels (a
    0-dim tensor for (3, H, W) inputs), in Lab units.  kind: '2000' (CIEDE2000, kL = kC = kH = 1) or '76' (the Euclidean
    distance in Lab).  pred, target: float (B, 3, H, W) or (3, H, W), any strides, clamped to [0, 1] as they are read; both go
    through the chain of srgb_to_lab in fp64 without its rounding (include/hg_post.h, hg_delta_e, states every formula and
    the conventions at the singular points).  weight: optional (B, H, W) / (B, 1, H, W) map (for (3, H, W) inputs also
    (H, W)), clamped to [0, 1]: the mean becomes sum w dE / sum w, and 0 for an all-zero map.

    Differentiable with respect to `pred` (finite everywhere; zero where pred == target and for components outside [0, 1]);
    target and weight get no gradient, and a weight that requires grad raises ValueError."""
    k = delta_e_kind(kind)
    if torch.is_tensor(weight) and weight.requires_grad:          # before any HIP call
        raise ValueError('delta_e: the weight map gets no gradient, but it requires grad; pass weight.detach()')
    single, p4, t4 = _de_batched(pred, target, 'delta_e')
    if weight is not None and single and torch.is_tensor(weight) and weight.dim() == 2:
        weight = weight.unsqueeze(0)
    out = DeltaEFunction.apply(p4, t4, weight, k)
    return out[0] if single else out


def delta_e_map(pred, target, kind='2000'):
    """The per-pixel dE of delta_e: fp32 (B, H, W), or (H, W) for (3, H, W) inputs.  Not differentiable: the result carries no
    graph whatever the inputs require."""
    k = delta_e_kind(kind, 'delta_e_map')
    single, p4, t4 = _de_batched(pred, target, 'delta_e_map')
    _, dmap, _ = _delta_e_launch(p4, t4, None, k, True, False, 'delta_e_map')
    return dmap[0] if single else dmap


# ---- device: SSIM and MS-SSIM (hg_ssim_fwd, hg_ssim_bwd) --------------------------------------------------------------
SSIM_TILE = 32                    # hg_ssim_tile(): a workgroup's tile of the map (forward) and of the input (backward)
SSIM_FINISH_THREADS = 256         # hg_ssim_finish_threads(): thread t of a sample's finish block sums partials t, t + 256, ...
SSIM_WINDOW = 11
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_SSIM_MIN_SIZE = SSIM_WINDOW << (len(MS_SSIM_WEIGHTS) - 1)          # 176 -> 88 -> 44 -> 22 -> 11
_SSIM_MODES = {'L': 0, 'rgb': 1}                  # HG_SSIM_L, HG_SSIM_RGB; + 2: HG_SSIM_PLANES1, HG_SSIM_PLANES3


def ssim_channels(channels, what='ssim'):
    """'L' | 'rgb' -> the C ABI's mode; anything else raises ValueError (no HIP call is made)."""
    if not isinstance(channels, str) or channels not in _SSIM_MODES:
        raise ValueError(f"{what}: channels must be 'L' (the lightness plane) or 'rgb' (the three components), not {channels!r}")
    return _SSIM_MODES[channels]


def _ssim_images(pred, target, channels, what, min_size):
    """Every refusal of ssim / ssim_map / ms_ssim, before any HIP call: (mode, single, pred (B, 3, H, W), target)."""
    mode = ssim_channels(channels, what)
    single, p4, t4 = _rgb_pair(pred, target, what)
    B, _, H, W = p4.shape
    if min(H, W) < min_size:
        raise ValueError(f'{what}: images must be at least {min_size} x {min_size}, got {H} x {W}')
    if not 1 <= B <= 65535:
        raise ValueError(f'{what}: the batch must be 1 .. 65535, got {B}')
    need_gpu(p4, what, _FOUND)
    return mode, single, p4, t4


def _ssim_fwd(x1, x2, mode, want_map=False, want_pool=False):
    """One hg_ssim_fwd call: x1, x2 fp32 (B, 3, H, W) images (mode 0, 1) or contiguous fp64 (B, planes, H, W) planes (mode 2,
    3) -> (means fp64 (B, 2) = (mean ssim, mean cs), map fp32 (B, H-10, W-10) or None, (pooled planes of x1, of x2) or None)."""
    B, _, H, W = x1.shape
    planes = 3 if mode in (1, 3) else 1
    dev = x1.device
    with on_device(dev):
        means = torch.empty((B, 2), dtype=torch.float64, device=dev)
        smap = torch.empty((B, H - 10, W - 10), dtype=torch.float32, device=dev) if want_map else None
        pools = tuple(torch.empty((B, planes, H // 2, W // 2), dtype=torch.float64, device=dev) for _ in range(2)) if want_pool else None
        nb = lib.hg_ssim_workspace_bytes(B, H, W)
        ws = workspace(nb, dev)
        pool1, pool2 = pools or (None, None)
        check(lib.hg_ssim_fwd(x1.data_ptr(), *x1.stride(), x2.data_ptr(), *x2.stride(), mode, means.data_ptr(), ptr(smap),
                              ptr(pool1), ptr(pool2), B, H, W, ws.data_ptr(), nb, raw_stream(dev)), 'hg_ssim_fwd')
    return means, smap, pools


def _ssim_bwd(x1, x2, mode, coef, coarse=None):
    """One hg_ssim_bwd call: the gradient of sum_b (coef[b, 0] mean_ssim[b] + coef[b, 1] mean_cs[b]) -- coef fp64 (B, 2) on
    the device -- plus the pooled planes' gradient `coarse`: fp32 (B, 3, H, W) for the images, fp64 for planes."""
    B, _, H, W = x1.shape
    dev = x1.device
    with on_device(dev):
        grad = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if mode < 2 else torch.empty_like(x1)
        check(lib.hg_ssim_bwd(x1.data_ptr(), *x1.stride(), x2.data_ptr(), *x2.stride(), mode, coef.data_ptr(), ptr(coarse),
                              grad.data_ptr(), B, H, W, raw_stream(dev)), 'hg_ssim_bwd')
    return grad


class SsimFunction(torch.autograd.Function):
    """Mean ssim per sample.  Only the images are kept: the backward kernel recomputes the moments, with the upstream vector
    as its coefficients, so the gradient is rounded once.  target gets no gradient."""

    @staticmethod
    def forward(ctx, pred, target, mode):
        x1, x2 = _detached_f32(pred), _detached_f32(target)
        means, _, _ = _ssim_fwd(x1, x2, mode)
        ctx.mode, ctx.dtype = mode, pred.dtype
        ctx.save_for_backward(x1, x2)
        return means[:, 0].float()

    @staticmethod
    def backward(ctx, up):
        x1, x2 = ctx.saved_tensors
        u = up.double()
        return _ssim_bwd(x1, x2, ctx.mode, torch.stack((u, torch.zeros_like(u)), dim=1)).to(ctx.dtype), None, None


class MsSsimFunction(torch.autograd.Function):
    """ms = prod_{s<5} max(mean cs_s, 0)^w_s * max(mean ssim_5, 0)^w_5: five forward launches, each writing the next level's
    pooled fp64 planes, and five backward launches from the coarsest level up; the per-level coefficients come from the fp64
    means by torch ops on the device.  Kept between the two: the images, the pooled planes and the means."""

    @staticmethod
    def forward(ctx, pred, target, mode):
        levels = len(MS_SSIM_WEIGHTS)
        planes = [(_detached_f32(pred), _detached_f32(target))]
        means = []
        for s in range(levels):
            m, _, pools = _ssim_fwd(*planes[s], mode if s == 0 else mode + 2, want_pool=s + 1 < levels)
            means.append(m)
            if pools is not None:
                planes.append(pools)
        means = torch.stack(means)                                              # (levels, B, 2)
        w = torch.tensor(MS_SSIM_WEIGHTS, dtype=torch.float64, device=means.device)[:, None]
        base = torch.cat((means[:-1, :, 1], means[-1:, :, 0]))                  # cs of levels 1-4, ssim of level 5
        ms = torch.prod(base.clamp(min=0.0) ** w, dim=0)
        ctx.mode, ctx.dtype = mode, pred.dtype
        ctx.save_for_backward(base, ms, w, *[t for pair in planes for t in pair])
        return ms.float()

    @staticmethod
    def backward(ctx, up):
        base, ms, w, *flat = ctx.saved_tensors
        levels = len(MS_SSIM_WEIGHTS)
        pos = base > 0                                                          # slope 0 at the clamp
        slope = torch.where(pos, w * ms / torch.where(pos, base, torch.ones_like(base)), torch.zeros_like(base)) * up.double()
        zero = torch.zeros_like(slope[0])
        g = None
        for s in reversed(range(levels)):
            coef = torch.stack((slope[s], zero) if s == levels - 1 else (zero, slope[s]), dim=1)
            g = _ssim_bwd(flat[2 * s], flat[2 * s + 1], ctx.mode if s == 0 else ctx.mode + 2, coef, g)
        return g.to(ctx.dtype), None, None


def ssim(pred, target, channels='L'):
    """SSIM between two sRGB images as a loss term: fp32 (B,) per-sample means of the ssim map (a 0-dim tensor for (3, H, W)
    inputs); 1 for equal images.  pred, target: float (B, 3, H, W) or (3, H, W), any strides, clamped to [0, 1] as they are
    read.  channels: 'L' -- one plane, CIE L* / 100 by the chain of srgb_to_lab in fp64 without its rounding -- or 'rgb' -- the
    three components, averaged.  11-tap Gaussian window (sigma 1.5), valid positions only, C1 = 1e-4, C2 = 9e-4;
    include/hg_post.h (hg_ssim_fwd) states every formula.  H, W >= 11.

    Differentiable with respect to `pred` (finite everywhere; exactly zero for equal images and for components outside
    [0, 1]); target gets no gradient."""
    mode, single, p4, t4 = _ssim_images(pred, target, channels, 'ssim', SSIM_WINDOW)
    out = SsimFunction.apply(p4, t4, mode)
    return out[0] if single else out


def ssim_map(pred, target, channels='L'):
    """The ssim map of `ssim`: fp32 (B, H - 10, W - 10), or (H - 10, W - 10) for (3, H, W) inputs; with 'rgb' the mean over the
    three planes.  Not differentiable: the result carries no graph whatever the inputs require."""
    mode, single, p4, t4 = _ssim_images(pred, target, channels, 'ssim_map', SSIM_WINDOW)
    _, smap, _ = _ssim_fwd(_detached_f32(p4), _detached_f32(t4), mode, want_map=True)
    return smap[0] if single else smap


def ms_ssim(pred, target, channels='L'):
    """Multi-scale SSIM (Wang, Simoncelli, Bovik 2003): fp32 (B,) (0-dim for (3, H, W) inputs).  Five levels with the weights
    MS_SSIM_WEIGHTS; between levels the PLANES of `ssim` are averaged over 2 x 2 blocks in fp64 (an odd trailing row or column
    is dropped); ms = prod_{s<5} max(mean cs_s, 0)^w_s * max(mean ssim_5, 0)^w_5 with slope 0 at the clamp.  min(H, W) >= 176.
    Differentiable with respect to `pred`."""
    mode, single, p4, t4 = _ssim_images(pred, target, channels, 'ms_ssim', MS_SSIM_MIN_SIZE)
    out = MsSsimFunction.apply(p4, t4, mode)
    return out[0] if single else out


# ---- device: pyramids -------------------------------------------------------------------------------------------------
def pyr_down(x):
    """OpenCV pyrDown of fp32 (C, H, W): (C, (H+1)//2, (W+1)//2)."""
    x = x.contiguous()
    C, H, W = x.shape
    out = torch.empty((C, (H + 1) // 2, (W + 1) // 2), dtype=torch.float32, device=x.device)
    check(lib.hg_pyr_down(x.data_ptr(), out.data_ptr(), C, H, W, raw_stream(x.device)), 'hg_pyr_down')
    return out


def pyr_up_add(prev, fine_a=None, coarse_a=None, wa=0.0, fine_b=None, coarse_b=None, wb=0.0):
    """pyrUp(prev) + wa*(fine_a - pyrUp(coarse_a)) + wb*(fine_b - pyrUp(coarse_b)), one launch (include/hg_post.h)."""
    C, h, w = prev.shape
    out = torch.empty((C, 2 * h, 2 * w), dtype=torch.float32, device=prev.device)
    fa, ca = (fine_a, coarse_a) if wa != 0 else (None, None)
    fb, cb = (fine_b, coarse_b) if wb != 0 else (None, None)
    check(lib.hg_pyr_up_add(prev.data_ptr(), ptr(fa), ptr(ca), float(wa), ptr(fb), ptr(cb), float(wb), out.data_ptr(), C, h, w,
                            raw_stream(prev.device)), 'hg_pyr_up_add')
    return out


def _as_chw3(t, what):
    if t.dim() == 4:
        if t.shape[0] != 1:
            raise ValueError(f'pyramid_upsampling: {what} must be a single image, got batch {t.shape[0]}')
        t = t[0]
    if t.dim() != 3 or t.shape[0] != 3:
        raise ValueError(f'pyramid_upsampling: {what} must be a 3-channel (3, H, W) image, got {tuple(t.shape)}')
    return t


def level_weights(levels, swapping_levels, blending):
    """(a_k, b_k) for k = 0..levels-1: the Laplacian used at level k is a_k * target's + b_k * reference's
    (utils/pyramid_upsampling.py:76-81).  Raises IndexError where the reference does."""
    if levels < 1:
        raise ValueError(f'pyramid_upsampling: levels must be >= 1, got {levels}')
    if swapping_levels < 0:
        raise ValueError(f'pyramid_upsampling: swapping_levels must be >= 0, got {swapping_levels}')
    if swapping_levels > levels:
        raise IndexError(f'pyramid_upsampling: swapping_levels={swapping_levels} exceeds levels={levels} (the '
                         'reference indexes past its pyramid)')
    ab = [(1.0, 0.0) if k < swapping_levels else (0.0, 1.0) for k in range(levels)]
    if blending and swapping_levels < levels:
        wts = np.linspace(0.0, 1.0, levels - swapping_levels + 1)
        if levels - 1 >= wts.size:
            raise IndexError(f'pyramid_upsampling: blending with swapping_levels={swapping_levels} >= 2 indexes '
                             f'past its {wts.size} blending weights (as the reference does)')
        for k in range(swapping_levels, levels):
            ab[k] = (1.0 - float(wts[k]), float(wts[k]))
    return ab


def padded_size(h, w, levels):
    """The reference's padding (utils/pyramid_upsampling.py:18-30): each side up to the next multiple of 2**levels."""
    m = 2 ** levels
    return (h if h % m == 0 else h + m - h % m), (w if w % m == 0 else w + m - w % m)


def pyramid_upsampling(target, reference, levels=5, swapping_levels=1, blending=False):
    """utils/pyramid_upsampling.py on the GPU.  target: float (1, 3, h, w) / (3, h, w), clamped to [0, 1] as it is read
    (the caller's tensor is not modified); reference: float (1, 3, H, W) / (3, H, W), or uint8 (H, W, 3) read as x/255.
    Returns fp32 (1, 3, H', W') on the device, where (H', W') is the reference's size padded up to multiples of
    2**levels: a reference whose side is not such a multiple is bicubic-resized up to it and the OUTPUT KEEPS THE
    PADDED SIZE, as the reference's does.  The Laplacian pyramid of the target (resized to that size) replaces the
    reference's first `swapping_levels` entries [gp[levels-1], L_{levels-1}, ..., L_1]; with `blending` the remaining
    entries are mixed with linspace(0, 1, levels - swapping_levels + 1) weights."""
    ab = level_weights(levels, swapping_levels, blending)
    need_gpu(target, 'pyramid_upsampling', _FOUND)
    need_gpu(reference, 'pyramid_upsampling', _FOUND)
    with on_device(reference.device):
        if reference.dtype == torch.uint8:
            if reference.dim() != 3 or reference.shape[2] != 3:
                raise ValueError('pyramid_upsampling: a uint8 reference must be (H, W, 3), got '
                                 f'{tuple(reference.shape)}')
            ref = u8_hwc_to_float(reference)
        else:
            ref = _as_chw3(reference, 'reference').float()
        tgt = _as_chw3(target, 'target').float()
        _, H, W = ref.shape
        Hp, Wp = padded_size(H, W, levels)
        if (Hp, Wp) != (H, W):
            ref = imresize(ref, output_shape=(Hp, Wp))
        ref = ref.contiguous()
        tgt = imresize(tgt, output_shape=(Hp, Wp), clamp=True)
        need_a = any(a != 0 for a, _ in ab)
        need_b = any(b != 0 for _, b in ab)
        gpa, gpb = [tgt], [ref]
        for _ in range(levels - 1):          # gp[levels] is never used
            if need_a:
                gpa.append(pyr_down(gpa[-1]))
            if need_b:
                gpb.append(pyr_down(gpb[-1]))
        top = levels - 1
        out = gpa[top] if ab[0][0] != 0 else gpb[top]
        for k in range(1, levels):
            a, b = ab[k]
            fine, coarse = top - k, top - k + 1
            out = pyr_up_add(out, gpa[fine] if a else None, gpa[coarse] if a else None, a,
                             gpb[fine] if b else None, gpb[coarse] if b else None, b)
        if out.data_ptr() == reference.data_ptr():
            out = out.clone()                # levels == 1 without swap: never hand back the caller's own storage
    return out.unsqueeze(0)


# ---- colour transfer (utils/color_transfer_MKL.py) ------------------------------------------------------------------
def MKL(A, B):
    """The Monge-Kantorovich linear map T with T A T = B for 3x3 covariances (fp64, host).  Negative eigenvalues are
    clamped to 0, and EPS is added to EVERY entry of the diagonal eigenvalue matrices before their square root,
    off-diagonal entries included (a ~1e-8 term, kept as the reference has it).  That term makes T depend on the
    eigenvector signs LAPACK returns, at a relative size of about sqrt(EPS / smallest eigenvalue of A); for a
    near-grey image (eigenvalue ~1e-5) a last-digit change of A moves T by ~3e-5, in the reference as here."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ea, Ua = np.linalg.eig(A)
    Da2 = np.diag(ea)
    Da2[Da2 < 0] = 0
    Da = np.sqrt(Da2 + EPS)
    C = Da @ Ua.T @ B @ Ua @ Da
    ec, Uc = np.linalg.eig(C)
    Dc2 = np.diag(ec)
    Dc2[Dc2 < 0] = 0
    Dc = np.sqrt(Dc2 + EPS)
    Da_inv = np.diag(1.0 / np.diag(Da))
    return Ua @ Da_inv @ Uc @ Dc @ Uc.T @ Da_inv @ Ua.T


def _pixels(t, what, fn='color_transfer_mkl'):
    """(tensor, n, pix_stride, chan_stride) of an (H, W, 3) fp32 view (a CHW image's .permute(1, 2, 0) is one)."""
    need_gpu(t, fn, _FOUND)
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f'{fn}: {what} must be an (H, W, 3) image, got {tuple(t.shape)}')
    t = t.float()
    if t.stride(0) != t.shape[1] * t.stride(1) or t.stride(1) <= 0 or t.stride(2) <= 0:
        t = t.contiguous()
    return t, t.shape[0] * t.shape[1], t.stride(1), t.stride(2)


def color_moments(x):
    """(mean (3,), covariance (3, 3)) in fp64 of an (H, W, 3) device image (np.mean / np.cov over its pixels)."""
    t, n, ps, cs = _pixels(x, 'image')
    if n < 2:
        raise ValueError('color_transfer_mkl: an image needs at least 2 pixels')
    with on_device(t.device):
        nb = lib.hg_color_moments_workspace_bytes(n)
        ws = workspace(nb, t.device)
        mom = torch.empty(12, dtype=torch.float64, device=t.device)
        check(lib.hg_color_moments(t.data_ptr(), n, ps, cs, mom.data_ptr(), ws.data_ptr(), nb, raw_stream(t.device)),
              'hg_color_moments')
        m = mom.cpu().numpy()
    return m[:3].copy(), m[3:].reshape(3, 3).copy()


def color_transfer_mkl(source, target, quantize=False):
    """utils/color_transfer_MKL.py on the GPU: maps the colours of `source` onto those of `target` with the linear
    Monge-Kantorovich transform.  source, target: (H, W, 3) fp32 device views.  Returns (out, T): out is (H, W, 3)
    fp32 clipped to [0, 1], or uint8 = (uint8)(out*255) (the caller's np.uint8(result*255)) when quantize; T the 3x3
    fp64 map."""
    src, n, ps, cs = _pixels(source, 'source')
    m0, A = color_moments(src)
    m1, B = color_moments(target)
    T = MKL(A, B)
    coef = np.concatenate([m0, T.real.reshape(-1), m1]).astype(np.float32)
    out = torch.empty(source.shape[:2] + (3,), dtype=torch.uint8 if quantize else torch.float32, device=src.device)
    with on_device(src.device):
        check(lib.hg_color_affine(src.data_ptr(), n, ps, cs, coef.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                  out.data_ptr(), int(quantize), raw_stream(src.device)), 'hg_color_affine')
    return out, T


# ---- iterative distribution transfer (hg_idt_*, include/hg_post.h) ---------------------------------------------------
def idt_rotations(iterations, seed=0):
    """The (iterations, 3, 3) fp64 rotations of color_transfer_idt (row a = axis a): the identity first, then proper rotations
    drawn from numpy.random.RandomState(seed) -- the Q of the QR decomposition of a 3x3 normal matrix, its columns multiplied
    by the signs of R's diagonal (which makes Q uniform over the orthogonal group) and the first column flipped when the
    determinant is negative."""
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError(f'idt_rotations: iterations must be at least 1, got {iterations}')
    rs = np.random.RandomState(seed)
    out = np.empty((iterations, 3, 3), dtype=np.float64)
    out[0] = np.eye(3)
    for i in range(1, iterations):
        q, r = np.linalg.qr(rs.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out[i] = q
    return out


def idt_encode_range(lo, hi):
    """A range set of include/hg_post.h, uint32[6], from three minima and three maxima (fp32): the order-preserving unsigned
    image of each float.  Returned as an int64 numpy array (torch has no uint32 arithmetic); idt_range_tensor uploads it."""
    f = np.concatenate([np.asarray(lo, dtype=np.float32).reshape(3), np.asarray(hi, dtype=np.float32).reshape(3)])
    u = f.view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, u ^ 0xffffffff, u | 0x80000000)


def idt_decode_range(enc):
    """(lo (3,), hi (3,)) fp32 of range sets (..., 6) read back from the device (any integer dtype holding the 32 bits)."""
    u = np.asarray(enc).astype(np.int64) & 0xffffffff
    bits = np.where(u & 0x80000000, u & 0x7fffffff, u ^ 0xffffffff).astype(np.uint32)
    f = bits.view(np.float32)
    return f[..., :3], f[..., 3:]


def idt_range_tensor(enc, device):
    """Encoded range sets as the int32 device tensor whose bits the kernels read as uint32."""
    return torch.from_numpy(np.asarray(enc, dtype=np.int64).astype(np.uint32).view(np.int32).copy()).to(device)


def color_transfer_idt(source, target, iterations=20, bins=256, relaxation=1.0, rotations=None, seed=0, quantize=False):
    """Iterative distribution transfer (Pitie, Kokaram, Dahyot 2007) on the GPU: maps the colours of `source` onto the colour
    DISTRIBUTION of `target`, not only its mean and covariance as color_transfer_mkl does.  Per rotation the colour cloud is
    projected on three orthogonal axes, each 1-D marginal is matched to the target's by CDF matching on a linear-binned
    `bins`-node histogram, and the pixels move by `relaxation` times the difference (hg_idt_run, include/hg_post.h holds the
    definition).  source, target: (H, W, 3) fp32 device views of any two sizes.  rotations: (iterations, 3, 3) orthonormal
    matrices, row a = axis a; None draws idt_rotations(iterations, seed).  Returns (out, rotations): out is (H, W, 3) fp32
    clipped to [0, 1], or uint8 = (uint8)(out*255) when quantize; rotations the fp64 array that was used (passed to the
    kernels as fp32).  The whole transfer is enqueued on the current stream without a host read-back, and its result does
    not depend on the order of any sum: two calls give the same bits.

    bins: the default of 256 is meant for photographs and 256x256 targets.  The quantile map is ill-conditioned where
    target nodes are empty, so more bins than about a sixteenth of the smaller image's pixels buy noise, not fidelity
    (with ~1000 pixels per image, 256 bins already differ by 1e-4 between fp32 and fp64 arithmetic, 1024 bins by 1e-2)."""
    fn = 'color_transfer_idt'
    src, n0, ps0, cs0 = _pixels(source, 'source', fn)
    tgt, n1, ps1, cs1 = _pixels(target, 'target', fn)
    if tgt.device != src.device:
        raise ValueError(f'{fn}: source and target must be on one device, got {src.device} and {tgt.device}')
    if rotations is None:
        rotations = idt_rotations(iterations, seed)
    rotations = np.ascontiguousarray(rotations, dtype=np.float64)
    if rotations.ndim != 3 or rotations.shape[1:] != (3, 3) or rotations.shape[0] < 1:
        raise ValueError(f'{fn}: rotations must be (iterations, 3, 3), got {rotations.shape}')
    iters, bins = rotations.shape[0], int(bins)
    out = torch.empty(source.shape[:2] + (3,), dtype=torch.uint8 if quantize else torch.float32, device=src.device)
    with on_device(src.device):
        rot = torch.from_numpy(rotations.astype(np.float32)).to(src.device)
        nb = lib.hg_idt_workspace_bytes(n0, n1, iters, bins)
        ws = workspace(nb, src.device)
        check(lib.hg_idt_run(src.data_ptr(), n0, ps0, cs0, tgt.data_ptr(), n1, ps1, cs1, rot.data_ptr(), iters, bins,
                             float(relaxation), out.data_ptr(), int(quantize), ws.data_ptr(), nb, raw_stream(src.device)),
              'hg_idt_run')
    return out, rotations


# ---- palettes (hg_palette_*, include/hg_post.h) -----------------------------------------------------------------------
Palette = namedtuple('Palette', 'rgb lab weight')
Palette.__doc__ = """K colours of an image: rgb (..., K, 3) sRGB in [0, 1], lab (..., K, 3) in CIE Lab units, weight (..., K) the
share of the image's weight each colour stands for (0: an empty cluster).  fp32, on the device."""
PALETTE_UNIT = 128                # a palette centre is an integer number of 1/128 Lab units
PALETTE_MAX_K = 16                # hg_palette_max_k()


def _palette_counts(k, iterations, what):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= PALETTE_MAX_K:
        raise ValueError(f'{what}: k must be an integer in 1 .. {PALETTE_MAX_K}, got {k!r}')
    if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 0:
        raise ValueError(f'{what}: iterations must be a non-negative integer, got {iterations!r}')


def _palette_weight(weight, B, H, W, single, device, what):
    """The rule "an optional weight map": None, or the float (B, H, W) view of a (H, W), (B, H, W) or (B, 1, H, W) map."""
    if weight is None:
        return None
    w = weight
    if torch.is_tensor(w):
        if single and w.dim() == 2:
            w = w.unsqueeze(0)
        if w.dim() == 4 and w.shape[1] == 1:
            w = w[:, 0]
    if not torch.is_tensor(w) or tuple(w.shape) != (B, H, W) or not w.is_floating_point() or w.device != device:
        got = f'{weight.dtype} {tuple(weight.shape)} on {weight.device}' if torch.is_tensor(weight) else type(weight).__name__
        raise ValueError(f'{what}: weight must be a float (H, W), (B, H, W) or (B, 1, H, W) map = {(B, H, W)} on {device}, got {got}')
    return w


def _lab_units_to_rgb(lab):
    """(B, K, 3) Lab units on the device -> (B, K, 3) sRGB through lab_to_srgb (the normalised form, rounded to fp32)."""
    norm = torch.stack((lab[..., 0] / 100.0, (lab[..., 1] + 128.0) / 255.0, (lab[..., 2] + 128.0) / 255.0), dim=1)
    return lab_to_srgb(norm.unsqueeze(2).float())[:, :, 0].permute(0, 2, 1).contiguous()


def _palette_run(x4, w, other4, k, iterations, want_labels=False, blocks=0):
    """One hg_palette_run: (centres int32 (B, K, 3), sums int64 (B, K, 4), centres_other or None, labels uint8 (B, H, W) or
    None)."""
    x4 = _detached_f32(x4)
    B, _, H, W = x4.shape
    dev = x4.device
    wstr = (0, 0, 0)
    if w is not None:
        w = _detached_f32(w)
        wstr = w.stride()
    ostr = (0, 0, 0, 0)
    if other4 is not None:
        other4 = _detached_f32(other4)
        ostr = other4.stride()
    with on_device(dev):
        centres = torch.empty((B, k, 3), dtype=torch.int32, device=dev)
        sums = torch.empty((B, k, 4), dtype=torch.int64, device=dev)
        centres_other = torch.empty((B, k, 3), dtype=torch.int32, device=dev) if other4 is not None else None
        labels = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_labels else None
        nb = lib.hg_palette_workspace_bytes(B, H * W, int(other4 is not None))
        ws = workspace(nb, dev)
        check(lib.hg_palette_run(x4.data_ptr(), *x4.stride(), ptr(w), *wstr, ptr(other4), *ostr, B, H, W, k, iterations, blocks,
                                 centres.data_ptr(), sums.data_ptr(), ptr(centres_other), ptr(labels), ws.data_ptr(), nb,
                                 raw_stream(dev)), 'hg_palette_run')
    return centres, sums, centres_other, labels


def _palettes_of(centres_list, sums, sort):
    """Palettes that share one clustering (its int64 sums): lab = centres / 128, rgb through lab_to_srgb, weight = W_k / sum W
    (0 without any weight); with `sort` by descending weight, stably, so that empty clusters trail."""
    W = sums[..., 0]
    weight = (W.double() / W.sum(dim=1, keepdim=True).clamp(min=1).double()).float()
    order = torch.sort(W, dim=1, descending=True, stable=True)[1] if sort else None
    out = []
    for c in centres_list:
        lab = c.float() / PALETTE_UNIT
        wt = weight
        if order is not None:
            lab, wt = torch.gather(lab, 1, order[..., None].expand(-1, -1, 3)), torch.gather(weight, 1, order)
        out.append(Palette(_lab_units_to_rgb(lab), lab, wt))
    return out


def _palette_images(image, others, k, iterations, weight, what):
    """Every refusal of palette / paired_palette, ValueError first: (single, image (B, 3, H, W), others, weight (B, H, W))."""
    _palette_counts(k, iterations, what)
    single, x4 = _rgb_batch(image, what)
    o4 = []
    for o in others:
        _, t4 = _rgb_batch(o, what, 'other')
        if t4.shape != x4.shape or t4.device != x4.device:
            raise ValueError(f'{what}: image and other must have one shape and device, got {tuple(x4.shape)} on {x4.device} and '
                             f'{tuple(t4.shape)} on {t4.device}')
        o4.append(t4)
    B, _, H, W = x4.shape
    w = _palette_weight(weight, B, H, W, single, x4.device, what)
    if H * W > (1 << 28) - 1 or not 1 <= B <= 65535:
        raise ValueError(f'{what}: at most 2^28 - 1 pixels per image and 65535 images, got {B} x {H} x {W}')
    need_gpu(x4, what, _FOUND)
    return single, x4, o4, w


def palette(image, k=6, iterations=16, weight=None, sort=True):
    """The K colours that describe an image: integer k-means in CIE Lab (hg_palette_run, include/hg_post.h holds the
    definition), seeded by weighted farthest-point selection over a 16^3 grid of Lab cells and refined by `iterations` Lloyd
    steps -- a fixed count, no convergence test, nothing read back: the whole run is enqueued on the current stream, and
    because every sum is an integer two calls give the same bits.  image: float (3, H, W) or (B, 3, H, W) sRGB, any strides,
    clamped to [0, 1]; weight: optional (H, W), (B, H, W) or (B, 1, H, W) map, clamped to [0, 1] (a mask, an alpha channel);
    pixels with a NaN or infinite channel or weight do not count.  Returns Palette(rgb, lab, weight) of shapes (..., K, 3),
    (..., K, 3), (..., K): lab the centres in Lab units (multiples of 1/128), rgb the same colours through lab_to_srgb, weight
    each cluster's share W_k / sum W.  sort: clusters by descending weight (stable), so that empty clusters -- weight 0, which an
    image with fewer than K distinct colours leaves -- trail."""
    single, x4, _, w = _palette_images(image, (), k, iterations, weight, 'palette')
    centres, sums, _, _ = _palette_run(x4, w, None, k, iterations)
    (pal,) = _palettes_of([centres], sums, sort)
    return Palette(*(t[0] for t in pal)) if single else pal


def paired_palette(image, other, k=6, iterations=16, weight=None):
    """(src, dst): the palette of `image` and, for each of its clusters, the mean Lab colour of `other` -- an image of the same
    H x W, paired with `image` pixel by pixel, e.g. a recolouring of it -- over the cluster's pixels.  There is no correspondence
    problem: dst[k] is where the pixels of src[k] went.  Both are sorted by descending weight and share it; an empty cluster has
    dst == src and weight 0."""
    single, x4, (o4,), w = _palette_images(image, (other,), k, iterations, weight, 'paired_palette')
    centres, sums, centres_other, _ = _palette_run(x4, w, o4, k, iterations)
    src, dst = _palettes_of([centres, centres_other], sums, True)
    if single:
        src, dst = Palette(*(t[0] for t in src)), Palette(*(t[0] for t in dst))
    return src, dst


def _palette_tensors(pal, what, name):
    """(lab (K, 3), weight (K,)) of one un-batched palette, ValueError otherwise (no device is touched)."""
    ok = isinstance(pal, Palette) and all(torch.is_tensor(t) for t in pal)
    if not ok or pal.lab.dim() != 2 or pal.lab.shape[1] != 3 or not 1 <= pal.lab.shape[0] <= PALETTE_MAX_K or \
            tuple(pal.weight.shape) != (pal.lab.shape[0],):
        got = f'lab {tuple(pal.lab.shape)}, weight {tuple(pal.weight.shape)}' if ok else type(pal).__name__
        raise ValueError(f'{what}: {name} must be a Palette of one image with 1 .. {PALETTE_MAX_K} colours (lab (K, 3), weight (K,)), '
                         f'got {got}')
    return pal.lab, pal.weight


def palette_from_rgb(colors, weight=None):
    """A Palette from colours typed in by a user: colors (K, 3) sRGB in [0, 1] on the device, weight (K,) or None for equal
    shares."""
    if not torch.is_tensor(colors) or colors.dim() != 2 or colors.shape[1] != 3 or not 1 <= colors.shape[0] <= PALETTE_MAX_K:
        raise ValueError(f'palette_from_rgb: colors must be a (K, 3) tensor with 1 .. {PALETTE_MAX_K} rows')
    need_gpu(colors, 'palette_from_rgb', _FOUND)
    K = colors.shape[0]
    rgb = colors.detach().float().clamp(0, 1)
    norm = srgb_to_lab(rgb.t().reshape(3, 1, K))[:, 0].t()
    lab = torch.stack((norm[:, 0] * 100.0, norm[:, 1] * 255.0 - 128.0, norm[:, 2] * 255.0 - 128.0), dim=1)
    wt = torch.full((K,), 1.0 / K, device=rgb.device) if weight is None else weight.detach().float().to(rgb.device)
    return Palette(rgb, lab, wt)


def palette_labels(image, pal):
    """The uint8 label map of `image` against the colours of `pal` (a Palette, or its lab tensor): for every pixel the index of
    the nearest centre in Lab (integer distances, the lowest index on ties), 255 for a pixel with a non-finite channel.  (H, W)
    for a (3, H, W) image and a (K, 3) palette, else (B, H, W) with a (B, K, 3) palette."""
    what = 'palette_labels'
    single, x4 = _rgb_batch(image, what)
    lab = pal.lab if isinstance(pal, Palette) else pal
    B, _, H, W = x4.shape
    if torch.is_tensor(lab) and single and lab.dim() == 2:
        lab = lab.unsqueeze(0)
    if not torch.is_tensor(lab) or lab.dim() != 3 or lab.shape[0] != B or lab.shape[2] != 3 or not 1 <= lab.shape[1] <= PALETTE_MAX_K:
        raise ValueError(f'{what}: the palette must hold (K, 3) Lab centres per image, 1 <= K <= {PALETTE_MAX_K}, for {B} image(s)')
    need_gpu(x4, what, _FOUND)
    need_gpu(lab, what, _FOUND)
    x4 = _detached_f32(x4)
    dev, K, n = x4.device, lab.shape[1], H * W
    with on_device(dev):
        centres = torch.round(lab.detach().double() * PALETTE_UNIT).to(torch.int32).contiguous()
        points = torch.empty((B, lib.hg_palette_point_stride(n), 4), dtype=torch.int16, device=dev)
        sums = torch.zeros((B, K, 4), dtype=torch.int64, device=dev)
        labels = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        st = raw_stream(dev)
        check(lib.hg_palette_quantize(x4.data_ptr(), *x4.stride(), None, 0, 0, 0, points.data_ptr(), B, H, W, st), 'hg_palette_quantize')
        check(lib.hg_palette_step(points.data_ptr(), points.data_ptr(), B, n, centres.data_ptr(), K, sums.data_ptr(),
                                  labels.data_ptr(), 0, st), 'hg_palette_step')
    return labels[0] if single else labels


def match_palettes(src, dst, by='lightness'):
    """`dst` reordered to pair with `src` by rank of L: the darkest colour of dst lands where the darkest of src is, and so on.
    For palettes typed in by a user, which carry no correspondence (paired_palette's need none).  Two stable torch.sort calls,
    nothing is read back.  Returns a Palette with dst's colours and weights in src's order."""
    if by != 'lightness':
        raise ValueError(f"match_palettes: by must be 'lightness', not {by!r}")
    s_lab, _ = _palette_tensors(src, 'match_palettes', 'src')
    d_lab, _ = _palette_tensors(dst, 'match_palettes', 'dst')
    if s_lab.shape != d_lab.shape:
        raise ValueError(f'match_palettes: src and dst must have one K, got {s_lab.shape[0]} and {d_lab.shape[0]}')
    need_gpu(s_lab, 'match_palettes', _FOUND)
    need_gpu(d_lab, 'match_palettes', _FOUND)
    rank = torch.sort(torch.sort(s_lab[:, 0], stable=True)[1], stable=True)[1]          # rank of every src colour
    pick = torch.sort(d_lab[:, 0], stable=True)[1][rank]
    return Palette(dst.rgb[pick], dst.lab[pick], dst.weight[pick])


def color_transfer_palette(source, src_palette, dst_palette, sigma=None, quantize=False):
    """Palette-based colour transfer (hg_palette_transfer): every pixel x of `source`, in CIE Lab, moves by a smooth blend of
    the per-cluster shifts, y = x + sum_k u_k (t_k - s_k) / sum_k u_k with u_k = exp(-(|x - s_k|^2 - min_l |x - s_l|^2) / (2
    sigma^2)) -- between color_transfer_mkl, one affine map for the whole image, and color_transfer_idt, which matches the whole
    distribution: different colour regions move independently and local structure survives.  source: (H, W, 3) fp32 device
    view; src_palette, dst_palette: Palettes of K colours each, colour k of the one paired with colour k of the other
    (paired_palette gives such a pair; match_palettes pairs typed-in ones).  Clusters of weight 0 in either are not live: they
    pull nothing.  sigma: in Lab units; None takes the mean distance over the live pairs of source colours (1 when there is one
    colour), computed on the device -- nothing is read back between an extraction and a transfer.  Returns (out, sigma_used):
    out (H, W, 3) fp32 clipped to [0, 1], or uint8 = (uint8)(out*255) when quantize; sigma_used a 0-d device tensor."""
    fn = 'color_transfer_palette'
    s_lab, s_w = _palette_tensors(src_palette, fn, 'src_palette')
    d_lab, d_w = _palette_tensors(dst_palette, fn, 'dst_palette')
    if s_lab.shape != d_lab.shape:
        raise ValueError(f'{fn}: src_palette and dst_palette must have one K, got {s_lab.shape[0]} and {d_lab.shape[0]}')
    if sigma is not None and not (isinstance(sigma, (int, float)) and 0 < float(sigma) < float('inf')):
        raise ValueError(f'{fn}: sigma must be a positive finite number of Lab units or None, got {sigma!r}')
    if torch.is_tensor(source) and (source.dim() != 3 or source.shape[2] != 3):
        raise ValueError(f'{fn}: source must be an (H, W, 3) image, got {tuple(source.shape)}')
    src, n, ps, cs = _pixels(source, 'source', fn)
    need_gpu(s_lab, fn, _FOUND)
    need_gpu(d_lab, fn, _FOUND)
    dev = src.device
    out = torch.empty(source.shape[:2] + (3,), dtype=torch.uint8 if quantize else torch.float32, device=dev)
    with on_device(dev):
        s32, d32 = s_lab.detach().float().contiguous(), d_lab.detach().float().contiguous()
        live = ((s_w > 0) & (d_w > 0)).to(torch.int32).contiguous()
        sigma_used = torch.empty((), dtype=torch.float32, device=dev)
        check(lib.hg_palette_transfer(src.data_ptr(), n, ps, cs, s32.data_ptr(), d32.data_ptr(), live.data_ptr(), s32.shape[0],
                                      0.0 if sigma is None else float(sigma), sigma_used.data_ptr(), out.data_ptr(), int(quantize),
                                      raw_stream(dev)), 'hg_palette_transfer')
    return out, sigma_used


def palette_histogram(hist_block, pal):
    """The histogram of a palette's K colours: `hist_block` (RGBuvHistBlock, rgChromaHistBlock or LabHistBlock) called on the
    1 x K image of the colours with the palette weights as its `weight=` map, so a handful of colours drives whatever takes a
    target histogram (recoloringTrainer's hist_batch among them).  A LabHistBlock built without from_rgb receives the colours
    as the normalised Lab it bins.  pal: a Palette of one image or of a batch."""
    if not isinstance(pal, Palette) or not torch.is_tensor(pal.rgb) or pal.rgb.dim() not in (2, 3) or pal.rgb.shape[-1] != 3:
        raise ValueError('palette_histogram: pal must be a Palette with rgb (K, 3) or (B, K, 3)')
    need_gpu(pal.rgb, 'palette_histogram', _FOUND)
    rgb, lab, wt = (t if pal.rgb.dim() == 3 else t.unsqueeze(0) for t in pal)
    if getattr(hist_block, 'from_rgb', True):
        img = rgb.permute(0, 2, 1)
    else:
        img = torch.stack((lab[..., 0] / 100.0, (lab[..., 1] + 128.0) / 255.0, (lab[..., 2] + 128.0) / 255.0), dim=1)
    return hist_block(img.unsqueeze(2).float().contiguous(), weight=wt.unsqueeze(1).float().contiguous())


# ---- 3D colour LUTs (hg_lut_*, include/hg_lut.h) --------------------------------------------------------------------------
LUT_MAX_N = 65
LUT_MAX_PIXELS = 1 << 22      # pixel pairs of one fit: the bound of the 64-bit integer sums
LUT_LAMBDA = 0.2              # the defaults of lut_fit, from the fp64 reference on the synthetic pair
LUT_SWEEPS = 128
LUT_GRAD_MAX_PIXELS = 1 << 26  # pixels of one lut_apply backward: the bound of its 64-bit integer sums
LUT_REFINE_STEPS = 50          # the defaults of lut_refine, from the fp64 reference loop
LUT_REFINE_LR = 5e-3
LUT_REFINE_LAMBDA = 0.01
LUT_ADAM_BETAS, LUT_ADAM_EPS = (0.9, 0.999), 1e-8
_LUT_INTERPOLATION = {'tetrahedral': 0, 'trilinear': 1}


def _lut_size(n, fn):
    if isinstance(n, bool) or not isinstance(n, int) or not 2 <= n <= LUT_MAX_N:
        raise ValueError(f'{fn}: n must be an integer in [2, {LUT_MAX_N}], got {n!r}')
    return n


def _lut_interpolation(interpolation, fn):
    if interpolation not in _LUT_INTERPOLATION:
        raise ValueError(f"{fn}: interpolation must be 'tetrahedral' or 'trilinear', got {interpolation!r}")
    return _LUT_INTERPOLATION[interpolation]


def _lut_shape(lut, fn, name='lut'):
    if not torch.is_tensor(lut) or lut.dim() != 4 or lut.shape[3] != 3 or not lut.shape[0] == lut.shape[1] == lut.shape[2]:
        raise ValueError(f'{fn}: {name} must be an (N, N, N, 3) tensor, got {tuple(lut.shape) if torch.is_tensor(lut) else type(lut).__name__}')
    if not 2 <= lut.shape[0] <= LUT_MAX_N:
        raise ValueError(f'{fn}: {name} must have N in [2, {LUT_MAX_N}], got {lut.shape[0]}')
    return lut.shape[0]


def _lut_image_shape(t, fn, name, u8_ok=False):
    if not torch.is_tensor(t) or t.dim() != 3 or t.shape[2] != 3 or t.numel() == 0:
        raise ValueError(f'{fn}: {name} must be an (H, W, 3) image, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}')
    if not (t.is_floating_point() or (u8_ok and t.dtype == torch.uint8)):
        raise ValueError(f'{fn}: {name} must be a float image' + (' or uint8' if u8_ok else '') + f', got {t.dtype}')


def lut_identity(n=33, device=None):
    """The LUT that maps every colour to itself: fp32 (n, n, n, 3), indexed [b, g, r, c] (red fastest, the row order of a
    .cube file), node (ir, ig, ib) holding (ir, ig, ib) / (n - 1).  device: None is the current GPU."""
    _lut_size(n, 'lut_identity')
    g = torch.arange(n, dtype=torch.float64, device=torch.device('cuda') if device is None else device) / (n - 1)
    lut = torch.stack((g.view(1, 1, n).expand(n, n, n), g.view(1, n, 1).expand(n, n, n), g.view(n, 1, 1).expand(n, n, n)), dim=3)
    return lut.float().contiguous()


def _lut_apply_launch(src, npix, ps, cs, table, n, tri, blocks):
    out = torch.empty((npix, 3), dtype=torch.float32, device=src.device)
    check(lib.hg_lut_apply(src.data_ptr(), 0, npix, ps, cs, table.data_ptr(), n, tri, out.data_ptr(), 0, blocks,
                           raw_stream(src.device)), 'hg_lut_apply')
    return out


def lut_apply_backward(image, lut, grad, interpolation='tetrahedral', want_image=True, want_lut=True, blocks=0, workspace_out=None):
    """hg_lut_apply_bwd as it stands in the C ABI: (gx (H, W, 3) or None, glut (N, N, N, 3) or None) for the fp32 device view
    `image`, the LUT and the upstream gradient `grad` (H, W, 3).  What lut_apply(differentiable=True) runs in its backward;
    workspace_out: a list that receives the workspace (the bits of gmax and the integer sums, include/hg_lut.h) for inspection."""
    fn = 'lut_apply_backward'
    tri = _lut_interpolation(interpolation, fn)
    n = _lut_shape(lut, fn)
    _lut_image_shape(image, fn, 'image')
    if not torch.is_tensor(grad) or tuple(grad.shape) != tuple(image.shape):
        raise ValueError(f'{fn}: grad must have the image\'s shape {tuple(image.shape)}, got '
                         f'{tuple(grad.shape) if torch.is_tensor(grad) else type(grad).__name__}')
    if not (want_image or want_lut):
        raise ValueError(f'{fn}: nothing to compute (want_image and want_lut are both False)')
    for t in (image, lut, grad):
        need_gpu(t, fn, _FOUND)
    dev = image.device
    with on_device(dev):
        src, npix, ps, cs = _pixels(image.detach(), 'image', fn)
        if npix > LUT_GRAD_MAX_PIXELS:
            raise ValueError(f'{fn}: at most 2^26 pixels per call (the bound of the integer sums), got {npix}')
        table, g = lut.detach().float().contiguous(), grad.detach().float().contiguous()
        gx = torch.empty(image.shape, dtype=torch.float32, device=dev) if want_image else None
        glut = torch.empty((n, n, n, 3), dtype=torch.float32, device=dev) if want_lut else None
        nb = lib.hg_lut_grad_workspace_bytes(n) if want_lut else 0
        ws = workspace(nb, dev) if want_lut else None
        check(lib.hg_lut_apply_bwd(src.data_ptr(), 0, npix, ps, cs, table.data_ptr(), n, tri, g.data_ptr(), ptr(gx), ptr(glut),
                                   ptr(ws), nb, blocks, raw_stream(dev)), 'hg_lut_apply_bwd')
    if workspace_out is not None:
        workspace_out.append(ws)
    return gx, glut


class LutApplyFunction(torch.autograd.Function):
    """lut_apply(differentiable=True): the forward is hg_lut_apply on the fp32 source (the bits of the default path), the
    backward hg_lut_apply_bwd for whichever of image / lut needs a gradient.  No double backward."""

    @staticmethod
    def forward(ctx, image, lut, interpolation, blocks):
        n, dev = lut.shape[0], image.device
        with on_device(dev):
            src, npix, ps, cs = _pixels(image.detach(), 'image', 'lut_apply')
            table = lut.detach().float().contiguous()
            out = _lut_apply_launch(src, npix, ps, cs, table, n, _LUT_INTERPOLATION[interpolation], blocks)
        ctx.save_for_backward(src, table)
        ctx.interpolation, ctx.blocks, ctx.dtypes = interpolation, blocks, (image.dtype, lut.dtype)
        return out.view(image.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        src, table = ctx.saved_tensors
        gx, glut = lut_apply_backward(src, table, grad, ctx.interpolation, ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                      ctx.blocks)
        return (None if gx is None else gx.to(ctx.dtypes[0]), None if glut is None else glut.to(ctx.dtypes[1]), None, None)


def lut_apply(image, lut, interpolation='tetrahedral', quantize=False, blocks=0, differentiable=False):
    """A 3D LUT applied to an image (hg_lut_apply): one memory-bound pass, no transcendental per pixel.  image: an (H, W, 3)
    fp32 device view in [0, 1] (a CHW image's .permute(1, 2, 0) is one; any strides) or a uint8 (H, W, 3) photo read as
    v / 255; values outside [0, 1] are clamped first and NaN reads as 0.  lut: fp32 (N, N, N, 3), 2 <= N <= 65 (lut_identity,
    lut_fit, lut_bake, load_cube).  interpolation: 'tetrahedral' (four nodes, the default) or 'trilinear' (eight).  Returns
    (H, W, 3) fp32 clipped to [0, 1], or uint8 = (uint8)(out*255) when quantize -- truncation, the rule of color_transfer_mkl,
    _idt and _palette, so an identity LUT on a uint8 photo is not an exact round trip.  blocks: 0 takes the kernel's plan.
    differentiable: False (the default) detaches both operands.  True returns the same bits with a grad_fn: the backward
    (hg_lut_apply_bwd) gives the gradient for whichever of image / lut requires one -- zero through a clipped output channel
    and for an input channel outside [0, 1]; the LUT's gradient is summed in integers, so it has the same bits in every run.
    A uint8 image or quantize=True has no gradient: ValueError.  At most 2^26 pixels; no double backward."""
    fn = 'lut_apply'
    tri = _lut_interpolation(interpolation, fn)
    n = _lut_shape(lut, fn)
    _lut_image_shape(image, fn, 'image', u8_ok=True)
    if differentiable:
        if quantize or image.dtype == torch.uint8:
            raise ValueError(f'{fn}: differentiable=True needs a float image and quantize=False (uint8 has no gradient)')
        if image.shape[0] * image.shape[1] > LUT_GRAD_MAX_PIXELS:
            raise ValueError(f'{fn}: differentiable=True takes at most 2^26 pixels, got {image.shape[0] * image.shape[1]}')
    need_gpu(image, fn, _FOUND)
    need_gpu(lut, fn, _FOUND)
    if differentiable:
        return LutApplyFunction.apply(image, lut, interpolation, blocks)
    dev = image.device
    H, W = image.shape[:2]
    with on_device(dev):
        table = lut.detach().float().contiguous()
        if image.dtype == torch.uint8:
            src, u8, ps, cs = image.contiguous(), 1, 3, 1
        else:
            src, _, ps, cs = _pixels(image.detach(), 'image', fn)
            u8 = 0
        out = torch.empty((H, W, 3), dtype=torch.uint8 if quantize else torch.float32, device=dev)
        check(lib.hg_lut_apply(src.data_ptr(), u8, H * W, ps, cs, table.data_ptr(), n, tri, out.data_ptr(), int(quantize), blocks,
                               raw_stream(dev)), 'hg_lut_apply')
    return out


def _lut_solver_args(lambda_smooth, iterations, fn):
    lam = LUT_LAMBDA if lambda_smooth is None else lambda_smooth
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0 <= float(lam) < float('inf'):
        raise ValueError(f'{fn}: lambda_smooth must be a non-negative finite number or None, got {lambda_smooth!r}')
    sweeps = LUT_SWEEPS if iterations is None else iterations
    if isinstance(sweeps, bool) or not isinstance(sweeps, int) or sweeps < 0:
        raise ValueError(f'{fn}: iterations must be a non-negative integer or None, got {iterations!r}')
    return float(lam), sweeps


def _lut_pair(source, target, weight, fn):
    _lut_image_shape(source, fn, 'source')
    _lut_image_shape(target, fn, 'target')
    if source.shape != target.shape:
        raise ValueError(f'{fn}: source and target must have one size, got {tuple(source.shape)} and {tuple(target.shape)}')
    if weight is not None and (not torch.is_tensor(weight) or tuple(weight.shape) != tuple(source.shape[:2])):
        raise ValueError(f'{fn}: weight must be an (H, W) map of the images\' size {tuple(source.shape[:2])}, got '
                         f'{tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__}')
    if source.shape[0] * source.shape[1] > LUT_MAX_PIXELS:
        raise ValueError(f'{fn}: at most 2^22 pixel pairs per fit (the bound of the integer sums), got {source.shape[0] * source.shape[1]}')
    for t in (source, target) + (() if weight is None else (weight,)):
        need_gpu(t, fn, _FOUND)
    s, npix, sps, scs = _pixels(source.detach(), 'source', fn)
    t, _, tps, tcs = _pixels(target.detach(), 'target', fn)
    w = None if weight is None else weight.detach().float().contiguous()
    return (s, sps, scs), (t, tps, tcs), w, npix


def lut_splat(source, target, n=33, weight=None, sums=None, blocks=0):
    """The integer normal sums of a fit (hg_lut_splat): int64 (n, n, n, 4) = (A, B_r, B_g, B_b) per lattice node, every pixel of
    the pair splatted trilinearly onto the 8 corners of its cell.  They are integers, so they do not depend on the order of
    the sums and add up over image pairs: pass the `sums` of earlier pairs to fit one LUT to several (2^22 pixels in all)."""
    fn = 'lut_splat'
    _lut_size(n, fn)
    if sums is not None and (not torch.is_tensor(sums) or sums.dtype != torch.int64 or tuple(sums.shape) != (n, n, n, 4)
                             or not sums.is_contiguous()):
        raise ValueError(f'{fn}: sums must be a contiguous int64 ({n}, {n}, {n}, 4) tensor')
    (s, sps, scs), (t, tps, tcs), w, npix = _lut_pair(source, target, weight, fn)
    dev = s.device
    with on_device(dev):
        if sums is None:
            sums = torch.zeros((n, n, n, 4), dtype=torch.int64, device=dev)
        need_gpu(sums, fn, _FOUND)
        check(lib.hg_lut_splat(s.data_ptr(), sps, scs, t.data_ptr(), tps, tcs, ptr(w), npix, n, sums.data_ptr(), blocks,
                               raw_stream(dev)), 'hg_lut_splat')
    return sums


def lut_solve(sums, lambda_smooth=None, iterations=None):
    """The LUT of the sums of lut_splat (hg_lut_solve): per channel (diag(a) + lambda L) d = b on the lattice -- a, b the sums
    scaled to mean(a) = 1, L the 6-neighbour Laplacian -- by `iterations` red-black Gauss-Seidel sweeps in fp64 from d = 0, and
    LUT = identity + d.  Where data is, the data wins; elsewhere d is the harmonic continuation of its surroundings; without
    any data the result is the identity.  None takes LUT_LAMBDA and LUT_SWEEPS."""
    fn = 'lut_solve'
    lam, sweeps = _lut_solver_args(lambda_smooth, iterations, fn)
    if not torch.is_tensor(sums) or sums.dtype != torch.int64 or sums.dim() != 4 or sums.shape[3] != 4 or \
            not sums.shape[0] == sums.shape[1] == sums.shape[2] or not 2 <= sums.shape[0] <= LUT_MAX_N:
        raise ValueError(f'{fn}: sums must be an int64 (N, N, N, 4) tensor with N in [2, {LUT_MAX_N}]')
    need_gpu(sums, fn, _FOUND)
    n, dev = sums.shape[0], sums.device
    with on_device(dev):
        sums = sums.contiguous()
        nb = lib.hg_lut_workspace_bytes(n)
        ws = workspace(nb, dev)
        lut = torch.empty((n, n, n, 3), dtype=torch.float32, device=dev)
        check(lib.hg_lut_solve(sums.data_ptr(), n, lam, sweeps, lut.data_ptr(), ws.data_ptr(), nb, raw_stream(dev)), 'hg_lut_solve')
    return lut


def lut_fit(source, target, n=33, weight=None, lambda_smooth=None, iterations=None):
    """Fit a 3D LUT to a pixel-paired image pair (hg_lut_fit): the general smooth pointwise colour map source -> target, next
    to color_transfer_mkl's single affine map.  source, target: (H, W, 3) fp32 device views of one size (the 256x256 input
    and the unclamped network output: targets in [-1, 2] are representable); weight: optional (H, W) map in [0, 1].  At most 2^22
    pixels.  lambda_smooth trades fidelity at the colours the pair has for smoothness (it does not depend on n or the image
    size); iterations is the number of Gauss-Seidel sweeps; None takes LUT_LAMBDA and LUT_SWEEPS.  Splat and solve run on the
    caller's stream with no read-back.  Returns the LUT, fp32 (n, n, n, 3); lut_fit(s, s) is the identity."""
    fn = 'lut_fit'
    _lut_size(n, fn)
    lam, sweeps = _lut_solver_args(lambda_smooth, iterations, fn)
    (s, sps, scs), (t, tps, tcs), w, npix = _lut_pair(source, target, weight, fn)
    dev = s.device
    with on_device(dev):
        nb = lib.hg_lut_workspace_bytes(n)
        ws = workspace(nb, dev)
        lut = torch.empty((n, n, n, 3), dtype=torch.float32, device=dev)
        check(lib.hg_lut_fit(s.data_ptr(), sps, scs, t.data_ptr(), tps, tcs, ptr(w), npix, n, lam, sweeps, lut.data_ptr(),
                             ws.data_ptr(), nb, raw_stream(dev)), 'hg_lut_fit')
    return lut


def lut_smoothness(lut):
    """R(d) = (N - 1)^2 * mean over the 3 N^2 (N - 1) lattice edges of |d_i - d_j|^2 for d = lut - identity: the discretised mean
    |grad d|^2 over the unit cube, so a weight on it means the same at every N.  A differentiable scalar from plain torch ops
    on the LUT's device (CPU tensors too) and in its dtype; hg_lut_adam_step adds the gradient of lambda R itself."""
    n = _lut_shape(lut, 'lut_smoothness')
    if not lut.is_floating_point():
        raise ValueError(f'lut_smoothness: lut must be a float tensor, got {lut.dtype}')
    d = lut - lut_identity(n, lut.device).to(lut.dtype)
    total = sum(((d.narrow(ax, 1, n - 1) - d.narrow(ax, 0, n - 1)) ** 2).sum() for ax in (2, 1, 0))
    return total * ((n - 1) ** 2 / (3 * n * n * (n - 1)))


def lut_adam_step(lut, grad, exp_avg, exp_avg_sq, step, lr=None, lambda_smooth=None, betas=LUT_ADAM_BETAS, eps=LUT_ADAM_EPS, out=None):
    """One Adam step on a LUT (hg_lut_adam_step, one launch): the new LUT from `lut`, its gradient `grad` plus the gradient
    of lambda_smooth * lut_smoothness, and the moments exp_avg / exp_avg_sq, which are updated in place.  step counts from 1.
    Out of place (the smoothness term reads neighbours): returns `out` or a new tensor.  None takes LUT_REFINE_LR / _LAMBDA."""
    fn = 'lut_adam_step'
    n = _lut_shape(lut, fn)
    lr = LUT_REFINE_LR if lr is None else lr
    lam = LUT_REFINE_LAMBDA if lambda_smooth is None else lambda_smooth
    _lut_refine_numbers(lr, lam, fn)
    if isinstance(step, bool) or not isinstance(step, int) or step < 1:
        raise ValueError(f'{fn}: step must be a positive integer, got {step!r}')
    out = torch.empty((n, n, n, 3), dtype=torch.float32, device=lut.device) if out is None else out
    for t, name in ((lut, 'lut'), (grad, 'grad'), (exp_avg, 'exp_avg'), (exp_avg_sq, 'exp_avg_sq'), (out, 'out')):
        if not torch.is_tensor(t) or tuple(t.shape) != (n, n, n, 3) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f'{fn}: {name} must be a contiguous fp32 ({n}, {n}, {n}, 3) tensor')
    if out.data_ptr() == lut.data_ptr():
        raise ValueError(f'{fn}: out must not be the LUT itself (the step is out of place)')
    for t in (lut, grad, exp_avg, exp_avg_sq, out):
        need_gpu(t, fn, _FOUND)
    with on_device(lut.device):
        check(lib.hg_lut_adam_step(lut.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), out.data_ptr(), n,
                                   float(lam), float(lr), betas[0], betas[1], eps, step, raw_stream(lut.device)), 'hg_lut_adam_step')
    return out


def _lut_refine_numbers(lr, lam, fn):
    if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not 0 < float(lr) < float('inf'):
        raise ValueError(f'{fn}: lr must be a positive finite number or None, got {lr!r}')
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0 <= float(lam) < float('inf'):
        raise ValueError(f'{fn}: lambda_smooth must be a non-negative finite number or None, got {lam!r}')


def lut_working_copy(image, hist_block, weight=None):
    """The (h, w, 3) fp32 image, and the (h, w) weight map or None, that `hist_block` bins when it is given `image` (H, W, 3):
    clamped to [0, 1] and, where a side exceeds the block's insz, reduced as the block reduces it ('interpolation': bilinear to
    insz x insz; 'sampling': h x h strided samples).  The block leaves an image of this size alone."""
    x = image.detach()
    x = (x.float() / 255.0 if x.dtype == torch.uint8 else x.float()).clamp(0, 1).permute(2, 0, 1).unsqueeze(0).contiguous()
    w = None if weight is None else weight.detach().float().clamp(0, 1)[None, None]
    H, W = x.shape[2:]
    if H > hist_block.insz or W > hist_block.insz:
        if hist_block.resizing == 'interpolation':
            size = (hist_block.insz, hist_block.insz)
            x = torch.nn.functional.interpolate(x, size=size, mode='bilinear', align_corners=False)
            w = None if w is None else torch.nn.functional.interpolate(w, size=size, mode='bilinear', align_corners=False)
        elif hist_block.resizing == 'sampling':
            r = torch.from_numpy(np.linspace(0, H, hist_block.h, endpoint=False).astype(np.int64)).to(x.device)
            c = torch.from_numpy(np.linspace(0, W, hist_block.h, endpoint=False).astype(np.int64)).to(x.device)
            x = x[:, :, r][:, :, :, c]
            w = None if w is None else w[:, :, r][:, :, :, c]
        else:
            raise ValueError(f'lut_refine: the block\'s resizing must be interpolation or sampling, got {hist_block.resizing!r}')
    return x[0].permute(1, 2, 0).contiguous(), None if w is None else w[0, 0].contiguous()


def lut_refine(lut, image, target_hist, hist_block, steps=None, lr=None, lambda_smooth=None, interpolation='tetrahedral',
               weight=None, return_losses=False):
    """Refine a LUT against a target colour histogram: `steps` Adam steps from `lut` on
        hist.hellinger_loss(target_hist, hist_block(LUT(image))) + lambda_smooth * lut_smoothness(LUT)
    -- the loss HistoGAN is trained on, with the LUT as the only unknown.  Start from lut_identity(n) to learn a LUT for a
    photo and a target histogram with no network at all; start from lut_fit's result to pull a fitted LUT towards the
    histogram it was meant to reach.  image: (H, W, 3) float in [0, 1] or uint8, on the GPU; it is reduced ONCE to the working
    copy the block would make of it (lut_working_copy), so a step costs the same for every photo size -- and what is matched
    is the histogram of LUT(reduced photo), not of the reduced LUT(photo) (DESIGN.md section 6k has the measured difference).
    target_hist: what hist_block returns for one image, (1, P, h, h) or (P, h, h).  hist_block: RGBuvHistBlock,
    rgChromaHistBlock or LabHistBlock(from_rgb=True) on the GPU.  weight: optional (H, W) map for the block's per-pixel weight.
    Each step is lut_apply, the histogram and the Hellinger loss forward and backward, hg_lut_apply_bwd and hg_lut_adam_step on
    the caller's stream with no read-back; two runs give the same bits.  None takes LUT_REFINE_STEPS, LUT_REFINE_LR and
    LUT_REFINE_LAMBDA.  Returns the refined LUT, fp32 (N, N, N, 3); with return_losses also a float (steps + 1,) tensor: the
    Hellinger term before every step and for the returned LUT (one more forward), read from the device once."""
    from .hist import hellinger_loss
    fn = 'lut_refine'
    _lut_interpolation(interpolation, fn)
    n = _lut_shape(lut, fn)
    _lut_image_shape(image, fn, 'image', u8_ok=True)
    steps = LUT_REFINE_STEPS if steps is None else steps
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 0:
        raise ValueError(f'{fn}: steps must be a non-negative integer or None, got {steps!r}')
    lr = LUT_REFINE_LR if lr is None else lr
    lam = LUT_REFINE_LAMBDA if lambda_smooth is None else lambda_smooth
    _lut_refine_numbers(lr, lam, fn)
    if not torch.is_tensor(target_hist) or target_hist.dim() not in (3, 4) or (target_hist.dim() == 4 and target_hist.shape[0] != 1):
        raise ValueError(f'{fn}: target_hist must be the (1, P, h, h) or (P, h, h) histogram of one image, got '
                         f'{tuple(target_hist.shape) if torch.is_tensor(target_hist) else type(target_hist).__name__}')
    if not callable(hist_block) or not all(hasattr(hist_block, a) for a in ('insz', 'resizing', 'h')):
        raise ValueError(f'{fn}: hist_block must be one of the histogram blocks (insz, resizing, h), got {type(hist_block).__name__}')
    if weight is not None and (not torch.is_tensor(weight) or tuple(weight.shape) != tuple(image.shape[:2])):
        raise ValueError(f'{fn}: weight must be an (H, W) map of the image\'s size {tuple(image.shape[:2])}, got '
                         f'{tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__}')
    for t in (lut, image, target_hist) + (() if weight is None else (weight,)):
        need_gpu(t, fn, _FOUND)
    dev = image.device
    with on_device(dev), torch.enable_grad():
        work, w = lut_working_copy(image, hist_block, weight)
        target = (target_hist if target_hist.dim() == 4 else target_hist.unsqueeze(0)).detach().float().contiguous()
        kw = {} if w is None else {'weight': w.unsqueeze(0)}
        cur = lut.detach().float().clone(memory_format=torch.contiguous_format)
        nxt, m, v = torch.empty_like(cur), torch.zeros_like(cur), torch.zeros_like(cur)
        losses = torch.zeros(steps + 1, dtype=torch.float32, device=dev)

        def loss_of(table):
            out = LutApplyFunction.apply(work, table, interpolation, 0)
            return hellinger_loss(target, hist_block(out.permute(2, 0, 1).unsqueeze(0), **kw), global_batch=False)

        for k in range(steps):
            leaf = cur.detach().requires_grad_(True)
            loss = loss_of(leaf)
            (glut,) = torch.autograd.grad(loss, leaf)
            losses[k].copy_(loss.detach())
            lut_adam_step(cur, glut.contiguous(), m, v, k + 1, lr, lam, out=nxt)
            cur, nxt = nxt, cur
        if return_losses:
            with torch.no_grad():
                losses[steps].copy_(loss_of(cur))
    return (cur, losses.cpu()) if return_losses else cur


def lut_bake(fn, n=33, device=None):
    """Bake a pointwise colour map into a LUT: `fn` maps an (H, W, 3) fp32 image in [0, 1] to one and is evaluated on the
    lattice viewed as an (n*n, n, 3) image.  A tuple result keeps its first element, so
    `lambda x: color_transfer_palette(x, ps, pd)` and an MKL map bake directly.  color_transfer_idt cannot be baked: it keeps
    no map that could be replayed on a lattice."""
    _lut_size(n, 'lut_bake')
    if not callable(fn):
        raise ValueError(f'lut_bake: fn must be callable, got {type(fn).__name__}')
    out = fn(lut_identity(n, device).view(n * n, n, 3))
    out = out[0] if isinstance(out, tuple) else out
    if not torch.is_tensor(out) or tuple(out.shape) != (n * n, n, 3) or not out.is_floating_point():
        raise ValueError(f'lut_bake: fn must return a float ({n * n}, {n}, 3) image, got '
                         f'{(out.dtype, tuple(out.shape)) if torch.is_tensor(out) else type(out).__name__}')
    return out.detach().float().reshape(n, n, n, 3).contiguous()


def lut_compose(first, second, interpolation='tetrahedral'):
    """The LUT of `first` followed by `second`: `second` applied to the entries of `first` (which are clamped to [0, 1], the
    domain of `second`, as lut_apply clamps its input; the result is clipped to [0, 1] like every lut_apply)."""
    fn = 'lut_compose'
    _lut_interpolation(interpolation, fn)
    n = _lut_shape(first, fn, 'first')
    _lut_shape(second, fn, 'second')
    need_gpu(first, fn, _FOUND)
    need_gpu(second, fn, _FOUND)
    return lut_apply(first.detach().float().contiguous().view(n * n, n, 3), second, interpolation).view(n, n, n, 3)


def save_cube(lut, path, title=None):
    """Write a LUT as a plain .cube file: optional TITLE, LUT_3D_SIZE N, DOMAIN_MIN 0 0 0, DOMAIN_MAX 1 1 1 and N^3 rows
    `r g b`, red fastest, with 9 significant digits -- load_cube(save_cube(l)) equals l bit for bit."""
    n = _lut_shape(lut, 'save_cube')
    if title is not None and (not isinstance(title, str) or '"' in title or '\n' in title or '\r' in title):
        raise ValueError(f'save_cube: title must be a string without quotes or line breaks, got {title!r}')
    rows = lut.detach().float().cpu().numpy().reshape(-1, 3)
    if not np.isfinite(rows).all():
        raise ValueError('save_cube: the LUT has non-finite entries')
    with open(path, 'w') as f:
        if title is not None:
            f.write(f'TITLE "{title}"\n')
        f.write(f'LUT_3D_SIZE {n}\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 1 1\n')
        f.write(''.join('%.9g %.9g %.9g\n' % (r[0], r[1], r[2]) for r in rows))
    return path


def load_cube(path, device=None):
    """Read a .cube file written by save_cube or by a grading tool: fp32 (N, N, N, 3), on `device` (None: the host).  `#`
    comments, blank lines and TITLE are skipped.  ValueError for a 1D LUT (LUT_1D_SIZE), a domain other than [0, 1], an N
    outside 2..65, an unknown keyword, a malformed row or a row count other than N^3."""
    n, rows, lo, hi = None, [], (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)

    def triple(parts, what):
        try:
            vals = tuple(float(p) for p in parts)
        except ValueError:
            vals = ()
        if len(vals) != 3 or len(parts) != 3:
            raise ValueError(f'load_cube: {path}: {what} needs three numbers, got {" ".join(parts)!r}')
        return vals

    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith('#'):
                continue
            key, rest = line.split()[0], line.split()[1:]
            if key == 'TITLE':
                continue
            if key == 'LUT_1D_SIZE':
                raise ValueError(f'load_cube: {path}: 1D LUTs (LUT_1D_SIZE) are not supported')
            if key == 'LUT_3D_SIZE':
                if n is not None or len(rest) != 1 or not rest[0].isdigit():
                    raise ValueError(f'load_cube: {path}: malformed or repeated LUT_3D_SIZE line {line!r}')
                n = int(rest[0])
                if not 2 <= n <= LUT_MAX_N:
                    raise ValueError(f'load_cube: {path}: LUT_3D_SIZE must lie in [2, {LUT_MAX_N}], got {n}')
            elif key == 'DOMAIN_MIN':
                lo = triple(rest, 'DOMAIN_MIN')
            elif key == 'DOMAIN_MAX':
                hi = triple(rest, 'DOMAIN_MAX')
            elif key[0].isalpha() or key[0] == '_':
                raise ValueError(f'load_cube: {path}: unknown keyword {key!r}')
            else:
                rows.append(triple(line.split(), 'a table row'))
    if n is None:
        raise ValueError(f'load_cube: {path}: no LUT_3D_SIZE line')
    if lo != (0.0, 0.0, 0.0) or hi != (1.0, 1.0, 1.0):
        raise ValueError(f'load_cube: {path}: only the domain [0, 1] is supported, got DOMAIN_MIN {lo} DOMAIN_MAX {hi}')
    if len(rows) != n ** 3:
        raise ValueError(f'load_cube: {path}: {len(rows)} rows for LUT_3D_SIZE {n} (expected {n ** 3})')
    lut = torch.from_numpy(np.asarray(rows, dtype=np.float64).astype(np.float32).reshape(n, n, n, 3))
    return lut if device is None else lut.to(device)


# ---- regrain (hg_regrain_*, include/hg_regrain.h) ---------------------------------------------------------------------------
REGRAIN_RHO = 0.2                 # the damping of the Jacobi sweep (fp32 in the kernels)
REGRAIN_MIN_SIDE = 20             # a coarser level exists while both of its sides exceed this
REGRAIN_ITERATIONS = (4, 16, 32, 64, 64, 64)
REGRAIN_MAX_FUSED = 8             # hg_regrain_max_fused()
REGRAIN_MAX_PIXELS = 1 << 28


def _regrain_args(iterations, smoothness, min_side, fn):
    """(iterations as a tuple of ints, smoothness as a float, min_side as an int), or ValueError (no HIP call is made)."""
    try:
        its = tuple(iterations)
    except TypeError:
        its = None
    if not its or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1 for n in its):
        raise ValueError(f'{fn}: iterations must be a non-empty sequence of positive integers, got {iterations!r}')
    ok = not isinstance(smoothness, bool) and isinstance(smoothness, (int, float, np.floating))
    if ok:
        with np.errstate(over='ignore', under='ignore'):
            ok = 0 < float(np.float32(smoothness)) < float('inf')          # the kernels take it as fp32
    if not ok:
        raise ValueError(f'{fn}: smoothness must be positive and finite, got {smoothness!r}')
    if isinstance(min_side, bool) or not isinstance(min_side, (int, np.integer)) or min_side < 1:
        raise ValueError(f'{fn}: min_side must be an integer of at least 1, got {min_side!r}')
    return tuple(int(n) for n in its), float(smoothness), int(min_side)


def regrain_levels(h, w, iterations=REGRAIN_ITERATIONS, min_side=REGRAIN_MIN_SIDE):
    """The level sizes [(h, w), (ceil(h / 2), ceil(w / 2)), ...] of regrain (include/hg_regrain.h, Levels): level l + 1 exists
    while `iterations` has an entry for it and both of its sides exceed min_side.  len() of it is hg_regrain_levels."""
    its, _, min_side = _regrain_args(iterations, 1.0, min_side, 'regrain_levels')
    if isinstance(h, bool) or isinstance(w, bool) or int(h) != h or int(w) != w or h < 2 or w < 2 or h * w > REGRAIN_MAX_PIXELS:
        raise ValueError(f'regrain_levels: an image of at least 2 x 2 and at most 2^28 pixels is needed, got {h} x {w}')
    sizes = [(int(h), int(w))]
    while len(sizes) < len(its):
        h2, w2 = (sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2
        if h2 <= min_side or w2 <= min_side:
            break
        sizes.append((h2, w2))
    return sizes


def _resize_planes_into(src, dst, method='bilinear'):
    """imresize(src, dst.shape[1:], method=method) written into `dst`: fp32 planes (C, H, W) -> contiguous fp32 (C, H', W') in
    the caller's memory; the same kernel, tables and axis order, so the same bits."""
    C, H, W = src.shape
    (Ho, Wo), scale = resize_plan((H, W), dst.shape[1:])
    order = [0, 1] if scale[0] <= scale[1] else [1, 0]
    cur = [H, W]
    cur_t, cur_s = src, tuple(src.stride())
    for step, axis in enumerate(order):
        ih, iw = cur
        cur[axis] = (Ho, Wo)[axis]
        h, w = cur
        out = dst if step == 1 else torch.empty((C, h, w), dtype=torch.float32, device=src.device)
        _resize_axis(cur_t, False, cur_s, C, ih, iw, axis, out, False, (h * w, w, 1), cur[axis], scale[axis], method, False)
        cur_t, cur_s = out, (h * w, w, 1)
    return dst


def _regrain_carve(ws, sizes):
    """The workspace of hg_regrain_workspace_bytes as per-level views: I (3), E (3), a (3), b (3), coef (4), scratch (1), each
    rounded up to 4 floats, level 0 first."""
    levels, off = [], 0
    for h, w in sizes:
        lv = {}
        for name, c in (('I', 3), ('E', 3), ('a', 3), ('b', 3), ('coef', 4), ('scratch', 1)):
            lv[name] = ws[off:off + c * h * w].view(c, h, w)
            off += (c * h * w + 3) // 4 * 4
        levels.append(lv)
    assert off == ws.numel()
    return levels


def _regrain_image(t, fn, name):
    if not torch.is_tensor(t) or t.dim() != 3 or t.shape[2] != 3 or not t.is_floating_point():
        raise ValueError(f'{fn}: {name} must be a float (H, W, 3) image, got '
                         f'{str(t.dtype) + " " + str(tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}')


def regrain_sweep(a, b, E, coef, n, fused=0):
    """hg_regrain_sweep on one level: n damped Jacobi sweeps from the (3, H, W) planes `a`, ping-ponging with `b`; E (3, H, W)
    and coef (4, H, W) as hg_regrain_coef wrote it.  Returns the one of a, b that holds the result."""
    _, H, W = a.shape
    with on_device(a.device):
        check(lib.hg_regrain_sweep(a.data_ptr(), b.data_ptr(), E.data_ptr(), coef.data_ptr(), H, W, n, fused, raw_stream(a.device)),
              'hg_regrain_sweep')
    k = fused if fused else lib.hg_regrain_plan_fused(H, W, n)
    return b if lib.hg_regrain_sweep_launches(n, k) % 2 else a


def regrain(original, transferred, iterations=REGRAIN_ITERATIONS, smoothness=1.0, min_side=REGRAIN_MIN_SIDE, quantize=False,
            fused=0):
    """Regrain (Pitie, Kokaram, Dahyot 2007), the step that follows a distribution transfer: the colours of `transferred` on
    the gradient field of `original`, which takes out the grain and the stretched compression blocks color_transfer_idt
    leaves on flat regions.  original, transferred: (H, W, 3) float device views of one size, H, W >= 2 (a CHW image's
    .permute(1, 2, 0) is one; any strides).  The solver works on the offset D = result - original (include/hg_regrain.h holds
    the definition): per level of a pyramid that halves down to min_side, iterations[l] damped Jacobi sweeps pull D towards
    transferred - original where `original` has structure and smooth it where `original` is flat -- by `smoothness`, larger is
    smoother -- and the coarser level's result starts the finer one.  regrain(x, x) is x bit for bit.  Returns (H, W, 3) fp32
    clipped to [0, 1], or uint8 = (uint8)(out*255) when quantize, as the transfers.  fused: sweeps per launch of the tiled
    kernel, 1 = one sweep per launch, 0 = the measured plan (hg_regrain_plan_fused); every setting gives the same bits.
    Everything is enqueued on the current stream without a host read-back; two calls give the same bits."""
    fn = 'regrain'
    its, smoothness, min_side = _regrain_args(iterations, smoothness, min_side, fn)
    _regrain_image(original, fn, 'original')
    _regrain_image(transferred, fn, 'transferred')
    if original.shape != transferred.shape:
        raise ValueError(f'{fn}: original and transferred must have one size, got {tuple(original.shape)} and '
                         f'{tuple(transferred.shape)}')
    if original.device != transferred.device:
        raise ValueError(f'{fn}: original and transferred must be on one device, got {original.device} and {transferred.device}')
    H, W = original.shape[:2]
    if H < 2 or W < 2 or H * W > REGRAIN_MAX_PIXELS:
        raise ValueError(f'{fn}: an image of at least 2 x 2 and at most 2^28 pixels is needed, got {H} x {W}')
    if isinstance(fused, bool) or not isinstance(fused, int) or not 0 <= fused <= REGRAIN_MAX_FUSED:
        raise ValueError(f'{fn}: fused must be an integer in [0, {REGRAIN_MAX_FUSED}], got {fused!r}')
    src, _, ps0, cs0 = _pixels(original.detach(), 'original', fn)
    tgt, _, ps1, cs1 = _pixels(transferred.detach(), 'transferred', fn)
    dev = src.device
    sizes = regrain_levels(H, W, its, min_side)
    out = torch.empty((H, W, 3), dtype=torch.uint8 if quantize else torch.float32, device=dev)
    with on_device(dev):
        st = raw_stream(dev)
        nb = lib.hg_regrain_workspace_bytes(H, W, len(sizes))
        lv = _regrain_carve(torch.empty(nb // 4, dtype=torch.float32, device=dev), sizes)
        check(lib.hg_regrain_begin(src.data_ptr(), ps0, cs0, tgt.data_ptr(), ps1, cs1, H, W, lv[0]['I'].data_ptr(),
                                   lv[0]['E'].data_ptr(), st), 'hg_regrain_begin')
        for l in range(1, len(sizes)):
            _resize_planes_into(lv[l - 1]['I'], lv[l]['I'])
            _resize_planes_into(lv[l - 1]['E'], lv[l]['E'])
        d = None
        for l in range(len(sizes) - 1, -1, -1):
            v = lv[l]
            h, w = sizes[l]
            check(lib.hg_regrain_coef(v['I'].data_ptr(), h, w, l, smoothness, v['coef'].data_ptr(), v['scratch'].data_ptr(), st),
                  'hg_regrain_coef')
            if d is None:
                v['a'].copy_(v['E'])
            else:
                _resize_planes_into(d, v['a'])
            d = regrain_sweep(v['a'], v['b'], v['E'], v['coef'], its[l], fused)
        check(lib.hg_regrain_finish(lv[0]['I'].data_ptr(), d.data_ptr(), H, W, out.data_ptr(), int(quantize), st),
              'hg_regrain_finish')
    return out


# ---- bilateral guided upsampling (upsampling/BGU.m, bguFit.m, bguSlice.m) -----------------------------------------------
BGU_DEPTH = 8             # luminance bins of the grid (getDefaultAffineGridSize.m)
BGU_CELL = 16             # low-resolution pixels per spatial bin


def _round_half_away(v):
    """MATLAB round() of a non-negative value (Python's round is half-to-even: round(2.5) == 2)."""
    return int(np.floor(v + 0.5))


def bgu_grid_size(h, w):
    """(gh, gw) = [round(h / 16), round(w / 16)] with MATLAB rounding, for an h x w low-resolution pair.  A side below 2
    vertices cannot be interpolated (ValueError)."""
    gh, gw = _round_half_away(h / BGU_CELL), _round_half_away(w / BGU_CELL)
    if gh < 2 or gw < 2:
        raise ValueError(f'bgu_grid_size: a {h}x{w} image gives a {gh}x{gw} grid; every side needs at least 2 vertices '
                         f'(24 pixels)')
    return gh, gw


def bgu_slab_axis(gh, gw):
    """0 when the slabs of the block-tridiagonal system run along y (gh >= gw), 1 when along x (include/hg_post.h)."""
    return 0 if gh >= gw else 1


def _path_laplacian(n):
    """D^T D of the n-1 first differences of n samples."""
    d = np.diff(np.eye(n), axis=0)
    return d.T @ d


@lru_cache(maxsize=8)
def _bgu_regulariser(h, w, gh, gw, gd, lambda_spatial, lambda_z):
    """(within, c_slab): the smoothness terms' part of N in the slab layout of hg_bgu_normal.  `within` (m, m) couples
    the unknowns of one slab (first differences along the shorter axis, second differences in z with first differences
    at both ends); along the slab axis the first differences add c_slab * (number of neighbouring slabs) to a slab's
    diagonal and -c_slab to the diagonal of each off-diagonal block."""
    bx, by, bz = w / gw, h / gh, 1.0 / gd
    cy, cx = (bx * bz / by) * lambda_spatial, (by * bz / bx) * lambda_spatial
    cz = (bx * by / (bz * bz)) * lambda_z
    c_slab, c_in = (cy, cx) if bgu_slab_axis(gh, gw) == 0 else (cx, cy)
    T = min(gh, gw)
    dz = np.zeros((gd, gd))
    dz[0, 0], dz[0, 1] = -1, 1
    for z in range(gd - 2):
        dz[z + 1, z:z + 3] = (1, -2, 1)
    dz[gd - 1, gd - 2], dz[gd - 1, gd - 1] = 1, -1
    within = c_in ** 2 * np.kron(_path_laplacian(T), np.eye(gd)) + cz ** 2 * np.kron(np.eye(T), dz.T @ dz)
    return torch.from_numpy(np.kron(within, np.eye(4))), c_slab ** 2


@lru_cache(maxsize=4)
def _bgu_regulariser_on(h, w, gh, gw, gd, lambda_spatial, lambda_z, device):
    """_bgu_regulariser with its block resident on `device`."""
    within, c = _bgu_regulariser(h, w, gh, gw, gd, lambda_spatial, lambda_z)
    return within.to(torch.device(device)), c


def bgu_regulariser_blocks(h, w, gh, gw, gd=BGU_DEPTH, lambda_spatial=1.0, lambda_z=4e-7):
    """The smoothness terms' R^T R as (diag (S, m, m), off (S - 1, m, m)) fp64 host tensors in the slab layout."""
    within, c = _bgu_regulariser(h, w, gh, gw, gd, float(lambda_spatial), float(lambda_z))
    S, m = max(gh, gw), within.shape[0]
    diag = within.repeat(S, 1, 1)
    off = torch.zeros((S - 1, m, m), dtype=torch.float64)
    _add_slab_coupling(diag, off, c)
    return diag, off


def _add_slab_coupling(diag, off, c):
    S = diag.shape[0]
    nb = torch.full((S,), 2.0, dtype=torch.float64, device=diag.device)
    nb[0] = nb[-1] = 1.0
    diag.diagonal(dim1=1, dim2=2).add_((c * nb)[:, None])
    off.diagonal(dim1=1, dim2=2).sub_(c)


def block_tridiag_solve(diag, off, rhs):
    """Solve the symmetric positive definite block-tridiagonal system with diagonal blocks diag (S, m, m) and
    sub-diagonal blocks off (S - 1, m, m), off[s] = N[s + 1, s], for rhs (k, S, m) by block Cholesky.  Runs on the
    tensors' device in their dtype; returns (k, S, m)."""
    S = diag.shape[0]
    L, B = [], [None]
    y = []
    for s in range(S):
        d = diag[s]
        r = rhs[:, s].transpose(0, 1)                     # (m, k)
        if s:
            # B_s = off[s-1] L_{s-1}^-T
            b = torch.linalg.solve_triangular(L[s - 1], off[s - 1].transpose(0, 1), upper=False).transpose(0, 1)
            B.append(b)
            d = d - b @ b.transpose(0, 1)
            r = r - b @ y[s - 1]
        L.append(torch.linalg.cholesky(d))
        y.append(torch.linalg.solve_triangular(L[s], r, upper=False))
    x = [None] * S
    for s in range(S - 1, -1, -1):
        r = y[s]
        if s + 1 < S:
            r = r - B[s + 1].transpose(0, 1) @ x[s + 1]
        x[s] = torch.linalg.solve_triangular(L[s].transpose(0, 1), r, upper=True)
    return torch.stack(x, 0).permute(2, 0, 1).contiguous()


def bgu_unknowns_to_gamma(x, gh, gw, gd=BGU_DEPTH):
    """(3, S, m) solutions in the slab layout -> gamma (gh, gw, gd, 3, 4)."""
    S, T = max(gh, gw), min(gh, gw)
    x = x.reshape(3, S, T, gd, 4)                          # [i][s][t][z][j]
    x = x.permute(1, 2, 3, 0, 4) if bgu_slab_axis(gh, gw) == 0 else x.permute(2, 1, 3, 0, 4)
    return x.contiguous()


def _bgu_pair(in_ds, out_ds, weight, what):
    need_gpu(in_ds, what, _FOUND)
    need_gpu(out_ds, what, _FOUND)
    if in_ds.dim() != 3 or in_ds.shape[0] != 3 or in_ds.shape != out_ds.shape:
        raise ValueError(f'{what}: in_ds and out_ds must both be (3, h, w), got {tuple(in_ds.shape)} and '
                         f'{tuple(out_ds.shape)}')
    if weight is not None:
        need_gpu(weight, what, _FOUND)
        if tuple(weight.shape) != tuple(in_ds.shape[1:]):
            raise ValueError(f'{what}: weight must be (h, w) = {tuple(in_ds.shape[1:])}, got {tuple(weight.shape)}')
        weight = weight.float().contiguous()
        if not bool((weight >= 0).all()):                 # NaN included: the fit takes sqrt(weight)
            raise ValueError(f'{what}: weight must be non-negative')
    return in_ds.float().contiguous(), out_ds.float().contiguous(), weight


def bgu_normal(in_ds, out_ds, weight=None, grid=None, gd=BGU_DEPTH):
    """hg_bgu_normal: (diag, off, rhs) of the data term, fp64 on the device, in the slab layout of include/hg_post.h.
    grid: (gh, gw), default bgu_grid_size."""
    x, o, wt = _bgu_pair(in_ds, out_ds, weight, 'bgu_normal')
    _, h, w = x.shape
    gh, gw = grid if grid is not None else bgu_grid_size(h, w)
    S, m = max(gh, gw), min(gh, gw) * gd * 4
    dev = x.device
    with on_device(dev):
        diag = torch.empty((S, m, m), dtype=torch.float64, device=dev)
        off = torch.empty((S - 1, m, m), dtype=torch.float64, device=dev)
        rhs = torch.empty((3, S, m), dtype=torch.float64, device=dev)
        nb = lib.hg_bgu_normal_workspace_bytes(gh, gw, gd)
        ws = workspace(nb, dev)
        check(lib.hg_bgu_normal(x.data_ptr(), o.data_ptr(), ptr(wt), h, w, gh, gw, gd,
                                diag.data_ptr(), off.data_ptr(), rhs.data_ptr(), ws.data_ptr(), nb, raw_stream(dev)),
              'hg_bgu_normal')
    return diag, off, rhs


def bgu_fit(in_ds, out_ds, weight=None, lambda_spatial=1.0, lambda_z=4e-7):
    """upsampling/bguFit.m with its defaults (second-derivative intensity constraint towards 0): the (gh, gw, 8) grid
    of 3x4 affine models that maps in_ds onto out_ds, both fp32 (3, h, w) on the device; weight: optional non-negative
    (h, w) map of where out_ds is defined.  The reference solves the stacked least-squares system with `A \\ b`; here
    the data term's normal equations come from hg_bgu_normal in fp64, the smoothness terms are added from a cached
    host table, and the block-tridiagonal system is solved by block Cholesky in fp64 on the device.  Returns gamma
    fp32 (gh, gw, 8, 3, 4)."""
    if lambda_spatial <= 0:
        raise ValueError('bgu_fit: lambda_spatial must be positive')
    in_ds, out_ds, weight = _bgu_pair(in_ds, out_ds, weight, 'bgu_fit')
    _, h, w = in_ds.shape
    gh, gw = bgu_grid_size(h, w)
    diag, off, rhs = bgu_normal(in_ds, out_ds, weight, (gh, gw))
    within, c = _bgu_regulariser_on(h, w, gh, gw, BGU_DEPTH, float(lambda_spatial), float(lambda_z), str(diag.device))
    with on_device(diag.device):
        diag += within
        _add_slab_coupling(diag, off, c)
        x = block_tridiag_solve(diag, off, rhs)
        return bgu_unknowns_to_gamma(x, gh, gw).float()


def bgu_slice(gamma, photo_u8, quantize=True):
    """upsampling/bguSlice.m: gamma (gh, gw, gd, 3, 4) interpolated trilinearly at (x, y, luminance) of every pixel of
    photo_u8, uint8 (H, W, 3) with any row stride, and applied to it.  Returns uint8 (H, W, 3) = round(255 clip(v, 0, 1))
    (MATLAB imwrite of a double image) when quantize, else the unclipped fp32 (3, H, W)."""
    need_gpu(gamma, 'bgu_slice', _FOUND)
    need_gpu(photo_u8, 'bgu_slice', _FOUND)
    if gamma.dim() != 5 or tuple(gamma.shape[3:]) != (3, 4):
        raise ValueError(f'bgu_slice: gamma must be (gh, gw, gd, 3, 4), got {tuple(gamma.shape)}')
    if photo_u8.dtype != torch.uint8 or photo_u8.dim() != 3 or photo_u8.shape[2] != 3:
        raise ValueError(f'bgu_slice: the photo must be uint8 (H, W, 3), got {photo_u8.dtype} {tuple(photo_u8.shape)}')
    g = gamma.float().contiguous()
    gh, gw, gd = g.shape[:3]
    H, W, _ = photo_u8.shape
    if min(photo_u8.stride()) < 0:
        photo_u8 = photo_u8.contiguous()
    dev = photo_u8.device
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if quantize else \
        torch.empty((3, H, W), dtype=torch.float32, device=dev)
    with on_device(dev):
        check(lib.hg_bgu_slice(g.data_ptr(), gh, gw, gd, photo_u8.data_ptr(), photo_u8.stride(0), photo_u8.stride(1),
                               photo_u8.stride(2), out.data_ptr(), int(quantize), H, W, raw_stream(dev)),
              'hg_bgu_slice')
    return out


def bgu_upsampling(target, reference, weight=None, max_side=300, quantize=False):
    """upsampling/BGU.m on the GPU: carry the low-resolution recolouring `target` back to the photo `reference` by
    fitting a bilateral grid of affine colour models at low resolution and slicing it at full resolution, so the
    result keeps the photo's own detail and its exact size (no padding).

    target: float (1, 3, h, w) / (3, h, w); it is quantised to uint8 as torchvision's save_image writes it and read
    back as v / 255, because the reference fits to the written file.  The JPEG loss of that file is deliberately NOT
    modelled: the fit sees the exact 8-bit image.  A target with a side above max_side is resized to
    max_side x max_side (bicubic, antialiased), as the reference does at 300.  reference: uint8 (H, W, 3), read as
    v / 255 and resized to the target's size for the fit.  weight: optional (h, w) map at the fit's resolution.
    Returns fp32 (1, 3, H, W), not clipped, or uint8 (H, W, 3) = round(255 clip(v, 0, 1)) when quantize."""
    need_gpu(target, 'bgu_upsampling', _FOUND)
    need_gpu(reference, 'bgu_upsampling', _FOUND)
    if reference.dtype != torch.uint8 or reference.dim() != 3 or reference.shape[2] != 3:
        raise ValueError(f'bgu_upsampling: reference must be uint8 (H, W, 3), got {reference.dtype} '
                         f'{tuple(reference.shape)}')
    with on_device(reference.device):
        out_ds = u8_hwc_to_float(float_to_u8_hwc(_as_chw3(target, 'target')))
        if out_ds.shape[1] > max_side or out_ds.shape[2] > max_side:
            out_ds = imresize(out_ds, output_shape=(max_side, max_side))
        if weight is not None and tuple(weight.shape) != tuple(out_ds.shape[1:]):
            raise ValueError(f'bgu_upsampling: weight must have the size the fit runs at, {tuple(out_ds.shape[1:])} '
                             f'(the target, or max_side x max_side when it is larger), got {tuple(weight.shape)}')
        in_ds = imresize(u8_hwc_to_float(reference), output_shape=tuple(out_ds.shape[1:]))
        gamma = bgu_fit(in_ds, out_ds, weight)
        out = bgu_slice(gamma, reference, quantize=quantize)
    return out if quantize else out.unsqueeze(0)


# ---- writer -----------------------------------------------------------------------------------------------------------
def save_rgb(u8_hwc, path):
    """Write one uint8 (H, W, 3) image with PIL's defaults -- what torchvision.utils.save_image writes for a batch of
    one (no grid border)."""
    from PIL import Image
    arr = u8_hwc.cpu().numpy() if torch.is_tensor(u8_hwc) else np.asarray(u8_hwc)
    Image.fromarray(arr).save(path)
