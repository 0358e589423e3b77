"""Drop-in for the reference's utils/imresize.py (`import utils.imresize as resize`, utils/pyramid_upsampling.py:4):
the same function names and signatures, MATLAB-style imresize computed on the GPU by histogan_amd/post.py over the
separable-resize kernel of include/hg_post.h.  Tables are built on the host in fp64 exactly as the reference builds
them; the image passes run in fp32.  Returns what the reference returns: float64 for float input, uint8 (clip +
round half to even after each pass) for uint8 input."""
from math import ceil

import numpy as np
import torch

from histogan_amd import post as _post
from histogan_amd.post import cubic, triangle  # noqa: F401  (re-exported: the reference's kernel functions)


def deriveSizeFromScale(img_shape, scale):
    return [int(ceil(scale[k] * img_shape[k])) for k in range(2)]


def deriveScaleFromSize(img_shape_in, img_shape_out):
    return [1.0 * img_shape_out[k] / img_shape_in[k] for k in range(2)]


def contributions(in_length, out_length, scale, kernel, k_width):
    """The reference's (weights, indices), shaped (out_length, 1, taps) as it returns them."""
    w, i = _post.contributions(in_length, out_length, scale, kernel, k_width)
    return w[:, None, :], i[:, None, :]


def imresize(I, scalar_scale=None, method='bicubic', output_shape=None, mode="vec"):
    """I: (H, W) or (H, W, C) numpy array.  `mode` is accepted for compatibility; both of the reference's modes
    compute the same result and here the GPU computes it."""
    if method not in _post.KERNELS:
        raise ValueError(f"imresize: method must be 'bicubic' or 'bilinear', not {method!r}")
    if scalar_scale is None and output_shape is None:
        raise ValueError('imresize: scalar_scale OR output_shape should be defined')
    I = np.asarray(I)
    dev = torch.device('cuda', torch.cuda.current_device())
    if I.dtype == np.uint8:
        out = _post.imresize(torch.from_numpy(np.ascontiguousarray(I)).to(dev), output_shape=output_shape,
                             scalar_scale=scalar_scale, method=method)
        return out.cpu().numpy()
    x = torch.from_numpy(np.ascontiguousarray(I, dtype=np.float32)).to(dev)
    x = x if x.dim() == 2 else x.permute(2, 0, 1)            # (C, H, W) view of the HWC upload, no copy
    out = _post.imresize(x, output_shape=output_shape, scalar_scale=scalar_scale, method=method).cpu().numpy()
    out = out if out.ndim == 2 else out.transpose(1, 2, 0)
    return np.ascontiguousarray(out, dtype=np.float64)


def convertDouble2Byte(I):
    return np.around(255 * np.clip(I, 0.0, 1.0)).astype(np.uint8)
