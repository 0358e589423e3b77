"""Drop-in for the reference's utils/pyramid_upsampling.py (`import utils.pyramid_upsampling as upsampling`,
ReHistoGAN/rehistoGAN.py:29): the same function and signature, computed on the GPU by histogan_amd/post.py over the
kernels of include/hg_post.h (bicubic resize, pyrDown, and pyrUp fused with the Laplacian add).

As in the reference, a reference image whose height or width is not a multiple of 2**levels is bicubic-resized UP to
the next multiple and the output keeps that padded size.  Unlike the reference, a CPU `target` is not clamped in place.
"""
import torch

from histogan_amd import post as _post


def pyramid_upsampling(target, reference, levels=5, swapping_levels=1, blending=False):
    """target (1, 3, h, w), reference (1, 3, H, W) tensors on any device; returns a CPU float64 (1, 3, H', W')."""
    dev = torch.device('cuda', torch.cuda.current_device())
    out = _post.pyramid_upsampling(target.detach().to(dev), reference.detach().to(dev), levels=levels,
                                   swapping_levels=swapping_levels, blending=blending)
    return out.cpu().double()
