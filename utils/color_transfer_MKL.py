"""Drop-in for the reference's utils/color_transfer_MKL.py (`from utils import color_transfer_MKL as ct`,
ReHistoGAN/rehistoGAN.py:28): the Monge-Kantorovich linear colour transfer with the image passes on the GPU
(histogan_amd/post.py over include/hg_post.h: fp64 colour moments, per-pixel affine) and the 3x3 algebra (`MKL`) on the
host in fp64."""
import numpy as np
import torch

from histogan_amd import post as _post
from histogan_amd.post import EPS, MKL  # noqa: F401


def color_transfer_MKL(source, target):
    """source, target: (H, W, 3) arrays; returns the recoloured source as a float64 (H, W, 3) array in [0, 1]."""
    source, target = np.asarray(source), np.asarray(target)
    if source.ndim != 3 or source.shape[-1] != 3:
        raise ValueError(f'color_transfer_MKL: images must be (H, W, 3), got source {source.shape}')
    dev = torch.device('cuda', torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    out, _ = _post.color_transfer_mkl(up(source), up(target))
    return out.cpu().numpy().astype(np.float64)
