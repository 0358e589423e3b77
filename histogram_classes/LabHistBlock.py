"""Drop-in for the reference's histogram_classes/LabHistBlock.py (same import path, ctor, forward): the Lab (a, b)
histogram of an image batch, on the gfx950 kernels of histogan_amd/csrc/hg_hist.hip (projection 'direct' of
include/hg_hist.h: one plane, shared clamp / resize / soft-binning / normalisation code with the RGB-uv block).

The reference leaves the sRGB -> Lab conversion to the caller (its README: "convert loaded images into the CIE LAB space
in the Dataset class").  `from_rgb=True` (an extension) puts that conversion inside the kernels, forward and backward
(projection 'lab'): the module then takes sRGB and is differentiable with respect to it.  histogan_amd.post.srgb_to_lab /
lab_to_srgb are the same conversion as stand-alone, non-differentiable data-side tools.
"""
import torch
import torch.nn as nn

from histogan_amd.hist import HistConfig, WeightGradCall, run_block

EPS = 1e-6


class LabHistBlock(WeightGradCall, nn.Module):
  def __init__(self, h=64, insz=150, resizing='interpolation',
               method='inverse-quadratic', sigma=0.02, intensity_scale=False,
               hist_boundary=None, device='cuda', from_rgb=False):
    """Same arguments as the reference class (LabHistBlock.py:30-71): h bins per axis; images larger than insz
    are resized ('interpolation' / 'sampling'); method in {'thresholding', 'RBF', 'inverse-quadratic'}; sigma;
    intensity_scale (weight = the L channel); hist_boundary (default [0, 1], sorted in place).  `device`: a GPU, or
    'cpu' for the HIP-free implementation (histogan_amd/hist_cpu.py).
    from_rgb (an extension, default False = the reference's behaviour): False -- the input is normalised CIE Lab,
    channels (L/100, (a+128)/255, (b+128)/255), binned as it is.  True -- the input is sRGB in [0, 1]; after the clamp and
    the resize every pixel is converted to that normalised Lab (D65, evaluated in fp64 and rounded once to fp32:
    include/hg_hist.h, HG_PROJ_LAB) and then binned; the gradient comes back with respect to the sRGB input.  The whole
    sRGB gamut lies inside the default boundary [0, 1]."""
    super(LabHistBlock, self).__init__()
    self.h = h
    self.insz = insz
    self.device = device
    self.from_rgb = bool(from_rgb)
    self.resizing = resizing
    self.method = method
    self.intensity_scale = intensity_scale
    if hist_boundary is None:
      hist_boundary = [0, 1]
    hist_boundary.sort()
    self.hist_boundary = hist_boundary
    if self.method == 'thresholding':
      self.eps = (abs(hist_boundary[0]) + abs(hist_boundary[1])) / h
    else:
      self.sigma = sigma

  def _config(self):
    return HistConfig(h=self.h, insz=self.insz, resizing=self.resizing, method=self.method,
                      sigma=getattr(self, 'sigma', 0.02), intensity_scale=self.intensity_scale,
                      hist_boundary=list(self.hist_boundary), projection='lab' if self.from_rgb else 'direct')

  def forward(self, x, weight=None):
    """x: float (B, C>=3, H, W) -> float32 (B, 1, h, h), L1-normalised per image, on `device`.  x is normalised Lab
    (from_rgb=False) or sRGB (from_rgb=True: L_n below is then the converted pixel's L / 100).
    weight (an extension; the reference signature is forward(x)): optional per-pixel weight map (B, 1, H, W) or
    (B, H, W), taken as clamp(weight, 0, 1) and resized with the image; pixel n counts with
    weight_n * L_n (weight_n alone without intensity_scale).  A constant: no gradient is produced for it.
    Calling the module with weight_grad=True -- block(x, weight=w, weight_grad=True) -- runs forward_weight_grad."""
    return run_block(x, self._config(), self.device, 'LabHistBlock', weight=weight)

  def forward_weight_grad(self, x, weight=None):
    """forward() with the weight map as a differentiable input: the map may require grad and receives the histogram's
    gradient (in its own shape; exactly 0 where the map is below 0 or above 1); weight=None raises ValueError."""
    return run_block(x, self._config(), self.device, 'LabHistBlock', weight=weight, weight_grad=True)
