"""RGB-uv histogram + Hellinger loss as torch.autograd Functions over the HIP C ABI.

Host-side mirror of histogram_classes/RGBuvHistBlock.py:75-228 (forward) and of the autograd
replay of it; Hellinger loss of histoGAN/histoGAN.py:957-960.  PyTorch is used only for device
memory (caching allocator), the current stream and autograd plumbing.
"""
import os
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import HgHistParams, check, lib, need_gpu, on_device, raw_stream, workspace

_IDX_CACHE = {}


def _sampling_idx(size, h, device):
    """torch.LongTensor(np.linspace(0, size, h, endpoint=False)) of RGBuvHistBlock.py:82-87."""
    key = (size, h, str(device))
    t = _IDX_CACHE.get(key)
    if t is None:
        t = torch.from_numpy(np.linspace(0, size, h, endpoint=False).astype(np.int64).astype(np.int32)).to(device)
        _IDX_CACHE[key] = t
    return t


class HistConfig:
    """Immutable description of one RGBuvHistBlock (ctor args, RGBuvHistBlock.py:29-73)."""
    __slots__ = ('h', 'insz', 'resizing', 'method', 'sigma', 'intensity_scale', 'lo', 'hi', 'green_only', 'projection')

    def __init__(self, h=64, insz=150, resizing='interpolation', method='inverse-quadratic', sigma=0.02,
                 intensity_scale=True, hist_boundary=None, green_only=False, projection='rgbuv'):
        """projection: 'rgbuv' (RGBuvHistBlock, 3 planes, default boundary [-3,3]), 'rgchroma' (rgChromaHistBlock),
        'direct' (LabHistBlock: the input already is normalised Lab) or 'lab' (LabHistBlock(from_rgb=True): the input is
        sRGB and every clamped / resized pixel is converted to normalised CIE Lab first, include/hg_hist.h HG_PROJ_LAB):
        one plane, default boundary [0,1]."""
        if projection not in _lib.HG_PROJ:
            raise ValueError(f'unknown projection {projection!r}')
        self.projection = projection
        if hist_boundary is None:
            hist_boundary = [-3, 3] if projection == 'rgbuv' else [0, 1]
        hb = sorted(hist_boundary)
        self.h, self.insz, self.resizing, self.method = int(h), insz, resizing, method
        self.sigma = sigma
        self.intensity_scale, self.green_only = bool(intensity_scale), bool(green_only)
        self.lo, self.hi = float(hb[0]), float(hb[1])


def check_weight(x, weight, weight_grad=False):
    """Validate a per-pixel weight map for x (B, C, H, W) and return it as a detached fp32 (B, H, W) view (no copy for
    fp32 input: the kernels take any strides).  (B, 1, H, W) or (B, H, W); it is a constant of the histogram -- unless
    weight_grad: then a map that requires grad is accepted and the view stays in its autograd graph."""
    if not torch.is_tensor(weight):
        raise ValueError(f'weight must be a tensor, got {type(weight).__name__}')
    if weight.requires_grad and not weight_grad:
        raise ValueError('weight requires grad, but the histogram produces no gradient for its weight map '
                         '(pass weight.detach())')
    B, _, H, W = x.shape
    if tuple(weight.shape) == (B, 1, H, W):
        weight = weight[:, 0]
    elif tuple(weight.shape) != (B, H, W):
        raise ValueError(f'weight must have shape {(B, 1, H, W)} or {(B, H, W)} for an input of shape '
                         f'{tuple(x.shape)}, got {tuple(weight.shape)}')
    return weight if weight.dtype == torch.float32 else weight.float()


def _make_params(x, cfg, pre_relu=False, weight=None):
    if x.dim() != 4 or x.shape[1] < 3:
        raise ValueError(f'expected (B, C>=3, H, W) input, got {tuple(x.shape)}')
    if cfg.method not in _lib.HG_METHOD:
        raise Exception(f'Wrong kernel method. It should be either thresholding, RBF,'
                        f' inverse-quadratic. But the given value is {cfg.method}.')
    B, C, H, W = x.shape
    p = HgHistParams()
    p.struct_size = ctypes.sizeof(HgHistParams)
    p.B, p.C, p.H, p.W = B, C, H, W
    p.stride_b, p.stride_c, p.stride_h, p.stride_w = x.stride()
    keep = []
    if H > cfg.insz or W > cfg.insz:
        if cfg.resizing == 'interpolation':
            p.resize_mode, p.Hs, p.Ws = _lib.HG_RESIZE_BILINEAR, int(cfg.insz), int(cfg.insz)
        elif cfg.resizing == 'sampling':
            r, c = _sampling_idx(H, cfg.h, x.device), _sampling_idx(W, cfg.h, x.device)
            keep = [r, c]
            p.resize_mode, p.Hs, p.Ws = _lib.HG_RESIZE_SAMPLING, cfg.h, cfg.h
            p.row_idx, p.col_idx = r.data_ptr(), c.data_ptr()
        else:
            raise Exception(f'Wrong resizing method. It should be: interpolation or sampling. '
                            f'But the given value is {cfg.resizing}.')
    else:
        p.resize_mode, p.Hs, p.Ws = _lib.HG_RESIZE_NONE, H, W
    p.h, p.lo, p.hi = cfg.h, cfg.lo, cfg.hi
    p.method = _lib.HG_METHOD[cfg.method]
    p.sigma = float(cfg.sigma) if cfg.method != 'thresholding' else 1.0
    p.intensity_scale, p.green_only = int(cfg.intensity_scale), int(cfg.green_only)
    p.projection = _lib.HG_PROJ[cfg.projection]
    p.pre_relu = int(bool(pre_relu))
    if weight is not None:                      # (B, H, W) fp32 on x's device (check_weight), any strides
        p.weight = weight.data_ptr()
        p.weight_stride_b, p.weight_stride_h, p.weight_stride_w = weight.stride()
    return p, keep


def _ws_bytes(p):
    f, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(lib.hg_rgbuv_hist_workspace_bytes(ctypes.byref(p), ctypes.byref(f), ctypes.byref(b)),
          'hg_rgbuv_hist_workspace_bytes')
    return f.value, b.value


_FOUND = 'input is on {}'     # need_gpu's wording here
_stream = raw_stream           # the former name, still bound: the C-ABI tests of the weighted histogram reach it


class RGBuvHistFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg, pre_relu=False, weight=None):
        # weight: None or a map already validated by rgbuv_hist (check_weight): fp32 (B, H, W) on x's device.  It is an
        # autograd input like x: a map that requires grad (weight_grad=True callers only) gets its gradient in backward
        need_gpu(x, 'RGBuvHistFunction', _FOUND)
        x = x.detach()
        if x.dtype != torch.float32:
            x = x.float()
        p, keep = _make_params(x, cfg, pre_relu, weight)
        ctx.pre_relu = pre_relu
        ctx.weight = None if weight is None else weight.detach()      # kept alive for the backward call, not saved
        ctx.weight_grad = weight is not None and ctx.needs_input_grad[3]
        fwd_b, _ = _ws_bytes(p)
        with on_device(x.device):
            # per-pixel projection cache for the backward (32 B per histogram pixel): only when a gradient will be asked
            # for and only when the dense MFMA kernels will run (the scatter paths -- thresholding, narrow RBF --
            # re-classify pixels cheaply and ignore it)
            cache = None
            if (ctx.needs_input_grad[0] or ctx.weight_grad) and lib.hg_rgbuv_hist_uses_proj_cache(ctypes.byref(p)) == 1:
                cache = torch.empty((p.B, p.Hs * p.Ws, 8), dtype=torch.float32, device=x.device)
                p.proj_cache = cache.data_ptr()
            ctx.cache = cache
            P = 1 if (cfg.green_only or cfg.projection != 'rgbuv') else 3
            out = torch.empty((p.B, P, cfg.h, cfg.h), dtype=torch.float32, device=x.device)
            sums = torch.empty((p.B,), dtype=torch.float32, device=x.device)
            ws = workspace(fwd_b, x.device)
            check(lib.hg_rgbuv_hist_fwd(ctypes.byref(p), x.data_ptr(), out.data_ptr(), sums.data_ptr(),
                                        ws.data_ptr(), ws.numel(), raw_stream(x.device)), 'hg_rgbuv_hist_fwd')
        ctx.cfg = cfg
        ctx.save_for_backward(x, out, sums)
        ctx._keep = keep
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, out, sums = ctx.saved_tensors
        cfg = ctx.cfg
        p, keep = _make_params(x, cfg, ctx.pre_relu, ctx.weight)
        if ctx.cache is not None:
            p.proj_cache = ctx.cache.data_ptr()
        if ctx.weight_grad:
            nb = ctypes.c_size_t(0)
            check(lib.hg_rgbuv_hist_bwd_w_workspace_bytes(ctypes.byref(p), ctypes.byref(nb)),
                  'hg_rgbuv_hist_bwd_w_workspace_bytes')
            bwd_b = nb.value
        else:
            _, bwd_b = _ws_bytes(p)
        g = grad_out.detach()
        if g.dtype != torch.float32:
            g = g.float()
        g = g.contiguous()
        with on_device(x.device):
            gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            ws = workspace(bwd_b, x.device)
            if ctx.weight_grad:               # (B, H, W), the shape forward was given; autograd undoes the caller's views
                gw = torch.empty(ctx.weight.shape, dtype=torch.float32, device=x.device)
                check(lib.hg_rgbuv_hist_bwd_w(ctypes.byref(p), x.data_ptr(), g.data_ptr(), out.data_ptr(),
                                              sums.data_ptr(), gx.data_ptr(), gw.data_ptr(), ws.data_ptr(), ws.numel(),
                                              raw_stream(x.device)), 'hg_rgbuv_hist_bwd_w')
                return gx, None, None, gw
            check(lib.hg_rgbuv_hist_bwd(ctypes.byref(p), x.data_ptr(), g.data_ptr(), out.data_ptr(),
                                        sums.data_ptr(), gx.data_ptr(), ws.data_ptr(), ws.numel(),
                                        raw_stream(x.device)), 'hg_rgbuv_hist_bwd')
        return gx, None, None, None


class WeightGradCall:
    """Mixin of the drop-in histogram modules: `block(x, ..., weight=w, weight_grad=True)`.  The keyword is taken by the
    call, not by forward() (whose parameter list stays the reference's plus the documented extensions), and runs the
    module's forward_weight_grad(); without it the call is nn.Module's, unchanged."""

    def __call__(self, *args, weight_grad=False, **kwargs):
        if not weight_grad:
            return super().__call__(*args, **kwargs)
        return self.forward_weight_grad(*args, **kwargs)


def run_block(x, cfg, device, what, pre_relu=False, weight=None, weight_grad=False):
    """forward() of the drop-in histogram modules: resolves the module's `device` argument the way the reference does
    ('cuda', 'cpu', an ordinal, a torch.device).  weight_grad: the weight map is a differentiable input (rgbuv_hist_wgrad).

    device='cpu' is what the reference's Dataset uses inside forked DataLoader workers (histoGAN/histoGAN.py:263-266,
    296-302): that call runs `hist_cpu.hist_cpu` -- PyTorch CPU ops only, no HIP call, no GPU memory (SURVEY.md
    section 8b: the replacement must not touch the GPU when device='cpu').  It is a separate implementation for that
    contract, not a fallback: a GPU module never takes it, and the HIP functions keep refusing CPU tensors."""
    dev = torch.device('cuda', device) if isinstance(device, int) else torch.device(device)
    if dev.type != 'cuda':
        from .hist_cpu import hist_cpu
        if weight is not None and torch.is_tensor(weight) and weight.is_cuda:
            weight = weight.cpu()
        return hist_cpu(x if not x.is_cuda else x.cpu(), cfg, pre_relu, weight, weight_grad=weight_grad)
    if not x.is_cuda:
        x = x.to(dev)
    if weight is not None and torch.is_tensor(weight) and weight.device != x.device:
        weight = weight.to(x.device)          # a CPU weight map follows x to the module's GPU
    return _rgbuv_hist(x, cfg, pre_relu, weight, weight_grad)


def rgbuv_hist(x, cfg, pre_relu=False, weight=None):
    """Differentiable RGB-uv histogram of x (B,C>=3,H,W) -> (B, 3|1, h, h), on x's GPU.  pre_relu: the result and
    gradient of `rgbuv_hist(F.relu(x))` (the train step's call, histoGAN/histoGAN.py:955) without the relu launch.
    weight: optional per-pixel weight map (B, 1, H, W) or (B, H, W), taken as clamp(weight, 0, 1) and resized with the
    image; pixel n counts with weight_n * I_y,n.  A constant: the gradient goes to x only, and a weight that requires
    grad is refused (ValueError).  None = every pixel counts (bit-identical to a map of ones)."""
    return _rgbuv_hist(x, cfg, pre_relu, weight, False)


def rgbuv_hist_wgrad(x, cfg, pre_relu=False, weight=None):
    """rgbuv_hist with the weight map as a differentiable input (`weight_grad=True` of the modules): the map may require
    grad and receives dL/dw -- per histogram pixel (I_y or its stand-in) * sum over planes of k(u)^T Ghat k(v), through the
    adjoint of the resize, and 0 outside the clamp (w < 0, w > 1).  The gradient comes back in the map's own shape; a map
    expanded over an axis is materialised first and autograd reduces its gradient.  The gradient for x is unchanged."""
    return _rgbuv_hist(x, cfg, pre_relu, weight, True)


def _rgbuv_hist(x, cfg, pre_relu, weight, weight_grad):
    if weight is None:
        if weight_grad:
            raise ValueError('weight_grad=True needs a weight map (weight=None)')
        return RGBuvHistFunction.apply(x, cfg, pre_relu)
    if x.dim() != 4 or x.shape[1] < 3:
        raise ValueError(f'expected (B, C>=3, H, W) input, got {tuple(x.shape)}')
    weight = check_weight(x, weight, weight_grad)
    if weight.device != x.device:
        raise ValueError(f'weight is on {weight.device}, the input on {x.device}')
    if weight_grad and weight.requires_grad and 0 in weight.stride():
        # a broadcast map has no element of its own per pixel for the kernels to write a gradient to
        weight = weight.clone(memory_format=torch.contiguous_format)
    return RGBuvHistFunction.apply(x, cfg, pre_relu, weight)


class HellingerFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, target, gen, alpha):
        need_gpu(gen, 'HellingerFunction', _FOUND)
        t = target.detach().float().contiguous()
        g = gen.detach().float().contiguous()
        if t.shape != g.shape:
            raise ValueError(f'shape mismatch {tuple(t.shape)} vs {tuple(g.shape)}')
        n = g.numel()
        with on_device(g.device):
            loss = torch.empty((), dtype=torch.float32, device=g.device)
            grad = torch.empty_like(g)
            wsb = lib.hg_hellinger_workspace_bytes(n)
            ws = torch.empty((wsb,), dtype=torch.uint8, device=g.device)
            check(lib.hg_hellinger_fwd_bwd(t.data_ptr(), g.data_ptr(), n, g.shape[0], float(alpha),
                                           loss.data_ptr(), grad.data_ptr(), ws.data_ptr(), wsb,
                                           raw_stream(g.device)), 'hg_hellinger_fwd_bwd')
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, gl):
        (grad,) = ctx.saved_tensors
        return None, grad * gl, None


class _GlobalHellinger(torch.autograd.Function):
    """The Hellinger loss of the GLOBAL batch under data parallelism: the reference takes ONE square root over the whole
    batch (histoGAN/histoGAN.py:957-960), so the per-rank value sqrt(S_r)/B_r is not a shard of it.  One fp32 all-reduce
    of S_r = sum (sqrt t - sqrt g)^2 gives every rank D = sqrt(sum_r S_r):
        loss = alpha/sqrt2 * D / B_global                                  (the same number on every rank)
        dloss/dg (this rank's samples) = local gradient * (B_r D_r) / (B_global D)
    and because the gradient all-reduce AVERAGES over ranks, the local gradient is scaled by world * that = D_r / D."""

    @staticmethod
    def forward(ctx, local_loss, alpha, batch_local):
        import torch.distributed as dist
        world = dist.get_world_size()
        d_local = local_loss.detach() * (2.0 ** 0.5) * batch_local / alpha          # sqrt(S_r)
        s = (d_local * d_local).reshape(1).clone()
        dist.all_reduce(s, op=dist.ReduceOp.SUM)
        d_glob = torch.sqrt(s[0])
        ctx.scale = d_local / d_glob
        return alpha / (2.0 ** 0.5) * d_glob / (batch_local * world)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.scale, None, None


HELLINGER_LOCAL = os.environ.get('HG_HELLINGER_LOCAL', '0') != '0'


def hellinger_loss(target_hist, gen_hist, alpha=1.0, global_batch=None):
    """alpha/sqrt(2) * sqrt(sum((sqrt(t)-sqrt(g))^2)) / B  (histoGAN/histoGAN.py:957-960).
    Gradient flows to gen_hist only (the reference's d/d target is computed and never used).
    global_batch: under data parallelism, evaluate the formula on the global batch (one scalar all-reduce; default when
    a process group with more than one rank is initialised, HG_HELLINGER_LOCAL=1 for the per-shard formula)."""
    loss = HellingerFunction.apply(target_hist, gen_hist, alpha)
    if global_batch is None:
        from . import ddp
        global_batch = ddp.is_dist() and not HELLINGER_LOCAL
    if global_batch:
        loss = _GlobalHellinger.apply(loss, float(alpha), int(gen_hist.shape[0]))
    return loss
