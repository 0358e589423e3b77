"""Dense contraction of the HistoGAN networks on the hand-written fp32-MFMA kernels of include/hg_conv.h.

`conv2d(x, w, bias=None, stride=1)` == `F.conv2d(x, w, bias, stride=stride, padding=k//2)` for k in {1, 3}
(stride 2 only for k = 3) -- the contraction inside Conv2DMod.forward (histoGAN/histoGAN.py:431-439, executed
with the shared weight on modulated activations) and every convolution of the discriminator (:510-518).

A convolution is bilinear in (x, w), so its output, data gradient and weight gradient are closed under
differentiation.  The three autograd Functions below call each other in their backward passes, which makes
the op differentiable to any order with only the three kernels (k_conv forward/dgrad, k_wgrad) -- the
gradient penalty (histoGAN/histoGAN.py:156-163) needs the second order.
"""
import contextlib
import functools
import os

import torch

from ._lib import check, f32c, lib, on_device, ptr, raw_stream, stream_of, workspace
from .launch import channel_sum
# The weight side: packed operands and their cache, flat gradient slots, the weight-gradient stream.  The launch wrappers reach
# the two operand accessors as `_wino_u` / `_direct_operand` of THIS module: replacing `_wino_u` switches the Winograd route off.
from .wpack import (PACK_DGRAD, PACK_FWD, WINO, _pack_weights, _wino_pack, build_pack_plans, cached,  # noqa: F401
                    drain_pack_streams, enable_pack_cache, grad_slot, on_wgrad_stream, pack_weights, prepack_async,
                    side_stream, weights_changed, wino_supported)
from .wpack import direct_operand as _direct_operand
from .wpack import wino_operand as _wino_u

_skip_wgrad = False
WINO_WGRAD = os.environ.get('HG_WINO_WGRAD', '1') != '0'


@functools.lru_cache(maxsize=None)
def wino_wgrad_supported(B, K, N, H, W):
    return bool(WINO and WINO_WGRAD and lib.hg_wino_wgrad_supported(B, K, N, H, W))


def wino_conv(x, u, N, iscale=None, oscale=None, bias=None, noise_w=None, noise_img=None, noise_S=0, slope=0.0, addend=None):
    """hg_wino_conv2d: the fused epilogue of hg_modconv2d_fwd / hg_conv2d_fwd_add on the Winograd form."""
    B, K, H, W = x.shape
    with on_device(x.device):
        out = torch.empty((B, N, H, W), dtype=torch.float32, device=x.device)
        nb = lib.hg_wino_workspace_bytes(B, K, N, H, W)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device) if nb else None
        check(lib.hg_wino_conv2d(x.data_ptr(), u.data_ptr(), out.data_ptr(), ptr(iscale), ptr(oscale), ptr(bias),
                                 ptr(noise_w), ptr(noise_img), noise_S, float(slope), ptr(addend), B, K, N, H, W,
                                 ptr(ws), nb, stream_of(x)), 'hg_wino_conv2d')
    return out


def modconv_fwd_packed(x, wt, N, ksize, iscale=None, oscale=None, bias=None, noise_w=None, noise_img=None, noise_S=0,
                       slope=0.0):
    """hg_modconv2d_fwd (stride 1): lrelu(oscale * conv(iscale * x) + bias + noise_w * noise_img) in one launch."""
    B, K, H, W = x.shape
    if ksize == 3 and (noise_img is None or noise_S % 2 == 0):
        u = _wino_u(wt, B, K, N, H, W)
        if u is not None:
            return wino_conv(x, u, N, iscale, oscale, bias, noise_w, noise_img, noise_S, slope)
    with on_device(x.device):
        out = torch.empty((B, N, H, W), dtype=torch.float32, device=x.device)
        nb = lib.hg_conv2d_workspace_bytes(B, K, N, H, W, ksize, 1, 0)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device) if nb else None
        check(lib.hg_modconv2d_fwd(x.data_ptr(), _direct_operand(wt).data_ptr(), out.data_ptr(), ptr(iscale), ptr(oscale), ptr(bias),
                                   ptr(noise_w), ptr(noise_img), noise_S, float(slope), B, K, N, H, W, ksize, ptr(ws), nb,
                                   stream_of(x)), 'hg_modconv2d_fwd')
    return out


@contextlib.contextmanager
def input_grads_only():
    """Inside this context the backward of conv2d does not compute weight / bias gradients (they come back as
    None).  For `torch.autograd.grad(out, inputs=images, create_graph=True)` (the gradient penalty), where the
    autograd engine would otherwise make every conv node produce a weight gradient nobody asked for."""
    global _skip_wgrad
    old, _skip_wgrad = _skip_wgrad, True
    try:
        yield
    finally:
        _skip_wgrad = old


def _out_size(n, stride):
    return (n - 1) // stride + 1


def _check_args(x, w, stride):
    if not x.is_cuda:
        raise RuntimeError(f'conv2d: tensor on {x.device}; the MI355X-native path has no CPU implementation')
    Co, Ci, k, k2 = w.shape
    if k != k2 or k not in (1, 3) or stride not in (1, 2) or (stride == 2 and k != 3):
        raise ValueError(f'conv2d: weight {tuple(w.shape)} stride {stride} not supported (1x1 / 3x3 stride 1, 3x3 stride 2)')


def conv_fwd_packed(x, wt, N, ksize, stride=1, iscale=None, oscale=None, bias=None):
    """out[b,n] = oscale[b,n] * sum_k conv(iscale[b,k] * x[b,k], Wt[.,k,n]) + bias[n]   (x: (B,K,H,W) contiguous)."""
    B, K, H, W = x.shape
    if ksize == 3 and stride == 1:
        u = _wino_u(wt, B, K, N, H, W)
        if u is not None:
            return wino_conv(x, u, N, iscale, oscale, bias)
    with on_device(x.device):
        out = torch.empty((B, N, _out_size(H, stride), _out_size(W, stride)), dtype=torch.float32, device=x.device)
        nb = lib.hg_conv2d_workspace_bytes(B, K, N, H, W, ksize, stride, 0)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device) if nb else None
        check(lib.hg_conv2d_fwd(x.data_ptr(), _direct_operand(wt).data_ptr(), out.data_ptr(), ptr(iscale), ptr(oscale), ptr(bias),
                                B, K, N, H, W, ksize, stride, ptr(ws), nb, stream_of(x)), 'hg_conv2d_fwd')
    return out


def conv_fwd_add_packed(x, wt, N, ksize, addend, bias=None, stride=1):
    """out = (conv(x, Wt) + bias[n]) + addend   (addend (B,N,Ho,Wo) contiguous: hg_conv2d_fwd_add)."""
    B, K, H, W = x.shape
    if ksize == 3 and stride == 1 and tuple(addend.shape) == (B, N, H, W):
        u = _wino_u(wt, B, K, N, H, W)
        if u is not None:
            return wino_conv(x, u, N, bias=bias, addend=addend)
    with on_device(x.device):
        out = torch.empty((B, N, _out_size(H, stride), _out_size(W, stride)), dtype=torch.float32, device=x.device)
        if addend.shape != out.shape:
            raise ValueError(f'conv2d_add: addend {tuple(addend.shape)} does not match the output {tuple(out.shape)}')
        nb = lib.hg_conv2d_workspace_bytes(B, K, N, H, W, ksize, stride, 0)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device) if nb else None
        check(lib.hg_conv2d_fwd_add(x.data_ptr(), _direct_operand(wt).data_ptr(), out.data_ptr(), addend.data_ptr(), ptr(bias),
                                    B, K, N, H, W, ksize, stride, ptr(ws), nb, stream_of(x)), 'hg_conv2d_fwd_add')
    return out


def lrelu_bwd_channel_sum(g, out, slope, want_sum=True):
    """(g * (out > 0 ? 1 : slope), its per-channel sum or None) in one pass (hg_lrelu_bwd_channel_sum)."""
    g, out = f32c(g), f32c(out)
    B, C, H, W = g.shape
    with on_device(g.device):
        gm = torch.empty_like(g)
        cs = torch.empty(C, dtype=torch.float32, device=g.device) if want_sum else None
        nb = lib.hg_nets_workspace_bytes(B, C, H, W)
        ws = workspace(nb, g.device)
        check(lib.hg_lrelu_bwd_channel_sum(g.data_ptr(), out.data_ptr(), float(slope), gm.data_ptr(), ptr(cs), B, C, H * W,
                                           ws.data_ptr(), ws.numel(), stream_of(g)), 'hg_lrelu_bwd_channel_sum')
    return gm, cs


def conv_dgrad_packed(g, wt, N, H, W, ksize, stride=1, iscale=None, oscale=None):
    """Data gradient: g (B,K,Ho,Wo) -> (B,N,H,W); wt packed with PACK_DGRAD."""
    B, K = g.shape[:2]
    if ksize == 3 and stride == 1:
        u = _wino_u(wt, B, K, N, H, W)
        if u is not None:
            return wino_conv(g, u, N, iscale, oscale)
    with on_device(g.device):
        gin = torch.empty((B, N, H, W), dtype=torch.float32, device=g.device)
        nb = lib.hg_conv2d_workspace_bytes(B, K, N, H, W, ksize, stride, 1)
        ws = torch.empty(nb, dtype=torch.uint8, device=g.device) if nb else None
        check(lib.hg_conv2d_dgrad(g.data_ptr(), _direct_operand(wt).data_ptr(), gin.data_ptr(), ptr(iscale), ptr(oscale),
                                  B, K, N, H, W, ksize, stride, ptr(ws), nb, stream_of(g)), 'hg_conv2d_dgrad')
    return gin


def conv_wgrad(x, gout, ksize, stride=1, iscale=None, gscale=None, out=None):
    """gw[n,k,dy,dx] = sum_{b,y,x} gscale[b,n] gout[b,n,y,x] * iscale[b,k] x[b,k,y*s+dy-p,x*s+dx-p].
    out: optional contiguous (N,K,k,k) tensor to write (e.g. the weight's slice of a flat gradient buffer)."""
    B, K, H, W = x.shape
    N = gout.shape[1]
    if ksize == 3 and stride == 1 and iscale is None and gscale is None and wino_wgrad_supported(B, K, N, H, W):
        with on_device(x.device):     # Winograd form (include/hg_wino.h): 16 instead of 36 multiplications per tile and (n, k)
            nbytes = lib.hg_wino_wgrad_workspace_bytes(B, K, N, H, W)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            gw = out if out is not None else torch.empty((N, K, 3, 3), dtype=torch.float32, device=x.device)
            check(lib.hg_wino_wgrad(x.data_ptr(), gout.data_ptr(), gw.data_ptr(), B, K, N, H, W, ws.data_ptr(), nbytes, stream_of(x)),
                  'hg_wino_wgrad')
        return gw
    with on_device(x.device):
        nbytes = lib.hg_conv2d_wgrad_workspace_bytes(B, K, N, H, W, ksize, stride)
        ws = workspace(nbytes, x.device)
        gw = out if out is not None else torch.empty((N, K, ksize, ksize), dtype=torch.float32, device=x.device)
        check(lib.hg_conv2d_wgrad(x.data_ptr(), gout.data_ptr(), gw.data_ptr(), ptr(iscale), ptr(gscale),
                                  B, K, N, H, W, ksize, stride, ws.data_ptr(), ws.numel(), stream_of(x)), 'hg_conv2d_wgrad')
    return gw


def _direct_wgrad(w, x, g, stride):
    """Weight gradient of conv(x, w) for upstream gradient g into w's flat-buffer slot on the weight-gradient stream; False if w
    has no writable slot (wpack.grad_slot; or a graph is being recorded): the caller then returns the gradient to autograd."""
    ws = grad_slot(w)
    if ws is None:
        return False
    xc, gc = f32c(x), f32c(g)
    if _batch_pieces(xc, w, stride) != 1:
        return False
    slot, flat, written, index = ws

    def run():
        if written:
            slot.add_(conv_wgrad(xc, gc, w.shape[2], stride))
        else:
            conv_wgrad(xc, gc, w.shape[2], stride, out=slot)
            flat.mark_written(index)
    on_wgrad_stream(x.device, run, (xc, gc))
    return True


def direct_demod_weight_term(w, gd, d, s1):
    """The demodulation coefficient's weight-gradient term (ops._DemodCoeff) added straight to w's flat-buffer slot on
    the weight-gradient stream by one kernel (hg_demod_weight_term: read w, read / write the slot) -- instead of a
    (N x B) @ (B x K) rocBLAS GEMM (314 us at 2048 x 2048: no library kernel for a 32-deep reduction), two element-wise
    launches over the weight, a gradient tensor for autograd and the `both` add of FlatParams.gather.  False: no slot
    (or a higher-order pass / a recording graph) -- the caller returns the term to autograd."""
    ws = grad_slot(w)
    if ws is None:
        return False
    slot, flat, written, index = ws
    gd, d, s1 = f32c(gd), f32c(d), f32c(s1)
    B, N = d.shape
    K, taps = w.shape[1], w.shape[2] * w.shape[3]

    def run():
        with on_device(w.device):
            check(lib.hg_demod_weight_term(w.data_ptr(), gd.data_ptr(), d.data_ptr(), s1.data_ptr(), slot.data_ptr(), B, N, K,
                                           taps, int(written), raw_stream(w.device)), 'hg_demod_weight_term')
        flat.mark_written(index)
    on_wgrad_stream(w.device, run, (gd, d, s1))
    return True


class _Conv(torch.autograd.Function):
    """y = conv(x, w) + bias."""

    @staticmethod
    def forward(ctx, x, w, bias, stride):
        _check_args(x, w, stride)
        if x.shape[1] != w.shape[1]:
            raise ValueError(f'conv2d: x {tuple(x.shape)} does not match w {tuple(w.shape)}')
        ctx.save_for_backward(x, w)
        ctx.stride, ctx.has_bias = stride, bias is not None
        xc, wc = f32c(x), f32c(w)
        bc = None if bias is None else f32c(bias)
        return conv_fwd_packed(xc, pack_weights(wc, PACK_FWD), w.shape[0], w.shape[2], stride, bias=bc)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _ConvDgrad.apply(g, w, x.shape[2], x.shape[3], ctx.stride)
        if not _skip_wgrad:
            if ctx.needs_input_grad[1] and not _direct_wgrad(w, x, g, ctx.stride):
                gw = _ConvWgrad.apply(g, x, w.shape[2], ctx.stride)
            if ctx.has_bias and ctx.needs_input_grad[2]:
                if torch.is_grad_enabled():     # higher-order pass: keep the sum on the autograd tape
                    gb = g.sum(dim=(0, 2, 3))
                else:
                    gb = channel_sum(g)
        return gx, gw, gb, None


class _ConvDgrad(torch.autograd.Function):
    """gx = conv^T(g, w): the data gradient of _Conv; bilinear in (g, w)."""

    @staticmethod
    def forward(ctx, g, w, H, W, stride):
        _check_args(g, w, stride)
        ctx.save_for_backward(g, w)
        ctx.stride = stride
        gc, wc = f32c(g), f32c(w)
        return conv_dgrad_packed(gc, pack_weights(wc, PACK_DGRAD), w.shape[1], H, W, w.shape[2], stride)

    @staticmethod
    def backward(ctx, ggx):
        g, w = ctx.saved_tensors
        gg = gw = None
        if ctx.needs_input_grad[0]:
            gg = _Conv.apply(ggx, w, None, ctx.stride)
        if ctx.needs_input_grad[1] and not _skip_wgrad and not _direct_wgrad(w, ggx, g, ctx.stride):
            gw = _ConvWgrad.apply(g, ggx, w.shape[2], ctx.stride)
        return gg, gw, None, None, None


class _ConvWgrad(torch.autograd.Function):
    """gw = sum_pixels g (x) x: the weight gradient of _Conv; bilinear in (g, x)."""

    @staticmethod
    def forward(ctx, g, x, ksize, stride):
        if not x.is_cuda:
            raise RuntimeError('conv2d: no CPU implementation')
        ctx.save_for_backward(g, x)
        ctx.stride = stride
        return conv_wgrad(f32c(x), f32c(g), ksize, stride)

    @staticmethod
    def backward(ctx, ggw):
        g, x = ctx.saved_tensors
        gg = gx = None
        if ctx.needs_input_grad[0]:
            gg = _Conv.apply(x, ggw, None, ctx.stride)
        if ctx.needs_input_grad[1]:
            gx = _ConvDgrad.apply(g, ggw, x.shape[2], x.shape[3], ctx.stride)
        return gg, gx, None, None


class _ConvLrelu(torch.autograd.Function):
    """y = leaky_relu(conv(x, w) + bias, slope) in ONE launch (the epilogue of the fused-extras k_conv instantiation):
    the `nn.Conv2d -> LeakyReLU(0.2)` pairs of DiscriminatorBlock.net (histoGAN/histoGAN.py:510-515).  The backward
    masks the incoming gradient with aten's leaky_relu_backward on the OUTPUT (sign(y) == sign(pre-activation)), which
    autograd can differentiate again, then continues with the bilinear conv Functions -> any-order differentiable."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, slope):
        _check_args(x, w, stride)
        if x.shape[1] != w.shape[1]:
            raise ValueError(f'conv2d: x {tuple(x.shape)} does not match w {tuple(w.shape)}')
        xc, wc = f32c(x), f32c(w)
        B, K, H, W = xc.shape
        N, k = w.shape[0], w.shape[2]
        wt = pack_weights(wc, PACK_FWD)
        bc = None if bias is None else f32c(bias)
        if stride != 1:
            raise ValueError('conv2d_lrelu: stride 1 only')
        out = modconv_fwd_packed(xc, wt, N, k, bias=bc, slope=slope)
        ctx.save_for_backward(x, w, out)
        ctx.stride, ctx.has_bias, ctx.slope = stride, bias is not None, float(slope)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, out = ctx.saved_tensors
        gx = gw = gb = None
        want_gb = ctx.has_bias and ctx.needs_input_grad[2] and not _skip_wgrad
        if torch.is_grad_enabled():      # a graph of this backward is being recorded (gradient penalty): differentiable ops
            gm = torch.ops.aten.leaky_relu_backward(g, out, ctx.slope, True)
            if want_gb:
                gb = gm.sum(dim=(0, 2, 3))
        else:                            # plain backward: the mask and the bias gradient from ONE pass over (g, out)
            gm, gb = lrelu_bwd_channel_sum(g, out, ctx.slope, want_gb)
        if ctx.needs_input_grad[0]:
            gx = _ConvDgrad.apply(gm, w, x.shape[2], x.shape[3], ctx.stride)
        if not _skip_wgrad:
            if ctx.needs_input_grad[1] and not _direct_wgrad(w, x, gm, ctx.stride):
                gw = _ConvWgrad.apply(gm, x, w.shape[2], ctx.stride)
        return gx, gw, gb, None, None


class _ConvAdd(torch.autograd.Function):
    """y = (conv(x, w) + bias) + addend in ONE launch: the residual sum of DiscriminatorBlock.forward
    (`x = self.net(x); x = x + res`, histoGAN/histoGAN.py:520-524) in the epilogue of the 1x1 `conv_res` launch.
    Bilinear part as _Conv (differentiable to any order), the addend's gradient is the incoming one."""

    @staticmethod
    def forward(ctx, x, w, bias, addend, stride):
        _check_args(x, w, stride)
        if x.shape[1] != w.shape[1]:
            raise ValueError(f'conv2d: x {tuple(x.shape)} does not match w {tuple(w.shape)}')
        ctx.save_for_backward(x, w)
        ctx.stride, ctx.has_bias = stride, bias is not None
        xc, wc = f32c(x), f32c(w)
        bc = None if bias is None else f32c(bias)
        return conv_fwd_add_packed(xc, pack_weights(wc, PACK_FWD), w.shape[0], w.shape[2], f32c(addend), bc, stride)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _ConvDgrad.apply(g, w, x.shape[2], x.shape[3], ctx.stride)
        if not _skip_wgrad:
            if ctx.needs_input_grad[1] and not _direct_wgrad(w, x, g, ctx.stride):
                gw = _ConvWgrad.apply(g, x, w.shape[2], ctx.stride)
            if ctx.has_bias and ctx.needs_input_grad[2]:
                if torch.is_grad_enabled():
                    gb = g.sum(dim=(0, 2, 3))
                else:
                    gb = channel_sum(g)
        return gx, gw, gb, (g if ctx.needs_input_grad[3] else None), None


_I32 = 2 ** 31 - 1


def _batch_pieces(x, w, stride):
    """The kernels index activations with 32-bit element offsets: a batch whose input or output tensor has >= 2^31
    elements (the 1024^2 configuration with attention: 16 x 512 x 512 x 512) is processed in batch slices (samples
    are independent; autograd sums the weight gradients of the slices)."""
    B, K, H, W = x.shape
    per = max(K * H * W, w.shape[0] * _out_size(H, stride) * _out_size(W, stride))
    if B * per <= _I32:
        return 1
    if per > _I32:
        raise ValueError(f'conv2d: one sample of shape {tuple(x.shape[1:])} -> {w.shape[0]} channels exceeds 2^31 elements')
    return -(-B // (_I32 // per))


def _sliced(fn, x, w, stride):
    n = _batch_pieces(x, w, stride)
    if n == 1:
        return fn(x)
    return torch.cat([fn(xs) for xs in x.chunk(n, dim=0)], dim=0)


def conv2d_lrelu(x, w, bias=None, slope=0.2):
    """leaky_relu(F.conv2d(x, w, bias, padding=k//2), slope) as one launch (stride 1)."""
    return _sliced(lambda t: _ConvLrelu.apply(t, w, bias, 1, slope), x, w, 1)


def conv2d(x, w, bias=None, stride=1):
    """F.conv2d(x, w, bias, stride=stride, padding=k//2) for k in {1,3} on the MFMA implicit-GEMM kernels."""
    return _sliced(lambda t: _Conv.apply(t, w, bias, stride), x, w, stride)


def conv2d_add(x, w, bias, addend, stride=1):
    """F.conv2d(x, w, bias, stride, padding=k//2) + addend as one launch."""
    if _batch_pieces(x, w, stride) != 1:
        return conv2d(x, w, bias, stride) + addend
    return _ConvAdd.apply(x, w, bias, addend, stride)


def conv2d_same(x, w, bias=None):
    return _sliced(lambda t: _Conv.apply(t, w, bias, 1), x, w, 1)
