"""autograd Functions over the generator kernels of include/hg_nets.h (first-order differentiable).

modulate            [bilinear x2 ->] x*(s+1)             prologue of Conv2DMod   (histoGAN/histoGAN.py:420-424, 447-448)
demod_noise_lrelu   lrelu(conv*d + noise)                epilogue               (histoGAN/histoGAN.py:427-429, 465-476)
upsample2x          nn.Upsample(bilinear, x2) of the RGB skip                   (histoGAN/histoGAN.py:377-378)
"""
import os
import ctypes

import torch

from . import conv as C
from . import launch
from ._lib import GlinLayer, check, f32c, lib, need_gpu, on_device, raw_stream, workspace


SKINNY_SPLIT = os.environ.get('HG_SKINNY_SPLIT', '1') != '0'   # _skinny_mm: chunked bmm + sum (0: plain mm)

channel_sum = launch.channel_sum


class _Modulate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s, upsample):
        need_gpu(x, 'modulate')
        x = f32c(x)
        s = None if s is None else f32c(s)
        ctx.save_for_backward(x, s)
        ctx.upsample = bool(upsample)
        return launch.modulate_fwd(x, s, upsample)

    @staticmethod
    def backward(ctx, g):
        x, s = ctx.saved_tensors
        gx, gs = launch.modulate_bwd(f32c(g), x, s, ctx.upsample)
        return gx, gs, None


def modulate(x, s, upsample=False):
    """(B,C,H,W), (B,C) -> [up2](x) * (s+1)[:, :, None, None]."""
    return _Modulate.apply(x, s, upsample)


def upsample2x(x):
    """Bilinear x2 (align_corners=False, edge clamp) == nn.Upsample(scale_factor=2, mode='bilinear')."""
    return _Modulate.apply(x, None, True)


def _square(t):
    if t.shape[2] != t.shape[3]:
        raise ValueError('square feature maps only (the noise permute of the reference needs H == W)')


class _DemodNoiseLrelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, conv, d, nzt, wn, bn):
        need_gpu(conv, 'demod_noise_lrelu')
        conv = f32c(conv)
        d = None if d is None else f32c(d)
        nzt = f32c(nzt)
        _square(conv)
        wn_ = f32c(wn.detach().reshape(-1))
        out = launch.dnl_fwd(conv, d, nzt, wn_, f32c(bn))
        # The convolution output is kept for the backward (no recovery rounding); recovering conv*d from `out` there instead
        # was measured at C3 within noise: 45.86 against 45.99 ms per plain step.
        ctx.save_for_backward(conv, d, nzt, out, wn_)
        return out

    @staticmethod
    def backward(ctx, g):
        conv, d, nzt, out, wn_ = ctx.saved_tensors
        gconv, gd, gw_p, gb_p = launch.dnl_bwd(f32c(g), out, conv, d, nzt, None, None)
        return gconv, gd, _noise_grad(ctx, 2, gconv, d, wn_, nzt), gw_p.sum(0).reshape(-1, 1), gb_p.sum(0)


def _noise_grad(ctx, arg, gconv, d, wn, nzt):
    """The gradient of a stage with respect to its transposed noise image nzt (the Function's argument number `arg`) from the
    stage's gconv -- one launch (hg_noise_grad), and only when autograd asks for it (projection: the noise image is
    optimised; training draws a fresh one that needs no gradient: no launch, no allocation)."""
    if not ctx.needs_input_grad[arg]:
        return None
    return launch.noise_grad(gconv, d, wn, torch.zeros_like(nzt), False)


def demod_noise_lrelu(conv, d, nzt, wn, bn):
    """lrelu_0.2(conv * d[:, :, None, None] + wn[o] * nzt[b, i, j] + bn[o]);  wn: Linear(1,O).weight (O,1)."""
    return _DemodNoiseLrelu.apply(conv, d, nzt, wn, bn)


TORGB = os.environ.get('HG_TORGB', '1') != '0'      # the to-RGB path as one stream over x per direction (hg_torgb_fwd / _bwd)


def torgb_supported(x, weight):
    return (TORGB and x.is_cuda and x.dtype == torch.float32 and weight.shape[2] == 1 and weight.shape[3] == 1
            and weight.shape[0] <= 4 and (x.shape[2] * x.shape[3]) % 4 == 0 and launch.torgb_fits(weight.shape[0], weight.shape[1]))


class _ToRGB(torch.autograd.Function):
    """rgb = conv1x1(x * (style + 1), W) [+ prev]: RGBBlock's modulated convolution without demodulation plus the running RGB
    image (histoGAN/histoGAN.py:380-390) as ONE pass over x forward (hg_torgb_fwd) and ONE backward (hg_torgb_bwd: gx, the
    style gradient and the weight gradient from the same read of x) -- instead of a modulated copy of x, a 3-row matrix
    launch and a residual add forward, and data gradient + weight gradient + modulation adjoint backward.  First order."""

    @staticmethod
    def forward(ctx, x, style, weight, prev):
        x_, s_, w_ = f32c(x), f32c(style), f32c(weight)
        ctx.save_for_backward(x_, s_, w_)
        ctx.has_prev = prev is not None
        return launch.torgb_fwd(x_, s_, w_, None if prev is None else f32c(prev))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        g = f32c(g)
        gx, gs, gw = launch.torgb_bwd(g, *ctx.saved_tensors)
        return gx, gs, gw, (g if ctx.has_prev else None)


def torgb(x, style, weight, prev=None):
    """conv1x1(x * (style + 1), weight) + prev in one launch per direction -- see _ToRGB."""
    return _ToRGB.apply(x, style, weight, prev)


class _ConvDnl(torch.autograd.Function):
    """out = lrelu_0.2(d[b,o] * conv(xm, W) + wn[o] * nzt[b,i,j] + bn[o]) on the already MODULATED input xm, as ONE launch
    (the fused epilogue of hg_wino_conv2d / hg_modconv2d_fwd): the training forward of a generator stage
    (histoGAN/histoGAN.py:431-439, 465-476) without the separate k_dnl_fwd pass and without storing the convolution output.
    Backward: k_dnl_bwd recovers conv * d from `out` (conv = NULL form), then the data gradient and the weight gradient
    (xm is materialised, so the weight gradient needs no modulation of its own -- the cost that made the fully fused stage
    lose, _ModConvStage).  First order only, like _DemodNoiseLrelu."""

    @staticmethod
    def forward(ctx, xm, w, d, nzt, wn, bn):
        need_gpu(xm, 'conv_dnl')
        xm_, w_ = f32c(xm), f32c(w)
        d_ = None if d is None else f32c(d)
        nzt_, wn_, bn_ = f32c(nzt), f32c(wn.detach().reshape(-1)), f32c(bn)
        N, k = w_.shape[0], w_.shape[2]
        _square(xm_)
        out = C.modconv_fwd_packed(xm_, C.pack_weights(w_, C.PACK_FWD), N, k, None, d_, bn_, wn_, nzt_, nzt_.shape[-1], 0.2)
        ctx.save_for_backward(xm, w, d_, nzt_, out, wn_, bn_)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        xm, w, d, nzt_, out, wn_, bn_ = ctx.saved_tensors
        K, k = w.shape[1], w.shape[2]
        gconv, gd, gw_p, gb_p = launch.dnl_bwd(f32c(g), out, None, d, nzt_, wn_, bn_)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = C.conv_dgrad_packed(gconv, C.pack_weights(f32c(w), C.PACK_DGRAD), K, xm.shape[2], xm.shape[3], k)
        if ctx.needs_input_grad[1] and not C._skip_wgrad and not C._direct_wgrad(w, xm, gconv, 1):
            gw = C.conv_wgrad(f32c(xm), gconv, k)
        return gx, gw, gd, _noise_grad(ctx, 3, gconv, d, wn_, nzt_), gw_p.sum(0).reshape(-1, 1), gb_p.sum(0)


def conv_dnl(xm, w, d, nzt, wn, bn):
    """lrelu_0.2(d * conv(xm, w) + wn * nzt + bn) in one forward launch -- see _ConvDnl."""
    return _ConvDnl.apply(xm, w, d, nzt, wn, bn)


class _ModConvStage(torch.autograd.Function):
    """One generator convolution stage as a single forward launch (hg_modconv2d_fwd):

        out = act( d[b,o] * conv(up?(x) * (style+1), W) + wn[o] * nzt[b,i,j] + bn[o] ),   d = demodulation

    == Conv2DMod.forward + noise add + LeakyReLU(0.2) of GeneratorBlock.forward (histoGAN/histoGAN.py:420-440,
    465-476); with act=False / no noise it is the to-RGB convolution (:375, 383).  The modulated input, the
    convolution output before demodulation and the pre-activation are never written to memory (for the up-sampled
    first convolution of a block the bilinear x2 + modulation prologue stays its own kernel).  First-order
    differentiable; the backward recovers conv*d from `out` (hg_demod_noise_lrelu_bwd with conv = NULL)."""

    @staticmethod
    def forward(ctx, x, style, weight, nzt, wn, bn, demod, upsample, act):
        need_gpu(x, 'modconv_stage')
        x, style, w = f32c(x), f32c(style), f32c(weight)
        N, _, k, _ = w.shape
        xin = launch.modulate_fwd(x, style, True) if upsample else x
        if demod:
            d, s1, _ = demod_fwd(style, w)
        else:
            d, s1 = None, style + 1.0
        iscale = None if upsample else s1
        if act:
            nzt_, wn_, bn_ = f32c(nzt), f32c(wn.detach().reshape(-1)), f32c(bn)
            S = nzt_.shape[-1]
        else:
            nzt_ = wn_ = bn_ = None
            S = 0
        wt = C.pack_weights(w, C.PACK_FWD)
        out = C.modconv_fwd_packed(xin, wt, N, k, iscale, d, bn_, wn_, nzt_, S, 0.2 if act else 0.0)
        ctx.save_for_backward(x, xin if upsample else None, style, w, d, out, nzt_, wn_, bn_)
        ctx.cfg = (bool(demod), bool(upsample), bool(act))
        return out

    @staticmethod
    def backward(ctx, g):
        x, xin, style, w, d, out, nzt_, wn_, bn_ = ctx.saved_tensors
        demod, upsample, act = ctx.cfg
        g = f32c(g)
        K = x.shape[1]
        k = w.shape[2]
        s1 = style + 1.0
        if xin is None:
            xin = x
        Hi, Wi = xin.shape[2], xin.shape[3]
        gwn = gbn = gd = gnzt = None
        if act:
            gconv, gd, gw_p, gb_p = launch.dnl_bwd(g, out, None, d, nzt_, wn_, bn_)
            gwn, gbn = gw_p.sum(0).reshape(-1, 1), gb_p.sum(0)
            gnzt = _noise_grad(ctx, 3, gconv, d, wn_, nzt_)
        else:
            if d is not None:
                raise RuntimeError('modconv_stage: demodulation without activation is not implemented')
            gconv = g
        t = C.conv_dgrad_packed(gconv, C.pack_weights(w, C.PACK_DGRAD), K, Hi, Wi, k)
        gx, gs = launch.modulate_bwd(t, x, style, upsample)
        gw = C.conv_wgrad(xin, gconv, k, iscale=None if upsample else s1)
        if d is not None:
            # not demod_bwd: a recomputed wsq and a plain mm here round differently from the cached wsq and _skinny_mm there
            wsq = w.pow(2).sum(dim=(2, 3))
            gq = gd * (-0.5) * d * d * d
            gs = gs + 2.0 * s1 * torch.mm(gq, wsq)
            gw = gw + 2.0 * w * torch.mm(gq.t(), s1 * s1)[:, :, None, None]
        return gx, gs, gw, gnzt, gwn, gbn, None, None, None


def modconv_stage(x, style, weight, nzt=None, wn=None, bn=None, demod=True, upsample=False, act=True):
    """act(demod * conv(up?(x)*(style+1), weight) + wn*nzt + bn) -- see _ModConvStage."""
    return _ModConvStage.apply(x, style, weight, nzt, wn, bn, demod, upsample, act)


def _skinny_mm(a, m, m_transposed):
    """a (B, R) @ M (R, C) for a small B and a deep reduction R, M = m (R, C) or m.t() with m (C, R), m contiguous.
    rocBLAS has no split-K pick for these: 32 x 2048 x 2048 runs as 64 workgroups, 60 us forward / 320 us for the
    transposed operand; as S batches over chunks of R (a strided bmm, no copies) plus a sum it is S times the workgroups."""
    B, R = a.shape
    S = min(16, R // 128)
    if not SKINNY_SPLIT or S < 4 or R % S or not m.is_contiguous() or not a.is_contiguous():
        return torch.mm(a, m.t() if m_transposed else m)
    r = R // S
    av = a.view(B, S, r).transpose(0, 1)
    mv = m.view(m.shape[0], S, r).permute(1, 2, 0) if m_transposed else m.view(S, r, m.shape[1])
    return torch.bmm(av, mv).sum(0)


def demod_fwd(s, w):
    """d[b,o] = rsqrt( sum_i (s[b,i]+1)^2 * wsq[o,i] + 1e-8 ),  wsq[o,i] = sum_k W[o,i,k]^2   (Conv2DMod demodulation,
    histoGAN/histoGAN.py:427-429, on the shared weight) -> (d, s + 1, wsq); s and w detached.  wsq only depends on the weight,
    so it is cached per optimizer step for registered training weights (conv.cached) instead of re-reducing up to 151 MB
    three times a step."""
    wsq = C.cached(w, 'wsq', lambda t: t.pow(2).sum(dim=(2, 3)))
    s1 = s + 1.0
    return torch.rsqrt(_skinny_mm(s1 * s1, wsq, True) + 1e-8), s1, wsq


def demod_bwd(gd, d, s1, wsq, w, want_style=True, want_weight=True):
    """d's adjoint -> (gy, gw): the style part (B, K), and the weight part -- None when it was added to the weight's flat
    gradient slot on the weight-gradient stream, BEHIND the convolution's weight gradient that wrote the slot (training:
    one kernel, hg_demod_weight_term)."""
    gy = gw = gq = None
    if want_style:
        if gd.is_cuda and not torch.is_grad_enabled() and wsq.is_contiguous():
            # one kernel pair (hg_demod_style_grad) instead of a skinny rocBLAS GEMM + five element-wise launches
            gy = launch.demod_style_grad(f32c(gd), d, s1, wsq)
        else:
            gq = gd * (-0.5) * d * d * d
            gy = 2.0 * s1 * _skinny_mm(gq, wsq, False)
    if want_weight and not (w.is_contiguous() and C.direct_demod_weight_term(w, gd, d, s1)):
        gq = gd * (-0.5) * d * d * d if gq is None else gq
        gw = 2.0 * w.detach() * torch.mm(gq.t(), s1 * s1)[:, :, None, None]
    return gy, gw


class _DemodCoeff(torch.autograd.Function):
    """demod_fwd / demod_bwd as an autograd node of the per-block path."""

    @staticmethod
    def forward(ctx, y, weight):
        w = weight.detach()
        d, s1, wsq = demod_fwd(y.detach(), w)
        ctx.save_for_backward(s1, wsq, d, w)
        return d

    @staticmethod
    def backward(ctx, gd):
        s1, wsq, d, w = ctx.saved_tensors
        return demod_bwd(gd, d, s1, wsq, w, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


def demod_coeff(y, weight):
    return _DemodCoeff.apply(y, weight)


# ---- grouped linear layers (include/hg_linear.h): the generator's 21 style projections as one launch per pass ----------
GROUPED_STYLES = os.environ.get('HG_GROUPED_STYLES', '1') != '0'   # 0: one F.linear (library GEMM) per projection


def _glin_table(xs, ws, bs, ys, groups, gws=None, gbs=None):
    n = len(ws)
    tab = (GlinLayer * n)()
    for i in range(n):
        t = tab[i]
        t.x, t.w, t.y = xs[groups[i]].data_ptr(), ws[i].data_ptr(), ys[i].data_ptr()
        t.b = bs[i].data_ptr() if bs is not None and bs[i] is not None else None
        t.gw = gws[i].data_ptr() if gws is not None else None
        t.gb = gbs[i].data_ptr() if gbs is not None and gbs[i] is not None else None
        t.N, t.group = ws[i].shape[0], groups[i]
    return tab


def _aligned16(t):
    return t.data_ptr() % 16 == 0


def _realigned(t):
    """f32c(t) on a 16-byte boundary: the same storage when it already is, a copy otherwise (a contiguous view into a flat
    buffer behind an odd-sized neighbour is contiguous and misaligned)."""
    t = f32c(t)
    return t if _aligned16(t) else t.clone()


def grouped_linear_supported(xs, ws):
    """Whether hg_grouped_linear_* serves these layers.  The kernels read whole rows of the WEIGHTS 16 bytes at a time in place
    (check_layers refuses any other address), so a weight that is a strided view, or a contiguous view into a flat parameter
    buffer behind an odd-sized parameter, takes the caller's per-layer path; inputs and incoming gradients are small and are
    realigned by a copy inside _GroupedLinear."""
    B, K = xs[0].shape
    return (GROUPED_STYLES and xs[0].is_cuda and B <= 64 and K % 32 == 0 and len(ws) <= 32
            and all(w.shape[0] % 4 == 0 and w.shape[1] == K and w.dtype == torch.float32 and w.is_contiguous() and _aligned16(w)
                    for w in ws))


class _GroupedLinear(torch.autograd.Function):
    """FIRST-ORDER ONLY (once_differentiable backward): a double backward through the generator's style projections
    (create_graph=True through G) raises -- set HG_GROUPED_STYLES=0 for such uses (one F.linear per projection,
    differentiable to any order); the trainer's path-length term is a finite difference and its gradient penalty is D-only.

    y_l = x_g(l) @ W_l^T + b_l for a list of nn.Linear layers whose inputs come in groups (histoGAN/histoGAN.py:372, 450,
    454: to_style1 / to_style2 / to_rgb.to_style of one generator block share the block's style vector).  ONE launch
    forward (hg_grouped_linear_fwd), three backward (input gradients: two, parameter gradients: one)."""

    @staticmethod
    def forward(ctx, groups, n_groups, *tensors):
        xs = [_realigned(t) for t in tensors[:n_groups]]
        n = (len(tensors) - n_groups) // 2
        ws = [t.detach() for t in tensors[n_groups:n_groups + n]]      # in place: grouped_linear_supported vouches for them
        bs = [f32c(t) for t in tensors[n_groups + n:]]
        B, K = xs[0].shape
        dev = xs[0].device
        ys = [torch.empty((B, w.shape[0]), dtype=torch.float32, device=dev) for w in ws]
        tab = _glin_table(xs, ws, bs, ys, groups)
        with on_device(dev):
            check(lib.hg_grouped_linear_fwd(tab, len(ws), B, K, raw_stream(dev)), 'hg_grouped_linear_fwd')
        ctx.groups, ctx.n_groups, ctx.n = groups, n_groups, n
        ctx.save_for_backward(*xs, *ws)
        return tuple(ys)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gys):
        groups, G, n = ctx.groups, ctx.n_groups, ctx.n
        saved = ctx.saved_tensors
        xs, ws = list(saved[:G]), list(saved[G:])
        B, K = xs[0].shape
        dev = xs[0].device
        gys = [(_realigned(g) if g is not None else torch.zeros((B, w.shape[0]), dtype=torch.float32, device=dev))
               for g, w in zip(gys, ws)]
        need_x = any(ctx.needs_input_grad[2:2 + G])
        need_p = any(ctx.needs_input_grad[2 + G:])
        gxs = [None] * G
        gws, gbs = [None] * n, [None] * n
        with on_device(dev):
            st = raw_stream(dev)
            if need_x:
                gxs = [torch.empty_like(x) for x in xs]
                tab = _glin_table(xs, ws, None, gys, groups)
                nb = lib.hg_grouped_linear_bwd_input_workspace_bytes(tab, n, B, K)
                wsb = workspace(nb, dev)
                ptrs = (ctypes.c_void_p * G)(*[g.data_ptr() for g in gxs])
                check(lib.hg_grouped_linear_bwd_input(tab, n, ptrs, G, B, K, wsb.data_ptr(), wsb.numel(), st),
                      'hg_grouped_linear_bwd_input')
            if need_p:
                gws = [torch.empty_like(w) for w in ws]
                gbs = [torch.empty((w.shape[0],), dtype=torch.float32, device=dev) for w in ws]
                tab = _glin_table(xs, ws, None, gys, groups, gws, gbs)
                check(lib.hg_grouped_linear_bwd_params(tab, n, B, K, st), 'hg_grouped_linear_bwd_params')
        return (None, None, *gxs, *gws, *gbs)


def grouped_linear(xs, layers, groups):
    """xs: list of (B, K) inputs; layers: list of nn.Linear (with bias); groups[i]: index into xs of layer i's input (non-
    decreasing).  Returns the list of outputs."""
    ws = [m.weight for m in layers]
    bs = [m.bias for m in layers]
    return list(_GroupedLinear.apply(tuple(groups), len(xs), *xs, *ws, *bs))
