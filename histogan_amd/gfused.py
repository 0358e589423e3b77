"""The generator's TRAINING pass as one hand-scheduled autograd node (first order).

`Generator.forward` (histoGAN/histoGAN.py:558-568) over `GeneratorBlock.forward` (:461-479), `Conv2DMod` (:420-440) and
`RGBBlock` (:380-390), with the per-block launch sequence of nets.GeneratorBlock._stage, but ONE autograd Function for the whole
network instead of ~90 nodes: the backward is written out by hand, and everything that sits between two convolutions of it
-- modulation adjoint (+ bilinear x2 adjoint), to-RGB adjoint, the sum of the two gradients of a block output, LeakyReLU /
noise / demodulation adjoint -- is ONE launch (`hg_gstage_bwd`, include/hg_nets.h) where autograd ran five to six in a row on
the critical path between one data gradient and the next (un-profiled phase probe, profiles/r06_phase_probe.txt: the
G-phase backward was 13.95 ms of a 35.2 ms step against 9.9 ms of convolution kernels in it).

The 21 style projections stay outside (ops.grouped_linear: their own node); the 14 demodulation coefficients are computed
and differentiated inside (`ops.demod_fwd` / `ops.demod_bwd`: the weight term is added to the flat gradient slot on the
weight-gradient stream right behind the convolution's weight gradient that wrote it), so that when the node's backward returns
every convolution weight of the generator has its final gradient.  HG_GFUSED=0 keeps the per-block autograd path.
"""
import os

import torch

from . import conv as C
from ._lib import f32c
from .launch import gstage_bwd, modulate_bwd, modulate_fwd, noise_grad, torgb_fits, torgb_fwd
from .ops import demod_bwd, demod_fwd

GFUSED = os.environ.get('HG_GFUSED', '1') != '0'
PER_BLOCK = 10        # tensors per block in the Function's argument list (see generator_train)
AFTER_BLOCKS = None    # trainer: called when the node's backward has enqueued the last convolution weight gradient
STAGE_OBSERVER = None  # tests: called with every stage output (two per block, forward order) -- the LeakyReLU branches taken


def _torgb(x, s, w, prev):
    Cr, O = w.shape
    if torgb_fits(Cr, O):
        return torgb_fwd(x, s, w, prev)
    # (the 8 192-channel blocks of the 1024^2 configuration: hg_torgb_fwd stages w (s + 1) in LDS; there the 1x1 modulated
    # convolution runs on the matrix kernel with the modulation as its input scale, plus the running-image add)
    rgb = C.conv_fwd_packed(x, C.pack_weights(w.reshape(Cr, O, 1, 1), C.PACK_FWD), Cr, 1, 1, iscale=s + 1.0)
    return rgb if prev is None else rgb.add_(prev)


def _wgrad(w, x, g):
    """Weight gradient of conv(x, w): into w's flat gradient slot on the weight-gradient stream (None returned), or a tensor."""
    if C._skip_wgrad or C._direct_wgrad(w, x, g, 1):
        return None
    return C.conv_wgrad(x, g, w.shape[2])


def _add(a, b):
    return b if a is None else (a if b is None else a + b)


class _GeneratorTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, nzt, *ts):
        L = len(ts) // PER_BLOCK
        nzt_ = f32c(nzt)
        S = nzt_.shape[-1]
        B = ts[0].shape[0]
        x = f32c(x0).expand(B, -1, -1, -1).contiguous()
        saved = [x, nzt_]
        prev = None
        rgb = None
        for i in range(L):
            s1, s2, srgb, w1, w2, wrgb, wn1, bn1, wn2, bn2 = [f32c(t) for t in ts[PER_BLOCK * i:PER_BLOCK * (i + 1)]]
            wn1, wn2 = wn1.reshape(-1), wn2.reshape(-1)
            N = w1.shape[0]
            d1, s1p, wsq1 = demod_fwd(s1, w1)
            xm1 = modulate_fwd(x, s1, i != 0)
            out1 = C.modconv_fwd_packed(xm1, C.pack_weights(w1, C.PACK_FWD), N, 3, None, d1, bn1, wn1, nzt_, S, 0.2)
            d2, s2p, wsq2 = demod_fwd(s2, w2)
            xm2 = modulate_fwd(out1, s2, False)
            out2 = C.modconv_fwd_packed(xm2, C.pack_weights(w2, C.PACK_FWD), N, 3, None, d2, bn2, wn2, nzt_, S, 0.2)
            rgb = _torgb(out2, srgb, wrgb.reshape(wrgb.shape[0], -1), prev)
            if i != L - 1:
                prev = modulate_fwd(rgb, None, True)
            x = out2
            if STAGE_OBSERVER is not None:
                STAGE_OBSERVER(out1)
                STAGE_OBSERVER(out2)
            saved += [xm1, out1, xm2, out2, s1, s2, srgb, d1, d2, wn1, bn1, wn2, bn2, s1p, s2p, wsq1, wsq2]
        ctx.save_for_backward(*saved)
        ctx.weights = [ts[PER_BLOCK * i + 3:PER_BLOCK * i + 6] for i in range(L)]      # the PARAMETERS (flat-slot lookup by address)
        ctx.L = L
        return rgb

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        L = ctx.L
        sv = ctx.saved_tensors
        x0e, nzt = sv[0], sv[1]
        per = 17
        blk = lambda i: sv[2 + per * i:2 + per * (i + 1)]
        grads = [None] * (PER_BLOCK * L)
        # What autograd asks for, per argument (x0, nzt, then PER_BLOCK per block).  Training asks for every parameter and
        # not for the noise; a projection (project.py) asks for the styles and the noise against frozen weights: then no
        # weight-gradient convolution runs and no flat gradient slot is touched.
        need = ctx.needs_input_grad
        need_params = need[0] or any(need[2 + PER_BLOCK * i + k] for i in range(L) for k in range(3, PER_BLOCK))
        # The noise image's gradient: one (B, S, S) buffer that the 2 L stages add their windows to (hg_noise_grad), each
        # right behind the stage kernel that wrote its gconv, on the main stream: the read-modify-write of the buffer has
        # to be ordered anyway, and 14 launches of microseconds are not worth a cross-stream event pair each.
        gnz = torch.zeros_like(nzt) if need[1] else None
        from . import nets as _N
        if _N.PHASE_HOOK is not None:
            _N.PHASE_HOOK('gb_generator_node_entered', True)
        g_rgb = f32c(g)
        ga = None          # d loss / d (modulated, up-sampled input of the NEXT block's first convolution)
        sa = None
        # The demodulation coefficients' adjoints (a small GEMM-like kernel pair + the weight term per convolution) only feed
        # the style gradients returned at the end.  They run inline: on the auxiliary stream, off the dgrad -> stage -> dgrad
        # chain, they measured 854.6 against 867.7 images/s -- they already hide under the
        # weight-gradient kernels.
        pend = []          # (index into grads, modulation part, demodulation part)
        wterm = {}

        def demod(idx, gd, d, s1p, wsq, wp):
            gy, wterm[idx] = demod_bwd(gd, d, s1p, wsq, wp, True, need[2 + idx])
            return gy
        for i in range(L - 1, -1, -1):
            xm1, out1, xm2, out2, s1, s2, srgb, d1, d2, wn1, bn1, wn2, bn2, s1p, s2p, wsq1, wsq2 = blk(i)
            w1p, w2p, wrgbp = ctx.weights[i]
            w1, w2, wrgb = f32c(w1p), f32c(w2p), f32c(wrgbp)
            Cr = wrgb.shape[0]
            base = PER_BLOCK * i
            # ---- at out2: next block's first convolution (behind the bilinear x2) + this block's to-RGB -> conv2's upstream gradient
            # (the to-RGB weight gradient straight into its flat slot when that slot has no writer yet this step)
            nd = need[2 + base:2 + base + PER_BLOCK]
            slot = C.grad_slot(wrgbp) if nd[5] and wrgbp.is_contiguous() else None
            if slot is not None and slot[2]:
                slot = None
            gconv2, gs_a, gs_rgb, gw_rgb, gd2, gwn2, gbn2 = gstage_bwd(out2, ga, sa, ga is not None, g_rgb, wrgb.reshape(Cr, -1),
                                                                       srgb, d2, nzt, wn2, bn2,
                                                                       None if slot is None else slot[0].view(Cr, -1))
            if ga is not None:
                pend.append((base + PER_BLOCK + 0, gs_a, gy_next))   # style of the next block's conv1: modulation + demodulation parts
            if gnz is not None:
                noise_grad(gconv2, d2, wn2, gnz, True)
            grads[base + 2] = gs_rgb
            if slot is not None:
                slot[1].mark_written(slot[3])
            elif nd[5]:
                grads[base + 5] = gw_rgb.reshape(wrgbp.shape)
            if nd[8]:
                grads[base + 8] = gwn2.reshape(-1, 1)
            if nd[9]:
                grads[base + 9] = gbn2
            g_xm2 = C.conv_dgrad_packed(gconv2, C.pack_weights(w2, C.PACK_DGRAD), w2.shape[1], xm2.shape[2], xm2.shape[3], 3)
            if nd[4]:
                grads[base + 4] = _wgrad(w2p, xm2, gconv2)
            gy2 = demod(base + 4, gd2, d2, s2p, wsq2, w2p)
            if i > 0:                                            # rgb_i = to_rgb(out2) + up2(rgb_{i-1})
                g_rgb_prev, _ = modulate_bwd(g_rgb, torch.empty((g_rgb.shape[0], Cr, g_rgb.shape[2] // 2, g_rgb.shape[3] // 2),
                                                                 dtype=torch.float32, device=g_rgb.device), None, True)
            # ---- at out1: conv2 (same resolution) -> conv1's upstream gradient
            gconv1, gs2, _, _, gd1, gwn1, gbn1 = gstage_bwd(out1, g_xm2, s2, False, None, None, None, d1, nzt, wn1, bn1)
            if gnz is not None:
                noise_grad(gconv1, d1, wn1, gnz, True)
            pend.append((base + 1, gs2, gy2))
            if nd[6]:
                grads[base + 6] = gwn1.reshape(-1, 1)
            if nd[7]:
                grads[base + 7] = gbn1
            ga = C.conv_dgrad_packed(gconv1, C.pack_weights(w1, C.PACK_DGRAD), w1.shape[1], xm1.shape[2], xm1.shape[3], 3)
            if nd[3]:
                grads[base + 3] = _wgrad(w1p, xm1, gconv1)
            gy_next = demod(base + 3, gd1, d1, s1p, wsq1, w1p)
            sa = s1
            if i > 0:
                g_rgb = g_rgb_prev
        # block 0's first convolution reads the learned constant directly (no upsample)
        gx0e, gs1_0 = modulate_bwd(ga, x0e, sa, False)
        pend.append((0, gs1_0, gy_next))
        g_x0 = gx0e.sum(0) if need[0] else None
        torch._foreach_add_([a for _, a, _ in pend], [b for _, _, b in pend])
        for idx, a, _ in pend:
            grads[idx] = a
        for idx, gwd in wterm.items():
            grads[idx] = _add(grads[idx], gwd)
        if _N.PHASE_HOOK is not None:
            _N.PHASE_HOOK('gb_generator_blocks_done', True)
        # (a conv / to-RGB weight gradient that goes back to autograd -- a slot written before this pass, a non-contiguous
        # weight -- reaches its flat slot only in gather(): the convolution-weight region is not final then)
        if AFTER_BLOCKS is not None and need_params and all(grads[PER_BLOCK * i + k] is None for i in range(L) for k in (3, 4, 5)):
            AFTER_BLOCKS()
        return (g_x0, gnz, *grads)


def generator_infer(gen, styles_t, nzt):
    """The same launch sequence without autograd (the D phase's generator forward, evaluate()): modulation inside the
    convolution kernel where there is no upsample in front of it, and the 14 demodulation coefficients -- six small dependent
    launches each, ~0.4 ms as links of the convolution chain -- computed AHEAD on the auxiliary stream (they depend on the
    styles and the weights only); the chain waits for its block's event."""
    dev = nzt.device
    main, aux = torch.cuda.current_stream(dev), nets_aux(dev)
    L = len(gen.blocks)
    B = styles_t[0].shape[0]
    S = nzt.shape[-1]
    aux.wait_event(main.record_event())
    ahead = []
    with torch.cuda.stream(aux):
        for i, b in enumerate(gen.blocks):
            w1, w2 = f32c(b.conv1.weight), f32c(b.conv2.weight)
            d1, s1p, _ = demod_fwd(f32c(styles_t[3 * i]), w1)
            d2, s2p, _ = demod_fwd(f32c(styles_t[3 * i + 1]), w2)
            ahead.append((d1, s1p, d2, s2p, aux.record_event()))
    for t in styles_t:
        t.record_stream(aux)
    x = f32c(gen.initial_block).expand(B, -1, -1, -1).contiguous()
    prev = rgb = None
    for i, b in enumerate(gen.blocks):
        d1, s1p, d2, s2p, ev = ahead[i]
        main.wait_event(ev)
        for t in (d1, s1p, d2, s2p):
            t.record_stream(main)
        w1, w2, wrgb = f32c(b.conv1.weight), f32c(b.conv2.weight), f32c(b.to_rgb.conv.weight)
        wn1, bn1 = f32c(b.to_noise1.weight).reshape(-1), f32c(b.to_noise1.bias)
        wn2, bn2 = f32c(b.to_noise2.weight).reshape(-1), f32c(b.to_noise2.bias)
        N = w1.shape[0]
        if i:
            x, isc = modulate_fwd(x, f32c(styles_t[3 * i]), True), None
        else:
            isc = s1p
        x = C.modconv_fwd_packed(x, C.pack_weights(w1, C.PACK_FWD), N, 3, isc, d1, bn1, wn1, nzt, S, 0.2)
        x = C.modconv_fwd_packed(x, C.pack_weights(w2, C.PACK_FWD), N, 3, s2p, d2, bn2, wn2, nzt, S, 0.2)
        rgb = _torgb(x, f32c(styles_t[3 * i + 2]), wrgb.reshape(wrgb.shape[0], -1), prev)
        if i != L - 1:
            prev = modulate_fwd(rgb, None, True)
    return rgb


def nets_aux(dev):
    from .nets import aux_stream
    return aux_stream(dev)


def supported(gen, styles_t, nzt, train=True):
    """Shapes / options the fused node serves (everything HistoGAN trains with); anything else takes the per-block path."""
    if not (GFUSED and torch.is_grad_enabled() == train and nzt.is_cuda and nzt.dtype == torch.float32):
        return False
    if not train and torch.cuda.is_current_stream_capturing():
        return False
    S = nzt.shape[-1]
    if S % 4 or gen.initial_block.shape[-1] % 4 or gen.initial_block.shape[-1] != gen.initial_block.shape[-2]:
        return False
    B = styles_t[0].shape[0]
    H = gen.initial_block.shape[-1]
    for i, b in enumerate(gen.blocks):
        if i:
            H *= 2
        for cv in (b.conv1, b.conv2):
            if not (cv.demod and cv.kernel == 3 and cv.stride == 1 and cv.dilation == 1 and cv.weight.dtype == torch.float32):
                return False
        r = b.to_rgb.conv
        if r.demod or r.kernel != 1 or r.stride != 1 or r.dilation != 1 or r.weight.shape[0] > 4:
            return False
        Cmax = max(b.conv1.weight.shape[0], b.conv1.weight.shape[1])
        if H > S or B * Cmax * H * H * 4 >= 2 ** 31:
            return False
        if (b.upsample is not None) != (i != 0) or (b.to_rgb.upsample is not None) != (i != len(gen.blocks) - 1):
            return False
    return all(t.dtype == torch.float32 for t in styles_t)


def generator_train(gen, styles_t, nzt):
    """rgb = Generator(...) given the 3 L projected styles `styles_t` ([to_style1, to_style2, to_rgb.to_style] per block) and the
    transposed noise image; differentiable (first order) w.r.t. the styles, the noise image and every generator parameter
    (each gradient is computed only where autograd asks for it: frozen weights cost no weight-gradient launch)."""
    args = []
    for i, b in enumerate(gen.blocks):
        s1, s2, srgb = styles_t[3 * i], styles_t[3 * i + 1], styles_t[3 * i + 2]
        args += [s1, s2, srgb, b.conv1.weight, b.conv2.weight, b.to_rgb.conv.weight,
                 b.to_noise1.weight, b.to_noise1.bias, b.to_noise2.weight, b.to_noise2.bias]
    return _GeneratorTrain.apply(gen.initial_block, nzt, *args)
