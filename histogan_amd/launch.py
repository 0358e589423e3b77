"""One plain function per generator kernel of include/hg_nets.h: the marshalling of its C-ABI call, without autograd.

ops.py (the per-block autograd Functions) and gfused.py (the whole generator as one node) both launch through these.  Every
tensor argument is fp32, contiguous and detached (`_lib.f32c`); a function allocates its outputs and its workspace and
nothing else.
"""
import torch

from ._lib import check, f32c, lib, on_device, ptr, stream_of, workspace

TORGB_LDS_BYTES = 48 * 1024     # hg_torgb_fwd / _bwd stage w (s + 1), C x O floats, in LDS


def torgb_fits(C, O):
    """Whether a C x O to-RGB weight fits the kernels' LDS stage (not the 8 192-channel blocks of the 1024^2 configuration)."""
    return C * O * 4 <= TORGB_LDS_BYTES


def _nets_ws(dev, B, C, H, W):
    n = lib.hg_nets_workspace_bytes(B, C, H, W)
    return workspace(n, dev), n


def channel_sum(g):
    """(B, C, H, W) -> (C): sum over batch and pixels (bias gradient), deterministic two-stage reduction."""
    g = f32c(g)
    B, C, H, W = g.shape
    with on_device(g.device):
        out = torch.empty(C, dtype=torch.float32, device=g.device)
        ws, n = _nets_ws(g.device, B, C, H, W)
        check(lib.hg_channel_sum(g.data_ptr(), out.data_ptr(), B, C, H * W, ws.data_ptr(), n, stream_of(g)), 'hg_channel_sum')
    return out


def modulate_fwd(x, s, upsample):
    """[up2](x) * (s + 1)[:, :, None, None]; s None: the bilinear x2 alone."""
    B, C, H, W = x.shape
    f = 2 if upsample else 1
    with on_device(x.device):
        out = torch.empty((B, C, H * f, W * f), dtype=torch.float32, device=x.device)
        check(lib.hg_modulate_fwd(x.data_ptr(), ptr(s), out.data_ptr(), B, C, H, W, int(upsample), stream_of(x)), 'hg_modulate_fwd')
    return out


def modulate_bwd(g, x, s, upsample):
    """-> (gx, gs); gs None without s (then x is only read for its shape)."""
    B, C, H, W = x.shape
    with on_device(x.device):
        gx = torch.empty_like(x)
        gs = None if s is None else torch.empty_like(s)
        ws, n = _nets_ws(x.device, B, C, H, W)
        check(lib.hg_modulate_bwd(g.data_ptr(), x.data_ptr(), ptr(s), gx.data_ptr(), ptr(gs), B, C, H, W, int(upsample),
                                  ws.data_ptr(), n, stream_of(x)), 'hg_modulate_bwd')
    return gx, gs


def dnl_fwd(conv, d, nzt, wn, bn):
    """lrelu_0.2(conv * d[:, :, None, None] + wn[o] * nzt[b, i, j] + bn[o]); d None: no demodulation."""
    B, O, H, _ = conv.shape
    with on_device(conv.device):
        out = torch.empty_like(conv)
        check(lib.hg_demod_noise_lrelu_fwd(conv.data_ptr(), ptr(d), nzt.data_ptr(), wn.data_ptr(), bn.data_ptr(), out.data_ptr(),
                                           B, O, H, nzt.shape[-1], stream_of(conv)), 'hg_demod_noise_lrelu_fwd')
    return out


def dnl_bwd(g, out, conv, d, nzt, wn, bn):
    """-> (gconv, gd, gw_partial, gb_partial), the partials (B, O): their sum over the batch is the gradient of wn / bn.
    conv None: conv * d is recovered from `out`, which takes wn and bn; gd None without d."""
    B, O, H, W = out.shape
    dev = out.device
    with on_device(dev):
        gconv = torch.empty_like(out)
        gd = None if d is None else torch.empty_like(d)
        gw_p = torch.empty((B, O), dtype=torch.float32, device=dev)
        gb_p = torch.empty((B, O), dtype=torch.float32, device=dev)
        ws, n = _nets_ws(dev, B, O, H, W)
        check(lib.hg_demod_noise_lrelu_bwd(g.data_ptr(), out.data_ptr(), ptr(conv), ptr(d), nzt.data_ptr(), ptr(wn), ptr(bn),
                                           gconv.data_ptr(), ptr(gd), gw_p.data_ptr(), gb_p.data_ptr(), B, O, H, nzt.shape[-1],
                                           ws.data_ptr(), n, stream_of(out)), 'hg_demod_noise_lrelu_bwd')
    return gconv, gd, gw_p, gb_p


def noise_grad(gconv, d, wn, gnzt, accumulate):
    """hg_noise_grad: gnzt[b, i, j] (+)= sum_o (wn[o] / d[b, o]) gconv[b, o, i, j] on the H x H window of the (B, S, S) buffer
    gnzt, in place (accumulate False: the window is overwritten); d None: no demodulation.  Returns gnzt."""
    B, O, H, _ = gconv.shape
    with on_device(gconv.device):
        check(lib.hg_noise_grad(gconv.data_ptr(), ptr(d), wn.data_ptr(), gnzt.data_ptr(), B, O, H, gnzt.shape[-1],
                                int(bool(accumulate)), stream_of(gconv)), 'hg_noise_grad')
    return gnzt


def torgb_fwd(x, s, w, prev):
    """conv1x1(x * (s + 1), w) [+ prev] as one stream over x; w (C, O) or (C, O, 1, 1), torgb_fits(C, O)."""
    B, O, H, W = x.shape
    C = w.shape[0]
    with on_device(x.device):
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
        check(lib.hg_torgb_fwd(x.data_ptr(), s.data_ptr(), w.data_ptr(), ptr(prev), out.data_ptr(), B, O, C, H * W, stream_of(x)),
              'hg_torgb_fwd')
    return out


def torgb_bwd(g, x, s, w):
    """-> (gx, gs, gw) from one read of x."""
    B, O, H, W = x.shape
    C = w.shape[0]
    with on_device(x.device):
        gx = torch.empty_like(x)
        gs = torch.empty_like(s)
        gw = torch.empty_like(w)
        nb = lib.hg_torgb_bwd_workspace_bytes(B, O, C, H * W)
        ws = workspace(nb, x.device)
        check(lib.hg_torgb_bwd(g.data_ptr(), x.data_ptr(), s.data_ptr(), w.data_ptr(), gx.data_ptr(), gs.data_ptr(), gw.data_ptr(),
                               B, O, C, H * W, ws.data_ptr(), nb, stream_of(x)), 'hg_torgb_bwd')
    return gx, gs, gw


def demod_style_grad(gd, d, s1, wsq):
    """The style part of the demodulation coefficient's adjoint, 2 s1 * ((-gd d^3 / 2) @ wsq), as one kernel pair."""
    B, N, K = d.shape[0], d.shape[1], s1.shape[1]
    with on_device(gd.device):
        gy = torch.empty_like(s1)
        nb = lib.hg_demod_style_grad_workspace_bytes(B, N, K)
        ws = workspace(nb, gd.device)
        check(lib.hg_demod_style_grad(gd.data_ptr(), d.data_ptr(), s1.data_ptr(), wsq.data_ptr(), gy.data_ptr(), B, N, K,
                                      ws.data_ptr(), nb, stream_of(gd)), 'hg_demod_style_grad')
    return gy


def gstage_bwd(out, ga, sa, up, g_rgb, w_rgb, s_rgb, d, nzt, wn, bn, gw_rgb_out=None):
    """hg_gstage_bwd: -> (gconv, gs_a, gs_rgb, gw_rgb, gd, gwn, gbn); see include/hg_nets.h.
    gw_rgb_out: where to write the to-RGB weight gradient (e.g. the weight's flat gradient slot)."""
    B, Cc, H, _ = out.shape
    S = nzt.shape[-1]
    dev = out.device
    Cr = 0 if g_rgb is None else g_rgb.shape[1]
    with on_device(dev):
        gconv = torch.empty_like(out)
        gs_a = torch.empty((B, Cc), dtype=torch.float32, device=dev) if (ga is not None and sa is not None) else None
        gs_rgb = torch.empty((B, Cc), dtype=torch.float32, device=dev) if (g_rgb is not None and s_rgb is not None) else None
        gw_rgb = None
        if g_rgb is not None:
            gw_rgb = gw_rgb_out if gw_rgb_out is not None else torch.empty((Cr, Cc), dtype=torch.float32, device=dev)
        gd = torch.empty((B, Cc), dtype=torch.float32, device=dev) if d is not None else None
        gwn = torch.empty((Cc,), dtype=torch.float32, device=dev)
        gbn = torch.empty((Cc,), dtype=torch.float32, device=dev)
        nb = lib.hg_gstage_bwd_workspace_bytes(B, Cc, H, int(bool(up)))
        ws = workspace(nb, dev)
        check(lib.hg_gstage_bwd(out.data_ptr(), ptr(ga), ptr(sa), int(bool(up)), ptr(g_rgb), ptr(w_rgb), ptr(s_rgb), Cr,
                                ptr(d), nzt.data_ptr(), wn.data_ptr(), bn.data_ptr(), S, gconv.data_ptr(), ptr(gs_a),
                                ptr(gs_rgb), ptr(gw_rgb), ptr(gd), gwn.data_ptr(), gbn.data_ptr(), B, Cc, H, ws.data_ptr(), nb,
                                stream_of(out)), 'hg_gstage_bwd')
    return gconv, gs_a, gs_rgb, gw_rgb, gd, gwn, gbn
