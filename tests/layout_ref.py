"""Test helper (NOT a test module): operand layouts for the generator / discriminator side kernels, and the fp64 torch
restatements that no other *_ref.py has (tests/test_operand_layout_gpu.py, tests/test_operand_layout_cpu.py).

These kernels take bare pointers plus shapes; `_lib.f32c` makes every operand fp32 and contiguous, nothing makes it 16-byte
aligned: a parameter and its gradient slot are contiguous views into an optim.FlatParams buffer and sit at any 4-byte address
behind an odd-sized parameter.

What each launcher does with a pointer that is 4-byte aligned only, read from histogan_amd/csrc (one line per launcher):

  scalar    4-byte accesses only
  global    8- / 16-byte accesses, all of them global or buffer loads / stores (dword alignment suffices; the offsets never
            reach an LDS address: every LDS index in these files comes from thread and loop indices)
  selected  the host picks another kernel when the pointer is not 16-byte aligned
  refused   the launcher returns HG_EINVAL

  hg_nets.hip
    hg_modulate_fwd          x, out: global (float4; up: scalar x, float2 out)      s: scalar
    hg_modulate_bwd          gout, x, gx: up -> selected (k_modulate_bwd<2> aligned and W even, else <1> scalar); no up: global
                             s, gs, workspace: scalar
    hg_demod_noise_lrelu_fwd conv, out, nzt: global when H % 4 == 0 (nzt rows at i S + j: any S >= H), else scalar
                             d, wn, bn: scalar
    hg_demod_noise_lrelu_bwd gout, out, conv, nzt, gconv: global when H % 4 == 0 and S % 4 == 0, else scalar
                             d, wn, bn, gd, gwn_part, gbn_part: scalar
    hg_noise_grad            gconv: selected (k_noise_grad<4> when H % 4 == 0 and aligned, else <1>)      d, wn, gnzt: scalar
    hg_channel_sum           g: global when HW % 4 == 0, else scalar      out: scalar
    hg_lrelu_bwd_channel_sum g, out, gm: global when HW % 4 == 0, else scalar      csum: scalar
    hg_demod_style_grad      gd, d, s1, wsq, gy: scalar
    hg_demod_weight_term     w, gw: global when K taps % 4 == 0, else scalar      gd, d, s1: scalar
    hg_diffgrad_step(_dev), hg_ema_update      every buffer: scalar
  hg_gstage.hip
    hg_gstage_bwd            out, ga, g_rgb, nzt, gconv: global (f32x4; behind the upsample f32x2 / f32x4 rows)
                             sa, s_rgb, w_rgb, d, wn, bn, gs_a, gs_rgb, gw_rgb, gd, gwn, gbn: scalar
  hg_torgb.hip
    hg_torgb_fwd             x, prev, out: global (f32x4)      s, w: scalar (w (s + 1) staged in LDS by element index)
    hg_torgb_bwd             g, x, gx: global (f32x4)      s, w, gs, gw: scalar
  hg_conv.hip
    hg_conv_pack_weights, _both, _multi        w, wsq: scalar; wt: scalar stores
    hg_conv2d_fwd, _fwd_add, hg_modconv2d_fwd, hg_conv2d_dgrad
                             in / gout, wt, iscale: global (buffer loads, b32 / b128)      out, addend, noise_img: global (f32x2)
                             bias, oscale, noise_w: scalar
    hg_conv2d_wgrad          in, gout: global (buffer loads)      gw: global (f32x4 store from the LDS transpose, whose LDS
                             side is indexed by row and lane) or scalar      slab: allocated by the caller
  hg_wino.hip
    hg_wino_pack_weights, _multi               w: scalar
    hg_wino_conv2d           in, u, iscale: global (buffer loads b32 / b64 / b128; the input descriptor's base is `in - (W + 1)`
                             floats: unaligned by construction)      out, addend, noise_img: global (f32x2 / f32x4)
                             bias, oscale, noise_w: scalar
    hg_wino_wgrad            in, gout: global (buffer loads)      gw: scalar
  hg_linear.hip
    hg_grouped_linear_fwd, _bwd_input, _bwd_params       x, w, y (backward: the incoming gradient), gx: refused
                             b, gw, gb: scalar
                             -> ops.grouped_linear_supported is False for such a weight; _GroupedLinear copies x and gy
  hg_recolor.hip
    hg_instnorm_lrelu_fwd / _bwd               x, out, gout, gx: global when HW % 4 == 0, else scalar      stats: scalar
    hg_stencil3              x, out: scalar
    hg_depthwise_valid       x, k, out: scalar (LDS tile indexed by tile coordinates)
  hg_augment.hip
    hg_augment_spatial       x, params, out: scalar
    hg_sample_mean           x: global when CHW % 4 == 0, else scalar      mean: scalar
    hg_augment_color         x, mean, color, out: scalar
  hg_hellinger.hip
    hg_hellinger_fwd_bwd     target, gen, grad_gen, loss_out: scalar
"""
import torch
import torch.nn.functional as F


def shifted(t, k):
    """A contiguous tensor equal to `t` (4-byte elements) whose data_ptr() % 16 == 4 k, k in {1, 2, 3}: carved from a
    buffer of numel + 4."""
    assert k in (1, 2, 3) and t.element_size() == 4
    t = t.detach()
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    base = buf.data_ptr()
    assert base % 4 == 0
    off = ((4 * k - base) % 16) // 4
    out = buf[off:off + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 * k and out.is_contiguous()
    return out


def layouts(t):
    """(name, view) pairs: views equal to `t` that are not contiguous.  'channels_last': the permuted storage viewed in the
    logical order (4-d: NHWC storage as NCHW; otherwise the last two dimensions swapped in storage); 'every_other_column': every
    second element of a last dimension twice as long; 'batch_expanded': one batch entry with stride 0, when all entries of
    `t` are equal.  Views that come out contiguous (an extent of 1) are left out."""
    t = t.detach()
    out = []
    if t.dim() == 4:
        out.append(('channels_last', t.contiguous(memory_format=torch.channels_last)))
    elif t.dim() >= 2:
        out.append(('channels_last', t.transpose(-1, -2).contiguous().transpose(-1, -2)))
    if t.dim() >= 1:
        wide = torch.empty(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
        wide.fill_(float('nan') if t.is_floating_point() else 0)
        v = wide[..., ::2]
        v.copy_(t)
        out.append(('every_other_column', v))
    if t.dim() >= 2 and t.shape[0] > 1 and bool((t == t[:1]).all()):
        out.append(('batch_expanded', t[:1].clone().expand(t.shape)))      # (a storage of ONE entry, as initial_block.expand)
    for name, v in out:
        if not v.is_contiguous():
            assert v.shape == t.shape and torch.equal(v, t)
            yield name, v


# ---- fp64 restatements ------------------------------------------------------------------------------------------------
def up2_fp64(x):
    return F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)


def modulate_fp64(x, s, up, gout):
    """[up2](x) (s + 1) and its adjoint for the upstream gradient gout -> (out, gx, gs); s None: no modulation, gs None."""
    xd = x.double().requires_grad_(True)
    sd = None if s is None else s.double().requires_grad_(True)
    y = up2_fp64(xd) if up else xd
    if sd is not None:
        y = y * (sd + 1)[:, :, None, None]
    g = torch.autograd.grad(y, [xd] + ([sd] if sd is not None else []), gout.double())
    return y.detach(), g[0], (g[1] if sd is not None else None)


def dnl_fp64(conv, d, nzt, wn, bn):
    """lrelu_0.2(conv d + wn nzt[:, :H, :H] + bn) in fp64 (GeneratorBlock.forward's epilogue with the noise image already
    transposed); d None: no demodulation."""
    H = conv.shape[-1]
    pre = conv.double() * (d.double()[:, :, None, None] if d is not None else 1.0) \
        + wn.double().reshape(1, -1, 1, 1) * nzt.double()[:, None, :H, :H] + bn.double().reshape(1, -1, 1, 1)
    return F.leaky_relu(pre, 0.2)


def dnl_bwd_fp64(g, out, conv, d, nzt):
    """The adjoint sums of hg_demod_noise_lrelu_bwd in fp64 on the LeakyReLU branches of `out` (the run's own output):
    m = g lrelu'(out) -> (gconv = m d, gd = sum m conv, gw_part = sum m nzt, gb_part = sum m), the last three (B, O)."""
    H = conv.shape[-1]
    m = g.double() * torch.where(out > 0, 1.0, 0.2).double()
    dd = d.double()[:, :, None, None] if d is not None else 1.0
    return (m * dd, (m * conv.double()).sum(dim=(2, 3)), (m * nzt.double()[:, None, :H, :H]).sum(dim=(2, 3)), m.sum(dim=(2, 3)))


def torgb_fp64(x, s, w, prev, gout):
    """conv1x1(x (s + 1), w) + prev and its adjoint -> (out, gx, gs, gw); w (C, O)."""
    xd, sd, wd = (t.double().requires_grad_(True) for t in (x, s, w))
    y = torch.einsum('co,bo,bohw->bchw', wd, sd + 1.0, xd)
    if prev is not None:
        y = y + prev.double()
    gx, gs, gw = torch.autograd.grad(y, [xd, sd, wd], gout.double())
    return y.detach(), gx, gs, gw


def demod_terms_fp64(w, gd, d, s1):
    """The demodulation coefficient's adjoint (ops._DemodCoeff.backward) in fp64 -> (style part gy (B, K), weight part gw)."""
    wd, gq = w.double(), gd.double() * (-0.5) * d.double() ** 3
    s = s1.double()
    return 2.0 * s * (gq @ wd.pow(2).sum(dim=(2, 3))), 2.0 * wd * (gq.t() @ (s * s))[:, :, None, None]


def instnorm_lrelu_fp64(x, gout, eps=1e-5, slope=0.2):
    """-> (out, gx, scale): scale = max |gout| rstd, what the gradient bar of test_instnorm_lrelu_matches_torch multiplies."""
    xd = x.double().requires_grad_(True)
    y = F.leaky_relu(F.instance_norm(xd, eps=eps), slope)
    gx, = torch.autograd.grad(y, xd, gout.double())
    rstd = 1.0 / torch.sqrt(xd.detach().var(dim=(2, 3), unbiased=False, keepdim=True) + eps)
    return y.detach(), gx, float((gout.double().abs() * rstd).max())


def stencil3_fp64(x, taps, gout):
    xd = x.double().requires_grad_(True)
    k = torch.as_tensor(taps, dtype=torch.float64, device=x.device).reshape(1, 1, 3, 3).expand(1, x.shape[1], 3, 3)
    y = F.conv2d(xd, k, padding=1)
    gx, = torch.autograd.grad(y, xd, gout.double())
    return y.detach(), gx


def gaussian_valid_fp64(x, k2, gout):
    xd = x.double().requires_grad_(True)
    C, KS = x.shape[1], k2.shape[-1]
    y = F.conv2d(xd, k2.double().reshape(1, 1, KS, KS).expand(C, 1, KS, KS), groups=C)
    gx, = torch.autograd.grad(y, xd, gout.double())
    return y.detach(), gx


def hellinger_fp64(t, g, alpha):
    """The reference's inline formula (histoGAN/histoGAN.py:957-960) and its gradient for the generated histogram."""
    gd = g.double().requires_grad_(True)
    loss = alpha * (0.5 ** 0.5) * torch.sqrt(torch.sum((torch.sqrt(t.double()) - torch.sqrt(gd)) ** 2)) / g.shape[0]
    grad, = torch.autograd.grad(loss, gd)
    return float(loss.detach()), grad


def augment_spatial_fp64(x, p):
    """hg_augment_spatial's forward map by index arithmetic (include/hg_augment.h: flip -> roll -> zero-filled shift ->
    cutout); p (B, 9) int rows [flip, roll_h, roll_w, shift_h, shift_w, r0, r1, c0, c1], rolls already reduced."""
    B, C, H, W = x.shape
    out = torch.zeros_like(x, dtype=torch.float64)
    xs = x.double()
    for b in range(B):
        flip, rh, rw, sh, sw, r0, r1, c0, c1 = (int(v) for v in p[b])
        for i in range(H):
            for j in range(W):
                ti, tj = i + sh, j + sw
                if (r0 <= i <= r1 and c0 <= j <= c1) or not (0 <= ti < H and 0 <= tj < W):
                    continue
                si, sj = (ti - rh) % H, (tj - rw) % W
                if flip:
                    sj = W - 1 - sj
                out[b, :, i, j] = xs[b, :, si, sj]
    return out


def augment_color_fp64(x, color):
    """utils/diff_augment.py brightness -> saturation -> contrast with given (B, 3) [offset, saturation, contrast]."""
    xs = x.double()
    br, sat, con = (color.double()[:, k].reshape(-1, 1, 1, 1) for k in range(3))
    xs = xs + br
    mc = xs.mean(dim=1, keepdim=True)
    xs = (xs - mc) * sat + mc
    m = xs.mean(dim=(1, 2, 3), keepdim=True)
    return (xs - m) * con + m
