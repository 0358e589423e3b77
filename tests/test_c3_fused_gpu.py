"""fp64 parity of the kernels fused AROUND the convolution GEMMs, at every launch shape of the C3 train step (BASELINE.json
configs[2]: 256^2, network_capacity 16, B = 32, latent 512, noise size 256).  tests/test_c3_parity_gpu.py pins the GEMMs
at these shapes; the fused epilogues / prologues / reductions were pinned only at toy shapes, which never select the
multi-block finish, the chunked planes, the many-planes-per-block layouts or the wrapping grid-stride loops.

Every case draws seeded fp32 inputs scaled like the live network and compares the HIP launch with a plain fp64 torch
expression of the same operation on the same device.  Every case also asserts that it is not vacuous: the share of
negative LeakyReLU pre-activations lies in [0.2, 0.8] and the reduced outputs are non-zero.

Bars (each no looser than the small-shape test of the same kernel):
* element-wise outputs -- max-norm relative error (conftest.relmax, evaluated on the device):
  - 2e-6 for pure element-wise outputs (modulated / up-sampled tensors and their data gradient, gconv of the stage
    backward, to-RGB output and data gradient): a handful of fp32 roundings of at most 19 terms;
  - 5e-6 for the fused convolution epilogues (generator stage forward, discriminator conv + LeakyReLU, residual add):
    the GEMM bar of the convolution census, the epilogue adds O(1) roundings;
  - 5e-6 / 1e-5 for the discriminator block's first-order data / weight gradients (the census bars of those GEMMs), 2e-5
    for its gradient-penalty (double backward) gradients, as in test_conv_gpu.test_conv2d_lrelu_and_its_double_backward;
  - 1e-6 for DiffGrad / EMA parameters and state (one update is a few roundings per element).
* reductions (gd, gwn, gbn, gs_a, gs_rgb, gw_rgb of the stage backward, the modulation / to-RGB style and weight
  gradients, channel sums, demodulation adjoints): |ours - fp64| <= 1e-6 * sum|terms| per output element, the fp64 sum of
  the absolute values of the summed terms computed from the same inputs.  A plain relmax would be flaky: at 2 M
  random-sign terms sum|terms| / |sum| reaches ~1e3.  fp32 summation of random-sign terms errs by ~eps * sum|terms|
  (6e-8); 1e-6 is ~16 eps.  The inputs the kernels get are exactly the ones the reference gets (drawn in fp32, or drawn in
  fp64 and rounded to fp32): an fp64-only input would hand the kernel a rounded style s next to a style-sum s + 1 that
  cancels where s ~ -1, and measured up to 2.5e-4 of sum|terms| in gd on 4x4 planes that is not the kernel's error.
* DiffGrad, one step from the same fp32 state: |p_ours - p_fp64| <= ulp(p_ours) / 2 + 1e-6 * step_size * dfc *
  (|b1 m| + |(1 - b1) g|) / (sqrt(v) + eps): the rounding of the stored parameter plus 1e-6 of the update's own terms
  (the first moment is a two-term sum that can cancel).  The four launch forms must be bit-identical.

Each reduction family also computes the distance of one deliberately wrong fp64 reference (a dropped last pixel row of
every plane, a dropped batch image, the bias correction of step t - 1) and asserts it exceeds the bar >= 10x: the bars
would catch such a bug.  Measured errors and those distances are recorded as test-suite properties (pytest --junitxml)."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

from gstage_ref import gstage_fp64, gstage_inputs, run_gstage

pytestmark = pytest.mark.gpu

B, LAT, S_, CAP = 32, 512, 256, 16
GF = [4 * CAP] + [CAP * 2 ** (i + 1) for i in range(7)][::-1]        # 64, 2048, 1024, ..., 32
DF = [3] + [CAP * 2 ** i for i in range(8)]                             # 3, 16, ..., 2048
EL, EL_CONV, RED, OPT = 2e-6, 5e-6, 1e-6, 1e-6
SENS = 10.0


def _record(record_testsuite_property, key, val):
    """A case's measured errors and sensitivity distances, as a test-suite property (kept by pytest --junitxml)."""
    record_testsuite_property(key, json.dumps(val, sort_keys=True))


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _gen(dev, *key):
    return torch.Generator(device=dev).manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _rel(a, b):
    """conftest.relmax on the device."""
    a, b = a.detach().double(), b.detach().double()
    den = b.abs().max()
    return float((a - b).abs().max() / (den if den > 0 else 1.0))


def _red(ours, ref, terms):
    """max |ours - ref| / sum|terms| (an element with no terms must be exact)."""
    err = (ours.detach().double() - ref.detach().double()).abs()
    return float((err / terms.clamp_min(1e-300)).max())


def _sens(dropped, terms):
    """Distance of a wrong reference that lacks the partial sum `dropped`, in units of the reduction bar."""
    return float((dropped.abs() / terms.clamp_min(1e-300)).max()) / RED


def _neg_share(pre):
    return float((pre < 0).double().mean())


def _up2t(a):
    """Adjoint of the bilinear x2 (align_corners=False, edge clamp): non-negative weights, so _up2t(|a|) bounds terms."""
    x = torch.zeros(a.shape[0], a.shape[1], a.shape[2] // 2, a.shape[3] // 2, dtype=a.dtype, device=a.device,
                    requires_grad=True)
    return torch.autograd.grad(F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False), x, a)[0]


def _up2(x):
    return F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)


# ---- 1. generator forward stage: conv + demodulation + noise + LeakyReLU in one launch ---------------------------------
def _gconvs():
    """(tag, K, N, H) of the 14 modulated convolutions (reference filter arithmetic, histoGAN/histoGAN.py:541-543)."""
    out = []
    for i in range(7):
        H = 4 * 2 ** i
        out += [(f'G{i}.conv1', GF[i], GF[i + 1], H), (f'G{i}.conv2', GF[i + 1], GF[i + 1], H)]
    return out


def _wino_served(K, H):
    """The plan this test pins: every modulated convolution at B = 32 takes k_wino except block 0's conv1 (64 -> 2048 at
    4x4), which takes the direct kernel.  Asserted against hg_wino_supported so that a dispatch change is noticed."""
    return not (K == 64 and H == 4)


FWD_CASES = [(tag, K, N, H, form, kern) for tag, K, N, H in _gconvs() for form in ('train', 'infer')
             for kern in (('wino', 'direct') if _wino_served(K, H) else ('direct',))]


def _direct_modconv(x, w, N, iscale, d, bn, wn, nzt):
    from histogan_amd import conv as C
    from histogan_amd._lib import check, lib, raw_stream
    Bx, K, H, W = x.shape
    wt = C._pack_weights(w, C.PACK_FWD)
    out = torch.empty((Bx, N, H, W), dtype=torch.float32, device=x.device)
    nb = lib.hg_conv2d_workspace_bytes(Bx, K, N, H, W, 3, 1, 0)
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=x.device)
    p = lambda t: None if t is None else t.data_ptr()
    check(lib.hg_modconv2d_fwd(x.data_ptr(), wt.data_ptr(), out.data_ptr(), p(iscale), d.data_ptr(), bn.data_ptr(),
                               wn.data_ptr(), nzt.data_ptr(), nzt.shape[-1], 0.2, Bx, K, N, H, W, 3, ws.data_ptr(), nb,
                               raw_stream(x.device)), 'hg_modconv2d_fwd')
    return out


@pytest.mark.parametrize('tag,K,N,H,form,kern', FWD_CASES, ids=lambda v: str(v))
def test_generator_stage_forward_matches_fp64(tag, K, N, H, form, kern, gpu_device, record_testsuite_property):
    """lrelu(d conv2d(x (s+1), W) + wn nz[:H,:H] + bn, 0.2) at B = 32: `train` feeds the modulated input with iscale=None
    (gfused._GeneratorTrain), `infer` the raw input with iscale = s + 1 (gfused.generator_infer).  Both kernels where both
    serve the shape; the dispatcher (conv.modconv_fwd_packed) must return the served kernel's result bit for bit."""
    from histogan_amd import conv as C
    dev = gpu_device
    g = _gen(dev, K, N, H, form == 'train', kern == 'wino')
    assert C.wino_supported(B, K, N, H, H) == _wino_served(K, H)
    x = torch.randn(B, K, H, H, generator=g, device=dev)
    s = torch.randn(B, K, generator=g, device=dev) * 0.5
    w = torch.randn(N, K, 3, 3, generator=g, device=dev) / (9 * K) ** 0.5
    d = torch.rand(B, N, generator=g, device=dev) + 0.5
    nzt = torch.rand(B, S_, S_, generator=g, device=dev)
    wn, bn = torch.randn(N, generator=g, device=dev) * 0.5, torch.randn(N, generator=g, device=dev) * 0.2
    s1 = s + 1.0
    xin, isc = ((x * s1[:, :, None, None]).contiguous(), None) if form == 'train' else (x, s1)
    if kern == 'wino':
        out = C.wino_conv(xin, C._wino_pack(w, C.PACK_FWD), N, isc, d, bn, wn, nzt, S_, 0.2)
    else:
        out = _direct_modconv(xin, w, N, isc, d, bn, wn, nzt)
    disp = C.modconv_fwd_packed(xin, C.pack_weights(w, C.PACK_FWD), N, 3, isc, d, bn, wn, nzt, S_, 0.2)
    served = 'wino' if _wino_served(K, H) else 'direct'
    if kern == served:
        assert torch.equal(disp, out)
    xd = xin.double() if isc is None else x.double() * s1.double()[:, :, None, None]
    pre = F.conv2d(xd, w.double(), padding=1) * d.double()[:, :, None, None] \
        + wn.double()[None, :, None, None] * nzt.double()[:, None, :H, :H] + bn.double()[None, :, None, None]
    ref = F.leaky_relu(pre, 0.2)
    e, neg = _rel(out, ref), _neg_share(pre)
    _record(record_testsuite_property, f'gfwd/{tag}/{form}/{kern}', dict(err=e, neg=neg, served=served))
    assert 0.2 <= neg <= 0.8
    assert e <= EL_CONV, e


# ---- 2. prologue: modulation (+ bilinear x2) and its adjoint -------------------------------------------------------------
def _mod_cases():
    out = [('G0.conv1', GF[0], 4, False, True)]
    for i in range(7):
        H = 4 * 2 ** i
        out.append((f'G{i}.conv2', GF[i + 1], H, False, True))
        if i < 6:
            out.append((f'G{i}.out2->G{i + 1}.conv1', GF[i + 1], H, True, True))
            out.append((f'G{i}.rgb->G{i + 1}.prev', 3, H, True, False))
    return out


@pytest.mark.parametrize('tag,Cc,H,up,with_s', _mod_cases(), ids=lambda v: str(v))
def test_modulate_matches_fp64(tag, Cc, H, up, with_s, gpu_device, record_testsuite_property):
    """hg_modulate_fwd / hg_modulate_bwd (ops.modulate) vs up2(x) (s + 1) and its fp64 autograd: output and data gradient
    relmax 2e-6, style gradient (a sum over the (2H)^2 pixels) against sum|terms|."""
    from histogan_amd import ops
    dev = gpu_device
    g = _gen(dev, Cc, H, up, with_s, 11)
    x = torch.randn(B, Cc, H, H, generator=g, device=dev)
    s = torch.randn(B, Cc, generator=g, device=dev) * 0.5 if with_s else None
    Ho = 2 * H if up else H
    go = torch.randn(B, Cc, Ho, Ho, generator=g, device=dev)
    xr = x.clone().requires_grad_(True)
    sr = s.clone().requires_grad_(True) if with_s else None
    y = ops.modulate(xr, sr, up)
    grads = torch.autograd.grad(y, [xr] + ([sr] if with_s else []), go)
    xd = x.double().requires_grad_(True)
    sd = s.double().requires_grad_(True) if with_s else None
    yd = _up2(xd) if up else xd
    if with_s:
        yd = yd * (sd + 1)[:, :, None, None]
    want = torch.autograd.grad(yd, [xd] + ([sd] if with_s else []), go.double())
    e = dict(out=_rel(y, yd), gx=_rel(grads[0], want[0]))
    assert e['out'] <= EL and e['gx'] <= EL, e
    if with_s:
        ux = _up2(x.double()) if up else x.double()
        terms = (go.double().abs() * ux.abs()).sum(dim=(2, 3))
        assert float(want[1].abs().max()) > 0
        e['gs'] = _red(grads[1], want[1], terms)
        e['gs_sens_last_row'] = _sens((go.double() * ux)[:, :, -1, :].sum(-1), terms)
        assert e['gs'] <= RED and e['gs_sens_last_row'] >= SENS, e
    _record(record_testsuite_property, f'modulate/{tag}', e)


# ---- 3. hg_gstage_bwd at the 14 stages of the generator ------------------------------------------------------------------
def _stages():
    out = []
    for i in range(7):
        H, Cc = 4 * 2 ** i, GF[i + 1]
        out.append((f'G{i}.stage1', Cc, H, False, False))
        out.append((f'G{i}.stage2', Cc, H, True, True) if i < 6 else (f'G{i}.stage2', Cc, H, None, True))
    return out


def _gstage_chunks(planes, H, up):
    """geom() of hg_gstage.hip: the number of chunks a plane is split into (recorded only)."""
    V = H * H // (2 if up else 4)
    if V <= 64:
        return 1
    c = (2048 + planes - 1) // planes
    return int(max(1, min(c, (V + 1023) // 1024, 64)))


@pytest.mark.parametrize('tag,Cc,H,up,rgb', _stages(), ids=lambda v: str(v))
def test_gstage_bwd_at_c3_stage_matches_fp64(tag, Cc, H, up, rgb, gpu_device, record_testsuite_property):
    """All seven outputs of hg_gstage_bwd against fp64 autograd of the replaced chain (tests/gstage_ref.py, as in
    test_gstage_gpu): gconv relmax 2e-6; gd, gwn, gbn, gs_a, gs_rgb, gw_rgb against sum|terms|."""
    dev = gpu_device
    g = _gen(dev, Cc, H, 0 if up is None else 1 + int(up), rgb, 3)
    inp = {k: None if v is None else v.float().double() for k, v in gstage_inputs(B, Cc, H, S_, up, rgb, g).items()}
    out, want = gstage_fp64(inp, up, rgb)
    gconv, gs_a, gs_rgb, gw_rgb, gd, gwn, gbn = run_gstage(out, inp, up, rgb, dev)
    pre_neg = float((out < 0).double().mean())
    # sum|terms| of every reduction (the kernel's own sums: include/hg_nets.h), and the signed terms of the last pixel row
    slope = (out > 0).double() * 0.8 + 0.2
    nz = inp['nzt'][:, None, :H, :H]
    Ga = torch.zeros_like(out)
    Gs = torch.zeros_like(out)
    terms, rows = {}, {}
    if up is not None:
        ga = inp['ga']
        Ta, Ts = (_up2t(ga.abs()), _up2t(ga)) if up else (ga.abs(), ga)
        Ga += Ta * (inp['sa'] + 1).abs()[:, :, None, None]
        Gs += Ts * (inp['sa'] + 1)[:, :, None, None]
        terms['gs_a'] = (out.abs() * Ta).sum(dim=(2, 3))
        rows['gs_a'] = (out * Ts)[:, :, -1].sum(-1)
        del Ta, Ts
    if rgb:
        w, gr = inp['w'], inp['g_rgb']
        TRa, TRs = torch.einsum('kc,bkij->bcij', w.abs(), gr.abs()), torch.einsum('kc,bkij->bcij', w, gr)
        Ga += TRa * (inp['srgb'] + 1).abs()[:, :, None, None]
        Gs += TRs * (inp['srgb'] + 1)[:, :, None, None]
        terms['gs_rgb'] = (out.abs() * TRa).sum(dim=(2, 3))
        rows['gs_rgb'] = (out * TRs)[:, :, -1].sum(-1)
        o1 = out * (inp['srgb'] + 1)[:, :, None, None]
        terms['gw_rgb'] = torch.einsum('bkij,bcij->kc', gr.abs(), o1.abs())
        rows['gw_rgb'] = torch.einsum('bkj,bcj->kc', gr[:, :, -1], o1[:, :, -1])
        del TRa, TRs, o1
    ma, ms = Ga * slope, Gs * slope
    del Ga, Gs
    terms['gd'] = (ma * inp['conv'].abs()).sum(dim=(2, 3))
    rows['gd'] = (ms * inp['conv'])[:, :, -1].sum(-1)
    terms['gwn'] = (ma * nz).sum(dim=(0, 2, 3))
    rows['gwn'] = (ms * nz)[:, :, -1].sum(dim=(0, 2))
    terms['gbn'] = ma.sum(dim=(0, 2, 3))
    rows['gbn'] = ms[:, :, -1].sum(dim=(0, 2))
    del ma, ms
    ours = dict(gd=gd, gwn=gwn, gbn=gbn, gs_a=gs_a, gs_rgb=gs_rgb, gw_rgb=gw_rgb)
    refs = dict(gd=want[1], gwn=want[2], gbn=want[3], gs_a=want[4], gs_rgb=want[5], gw_rgb=want[6])
    e = dict(gconv=_rel(gconv, want[0]), neg=pre_neg, chunks=_gstage_chunks(B * Cc, H, bool(up)))
    for k in terms:
        assert float(refs[k].abs().max()) > 0, k
        e[k] = _red(ours[k], refs[k], terms[k])
        e[k + '_sens_last_row'] = _sens(rows[k], terms[k])
    _record(record_testsuite_property, f'gstage/{tag}', e)
    assert 0.2 <= pre_neg <= 0.8
    assert e['gconv'] <= EL, e
    for k in terms:
        assert e[k] <= RED, (k, e)
        assert e[k + '_sens_last_row'] >= SENS, (k, e)


# ---- 4. to-RGB -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blk', range(7))
def test_torgb_matches_fp64(blk, gpu_device, record_testsuite_property):
    """ops.torgb (hg_torgb_fwd / hg_torgb_bwd) with the running image at each block's (B = 32, O, 3, S): output and data
    gradient relmax 2e-6, style and weight gradients against sum|terms|, the running image's gradient passed through."""
    from histogan_amd import ops
    dev = gpu_device
    O, H = GF[blk + 1], 4 * 2 ** blk
    g = _gen(dev, O, H, 5)
    x = torch.randn(B, O, H, H, generator=g, device=dev)
    s = torch.randn(B, O, generator=g, device=dev) * 0.5
    w = torch.randn(3, O, 1, 1, generator=g, device=dev) / O ** 0.5
    prev = torch.randn(B, 3, H, H, generator=g, device=dev)
    go = torch.randn(B, 3, H, H, generator=g, device=dev)
    leaves = [t.clone().requires_grad_(True) for t in (x, s, w, prev)]
    rgb = ops.torgb(*leaves)
    gx, gs, gw, gp = torch.autograd.grad(rgb, leaves, go)
    dl = [t.double().requires_grad_(True) for t in (x, s, w, prev)]
    xd, sd, wd, pd = dl
    ref = torch.einsum('ko,bohw->bkhw', wd[:, :, 0, 0], xd * (sd + 1)[:, :, None, None]) + pd
    want = torch.autograd.grad(ref, dl, go.double())
    x64, s1, w64, g64 = x.double(), s.double() + 1, w.double()[:, :, 0, 0], go.double()
    tr_a, tr_s = torch.einsum('ko,bkhw->bohw', w64.abs(), g64.abs()), torch.einsum('ko,bkhw->bohw', w64, g64)
    t_gs = (x64.abs() * tr_a).sum(dim=(2, 3))
    t_gw = torch.einsum('bkhw,bohw->ko', g64.abs(), x64.abs() * s1.abs()[:, :, None, None])
    e = dict(out=_rel(rgb, ref), gx=_rel(gx, want[0]), gs=_red(gs, want[1], t_gs),
             gw=_red(gw.reshape(3, O), want[2][:, :, 0, 0], t_gw),
             gs_sens_last_row=_sens((x64 * tr_s)[:, :, -1].sum(-1), t_gs),
             gw_sens_last_image=_sens(torch.einsum('khw,ohw->ko', g64[-1], x64[-1] * s1[-1][:, None, None]), t_gw))
    _record(record_testsuite_property, f'torgb/G{blk}', e)
    assert torch.equal(gp, go)
    assert float(want[1].abs().max()) > 0 and float(want[2].abs().max()) > 0
    assert e['out'] <= EL and e['gx'] <= EL and e['gs'] <= RED and e['gw'] <= RED, e
    assert e['gs_sens_last_row'] >= SENS and e['gw_sens_last_image'] >= SENS, e


# ---- 5. demodulation adjoints --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,K,N,H', _gconvs(), ids=lambda v: str(v))
def test_demod_adjoints_at_c3_shapes_match_fp64(tag, K, N, H, gpu_device, record_testsuite_property):
    """hg_demod_style_grad and hg_demod_weight_term (written and accumulated) at the 14 (B = 32, N, K) of the modulated
    convolutions, against the fp64 formula of ops._DemodCoeff.backward, each element against sum|terms|."""
    from histogan_amd._lib import check, lib, raw_stream
    dev = gpu_device
    g = _gen(dev, K, N, 13)
    w = torch.randn(N, K, 3, 3, generator=g, device=dev) / (9 * K) ** 0.5
    wsq = w.pow(2).sum(dim=(2, 3))
    s1 = torch.randn(B, K, generator=g, device=dev) * 0.5 + 1.0
    gd = torch.randn(B, N, generator=g, device=dev)
    d = torch.rsqrt((s1 * s1) @ wsq.t() + 1e-8)
    wd, sd, gdd, dd, wsqd = (t.double() for t in (w, s1, gd, d, wsq))
    gq = gdd * (-0.5) * dd ** 3
    # style side: gy[b,k] = 2 s1[b,k] sum_n gq[b,n] wsq[n,k]
    ref_y = 2.0 * sd * (gq @ wsqd)
    t_y = 2.0 * sd.abs() * (gq.abs() @ wsqd)
    gy = torch.full((B, K), float('nan'), device=dev)
    nb = lib.hg_demod_style_grad_workspace_bytes(B, N, K)
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
    check(lib.hg_demod_style_grad(gd.data_ptr(), d.data_ptr(), s1.data_ptr(), wsq.data_ptr(), gy.data_ptr(), B, N, K,
                                  ws.data_ptr(), nb, raw_stream(dev)), 'hg_demod_style_grad')
    # weight side: gw[n,k,t] (+)= 2 w[n,k,t] sum_b gq[b,n] s1[b,k]^2
    ref_w = 2.0 * wd * (gq.t() @ (sd * sd))[:, :, None, None]
    t_w = 2.0 * wd.abs() * (gq.abs().t() @ (sd * sd))[:, :, None, None]
    prior = torch.randn(N, K, 3, 3, generator=g, device=dev) / (9 * K) ** 0.5
    e = dict(gy=_red(gy, ref_y, t_y), gy_sens_last_n=_sens(2.0 * sd * (gq[:, -1:] @ wsqd[-1:]), t_y),
             gw_sens_last_image=_sens(2.0 * wd * (gq[-1][:, None] * (sd[-1] ** 2)[None, :])[:, :, None, None], t_w))
    for acc in (0, 1):
        out = prior.clone()
        check(lib.hg_demod_weight_term(w.data_ptr(), gd.data_ptr(), d.data_ptr(), s1.data_ptr(), out.data_ptr(), B, N, K, 9,
                                       acc, raw_stream(dev)), 'hg_demod_weight_term')
        want = ref_w + prior.double() if acc else ref_w
        e[f'gw_acc{acc}'] = _red(out, want, t_w + (prior.double().abs() if acc else 0.0))
    _record(record_testsuite_property, f'demod/{tag}', e)
    assert float(ref_y.abs().max()) > 0 and float(ref_w.abs().max()) > 0
    assert e['gy'] <= RED and e['gw_acc0'] <= RED and e['gw_acc1'] <= RED, e
    assert e['gy_sens_last_n'] >= SENS and e['gw_sens_last_image'] >= SENS, e


# ---- 6. discriminator epilogues ------------------------------------------------------------------------------------------
D_CASES = [(f'D{i}', DF[i], DF[i + 1], 256 // 2 ** i, b) for i in range(8) for b in (2 * B, B)]


@pytest.mark.parametrize('tag,ci,co,S,b', D_CASES, ids=lambda v: str(v))
def test_d_channel_sums_match_fp64(tag, ci, co, S, b, gpu_device, record_testsuite_property):
    """ops.channel_sum (the residual launch's bias gradient) and conv.lrelu_bwd_channel_sum (the LeakyReLU-masked gradient
    and its bias gradient) at the (b, co, S, S) of the layer -- 64 x 256^2 = 4.2 M terms per channel at D0: the masked
    gradient bit-identical to aten's leaky_relu_backward, the sums against sum|terms|."""
    from histogan_amd import ops
    from histogan_amd.conv import lrelu_bwd_channel_sum
    dev = gpu_device
    g = _gen(dev, co, S, b, 17)
    gr = torch.randn(b, co, S, S, generator=g, device=dev)
    out = torch.randn(b, co, S, S, generator=g, device=dev)
    gm, cs = lrelu_bwd_channel_sum(gr, out, 0.2)
    cs2 = ops.channel_sum(gr)
    assert torch.equal(gm, torch.ops.aten.leaky_relu_backward(gr, out, 0.2, True))
    g64 = gr.double()
    m64 = torch.where(out > 0, g64, 0.2 * g64)
    neg = _neg_share(out)
    t_m, t_g = m64.abs().sum(dim=(0, 2, 3)), g64.abs().sum(dim=(0, 2, 3))
    e = dict(lrelu_csum=_red(cs, m64.sum(dim=(0, 2, 3)), t_m), csum=_red(cs2, g64.sum(dim=(0, 2, 3)), t_g), neg=neg,
             lrelu_csum_sens_last_image=_sens(m64[-1].sum(dim=(1, 2)), t_m),
             csum_sens_last_row=_sens(g64[:, :, -1].sum(dim=(0, 2)), t_g))
    _record(record_testsuite_property, f'dsum/{tag}/b{b}', e)
    assert 0.2 <= neg <= 0.8
    assert e['lrelu_csum'] <= RED and e['csum'] <= RED, e
    assert e['lrelu_csum_sens_last_image'] >= SENS and e['csum_sens_last_row'] >= SENS, e


GP_NAMES = ('gw1', 'gw2', 'gwr')    # (with the LeakyReLU branches fixed the penalty does not depend on the biases)


def _masked(p, m):
    return torch.where(m, p, 0.2 * p)


@pytest.mark.parametrize('tag,ci,co,S,b', D_CASES, ids=lambda v: str(v))
def test_d_block_epilogues_match_fp64(tag, ci, co, S, b, gpu_device, record_testsuite_property):
    """One DiscriminatorBlock body at its C3 shape: conv2d_lrelu -> conv2d_lrelu -> conv2d_add (residual 1x1), as
    nets.DiscriminatorBlock.forward.  Forward per launch from the inputs that launch got (5e-6); first-order gradients of
    every input (5e-6 data, 1e-5 weights, bias gradients -- lrelu_bwd_channel_sum / channel_sum -- against sum|terms|) and
    the gradient-penalty gradients (double backward, 2e-5) against fp64 autograd.  The fp64 chain takes the LeakyReLU
    branches OUR forward took (oracle_step.LreluMasks); disagreements with the fp64 sign are counted and must be
    rounding-sized (<= 1e-5 of the elements, |pre| <= 2e-6 of its layer's max)."""
    from histogan_amd.conv import conv2d_add, conv2d_lrelu, input_grads_only
    dev = gpu_device
    g = _gen(dev, ci, co, S, b, 19)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
    x = rnd(b, ci, S, S)
    w1, b1 = rnd(co, ci, 3, 3) / (9 * ci) ** 0.5, rnd(co) * 0.1
    w2, b2 = rnd(co, co, 3, 3) / (9 * co) ** 0.5, rnd(co) * 0.1
    wr, br = rnd(co, ci, 1, 1) / ci ** 0.5, rnd(co) * 0.1
    go = rnd(b, co, S, S)
    leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2, wr, br)]
    lx, lw1, lb1, lw2, lb2, lwr, lbr = leaves
    h1 = conv2d_lrelu(lx, lw1, lb1, 0.2)
    h2 = conv2d_lrelu(h1, lw2, lb2, 0.2)
    y = conv2d_add(lx, lwr, lbr, h2)
    m1, m2 = h1.detach() > 0, h2.detach() > 0
    e = {}
    with torch.no_grad():          # forward, launch by launch
        pre1 = F.conv2d(x.double(), w1.double(), b1.double(), padding=1)
        pre2 = F.conv2d(h1.double(), w2.double(), b2.double(), padding=1)
        e['h1'] = _rel(h1, F.leaky_relu(pre1, 0.2))
        e['h2'] = _rel(h2, F.leaky_relu(pre2, 0.2))
        e['y'] = _rel(y, F.conv2d(x.double(), wr.double(), br.double()) + h2.double())
        e['neg1'], e['neg2'] = _neg_share(pre1), _neg_share(pre2)
        del pre1, pre2
    # first order
    gr = torch.autograd.grad(y, leaves, go, retain_graph=True)
    dl = [t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2, wr, br)]
    dx, dw1, db1, dw2, db2, dwr, dbr = dl
    flips, total, margin = 0, 0, 0.0

    def chain(xx):
        nonlocal flips, total, margin
        p1 = F.conv2d(xx, dw1, db1, padding=1)
        a1 = _masked(p1, m1)
        p2 = F.conv2d(a1, dw2, db2, padding=1)
        a2 = _masked(p2, m2)
        for p, m in ((p1, m1), (p2, m2)):
            diff = (p.detach() > 0) != m
            n = int(diff.sum())
            total += p.numel()
            if n:
                flips += n
                margin = max(margin, float(p.detach().abs()[diff].max() / p.detach().abs().max()))
        return F.conv2d(xx, dwr, dbr) + a2, a2
    yd, _ = chain(dx)
    want = torch.autograd.grad(yd, dl, go.double())
    del yd
    names = ['gx', 'gw1', 'gb1', 'gw2', 'gb2', 'gwr', 'gbr']
    # the masked gradients in fp64 (their channel sums are gb2 and gb1)
    sl1, sl2 = m1.double() * 0.8 + 0.2, m2.double() * 0.8 + 0.2
    gm2 = go.double() * sl2
    a1z = torch.zeros(b, co, S, S, dtype=torch.float64, device=dev, requires_grad=True)
    gm1 = torch.autograd.grad(F.conv2d(a1z, dw2.detach(), None, padding=1), a1z, gm2)[0] * sl1
    terms = dict(gb1=gm1.abs().sum(dim=(0, 2, 3)), gb2=gm2.abs().sum(dim=(0, 2, 3)),
                 gbr=go.double().abs().sum(dim=(0, 2, 3)))
    for n, a, w_ in zip(names, gr, want):
        if n in terms:
            e[n] = _red(a, w_, terms[n])
        else:
            e[n] = _rel(a, w_)
    del gm1, gm2, a1z
    # gradient penalty: d/dparams of (|| d <y, go> / dx || - 1)^2, through input_grads_only as in the trainer
    with input_grads_only():
        gxo, = torch.autograd.grad((y * go).sum(), lx, create_graph=True)
    gp = ((gxo.reshape(b, -1).norm(2, dim=1) - 1) ** 2).mean()
    g2 = torch.autograd.grad(gp, [lw1, lw2, lwr])
    yd2, _ = chain(dx)
    gxd, = torch.autograd.grad((yd2 * go.double()).sum(), dx, create_graph=True)
    gpd = ((gxd.reshape(b, -1).norm(2, dim=1) - 1) ** 2).mean()
    want2 = torch.autograd.grad(gpd, [dw1, dw2, dwr])
    e['gp'] = abs(float(gp.detach()) - float(gpd.detach())) / max(1.0, abs(float(gpd.detach())))
    for n, a, w_ in zip(GP_NAMES, g2, want2):
        e['gp_' + n] = _rel(a, w_)
    e.update(flips=flips, total=total, flip_margin=margin)
    _record(record_testsuite_property, f'dblock/{tag}/b{b}', e)
    assert 0.2 <= e['neg1'] <= 0.8 and 0.2 <= e['neg2'] <= 0.8, e
    assert flips <= 1e-5 * total and margin <= 2e-6, e
    assert e['h1'] <= EL_CONV and e['h2'] <= EL_CONV and e['y'] <= EL_CONV, e
    assert e['gx'] <= 5e-6 and max(e['gw1'], e['gw2'], e['gwr']) <= 1e-5, e
    assert max(e['gb1'], e['gb2'], e['gbr']) <= RED, e
    assert e['gp'] <= 1e-5 and max(e['gp_' + n] for n in GP_NAMES) <= 2e-5, e
    assert all(float(w_.abs().max()) > 0 for w_ in list(want) + list(want2))


# ---- 7. DiffGrad and EMA over the real flat buffers ----------------------------------------------------------------------
LR, BETAS, EPS, STEPS = 2e-4, (0.5, 0.9), 1e-8, 3


class _StubReducer:
    """ddp.GradAllReduce's interface for DiffGrad.step_buckets: buckets with odd, unaligned boundaries."""

    def __init__(self, n, n_conv):
        cuts = sorted({0, 1, 4097, n_conv // 3 + 1, n_conv - 5, n_conv + 3, n - 7, n})
        self.ranges = list(zip(cuts[:-1], cuts[1:]))
        self.waited, self.finished = [], 0

    def wait(self, i):
        self.waited.append(i)

    def finish(self):
        self.finished += 1


def _net_shapes(which):
    from histogan_amd.nets import Discriminator, Generator
    from histogan_amd.optim import conv_first
    with torch.device('meta'):
        net = Generator(S_, LAT, CAP) if which == 'G' else Discriminator(S_, CAP)
    return [tuple(p.shape) for p in conv_first(list(net.parameters()))]


def _grads(n, t, prev, g):
    """Step t's gradient: magnitudes 1e-6 ... 10 of random sign, ~1% exact zeros and (t > 1) ~1% equal to the previous
    gradient (dfc = sigmoid(0) = 0.5)."""
    dev = prev.device
    mag = torch.pow(10.0, torch.rand(n, generator=g, device=dev) * 7 - 6)
    gr = mag * torch.where(torch.rand(n, generator=g, device=dev) < 0.5, -1.0, 1.0)
    u = torch.rand(n, generator=g, device=dev)
    gr = torch.where(u < 0.01, torch.zeros_like(gr), gr)
    if t > 1:
        gr = torch.where((u >= 0.01) & (u < 0.02), prev, gr)
    return gr


def _ulp(x):
    a = x.abs()
    return (torch.nextafter(a, torch.full_like(a, float('inf'))) - a).double()


@pytest.mark.parametrize('which', ['G', 'D'])
def test_diffgrad_and_ema_on_flat_buffers_match_fp64(which, gpu_device, record_testsuite_property):
    """FlatParams of Generator(256, 512, 16) / Discriminator(256, 16) (83 M / 91 M elements: the grid-stride loops wrap
    ~80x), 3 DiffGrad steps: (a) one hg_diffgrad_step, (b) split at n_conv (two offset launches, as step_buckets does per bucket),
    (c) DiffGrad.step_buckets behind a stub reducer, (d) hg_diffgrad_step_dev fed by hg_diffgrad_step_size -- all
    bit-identical in parameters and state; (a) against oracle.histogan_nets.diffgrad_step in fp64 step by step (update
    bar in the module docstring) and over the whole run (relmax 1e-6); then ema_update against fp64."""
    from histogan_amd._lib import check, lib, raw_stream
    from histogan_amd.optim import DiffGrad, FlatParams, ema_update
    from oracle import histogan_nets as N
    dev = gpu_device
    shapes = _net_shapes(which)
    g = _gen(dev, len(shapes), 23)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g, device=dev) * 0.05) for s in shapes]
    flat = FlatParams(ps)
    n, n_conv = flat.numel, flat.n_conv
    assert 0 < n_conv < n and n > 4096 * 256 * 16
    b1, b2 = BETAS
    opt = DiffGrad(flat, lr=LR, betas=BETAS, eps=EPS)                      # (a)
    forms = {k: [flat.data.clone()] + [torch.zeros(n, device=dev) for _ in range(3)] for k in 'bd'}
    red = _StubReducer(n, n_conv)
    fc = FlatParams([torch.nn.Parameter(flat.data.clone())])              # (c): a DiffGrad of its own over a copy
    opt_c = DiffGrad(fc, lr=LR, betas=BETAS, eps=EPS)
    ssz = torch.zeros((), dtype=torch.float32, device=dev)
    st = raw_stream(dev)
    t64 = dict(step=0, exp_avg=torch.zeros(n, dtype=torch.float64, device=dev),
               exp_avg_sq=torch.zeros(n, dtype=torch.float64, device=dev),
               previous_grad=torch.zeros(n, dtype=torch.float64, device=dev))
    p64 = flat.data.double()
    prev = torch.zeros(n, device=dev)
    e = {}
    for t in range(1, STEPS + 1):
        gr = _grads(n, t, prev, g)
        prev = gr
        # one step of the fp64 oracle from OUR fp32 state (and the same with the bias correction of step t - 1)
        p_old, m_old, v_old, pg_old = (a.double() for a in (flat.data, opt.exp_avg, opt.exp_avg_sq, opt.previous_grad))
        one = dict(step=t - 1, exp_avg=m_old.clone(), exp_avg_sq=v_old.clone(), previous_grad=pg_old.clone())
        p_one = p_old.clone()
        N.diffgrad_step(p_one, gr.double(), one, lr=LR, betas=BETAS, eps=EPS)
        dfc = 1.0 / (1.0 + torch.exp(-(pg_old - gr.double()).abs()))
        ssz64 = LR * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        m_terms = (b1 * m_old).abs() + ((1 - b1) * gr.double()).abs()
        upd_terms = ssz64 * dfc * m_terms / (one['exp_avg_sq'].sqrt() + EPS)
        if t > 1:
            ssz_wrong = LR * math.sqrt(1 - b2 ** (t - 1)) / (1 - b1 ** (t - 1))
            dist = ((ssz_wrong - ssz64) / ssz64 * (p_old - p_one)).abs()
            e[f'sens_step{t}_bias_correction_t-1'] = float((dist / (0.5 * _ulp(p_one.float()) + OPT * upd_terms)).max())
        del p_old, m_old, v_old, pg_old
        # (a) the whole buffer in one launch
        p_before = flat.data.clone()
        flat.grad.copy_(gr)
        opt.step()
        # (b) split at n_conv
        pb, mb, vb, gb = forms['b']
        for lo, hi in ((0, n_conv), (n_conv, n)):
            o = 4 * lo
            check(lib.hg_diffgrad_step(pb.data_ptr() + o, gr.data_ptr() + o, mb.data_ptr() + o, vb.data_ptr() + o,
                                       gb.data_ptr() + o, hi - lo, LR, b1, b2, EPS, t, st), 'hg_diffgrad_step')
        # (c) bucketed
        fc.grad.copy_(gr)
        red.waited = []
        opt_c.step_buckets(red)
        assert red.waited == list(range(len(red.ranges))) and red.finished == t
        # (d) device-resident step size
        pd_, md, vd, gd_ = forms['d']
        ssz.fill_(lib.hg_diffgrad_step_size(LR, b1, b2, t))
        check(lib.hg_diffgrad_step_dev(pd_.data_ptr(), gr.data_ptr(), md.data_ptr(), vd.data_ptr(), gd_.data_ptr(), n,
                                       ssz.data_ptr(), b1, b2, EPS, st), 'hg_diffgrad_step_dev')
        ref_state = (flat.data, opt.exp_avg, opt.exp_avg_sq, opt.previous_grad)
        for k, got in (('b', forms['b']), ('c', (fc.data, opt_c.exp_avg, opt_c.exp_avg_sq, opt_c.previous_grad)),
                       ('d', forms['d'])):
            assert all(torch.equal(a, r) for a, r in zip(got, ref_state)), (k, t)
        # the step against the fp64 oracle from the same state
        bound = 0.5 * _ulp(flat.data) + OPT * upd_terms
        e[f'step{t}_update'] = float(((flat.data.double() - p_one).abs() / bound).max())
        e[f'step{t}_m'] = _rel(opt.exp_avg, one['exp_avg'])
        e[f'step{t}_v'] = _rel(opt.exp_avg_sq, one['exp_avg_sq'])
        assert torch.equal(opt.previous_grad, gr)
        e[f'step{t}_moved'] = float((flat.data != p_before).double().mean())
        assert e[f'step{t}_moved'] >= 0.5, e
        del p_one, one, dfc, m_terms, upd_terms, bound, p_before
        # the fp64 run of the oracle from the start
        N.diffgrad_step(p64, gr.double(), t64, lr=LR, betas=BETAS, eps=EPS)
    e['run_p'] = _rel(flat.data, p64)
    e['run_m'] = _rel(opt.exp_avg, t64['exp_avg'])
    e['run_v'] = _rel(opt.exp_avg_sq, t64['exp_avg_sq'])
    # EMA over the same buffers
    ma = FlatParams([torch.nn.Parameter(torch.randn(n, generator=g, device=dev) * 0.05)], with_grad=False)
    ma0 = ma.data.double()
    ema_update(ma, flat, 0.995)
    e['ema'] = _rel(ma.data, ma0 * 0.995 + 0.005 * flat.data.double())
    e['n'], e['n_conv'] = n, n_conv
    _record(record_testsuite_property, f'diffgrad/{which}', e)
    for t in range(1, STEPS + 1):
        assert e[f'step{t}_update'] <= 1.0 and e[f'step{t}_m'] <= OPT and e[f'step{t}_v'] <= OPT, e
        if t > 1:
            assert e[f'sens_step{t}_bias_correction_t-1'] >= SENS, e
    assert e['run_p'] <= OPT and e['run_m'] <= OPT and e['run_v'] <= OPT and e['ema'] <= OPT, e
