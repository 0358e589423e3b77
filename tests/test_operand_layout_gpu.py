"""Generator / discriminator side kernels on the operands they really get: contiguous tensors that are only 4-byte aligned
(views into an optim.FlatParams buffer behind an odd-sized parameter), shapes off the power-of-two path, and non-contiguous or
non-fp32 inputs of the public ops.  tests/layout_ref.py has the per-launcher table these tests rest on.

A. every launcher: one aligned call, then each tensor operand shifted alone to data_ptr() % 16 == 4 and all operands shifted
   to 4, 8 and 12.  Every call meets the fp64 bar of the op's existing test (named at each test), and a shifted call gives the
   bits of the aligned one -- except where the HOST picks another kernel by alignment (only the fp64 bar there):
     hg_modulate_bwd   upsample, W even: k_modulate_bwd<2> needs gout, x, gx aligned, else <1>: gx is still the same bits
                       (tests/test_nets_gpu.py::test_upsample_adjoint_paths_agree), the chunked sum gs is not
     hg_noise_grad     H % 4 == 0: k_noise_grad<4> needs gconv aligned, else <1> (another split of the channel sum)
     hg_grouped_linear_*  refuse: ops.grouped_linear_supported is False for such a weight (per-layer path), x / gy are copied
   (the histogram's direct / lean and slab choices are alignment-selected too; its strided C ABI has its own tests).
B. the flat buffers the trainers build, behind a pad parameter of 0 ... 4 elements: same bits for every pad.
C. non-contiguous, fp64 and fp16 inputs of the public ops equal the call on t.float().contiguous().
"""
import collections
import copy
import json
import zlib

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import relmax

import layout_ref as LR
import noise_grad_ref as NR
import test_wino_route_gpu as WR

pytestmark = pytest.mark.gpu

WORST = collections.defaultdict(float)      # op/output -> largest relmax against fp64 over every call of this module
CALLS = collections.Counter()               # op -> calls made (aligned + shifted)


def _cpu_gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _bar(errs, name, got, ref, tol, what=''):
    e = relmax(got.detach().cpu().numpy(), ref.detach().cpu().numpy())
    errs[name] = max(errs.get(name, 0.0), e)
    assert tuple(got.shape) == tuple(ref.shape) and e <= tol, (what, name, e, tol)


def _variants(operands):
    """(tag, operands of the call, names shifted).  Every call gets copies of its own (slots are written)."""
    live = [n for n, t in operands.items() if t is not None]
    cp = lambda t: None if t is None else t.clone()
    yield 'aligned', {n: cp(t) for n, t in operands.items()}, frozenset()
    for m in live:
        yield m + '@4', {n: (LR.shifted(t, 1) if n == m else cp(t)) for n, t in operands.items()}, frozenset([m])
    for k in (1, 2, 3):
        yield 'all@%d' % (4 * k), {n: (None if t is None else LR.shifted(t, k)) for n, t in operands.items()}, frozenset(live)


def _sweep(op, operands, run, check, selected=None):
    """run(**operands) -> {output: tensor or None}; check(outputs) asserts the fp64 bars and returns {output: relmax};
    selected(names shifted) -> the outputs an alignment-selected kernel computes for that call (no bit comparison)."""
    base = None
    for tag, v, sh in _variants(operands):
        assert all(t is None or (t.is_contiguous() and (t.data_ptr() % 16 != 0) == (n in sh)) for n, t in v.items()), tag
        outs = run(**v)
        for name, e in check(outs).items():
            WORST[op + '/' + name] = max(WORST[op + '/' + name], e)
        CALLS[op] += 1
        if base is None:
            base = outs
            continue
        loose = set(selected(sh)) if selected else set()
        for name, t in outs.items():
            if t is not None and name not in loose:
                assert torch.equal(t, base[name]), '%s %s: %s differs from the aligned call' % (op, tag, name)


def _record(record_testsuite_property, prefix):
    val = {k: v for k, v in WORST.items() if k.startswith(prefix)}
    calls = {k: v for k, v in CALLS.items() if k.startswith(prefix)}
    print('operand_layout %s: calls %s worst %s' % (prefix, json.dumps(calls, sort_keys=True), json.dumps(val, sort_keys=True)))
    record_testsuite_property('operand_layout/' + prefix, json.dumps(dict(calls=calls, worst=val), sort_keys=True))


# ---- A. per-launcher operand sweep -------------------------------------------------------------------------------------
MOD = [((2, 5, 4, 4), False), ((2, 3, 2, 2), True), ((1, 2, 6, 6), True), ((2, 3, 5, 7), True)]


@pytest.mark.parametrize('shape,up', MOD)
def test_modulate_operands(shape, up, gpu_device, record_testsuite_property):
    """launch.modulate_fwd / modulate_bwd; bars of tests/test_nets_gpu.py::test_modulate_matches_torch (1e-6 / 1e-5)."""
    from histogan_amd import launch
    B, C, H, W = shape
    f = 2 if up else 1
    g = _cpu_gen('mod', shape, up)
    x, s, go = torch.randn(B, C, H, W, generator=g), 0.5 * torch.randn(B, C, generator=g), torch.randn(B, C, H * f, W * f, generator=g)
    r_out, r_gx, r_gs = LR.modulate_fp64(x, s, up, go)
    x, s, go = x.to(gpu_device), s.to(gpu_device), go.to(gpu_device)

    def chk_f(o):
        e = {}
        _bar(e, 'out', o['out'], r_out, 1e-6, shape)
        return e

    def chk_b(o):
        e = {}
        _bar(e, 'gx', o['gx'], r_gx, 1e-5, shape)
        _bar(e, 'gs', o['gs'], r_gs, 1e-5, shape)
        return e

    _sweep('modulate_fwd', dict(x=x, s=s), lambda x, s: dict(out=launch.modulate_fwd(x, s, up)), chk_f)
    _sweep('modulate_bwd', dict(g=go, x=x, s=s), lambda g, x, s: dict(zip(('gx', 'gs'), launch.modulate_bwd(g, x, s, up))), chk_b,
           selected=lambda sh: {'gs'} if up and W % 2 == 0 and sh & {'g', 'x'} else ())
    _record(record_testsuite_property, 'modulate')


# (B, O, H, S): the vector branch, a window inside a larger image, the scalar branch twice (H % 4 != 0), the vector branch of
# k_dnl_fwd with S % 4 != 0 twice (k_dnl_bwd takes its scalar branch there)
DNL = [(2, 6, 4, 4), (2, 5, 8, 16), (2, 3, 5, 6), (1, 4, 7, 7), (2, 6, 4, 6), (2, 3, 8, 10)]


@pytest.mark.parametrize('demod', [True, False], ids=['d', 'no_d'])
@pytest.mark.parametrize('B,O,H,S', DNL)
def test_demod_noise_lrelu_operands(B, O, H, S, demod, gpu_device, record_testsuite_property):
    """launch.dnl_fwd and dnl_bwd (conv given, and conv = None: recovered from out) against fp64 at the bars
    tests/test_nets_gpu.py::test_demod_noise_lrelu_matches_torch holds against fp32 torch: 1e-6 output, 1e-5 gradients."""
    from histogan_amd import launch
    g = _cpu_gen('dnl', B, O, H, S, demod)
    conv, nzt, go = torch.randn(B, O, H, H, generator=g), torch.rand(B, S, S, generator=g), torch.randn(B, O, H, H, generator=g)
    d = torch.rand(B, O, generator=g) + 0.5 if demod else None
    wn, bn = 0.5 * torch.randn(O, generator=g), 0.2 * torch.randn(O, generator=g)
    r_out = LR.dnl_fp64(conv, d, nzt, wn, bn)
    dev = gpu_device
    T = lambda t: None if t is None else t.to(dev)
    conv_, d_, nzt_, wn_, bn_, go_ = T(conv), T(d), T(nzt), T(wn), T(bn), T(go)

    def chk_f(o):
        e = {}
        _bar(e, 'out', o['out'], r_out, 1e-6, (B, O, H, S))
        return e

    _sweep('dnl_fwd', dict(conv=conv_, d=d_, nzt=nzt_, wn=wn_, bn=bn_),
           lambda conv, d, nzt, wn, bn: dict(out=launch.dnl_fwd(conv, d, nzt, wn, bn)), chk_f)
    out_ = launch.dnl_fwd(conv_, d_, nzt_, wn_, bn_)
    refs = LR.dnl_bwd_fp64(go, out_.cpu(), conv, d, nzt)

    def chk_b(o):
        e = {}
        for name, r in zip(('gconv', 'gd', 'gwn_part', 'gbn_part'), refs):
            if o[name] is not None:
                _bar(e, name, o[name], r, 1e-5, (B, O, H, S))
        return e

    names = ('gconv', 'gd', 'gwn_part', 'gbn_part')
    for with_conv in (True, False):
        ops_ = dict(g=go_, out=out_, conv=conv_ if with_conv else None, d=d_, nzt=nzt_, wn=None if with_conv else wn_,
                    bn=None if with_conv else bn_)
        _sweep('dnl_bwd' + ('' if with_conv else '_recovered'), ops_,
               lambda g, out, conv, d, nzt, wn, bn: dict(zip(names, launch.dnl_bwd(g, out, conv, d, nzt, wn, bn))), chk_b)
    _record(record_testsuite_property, 'dnl')


@pytest.mark.parametrize('B,O,H,S', DNL)
def test_noise_grad_operands(B, O, H, S, gpu_device, record_testsuite_property):
    """launch.noise_grad, overwrite and accumulate, at TOL = 2e-5 of tests/test_noise_grad_gpu.py.  The launcher has no route
    query: its host condition ((H & 3) == 0 and gconv 16-byte aligned -> k_noise_grad<4>, else <1>) is restated here to say
    which calls must reproduce the aligned bits; with H % 4 == 0 a shifted gconv lands in k_noise_grad<1>, with H % 4 != 0
    every call does."""
    from histogan_amd import launch
    demod = O != 3
    gconv, d, wn = NR.noise_grad_inputs(B, O, H, demod, B * 1000 + O * 10 + H + S)
    want = NR.noise_grad_fp64(gconv, d, wn)
    old = torch.randn(B, S, S, generator=_cpu_gen('ng', B, S))
    dev = gpu_device
    outside = torch.ones(B, S, S, dtype=torch.bool)
    outside[:, :H, :H] = False
    for acc in (False, True):
        target = old[:, :H, :H].double() + want if acc else want

        def chk(o):
            e = {}
            buf = o['gnzt'].cpu()
            _bar(e, 'window', buf[:, :H, :H], target, 2e-5, (B, O, H, S, acc))
            assert torch.equal(buf[outside], old[outside]), 'noise_grad wrote outside its window'
            return e

        _sweep('noise_grad' + ('_acc' if acc else ''), dict(gconv=gconv.to(dev), d=None if d is None else d.to(dev), wn=wn.to(dev),
                                                              gnzt=old.to(dev)),
               lambda gconv, d, wn, gnzt: dict(gnzt=launch.noise_grad(gconv, d, wn, gnzt, acc)), chk,
               selected=lambda sh: {'gnzt'} if H % 4 == 0 and 'gconv' in sh else ())
    _record(record_testsuite_property, 'noise_grad')


@pytest.mark.parametrize('shape', [(3, 5, 4, 4), (7, 3, 5, 9)])
def test_channel_sums_operands(shape, gpu_device, record_testsuite_property):
    """launch.channel_sum and conv.lrelu_bwd_channel_sum (vector and scalar branch); bars of
    tests/test_nets_gpu.py::test_channel_sum_matches_torch and tests/test_conv_gpu.py::test_lrelu_bwd_channel_sum_matches_aten:
    sums 1e-6, the masked gradient equal to aten's."""
    from histogan_amd import launch
    from histogan_amd.conv import lrelu_bwd_channel_sum
    g = _cpu_gen('csum', shape)
    gr, out = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    out[0, 0, 0, 0] = 0.0
    r_sum = gr.double().sum(dim=(0, 2, 3))
    r_gm = torch.ops.aten.leaky_relu_backward(gr, out, 0.2, True)
    r_cs = r_gm.double().sum(dim=(0, 2, 3))

    def chk(o):
        e = {}
        _bar(e, 'sum', o['sum'], r_sum, 1e-6, shape)
        return e

    def chk2(o):
        e = {}
        assert torch.equal(o['gm'].cpu(), r_gm)
        _bar(e, 'csum', o['csum'], r_cs, 1e-6, shape)
        return e

    _sweep('channel_sum', dict(g=gr.to(gpu_device)), lambda g: dict(sum=launch.channel_sum(g)), chk)
    _sweep('lrelu_bwd_channel_sum', dict(g=gr.to(gpu_device), out=out.to(gpu_device)),
           lambda g, out: dict(zip(('gm', 'csum'), lrelu_bwd_channel_sum(g, out, 0.2))), chk2)
    _record(record_testsuite_property, 'channel_sum')
    _record(record_testsuite_property, 'lrelu_bwd')


def _torgb_bwd_into(g, x, s, w, gw):
    """hg_torgb_bwd with the weight gradient written where the caller says (launch.torgb_bwd allocates its own)."""
    from histogan_amd._lib import check, lib, stream_of, workspace
    B, O, H, W = x.shape
    C = w.shape[0]
    gx, gs = torch.empty_like(x), torch.empty_like(s)
    nb = lib.hg_torgb_bwd_workspace_bytes(B, O, C, H * W)
    ws = workspace(nb, x.device)
    check(lib.hg_torgb_bwd(g.data_ptr(), x.data_ptr(), s.data_ptr(), w.data_ptr(), gx.data_ptr(), gs.data_ptr(), gw.data_ptr(),
                           B, O, C, H * W, ws.data_ptr(), nb, stream_of(x)), 'hg_torgb_bwd')
    return gx, gs, gw


@pytest.mark.parametrize('B,O,C,S,with_prev', [(2, 32, 3, 4, True), (5, 40, 4, 8, False)])
def test_torgb_operands(B, O, C, S, with_prev, gpu_device, record_testsuite_property):
    """launch.torgb_fwd / hg_torgb_bwd with gw written into a shifted slot; bars of
    tests/test_nets_gpu.py::test_torgb_matches_fp64: 2e-6 output, 5e-6 gradients."""
    from histogan_amd import launch
    g = _cpu_gen('torgb', B, O, C, S)
    x, st = torch.randn(B, O, S, S, generator=g), 0.4 * torch.randn(B, O, generator=g)
    w = torch.randn(C, O, generator=g) / O ** 0.5
    prev = torch.randn(B, C, S, S, generator=g) if with_prev else None
    go = torch.randn(B, C, S, S, generator=g)
    r_out, r_gx, r_gs, r_gw = LR.torgb_fp64(x, st, w, prev, go)
    dev = gpu_device
    T = lambda t: None if t is None else t.to(dev)

    def chk_f(o):
        e = {}
        _bar(e, 'out', o['out'], r_out, 2e-6, (B, O, C, S))
        return e

    def chk_b(o):
        e = {}
        for name, r in (('gx', r_gx), ('gs', r_gs), ('gw', r_gw)):
            _bar(e, name, o[name], r, 5e-6, (B, O, C, S))
        return e

    _sweep('torgb_fwd', dict(x=T(x), s=T(st), w=T(w), prev=T(prev)),
           lambda x, s, w, prev: dict(out=launch.torgb_fwd(x, s, w, prev)), chk_f)
    slot = torch.randn(C, O, generator=g)          # (finite: the kernel must overwrite every element of it)
    _sweep('torgb_bwd', dict(g=T(go), x=T(x), s=T(st), w=T(w), gw=T(slot)),
           lambda g, x, s, w, gw: dict(zip(('gx', 'gs', 'gw'), _torgb_bwd_into(g, x, s, w, gw))), chk_b)
    _record(record_testsuite_property, 'torgb')


# one case per `up` of tests/test_gstage_gpu.py::CASES at H <= 16; its to-RGB-only cases start at H = 32, so that one is CASES'
# (2, 16, 32, 32, None, True) at H = S = 16
GSTAGE = [(2, 8, 4, 16, True, True), (2, 7, 16, 32, False, True), (2, 16, 16, 16, None, True)]


@pytest.mark.parametrize('B,Cc,H,S,up,rgb', GSTAGE)
def test_gstage_operands(B, Cc, H, S, up, rgb, gpu_device, record_testsuite_property):
    """launch.gstage_bwd with gw_rgb_out a shifted slot; the 2e-5 of tests/test_gstage_gpu.py."""
    from gstage_ref import gstage_fp64, gstage_inputs
    from histogan_amd import launch
    g = torch.Generator().manual_seed(B * 1000 + Cc * 10 + H)
    inp = gstage_inputs(B, Cc, H, S, up, rgb, g)
    out, want = gstage_fp64(inp, up, rgb)
    has_a = up is not None
    dev = gpu_device
    T = lambda t: None if t is None else t.detach().float().to(dev).contiguous()
    ops_ = dict(out=T(out), ga=T(inp['ga']), sa=T(inp['sa']) if has_a else None, g_rgb=T(inp['g_rgb']), w_rgb=T(inp['w']),
                s_rgb=T(inp['srgb']), d=T(inp['d']), nzt=T(inp['nzt']), wn=T(inp['wn']), bn=T(inp['bn']),
                slot=torch.randn(3, Cc, generator=g).to(dev))
    names = ('gconv', 'gs_a', 'gs_rgb', 'gw_rgb', 'gd', 'gwn', 'gbn')
    refs = dict(gconv=want[0], gd=want[1], gwn=want[2], gbn=want[3], gs_a=want[4], gs_rgb=want[5], gw_rgb=want[6])

    def run(out, ga, sa, g_rgb, w_rgb, s_rgb, d, nzt, wn, bn, slot):
        res = dict(zip(names, launch.gstage_bwd(out, ga, sa, up, g_rgb, w_rgb, s_rgb, d, nzt, wn, bn, gw_rgb_out=slot)))
        assert res['gw_rgb'].data_ptr() == slot.data_ptr()
        return res

    def chk(o):
        e = {}
        for name in names:
            if o[name] is not None:
                _bar(e, name, o[name], refs[name], 2e-5, (B, Cc, H, S, up))
        return e

    _sweep('gstage_bwd', ops_, run, chk)
    _record(record_testsuite_property, 'gstage')


@pytest.mark.parametrize('B,N,K', [(4, 5, 3), (32, 64, 48)])
def test_demod_terms_operands(B, N, K, gpu_device, record_testsuite_property):
    """launch.demod_style_grad and hg_demod_weight_term (k = 3) writing / accumulating into a shifted slot; the 2e-6 of
    tests/test_conv_gpu.py::test_demod_weight_term_kernel_matches_fp64 and ::test_demod_style_grad_kernel_matches_fp64.
    K taps = 27: the scalar branch of k_demod_weight_term; 432: its 16-byte branch."""
    from histogan_amd import launch
    from histogan_amd._lib import check, lib, raw_stream
    g = _cpu_gen('demod', B, N, K)
    w = torch.randn(N, K, 3, 3, generator=g) / (K * 9) ** 0.5
    s1 = torch.randn(B, K, generator=g) * 0.5 + 1.0
    gd = torch.randn(B, N, generator=g)
    wsq = w.pow(2).sum(dim=(2, 3))
    d = torch.rsqrt((s1 * s1) @ wsq.t() + 1e-8)
    prior = torch.randn(N, K, 3, 3, generator=g)
    r_gy, r_gw = LR.demod_terms_fp64(w, gd, d, s1)
    r_gy = 2.0 * s1.double() * ((gd.double() * (-0.5) * d.double() ** 3) @ wsq.double())     # (on the fp32 wsq the kernel reads)
    dev = gpu_device

    def chk_s(o):
        e = {}
        _bar(e, 'gy', o['gy'], r_gy, 2e-6, (B, N, K))
        return e

    _sweep('demod_style_grad', dict(gd=gd.to(dev), d=d.to(dev), s1=s1.to(dev), wsq=wsq.to(dev)),
           lambda gd, d, s1, wsq: dict(gy=launch.demod_style_grad(gd, d, s1, wsq)), chk_s)
    for acc in (0, 1):
        target = r_gw + prior.double() if acc else r_gw

        def run(w, gd, d, s1, gw):
            check(lib.hg_demod_weight_term(w.data_ptr(), gd.data_ptr(), d.data_ptr(), s1.data_ptr(), gw.data_ptr(), B, N, K, 9, acc,
                                           raw_stream(dev)), 'hg_demod_weight_term')
            return dict(gw=gw)

        def chk_w(o):
            e = {}
            _bar(e, 'gw', o['gw'], target, 2e-6, (B, N, K, acc))
            return e

        _sweep('demod_weight_term' + ('_acc' if acc else ''), dict(w=w.to(dev), gd=gd.to(dev), d=d.to(dev), s1=s1.to(dev), gw=prior.to(dev)),
               run, chk_w)
    _record(record_testsuite_property, 'demod')


# One smallest case per route of tests/test_conv_route_gpu.py::CASES (the direct 3x3, stride 2 forward, the one-launch and the
# per-class stride-2 data gradient, 1x1, the K split of the 64 x 64 tile with its reduce, weight gradients with one slab and with
# several), straight through the C ABI as there: the Python dispatch would send the 3x3 stride-1 shapes it likes to hg_wino.
def _conv_cases():
    from test_conv_route_gpu import CASES, Case
    pick = [Case(2, 5, 7, 11, 13, 3, 1, False), Case(2, 5, 7, 11, 13, 3, 1, True), Case(2, 5, 7, 11, 13, 1, 1, False),
            Case(2, 5, 7, 21, 23, 3, 2, False), Case(2, 64, 70, 3, 3, 3, 1, False), Case(2, 64, 70, 3, 3, 1, 1, False),
            Case(2, 7, 5, 11, 13, 3, 1, False, 'dgrad'), Case(2, 5, 7, 5, 7, 3, 2, False, 'dgrad'),
            Case(3, 128, 70, 4, 6, 3, 2, False, 'dgrad'), Case(2, 5, 7, 1, 9, 3, 2, False, 'dgrad'),
            Case(2, 5, 7, 11, 13, 3, 1, False, 'wgrad'), Case(1, 5, 7, 3, 2, 1, 1, False, 'wgrad'),
            Case(2, 40, 20, 9, 11, 3, 1, True, 'wgrad'), Case(1, 68, 100, 8, 8, 3, 1, False, 'wgrad'),
            Case(2, 20, 24, 9, 13, 3, 2, False, 'wgrad')]
    by_key = {c[:10]: c for c in CASES}
    return [by_key[p[:10]] for p in pick]


def _conv_raw(c, x, gout, w, iscale, oscale, bias, out):
    """The case's C-ABI call as tests/test_conv_route_gpu.py::run_case makes it, on the caller's operands and output."""
    from histogan_amd._lib import check, lib, ptr, raw_stream
    from test_conv_route_gpu import _ws_bytes
    dev = w.device if w is not None else x.device
    st = raw_stream(dev)
    nb = _ws_bytes(c)
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
    if c.op == 'wgrad':
        check(lib.hg_conv2d_wgrad(x.data_ptr(), gout.data_ptr(), out.data_ptr(), ptr(iscale), ptr(oscale), c.B, c.K, c.N, c.H, c.W,
                                  c.ksize, c.stride, ws.data_ptr(), nb, st), 'hg_conv2d_wgrad')
        return out
    Co, Ci, mode = (c.K, c.N, 1) if c.op == 'dgrad' else (c.N, c.K, 0)
    wt = torch.empty(lib.hg_conv_packed_elems(Co, Ci, c.ksize, mode), device=dev)
    check(lib.hg_conv_pack_weights(w.data_ptr(), wt.data_ptr(), Co, Ci, c.ksize, mode, st), 'hg_conv_pack_weights')
    if c.op == 'dgrad':
        check(lib.hg_conv2d_dgrad(gout.data_ptr(), wt.data_ptr(), out.data_ptr(), ptr(iscale), ptr(oscale), c.B, c.K, c.N, c.H, c.W,
                                  c.ksize, c.stride, ws.data_ptr(), nb, st), 'hg_conv2d_dgrad')
    else:
        check(lib.hg_conv2d_fwd(x.data_ptr(), wt.data_ptr(), out.data_ptr(), ptr(iscale), ptr(oscale), ptr(bias), c.B, c.K, c.N,
                                c.H, c.W, c.ksize, c.stride, ws.data_ptr(), nb, st), 'hg_conv2d_fwd')
    return out


@pytest.mark.parametrize('i', range(15))
def test_conv_operands(i, gpu_device, record_testsuite_property):
    """hg_conv_pack_weights + hg_conv2d_fwd (with a bias) / _dgrad / _wgrad on shifted input, weight, scales, bias and OUTPUT (a
    flat gradient slot for the weight gradient); the route asserted as in tests/test_conv_route_gpu.py, whose bars these are:
    2e-6 output and data gradient, 5e-6 weight gradient."""
    from histogan_amd import _lib as L
    import test_conv_route_gpu as CR
    cases = _conv_cases()
    assert len(cases) == 15
    c = cases[i]
    if c.op == 'wgrad':
        assert CR.wgrad_splits(c) == c.route
    else:
        r = L.conv_route(c.B, c.K, c.N, c.H, c.W, c.ksize, c.stride, dgrad=c.op == 'dgrad', fe=c.fe, workspace_bytes=CR._ws_bytes(c))
        assert (L.HG_CONV_KIND[r.kind], L.HG_CONV_TILE[r.tile], r.kchunk, r.ksplit) == c.route
    t = CR.make_inputs(c, gpu_device)
    ref = CR.reference(c, t)
    bias = None
    if c.op == 'fwd':
        bias = torch.randn(c.N, generator=_cpu_gen('bias', i)).to(gpu_device)
        ref = ref + bias.double()[None, :, None, None]
    name, tol = {'fwd': ('out', 2e-6), 'dgrad': ('gin', 2e-6), 'wgrad': ('gw', 5e-6)}[c.op]
    out0 = torch.randn(ref.shape, generator=_cpu_gen('out', i)).to(gpu_device)

    def chk(o):
        e = {}
        _bar(e, name, o[name], ref, tol, CR.case_id(c))
        return e

    _sweep('conv_' + c.op, dict(x=t.get('x'), gout=t['gout'] if c.op != 'fwd' else None, w=t['w'] if c.op != 'wgrad' else None,
                                iscale=t['iscale'], oscale=t['oscale'], bias=bias, out=out0),
           lambda **kw: {name: _conv_raw(c, **kw)}, chk)
    _record(record_testsuite_property, 'conv_' + c.op)


# Every plan branch of tests/test_wino_route_gpu.py's FWD (the full-workspace cases) and WG lists, on the forward operand; the
# data-gradient launches of that module are the same kernel on the flipped operand and stay there.
WINO_FWD = [tuple(c[:5]) for c in WR.FWD if c.ws == 'full']
WINO_WG = [tuple(c[:5]) for c in WR.WG]


def _wino_case(lst, key):
    return next(c for c in lst if tuple(c[:5]) == key and getattr(c, 'ws', 'full') == 'full')


@pytest.mark.parametrize('key', WINO_FWD, ids=lambda k: 'x'.join(map(str, k)))
def test_wino_forward_operands(key, gpu_device, record_testsuite_property):
    """hg_wino_pack_weights + hg_wino_conv2d with the generator epilogue (input / output scales, bias, noise image, LeakyReLU) and
    with bias + addend, every operand and the output shifted; route asserted and 2e-6 as in tests/test_wino_route_gpu.py."""
    from histogan_amd import _lib as L
    c = _wino_case(WR.FWD, key)
    B, K, N, H, W = key
    for fe in (0, 1):
        WR._assert_route(L.wino_route(B, K, N, H, W, fe=fe), c.want, H, W, 'fwd fe=%d' % fe)
    g = torch.Generator().manual_seed(B * 131 + K + 7 * N + H)
    dev = gpu_device
    x = torch.randn(B, K, H, W, generator=g)
    w = torch.randn(N, K, 3, 3, generator=g) / (K * 9) ** 0.5
    bias, isc, osc = torch.randn(N, generator=g), torch.randn(B, K, generator=g) * 0.3 + 1, torch.rand(B, N, generator=g) + 0.5
    S = max(H, W) + 2
    nimg, nw, ad = torch.randn(B, S, S, generator=g), torch.randn(N, generator=g), torch.randn(B, N, H, W, generator=g)
    D = lambda t: t.to(dev).double()                       # (the references on the GPU in fp64, as in that module)
    conv64 = lambda v: F.conv2d(v, D(w), padding=1)
    b64 = D(bias)[None, :, None, None]
    r_gen = F.leaky_relu(conv64(D(x) * D(isc)[:, :, None, None]) * D(osc)[:, :, None, None] + b64
                         + D(nw)[None, :, None, None] * D(nimg)[:, None, :H, :W], 0.2).cpu()
    r_add = (conv64(D(x)) + b64 + D(ad)).cpu()
    nb = L.lib.hg_wino_workspace_bytes(B, K, N, H, W)

    def run(x, w, out, iscale=None, oscale=None, bias=None, noise_w=None, noise_img=None, addend=None):
        u = WR._pack(w, 0)
        ws = torch.full((max(nb // 4, 4),), float('nan'), dtype=torch.float32, device=dev)
        p = WR._p
        L.check(L.lib.hg_wino_conv2d(x.data_ptr(), u.data_ptr(), out.data_ptr(), p(iscale), p(oscale), p(bias), p(noise_w), p(noise_img),
                                     S if noise_img is not None else 0, 0.2 if noise_img is not None else 0.0, p(addend), B, K, N, H, W,
                                     ws.data_ptr(), nb, L.raw_stream(dev)), 'hg_wino_conv2d')
        return dict(out=out)

    def chk(ref):
        def f(o):
            e = {}
            _bar(e, 'out', o['out'], ref, 2e-6, key)
            return e
        return f

    T = lambda t: t.to(dev)
    out0 = torch.randn(B, N, H, W, generator=g)
    _sweep('wino_generator', dict(x=T(x), w=T(w), out=T(out0), iscale=T(isc), oscale=T(osc), bias=T(bias), noise_w=T(nw), noise_img=T(nimg)),
           run, chk(r_gen))
    _sweep('wino_addend', dict(x=T(x), w=T(w), out=T(out0), bias=T(bias), addend=T(ad)), run, chk(r_add))
    _record(record_testsuite_property, 'wino_')


@pytest.mark.parametrize('key', WINO_WG, ids=lambda k: 'x'.join(map(str, k)))
def test_wino_wgrad_operands(key, gpu_device, record_testsuite_property):
    """hg_wino_wgrad into a shifted slot; route asserted and 4e-6 as in tests/test_wino_route_gpu.py."""
    from histogan_amd import _lib as L
    c = _wino_case(WR.WG, key)
    B, K, N, H, W = key
    WR._assert_route(L.wino_wgrad_route(B, K, N, H, W), c.want, H, W, 'wgrad')
    g = torch.Generator().manual_seed(B * 17 + K + 3 * N + H + 5 * W)
    x, go = torch.randn(B, K, H, W, generator=g), torch.randn(B, N, H, W, generator=g)
    dev = gpu_device
    ref = torch.nn.grad.conv2d_weight(x.to(dev).double(), (N, K, 3, 3), go.to(dev).double(), padding=1).cpu()
    nb = L.lib.hg_wino_wgrad_workspace_bytes(B, K, N, H, W)

    def run(x, go, gw):
        ws = torch.full((max(nb // 4, 4),), float('nan'), dtype=torch.float32, device=dev)
        L.check(L.lib.hg_wino_wgrad(x.data_ptr(), go.data_ptr(), gw.data_ptr(), B, K, N, H, W, ws.data_ptr(), nb, L.raw_stream(dev)),
                'hg_wino_wgrad')
        return dict(gw=gw)

    def chk(o):
        e = {}
        _bar(e, 'gw', o['gw'], ref, 4e-6, key)
        return e

    _sweep('wino_wgrad', dict(x=x.to(dev), go=go.to(dev), gw=torch.randn(N, K, 3, 3, generator=g).to(dev)), run, chk)
    _record(record_testsuite_property, 'wino_wgrad')


@pytest.mark.parametrize('k,stride,lrelu', [(3, 1, False), (3, 2, False), (1, 1, False), (3, 1, True)])
def test_conv2d_public_operands(k, stride, lrelu, gpu_device, record_testsuite_property):
    """conv.conv2d / conv2d_lrelu through autograd (whatever route the dispatch takes: it does not depend on addresses): shifted
    input, weight, bias and upstream gradient give the aligned call's output, data, weight and bias gradient bit for bit, at
    the bars of tests/test_conv_gpu.py (2e-6 output and data gradient, 5e-6 weight gradient; the bias gradient is
    hg_channel_sum / hg_lrelu_bwd_channel_sum: 1e-6)."""
    from histogan_amd import conv as C
    B, K, N, H, W = 2, 5, 7, 11, 13
    g = _cpu_gen('pub', k, stride, lrelu)
    x, w = torch.randn(B, K, H, W, generator=g), torch.randn(N, K, k, k, generator=g) / (K * k * k) ** 0.5
    b = torch.randn(N, generator=g)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(xd, wd, bd, stride=stride, padding=k // 2)
    if lrelu:
        y = F.leaky_relu(y, 0.2)
    go = torch.randn(y.shape, generator=g)
    rgx, rgw, rgb = torch.autograd.grad(y, (xd, wd, bd), go.double())
    dev = gpu_device

    def run(x, w, b, go):
        x, w, b = (t.requires_grad_(True) for t in (x, w, b))
        out = C.conv2d_lrelu(x, w, b, 0.2) if lrelu else C.conv2d(x, w, b, stride)
        gx, gw, gb = torch.autograd.grad(out, (x, w, b), go)
        return dict(out=out.detach(), gx=gx, gw=gw, gb=gb)

    def chk(o):
        e = {}
        _bar(e, 'out', o['out'], y.detach(), 2e-6)
        _bar(e, 'gx', o['gx'], rgx, 2e-6)
        _bar(e, 'gw', o['gw'], rgw, 5e-6)
        _bar(e, 'gb', o['gb'], rgb, 1e-6)
        return e

    _sweep('conv2d_public', dict(x=x.to(dev), w=w.to(dev), b=b.to(dev), go=go.to(dev)), run, chk)
    _record(record_testsuite_property, 'conv2d_public')


def test_grouped_linear_operands(gpu_device, record_testsuite_property):
    """ops.grouped_linear at (8, 64, [128, 4, 260], [0, 1, 1]) of tests/test_linear_gpu.py (2e-6): shifted inputs, biases and
    upstream gradients are served (the inputs and gradients by a copy) with the aligned call's bits; a shifted or strided
    weight is refused by grouped_linear_supported, which Generator.forward asks."""
    from histogan_amd import ops
    B, K, Ns, groups = 8, 64, [128, 4, 260], [0, 1, 1]
    g = _cpu_gen('glin')
    dev = gpu_device
    xs = [torch.randn(B, K, generator=g) for _ in range(2)]
    ws = [torch.randn(n, K, generator=g) / K ** 0.5 for n in Ns]
    bs = [torch.randn(n, generator=g) for n in Ns]
    gos = [torch.randn(B, n, generator=g) for n in Ns]
    xd, wd, bd = ([t.double().requires_grad_(True) for t in l] for l in (xs, ws, bs))
    yr = [F.linear(xd[gr], wd[i], bd[i]) for i, gr in enumerate(groups)]
    gr_ = torch.autograd.grad(yr, xd + wd + bd, [t.double() for t in gos])
    wg = [t.to(dev) for t in ws]
    assert ops.grouped_linear_supported([xs[0].to(dev)], wg)
    for k in (1, 2, 3):
        for i in range(3):
            bad = list(wg)
            bad[i] = LR.shifted(wg[i], k)
            assert not ops.grouped_linear_supported([xs[0].to(dev)], bad)
    for _, v in LR.layouts(wg[2]):
        assert not ops.grouped_linear_supported([xs[0].to(dev)], [wg[0], wg[1], v])
    names = ['y%d' % i for i in range(3)] + ['gx%d' % i for i in range(2)] + ['gw%d' % i for i in range(3)] + ['gb%d' % i for i in range(3)]

    def run(**kw):
        x = [kw['x%d' % i].requires_grad_(True) for i in range(2)]
        layers = []
        for i, n in enumerate(Ns):
            m = nn.Linear(K, n).to(dev)
            m.weight.data, m.bias.data = wg[i], kw['b%d' % i]
            layers.append(m)
        ys = ops.grouped_linear(x, layers, groups)
        grads = torch.autograd.grad(ys, x + [m.weight for m in layers] + [m.bias for m in layers], [kw['go%d' % i] for i in range(3)])
        return dict(zip(names, [y.detach() for y in ys] + list(grads)))

    def chk(o):
        e = {}
        for name, r in zip(names, [y.detach() for y in yr] + list(gr_)):
            _bar(e, name[:2], o[name], r, 2e-6, name)
        return e

    operands = {'x%d' % i: t.to(dev) for i, t in enumerate(xs)}
    operands.update({'b%d' % i: t.to(dev) for i, t in enumerate(bs)})
    operands.update({'go%d' % i: t.to(dev) for i, t in enumerate(gos)})
    _sweep('grouped_linear', operands, run, chk)
    _record(record_testsuite_property, 'grouped_linear')


@pytest.mark.parametrize('shape', [(3, 5, 7, 9), (2, 4, 8, 8), (1, 2, 15, 15)])
def test_reops_operands(shape, gpu_device, record_testsuite_property):
    """reops.instnorm_lrelu, stencil3 and gaussian_valid (15 x 15 where the map allows it, else 5 x 5), input and upstream
    gradient shifted; bars of tests/test_rehistogan_gpu.py: instance norm 2e-6 output and 2e-5 scale gradient, the two linear
    filters 1e-6."""
    from histogan_amd import reops
    g = _cpu_gen('reops', shape)
    dev = gpu_device
    x = torch.randn(shape, generator=g) * 3 + 5
    go = torch.randn(shape, generator=g)
    r_y, r_gx, scale = LR.instnorm_lrelu_fp64(x, go)

    def run_in(x, go):
        x = x.requires_grad_(True)
        y = reops.instnorm_lrelu(x)
        gx, = torch.autograd.grad(y, x, go)
        return dict(out=y.detach(), gx=gx)

    def chk_in(o):
        e = {}
        _bar(e, 'out', o['out'], r_y, 2e-6, shape)
        err = float((o['gx'].cpu().double() - r_gx).abs().max())
        e['gx_over_scale'] = err / scale
        assert err <= 2e-5 * scale, (shape, err, scale)
        return e

    _sweep('instnorm_lrelu', dict(x=x.to(dev), go=go.to(dev)), run_in, chk_in)

    taps = torch.randn(3, 3, generator=g)
    go1 = torch.randn(shape[0], 1, shape[2], shape[3], generator=g)
    r_sy, r_sgx = LR.stencil3_fp64(x, taps, go1)

    def run_st(x, go):
        x = x.requires_grad_(True)
        y = reops.stencil3(x, taps)
        gx, = torch.autograd.grad(y, x, go)
        return dict(out=y.detach(), gx=gx)

    def chk_lin(r_out, r_g):
        def f(o):
            e = {}
            _bar(e, 'out', o['out'], r_out, 1e-6, shape)
            _bar(e, 'gx', o['gx'], r_g, 1e-6, shape)
            return e
        return f

    _sweep('stencil3', dict(x=x.to(dev), go=go1.to(dev)), run_st, chk_lin(r_sy, r_sgx))

    ks = 15 if min(shape[2:]) >= 15 else 5
    k2 = torch.rand(ks, ks, generator=g) + 0.1
    k2 = k2 / k2.sum()
    gog = torch.randn(shape[0], shape[1], shape[2] - ks + 1, shape[3] - ks + 1, generator=g)
    r_gy, r_ggx = LR.gaussian_valid_fp64(x, k2, gog)

    def run_g(x, go, k):
        x = x.requires_grad_(True)
        y = reops.gaussian_valid(x, k)
        gx, = torch.autograd.grad(y, x, go)
        return dict(out=y.detach(), gx=gx)

    _sweep('gaussian_valid', dict(x=x.to(dev), go=gog.to(dev), k=k2.to(dev)), run_g, chk_lin(r_gy, r_ggx))
    for p in ('instnorm', 'stencil3', 'gaussian'):
        _record(record_testsuite_property, p)


@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (2, 4, 8, 8)])
def test_augment_operands(shape, gpu_device, record_testsuite_property):
    """hg_augment_spatial (forward and adjoint), hg_sample_mean and hg_augment_color with the image, the parameter table, the
    colour table and the upstream gradient shifted.  Bars of tests/test_augment_shapes_gpu.py: the spatial maps exact, colour
    2e-6 forward / 1e-5 adjoint, the mean 2e-6."""
    from histogan_amd import augment as A
    B, C, H, W = shape
    g = _cpu_gen('aug', shape)
    dev = gpu_device
    x, go = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    p = torch.tensor([[1, 2, 3, 1, -1, 1, 2, 0, 3], [0, H - 1, 1, -2, 2, 3, 2, 0, W - 1]], dtype=torch.int32)
    r_sp = LR.augment_spatial_fp64(x, p)
    # the adjoint of a 0/1 gather: <A x, go> = <x, A^T go>, built column by column from the forward map on an index image
    idx = torch.arange(x.numel(), dtype=torch.float64).reshape(shape) + 1
    src = LR.augment_spatial_fp64(idx, p).long() - 1                  # source element of every output element (-1: none)
    r_adj = torch.zeros(x.numel(), dtype=torch.float64)
    m = src.flatten() >= 0
    r_adj.index_add_(0, src.flatten()[m], go.double().flatten()[m])
    r_adj = r_adj.reshape(shape)

    def run_sp(x, p, go):
        x = x.requires_grad_(True)
        y = A._Spatial.apply(x, p, False)
        gx, = torch.autograd.grad(y, x, go)
        return dict(out=y.detach(), gx=gx)

    def chk_sp(o):
        assert torch.equal(o['out'].cpu().double(), r_sp) and torch.equal(o['gx'].cpu().double(), r_adj)
        return dict(out=0.0, gx=0.0)

    _sweep('augment_spatial', dict(x=x.to(dev), p=p.to(dev), go=go.to(dev)), run_sp, chk_sp)

    color = torch.stack([torch.rand(B, generator=g) - 0.5, torch.rand(B, generator=g) * 2, torch.rand(B, generator=g) + 0.5], dim=1)
    r_col = LR.augment_color_fp64(x, color)
    xd = x.double().requires_grad_(True)
    lin = color.clone()
    lin[:, 0] = 0
    r_cadj, = torch.autograd.grad(LR.augment_color_fp64(xd, lin), xd, go.double())
    r_mean = x.double().mean(dim=(1, 2, 3))

    def run_col(x, color, go):
        x = x.requires_grad_(True)
        y = A._Color.apply(x, color, False)
        gx, = torch.autograd.grad(y, x, go)
        return dict(out=y.detach(), gx=gx, mean=A._sample_mean(x.detach()))

    def chk_col(o):
        e = {}
        _bar(e, 'out', o['out'], r_col, 2e-6, shape)
        _bar(e, 'gx', o['gx'], r_cadj, 1e-5, shape)
        _bar(e, 'mean', o['mean'], r_mean, 2e-6, shape)
        return e

    _sweep('augment_color', dict(x=x.to(dev), color=color.to(dev), go=go.to(dev)), run_col, chk_col)
    _record(record_testsuite_property, 'augment')


@pytest.mark.parametrize('h', [32, 33])
def test_hellinger_operands(h, gpu_device, record_testsuite_property):
    """hist.hellinger_loss at one workgroup (n = 1024) and just beyond (n = 1089: two), histograms shifted; the bars of
    tests/test_hellinger_shapes_gpu.py: loss 1e-6 absolute, gradient 1e-5."""
    from histogan_amd.hist import hellinger_loss
    n = h * h
    assert min(max((n + 1023) // 1024, 1), 1024) == (1 if h == 32 else 2)
    g = _cpu_gen('hell', h)
    t, gen = (torch.rand(1, 1, h, h, generator=g) + 0.05 for _ in range(2))
    t, gen = t / t.sum(), gen / gen.sum()
    ref, gref = LR.hellinger_fp64(t, gen, 2.0)

    def run(t, gen):
        gen = gen.requires_grad_(True)
        loss = hellinger_loss(t, gen, 2.0)
        grad, = torch.autograd.grad(loss, gen)
        return dict(loss=loss.detach(), grad=grad)

    def chk(o):
        e = dict(loss_abs=abs(float(o['loss']) - ref))
        assert e['loss_abs'] <= 1e-6, e
        _bar(e, 'grad', o['grad'], gref, 1e-5, h)
        return e

    _sweep('hellinger', dict(t=t.to(gpu_device), gen=gen.to(gpu_device)), run, chk)
    _record(record_testsuite_property, 'hellinger')


# ---- B. the flat buffers the trainers build ----------------------------------------------------------------------------
PADS = (0, 1, 2, 3, 4)


def _flat_behind_pad(module, pad, dev):
    """The module's parameters re-homed as the trainers do it (FlatParams, DiffGrad, enable_pack_cache) behind a parameter of
    `pad` elements."""
    from histogan_amd.conv import enable_pack_cache
    from histogan_amd.optim import DiffGrad, FlatParams
    head = [nn.Parameter(torch.zeros(pad, device=dev))] if pad else []
    flat = FlatParams(head + list(module.parameters()))
    enable_pack_cache(list(module.parameters()))
    return flat, DiffGrad(flat, lr=2e-4, betas=(0.5, 0.9))


def _named_state(module, flat, outputs):
    """After backward: gather, then every parameter's slice of the flat gradient; one optimizer step; the parameters."""
    flat.gather()
    torch.cuda.synchronize()
    st = dict(outputs)
    for n, p in module.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == flat.grad.data_ptr() + (p.data_ptr() - flat.data.data_ptr())
        st['grad/' + n] = p.grad.detach().clone()
    return st


def _after_step(module, opt, st):
    opt.step()
    torch.cuda.synchronize()
    for n, p in module.named_parameters():
        st['param/' + n] = p.detach().clone()
    return st


def _differing(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


def _generator(dev):
    from histogan_amd.nets import Generator
    torch.manual_seed(11)
    G = Generator(32, 512, network_capacity=2)
    with torch.no_grad():
        for b in G.blocks:                      # (the reference initialises the noise projections to zero: make them count)
            for m in (b.to_noise1, b.to_noise2):
                m.weight.normal_(std=0.3)
                m.bias.normal_(std=0.1)
    return G.to(dev)


@pytest.fixture(scope='module')
def gen_setup(gpu_device):
    """One generator and one set of inputs for the pad sweeps (left unchanged: every run works on a deep copy)."""
    dev = gpu_device
    G0 = _generator(dev)
    g = _cpu_gen('gen_inputs')
    B, L, S = 2, G0.num_layers, 32
    styles = torch.randn(B, L - 2, 512, generator=g).to(dev)
    hists = torch.randn(B, 2, 512, generator=g).to(dev)
    noise = torch.rand(B, S, S, 1, generator=g).to(dev)
    gout = torch.randn(B, 3, S, S, generator=g).to(dev)
    with torch.no_grad():       # the projected styles, from the ALIGNED weights: the same tensors for every pad
        sty = torch.cat((styles.transpose(0, 1), hists.transpose(0, 1)), dim=0)
        t = [F.linear(sty[i], m.weight, m.bias) for i, b in enumerate(G0.blocks) for m in (b.to_style1, b.to_style2, b.to_rgb.to_style)]
    return dict(G0=G0, styles=styles, hists=hists, noise=noise, gout=gout, t=[u.clone() for u in t])


def _misaligned(module, suffixes):
    return [n for n, p in module.named_parameters() if n.endswith(suffixes) and p.data_ptr() % 16 != 0]


@pytest.mark.parametrize('mode', ['per_block', 'one_node'])
def test_generator_stages_are_the_same_bits_behind_any_pad(mode, gen_setup, gpu_device):
    """Generator(32, 512, network_capacity=2) in a flat buffer behind a pad of 0 ... 4 floats, training forward and plain backward
    after flat.zero_grad() (conv._direct_wgrad, direct_demod_weight_term and the one-node pass's to-RGB slot write fire), gather,
    one DiffGrad step: the image, the gradients of the projected styles, every parameter's slice of flat.grad and the stepped
    parameters are bit-identical for every pad (pad 4 is the aligned control).  The projected styles are inputs here -- the same
    tensors for every pad -- because a misaligned to_style weight takes the per-layer F.linear path (torch's GEMM), see
    test_generator_forward_behind_any_pad.  No alignment-selected kernel lies on this path: hg_modulate_bwd and hg_noise_grad only
    read activations and workspaces, which are fresh allocations."""
    from histogan_amd import gfused
    from histogan_amd.nets import _noise_t
    dev = gpu_device
    res = {}
    for pad in PADS:
        G = copy.deepcopy(gen_setup['G0'])
        flat, opt = _flat_behind_pad(G, pad, dev)
        if pad in (1, 2, 3):
            assert _misaligned(G, ('conv1.weight', 'conv2.weight')) and _misaligned(G, ('to_style1.weight', 'to_style.weight'))
            assert _misaligned(G, ('to_rgb.conv.weight',)) and _misaligned(G, ('to_noise1.weight', 'to_noise1.bias'))
        else:
            assert not _misaligned(G, ('.weight', '.bias', 'initial_block'))
        G.train()
        t = [u.clone().requires_grad_(True) for u in gen_setup['t']]
        noise = gen_setup['noise']
        flat.zero_grad()
        if mode == 'one_node':
            nzt = _noise_t(noise)
            assert gfused.supported(G, t, nzt)
            rgb = gfused.generator_train(G, t, nzt)
        else:
            x, rgb = G.initial_block.expand(noise.shape[0], -1, -1, -1), None
            for i, blk in enumerate(G.blocks):
                x, rgb = blk.forward_(x, rgb, t[3 * i], t[3 * i + 1], t[3 * i + 2], inoise=noise)
        rgb.backward(gen_setup['gout'])
        assert flat.written, 'no gradient was written straight into a flat slot'
        st = _named_state(G, flat, dict(rgb=rgb.detach().clone(), **{'gt%d' % i: u.grad.clone() for i, u in enumerate(t)}))
        res[pad] = _after_step(G, opt, st)
        assert all(bool(torch.isfinite(v).all()) for v in res[pad].values())
    for pad in PADS[1:]:
        assert _differing(res[0], res[pad]) == [], (mode, pad)


def _run_recorded(G, styles, hists, noise, fused):
    """G(styles, hists, noise) with the LeakyReLU branches of its stages recorded in forward order (as
    tests/test_noise_grad_gpu.py does for the same oracle comparison)."""
    from histogan_amd import gfused, ops
    masks, orig_dnl, orig_cdnl = [], ops.demod_noise_lrelu, ops.conv_dnl

    def recording(orig):
        def f(*a):
            out = orig(*a)
            masks.append(out.detach().cpu() > 0)
            return out
        return f

    ops.demod_noise_lrelu, ops.conv_dnl = recording(orig_dnl), recording(orig_cdnl)
    gfused.STAGE_OBSERVER = lambda out: masks.append(out.detach().cpu() > 0)
    gfused.GFUSED = fused
    try:
        rgb = G(styles, hists, noise)
    finally:
        ops.demod_noise_lrelu, ops.conv_dnl = orig_dnl, orig_cdnl
        gfused.STAGE_OBSERVER = None
        gfused.GFUSED = True
    assert len(masks) == 2 * len(G.blocks)
    return rgb, masks


@pytest.mark.parametrize('fused', [True, False], ids=['one_node', 'per_block'])
def test_generator_forward_behind_any_pad(fused, gen_setup, gpu_device, record_testsuite_property):
    """Generator.forward itself behind the same pads.  pad 0 meets the bars of
    tests/test_gstage_gpu.py::test_fused_generator_node_equals_per_block_autograd (1e-6 image, 2e-5 gradients) against
    oracle.histogan_nets in fp64 on the run's own LeakyReLU branches, so the bit-identity of the stage test cannot hold with all
    pads wrong together.  pad 4 repeats pad 0 bit for bit.  Behind pads 1 ... 3 the to_style weights are off a 16-byte boundary:
    hg_grouped_linear_* would refuse them, ops.grouped_linear_supported says so, and forward takes one F.linear per projection and
    the per-block path instead of raising -- another route, held to the route-versus-route bar of
    tests/test_linear_gpu.py::test_generator_with_grouped_projections_equals_per_layer_gemms (1e-5 image, 1e-4 gradients)."""
    from oracle import histogan_nets as N
    from oracle_step import LreluMasks
    dev = gpu_device
    res, worst = {}, {}
    for pad in PADS:
        G = copy.deepcopy(gen_setup['G0'])
        flat, opt = _flat_behind_pad(G, pad, dev)
        G.train()
        styles, hists = gen_setup['styles'].clone().requires_grad_(True), gen_setup['hists'].clone().requires_grad_(True)
        flat.zero_grad()
        rgb, masks = _run_recorded(G, styles, hists, gen_setup['noise'], fused)
        rgb.backward(gen_setup['gout'])
        res[pad] = _named_state(G, flat, dict(rgb=rgb.detach().clone(), g_styles=styles.grad.clone(), g_hists=hists.grad.clone()))
        if pad == 0:
            sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in G.state_dict().items()}
            s64, h64 = (v.detach().cpu().double().requires_grad_(True) for v in (styles, hists))
            with LreluMasks(masks) as lm:
                o = N.generator(sd, s64, h64, gen_setup['noise'].cpu().double(), G.num_layers)
            assert lm.k == len(masks) and lm.flips <= 1e-5 * lm.total and lm.flip_margin <= 2e-6, (lm.flips, lm.total, lm.flip_margin)
            names = list(sd)
            truth = torch.autograd.grad(o, [s64, h64] + [sd[n] for n in names], gen_setup['gout'].cpu().double())
            worst['rgb'] = relmax(res[0]['rgb'].cpu().numpy(), o.detach().numpy())
            worst['grads'] = {}
            for n, tr in zip(['g_styles', 'g_hists'] + ['grad/' + n for n in names], truth):
                worst['grads'][n] = relmax(res[0][n].cpu().numpy(), tr.numpy())
    print('generator pad 0 against fp64 (fused=%s): rgb %.2e, worst gradient %s' % (fused, worst['rgb'],
                                                                                  max(worst['grads'].items(), key=lambda kv: kv[1])))
    record_testsuite_property('operand_layout/generator_fp64/%s' % ('one_node' if fused else 'per_block'),
                              json.dumps(dict(rgb=worst['rgb'], grad=max(worst['grads'].values()))))
    assert worst['rgb'] <= 1e-6
    assert all(e <= 2e-5 for e in worst['grads'].values()), {n: e for n, e in worst['grads'].items() if e > 2e-5}
    assert _differing(res[0], res[4]) == []
    for pad in (1, 2, 3):
        for k, v in res[pad].items():
            e = relmax(v.cpu().numpy(), res[0][k].cpu().numpy())
            assert e <= (1e-5 if k == 'rgb' else 1e-4), (pad, k, e)


@pytest.mark.parametrize('attn', [(), (1,)], ids=['plain', 'attention'])
def test_discriminator_is_the_same_bits_behind_any_pad(attn, gpu_device):
    """Discriminator(32, 2), without and with attention (whose 1-element Rezero.g shifts everything behind it), behind a pad of
    0 ... 4 floats: forward, a plain backward after flat.zero_grad() (direct weight-gradient writes), gather, one DiffGrad step --
    logits, every slice of flat.grad and the stepped parameters are bit-identical for every pad."""
    from histogan_amd.nets import Discriminator, Rezero
    dev = gpu_device
    torch.manual_seed(13)
    D0 = Discriminator(32, 2, attn_layers=list(attn))
    with torch.no_grad():
        for m in D0.modules():
            if isinstance(m, Rezero):
                m.g.fill_(0.5)               # (zero as initialised: the attention branch would carry no gradient)
    D0 = D0.to(dev)
    g = _cpu_gen('disc', attn)
    x, gl = torch.randn(3, 3, 32, 32, generator=g).to(dev), torch.randn(3, generator=g).to(dev)
    res = {}
    for pad in PADS:
        D = copy.deepcopy(D0)
        flat, opt = _flat_behind_pad(D, pad, dev)
        if pad in (1, 2, 3) or attn:
            assert _misaligned(D, ('.weight',)) and _misaligned(D, ('.bias',))
        D.train()
        flat.zero_grad()
        logits, _ = D(x)
        logits.backward(gl)
        assert flat.written
        res[pad] = _after_step(D, opt, _named_state(D, flat, dict(logits=logits.detach().clone())))
        assert all(bool(torch.isfinite(v).all()) for v in res[pad].values())
    for pad in PADS[1:]:
        assert _differing(res[0], res[pad]) == [], (attn, pad)


def test_rehistogan_flat_order_gives_the_bits_of_the_aligned_order(gpu_device):
    """RecoloringEncoderDecoder + RecoloringGAN + HistVectorizer at image size 64 in the parameter order retrainer.recoloringGAN
    flattens them in (ED, G, H: the two 3-element conv_out_rgb biases put every RecoloringGAN weight 8 bytes off a 16-byte
    boundary) and re-homed with conv_first (every convolution weight in front, aligned): same recoloured image, same gradients,
    same parameters after a DiffGrad step.  network_capacity = 4, the smallest at which the premise holds: at 2 the 54-element
    first encoder weight already misaligns the conv_first order as well."""
    from histogan_amd.conv import enable_pack_cache
    from histogan_amd.nets import HistVectorizer
    from histogan_amd.optim import DiffGrad, FlatParams, conv_first
    from histogan_amd.renets import RecoloringEncoderDecoder, RecoloringGAN
    dev = gpu_device
    torch.manual_seed(17)
    size, cap, lat = 64, 4, 64
    mods0 = nn.ModuleDict(dict(ED=RecoloringEncoderDecoder(size, network_capacity=cap, hist=64, latent_dim=lat, style_depth=2),
                               G=RecoloringGAN(size, lat, cap), H=HistVectorizer(64, lat, 2)))
    with torch.no_grad():
        for b in mods0['G'].blocks:
            for m in (b.to_noise1, b.to_noise2):
                m.weight.normal_(std=0.3)
                m.bias.normal_(std=0.1)
    mods0 = mods0.to(dev)
    g = _cpu_gen('rehistogan')
    B = 2
    x = torch.rand(B, 3, size, size, generator=g).to(dev)
    hist = torch.rand(B, 3, 64, 64, generator=g)
    hist = (hist / hist.sum(dim=(1, 2, 3), keepdim=True)).to(dev)
    noise = torch.rand(B, size, size, 1, generator=g).to(dev)
    gout = torch.randn(B, 3, size, size, generator=g).to(dev)
    res = {}
    for order in ('retrainer', 'conv_first'):
        mods = copy.deepcopy(mods0)
        ED, G, H = mods['ED'], mods['G'], mods['H']
        learnable = list(ED.parameters()) + list(G.parameters()) + list(H.parameters())
        flat = FlatParams(learnable if order == 'retrainer' else conv_first(learnable))
        enable_pack_cache(list(ED.parameters()) + list(G.parameters()))
        opt = DiffGrad(flat, lr=2e-4, betas=(0.5, 0.9))
        convs = [p for p in G.parameters() if p.dim() == 4]
        if order == 'retrainer':
            assert all(p.data_ptr() % 16 == 8 for p in convs) and all(p.grad.data_ptr() % 16 == 8 for p in convs)
        else:
            assert all(p.data_ptr() % 16 == 0 for p in mods.parameters() if p.dim() == 4)
        mods.train()
        flat.zero_grad()
        hw = H(hist)
        latent, rgb = ED(x, hist)
        gen = G(latent, rgb, hw, noise)
        gen.backward(gout)
        assert flat.written
        res[order] = _after_step(mods, opt, _named_state(mods, flat, dict(gen=gen.detach().clone())))
        assert all(bool(torch.isfinite(v).all()) for v in res[order].values())
    assert _differing(res['retrainer'], res['conv_first']) == []


# ---- C. non-contiguous and non-fp32 inputs of the public ops ---------------------------------------------------------------
def _input_variants(t):
    """(tag, tensor the caller passes) for every layout of LR.layouts and the two other dtypes.  fp16 rounds: the tensor under
    test is made exactly representable in fp16 first (see _fp16_exact), so every variant carries the same values."""
    for name, v in LR.layouts(t):
        yield name, v
    yield 'fp64', t.double()
    yield 'fp16', t.half()


def _fp16_exact(t):
    return t.half().float()


def _check_inputs(op, args, fn, vary):
    """fn(*args) -> outputs (tuple of tensors) computed with autograd on the entries of `vary`: every variant of every such
    argument gives the outputs and the input gradients of the call on t.float().contiguous(), bit for bit, the gradients in
    the caller's shape and dtype."""
    def call(a):
        a = [t.detach().requires_grad_(True) if i in vary else t for i, t in enumerate(a)]
        outs = fn(*a)
        outs = outs if isinstance(outs, (tuple, list)) else (outs,)
        gos = [torch.ones_like(o) * 0.5 for o in outs]
        grads = torch.autograd.grad(outs, [a[i] for i in vary], gos, allow_unused=True)
        return [o.detach() for o in outs], dict(zip(vary, grads)), a

    base_o, base_g, _ = call(args)
    n = 0
    for i in vary:
        for tag, v in _input_variants(args[i]):
            a = list(args)
            a[i] = v
            o, gr, used = call(a)
            for x, y in zip(o, base_o):
                assert x.dtype == torch.float32 and torch.equal(x, y), (op, i, tag, 'output')
            for j in vary:
                if base_g[j] is None:
                    assert gr[j] is None
                    continue
                assert gr[j].shape == used[j].shape and gr[j].dtype == used[j].dtype, (op, i, tag, j, 'gradient shape / dtype')
                if gr[j].dtype == torch.float16:
                    assert torch.equal(gr[j], base_g[j].half()), (op, i, tag, j, 'gradient')
                else:
                    assert torch.equal(gr[j].float(), base_g[j]), (op, i, tag, j, 'gradient')
            n += 1
    CALLS['inputs/' + op] += n
    return n


def test_public_ops_copy_every_strided_or_typed_input(gpu_device, record_testsuite_property):
    """ops.modulate, upsample2x, demod_noise_lrelu, torgb, conv_dnl, modconv_stage, grouped_linear, conv.conv2d, the three reops
    functions and hist.hellinger_loss on channels-last, every-other-column and batch-expanded views and on fp64 / fp16 tensors, one
    operand at a time: the result equals the call on t.float().contiguous() bit for bit (f32c reaches every operand) and the
    gradients come back in the caller's shape and dtype."""
    from histogan_amd import conv as C, ops, reops
    from histogan_amd.hist import hellinger_loss
    dev = gpu_device
    g = _cpu_gen('inputs')
    B, K, N, H, S = 2, 8, 12, 4, 8
    R = lambda *s: _fp16_exact(torch.randn(*s, generator=g)).to(dev)
    rep = lambda t: t[:1].repeat(B, *([1] * (t.dim() - 1)))      # equal batch entries: the stride-0 view exists
    x, s = rep(R(B, K, H, H)), R(B, K) * 0.5
    n = _check_inputs('modulate', [x, s], lambda x, s: ops.modulate(x, s, False), [0, 1])
    n += _check_inputs('modulate_up', [x, s], lambda x, s: ops.modulate(x, s, True), [0, 1])
    n += _check_inputs('upsample2x', [x], ops.upsample2x, [0])
    conv, d, nzt = rep(R(B, N, H, H)), _fp16_exact(torch.rand(B, N, generator=g) + 0.5).to(dev), rep(_fp16_exact(torch.rand(B, S, S, generator=g)).to(dev))
    wn, bn = R(N, 1) * 0.5, R(N) * 0.25
    n += _check_inputs('demod_noise_lrelu', [conv, d, nzt, wn, bn], ops.demod_noise_lrelu, [0, 1, 2, 3, 4])
    xr, st, wr, prev = rep(R(B, N, H, H)), R(B, N) * 0.5, R(3, N, 1, 1) * 0.25, rep(R(B, 3, H, H))
    n += _check_inputs('torgb', [xr, st, wr, prev], ops.torgb, [0, 1, 2, 3])
    w = R(N, K, 3, 3) * 0.125
    n += _check_inputs('conv_dnl', [x, w, d, nzt, wn, bn], ops.conv_dnl, [0, 1, 2, 3, 4, 5])
    n += _check_inputs('modconv_stage', [x, s, w, nzt, wn, bn], lambda *a: ops.modconv_stage(*a, demod=True, upsample=False, act=True),
                       [0, 1, 2, 3, 4, 5])
    b = R(N)
    n += _check_inputs('conv2d', [x, w, b], lambda x, w, b: C.conv2d(x, w, b, 1), [0, 1, 2])
    xi = _fp16_exact(rep(R(B, 3, 8, 8)) * 2 + 3)
    n += _check_inputs('instnorm_lrelu', [xi], reops.instnorm_lrelu, [0])
    n += _check_inputs('stencil3', [xi], lambda t: reops.stencil3(t, (1., 2., 1., 0., 0.5, 0., -1., -2., -1.)), [0])
    k2 = _fp16_exact(torch.rand(5, 5, generator=g) + 0.1).to(dev)
    n += _check_inputs('gaussian_valid', [xi], lambda t: reops.gaussian_valid(t, k2), [0])
    th, gh = (rep(_fp16_exact(torch.rand(B, 3, 8, 8, generator=g) + 0.05).to(dev)) for _ in range(2))
    n += _check_inputs('hellinger', [th, gh], lambda t, q: hellinger_loss(t, q, 2.0), [1])
    # hellinger's target gets no gradient but is an operand like the other: its layouts through the loss value
    base = hellinger_loss(th, gh, 2.0)
    for tag, v in _input_variants(th):
        assert torch.equal(hellinger_loss(v, gh, 2.0), base), tag
        n += 1
    # grouped linear: the inputs in any layout or dtype (copied and realigned); the weights are the module's own parameters
    layers = [nn.Linear(64, m).to(dev) for m in (128, 4, 260)]
    xs = [rep(R(8, 64)), rep(R(8, 64))]
    assert ops.grouped_linear_supported(xs, [m.weight for m in layers])
    n += _check_inputs('grouped_linear', xs, lambda a, c: tuple(ops.grouped_linear([a, c], layers, [0, 1, 1])), [0, 1])
    print('operand_layout inputs: %d calls on a strided or typed operand' % n)
    record_testsuite_property('operand_layout/inputs', json.dumps(dict(calls=n)))
