"""One case per route the convolution host side (hg_conv.hip make_conv_route / make_wgrad_plan) can take, each at the smallest
shape that reaches it on a 256-CU chip, straight through the C ABI (the Python dispatch would send many of them to the Winograd
kernels).  Every case first asserts that hg_conv2d_route still answers the route it was chosen for -- a planning change shows
up as that assertion, not as a silently untested kernel -- and then compares the result with F.conv2d / its autograd in fp64
at the tolerances of tests/test_conv_gpu.py (output and data gradient 2e-6, weight gradient 5e-6, max-norm relative).

tools/conv_route_check.py gpu runs the same list (run_case) in a tree and records launches and result hashes."""
import collections

import pytest
import torch
import torch.nn.functional as F

from conftest import relmax

# op: 'fwd' (hg_conv2d_fwd), 'dgrad' (hg_conv2d_dgrad), 'wgrad' (hg_conv2d_wgrad); B, K, N, H, W, ksize, stride as that call
# takes them (dgrad: K = the convolution's output channels, N = its input channels, H x W = its input).  fe: with input and
# output scales.  ws: 'full' = the workspace the query asks for, 'short' = one byte less, 'none' = NULL.
# route: (kind, tile, kchunk, ksplit) expected of hg_conv2d_route; wgrad cases: the expected number of splits.
Case = collections.namedtuple('Case', 'B K N H W ksize stride fe op ws route', defaults=('fwd', 'full', None))

S, P4, PC = 'SINGLE', 'PARITY4', 'PER_CLASS'
CASES = [
    # the six tiles, 3x3 stride 1, plain: odd sizes, more than one block; the 2-channel K chunks of the 32 / 64 / 128-channel tiles
    # (1024 blocks: whole rounds at 4 per CU) and the 4-channel chunks of the latter two; the K split of the 128 x 128 tile
    Case(2, 5, 7, 11, 13, 3, 1, False, route=(S, '16x256', 4, 1)),
    Case(2, 5, 20, 11, 13, 3, 1, False, route=(S, '32x256', 2, 1)),
    Case(3, 4, 40, 192, 192, 3, 1, False, route=(S, '64x256', 4, 1)),
    Case(4, 4, 40, 256, 256, 3, 1, False, route=(S, '64x256', 2, 1)),
    Case(1, 4, 136, 128, 128, 3, 1, False, route=(S, '128x128', 4, 1)),
    Case(1, 4, 136, 256, 256, 3, 1, False, route=(S, '128x128', 2, 1)),
    Case(3, 128, 136, 24, 27, 3, 1, False, route=(S, '128x128', 4, 4)),
    Case(64, 128, 512, 4, 4, 3, 1, False, route=(S, '128x128_SM', 4, 4)),
    Case(3, 5, 7, 5, 6, 3, 1, False, route=(S, '64x64', 8, 1)),
    Case(2, 64, 70, 3, 3, 3, 1, False, route=(S, '64x64', 8, 2)),
    # the same with input / output scales: the two larger tiles keep the 4-channel chunks
    Case(2, 5, 7, 11, 13, 3, 1, True, route=(S, '16x256', 4, 1)),
    Case(2, 5, 20, 11, 13, 3, 1, True, route=(S, '32x256', 2, 1)),
    Case(4, 4, 40, 256, 256, 3, 1, True, route=(S, '64x256', 4, 1)),
    Case(1, 4, 136, 256, 256, 3, 1, True, route=(S, '128x128', 4, 1)),
    Case(3, 128, 136, 24, 27, 3, 1, True, route=(S, '128x128', 4, 4)),
    Case(2, 64, 70, 3, 3, 3, 1, True, route=(S, '64x64', 8, 2)),
    # 1x1
    Case(2, 5, 7, 11, 13, 1, 1, False, route=(S, '16x256', 4, 1)),
    Case(2, 5, 20, 11, 13, 1, 1, True, route=(S, '32x256', 4, 1)),
    Case(3, 4, 40, 192, 192, 1, 1, False, route=(S, '64x256', 4, 1)),
    Case(1, 4, 136, 128, 128, 1, 1, False, route=(S, '128x128', 4, 1)),
    Case(3, 256, 256, 24, 27, 1, 1, False, route=(S, '128x128', 4, 4)),
    Case(64, 128, 512, 4, 4, 1, 1, False, route=(S, '128x128_SM', 4, 4)),
    Case(3, 5, 7, 5, 6, 1, 1, True, route=(S, '64x64', 8, 1)),
    Case(2, 64, 70, 3, 3, 1, 1, False, route=(S, '64x64', 8, 2)),
    # stride-2 forward
    Case(2, 5, 7, 21, 23, 3, 2, False, route=(S, '16x256', 4, 1)),
    Case(2, 5, 20, 21, 23, 3, 2, True, route=(S, '32x256', 4, 1)),
    Case(1, 4, 136, 256, 256, 3, 2, False, route=(S, '128x128', 4, 1)),
    Case(3, 5, 7, 9, 13, 3, 2, False, route=(S, '64x64', 8, 1)),
    Case(2, 64, 70, 5, 6, 3, 2, False, route=(S, '64x64', 8, 2)),
    Case(8, 40, 72, 4, 4, 3, 2, True, route=(S, '64x64', 8, 1)),
    # stride-1 data gradient (the forward kernels on the flipped operand)
    Case(2, 7, 5, 11, 13, 3, 1, False, 'dgrad', route=(S, '16x256', 4, 1)),
    Case(3, 128, 136, 24, 27, 3, 1, True, 'dgrad', route=(S, '128x128', 4, 4)),
    Case(2, 70, 64, 3, 3, 1, 1, False, 'dgrad', route=(S, '64x64', 8, 2)),
    # stride-2 data gradient in one launch, small maps (64 x 64 tile): without and with the K split (half the split planned per
    # class), with scales; one byte of workspace too few, and none: no split
    Case(2, 5, 7, 5, 7, 3, 2, False, 'dgrad', route=(P4, '64x64', 8, 1)),
    Case(3, 128, 70, 4, 6, 3, 2, False, 'dgrad', route=(P4, '64x64', 8, 2)),
    Case(3, 256, 70, 4, 6, 3, 2, True, 'dgrad', route=(P4, '64x64', 8, 4)),
    Case(3, 256, 70, 4, 6, 3, 2, False, 'dgrad', 'short', route=(P4, '64x64', 8, 1)),
    Case(3, 256, 70, 4, 6, 3, 2, False, 'dgrad', 'none', route=(P4, '64x64', 8, 1)),
    # ... large maps (the tile planned for the smallest class, XCD-paired block order from 64 pixel tiles per class on)
    Case(2, 5, 7, 21, 23, 3, 2, False, 'dgrad', route=(P4, '16x256', 4, 1)),
    Case(2, 5, 20, 21, 23, 3, 2, False, 'dgrad', route=(P4, '32x256', 4, 1)),
    Case(8, 4, 40, 255, 257, 3, 2, False, 'dgrad', route=(P4, '64x256', 4, 1)),
    Case(1, 4, 136, 259, 261, 3, 2, False, 'dgrad', route=(P4, '128x128', 4, 1)),
    Case(2, 5, 7, 255, 257, 3, 2, False, 'dgrad', route=(P4, '16x256', 4, 1)),
    # ... one launch per class: 1 x N and N x 1 images (empty classes), classes on either side of a tile rule, large maps with scales
    Case(2, 5, 7, 1, 9, 3, 2, False, 'dgrad', route=(PC, '64x64', 8, 1)),
    Case(2, 5, 7, 9, 1, 3, 2, True, 'dgrad', route=(PC, '64x64', 8, 1)),
    Case(1, 3, 2, 1, 1, 3, 2, False, 'dgrad', route=(PC, '64x64', 8, 1)),
    Case(2, 5, 7, 17, 17, 3, 2, False, 'dgrad', route=(PC, '16x256', 4, 1)),
    Case(1, 4, 136, 255, 257, 3, 2, False, 'dgrad', route=(PC, '128x128', 4, 1)),
    Case(2, 5, 20, 21, 23, 3, 2, True, 'dgrad', route=(PC, '32x256', 4, 1)),
    # a forward given one byte of workspace too few for its split, and none
    Case(3, 128, 136, 24, 27, 3, 1, False, 'fwd', 'short', route=(S, '128x128', 4, 1)),
    Case(2, 64, 70, 3, 3, 3, 1, False, 'fwd', 'short', route=(S, '64x64', 8, 1)),
    Case(2, 64, 70, 3, 3, 3, 1, False, 'fwd', 'none', route=(S, '64x64', 8, 1)),
    # weight gradient: the 16x16 MFMA tile; 1 x 1, 2 x 1, 1 x 2 and 2 x 2 waves per tile; 3x3 / 1x1 / stride 2; one slab (direct
    # store) and several (k_wgrad_reduce); rows of 2 ... 32 pixels
    Case(2, 5, 7, 11, 13, 3, 1, False, 'wgrad', route=4),
    Case(1, 5, 7, 3, 2, 1, 1, False, 'wgrad', route=1),
    Case(2, 5, 7, 21, 23, 3, 2, False, 'wgrad', route=12),
    Case(2, 20, 24, 9, 11, 3, 1, False, 'wgrad', route=4),
    Case(2, 20, 40, 9, 11, 3, 1, False, 'wgrad', route=4),
    Case(2, 40, 20, 9, 11, 3, 1, True, 'wgrad', route=4),
    Case(2, 40, 72, 33, 35, 3, 1, False, 'wgrad', route=68),
    Case(1, 20, 24, 8, 8, 3, 1, False, 'wgrad', route=1),
    Case(1, 20, 40, 8, 8, 3, 1, False, 'wgrad', route=1),
    Case(1, 68, 100, 8, 8, 3, 1, False, 'wgrad', route=1),
    Case(512, 68, 100, 1, 1, 3, 1, False, 'wgrad', route=32),
    Case(2, 40, 72, 9, 11, 1, 1, False, 'wgrad', route=6),
    Case(2, 20, 24, 9, 11, 1, 1, True, 'wgrad', route=6),
    Case(1, 68, 40, 8, 8, 1, 1, False, 'wgrad', route=1),
    Case(2, 40, 72, 9, 13, 3, 2, False, 'wgrad', route=4),
    Case(2, 20, 24, 9, 13, 3, 2, False, 'wgrad', route=4),
    Case(1, 72, 40, 8, 8, 3, 2, False, 'wgrad', route=1),
]


def case_id(c):
    return '%s-%dx%d->%d-%dx%d-k%d-s%d%s%s' % (c.op, c.B, c.K, c.N, c.H, c.W, c.ksize, c.stride, '-fe' if c.fe else '',
                                                '' if c.ws == 'full' else '-ws_' + c.ws)


def _ws_bytes(c):
    from histogan_amd._lib import lib
    if c.op == 'wgrad':
        return lib.hg_conv2d_wgrad_workspace_bytes(c.B, c.K, c.N, c.H, c.W, c.ksize, c.stride)
    nb = lib.hg_conv2d_workspace_bytes(c.B, c.K, c.N, c.H, c.W, c.ksize, c.stride, int(c.op == 'dgrad'))
    return {'full': nb, 'short': nb - 1, 'none': 0}[c.ws]


def make_inputs(c, dev):
    """The case's tensors (seeded by the case): x / gout as the call reads them, the unpacked weight (out ch, in ch, k, k) of
    the convolution, and the scales (None without fe)."""
    g = torch.Generator().manual_seed(hash(tuple(c[:8])) % (1 << 31))
    Ho, Wo = (c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    t = {}
    if c.op == 'dgrad':      # the convolution maps N -> K channels
        t['w'] = rnd(c.K, c.N, c.ksize, c.ksize) / (c.K * c.ksize ** 2) ** 0.5
        t['gout'] = rnd(c.B, c.K, Ho, Wo)
    else:
        t['w'] = rnd(c.N, c.K, c.ksize, c.ksize) / (c.K * c.ksize ** 2) ** 0.5
        t['x'] = rnd(c.B, c.K, c.H, c.W)
        t['gout'] = rnd(c.B, c.N, Ho, Wo)
    t['iscale'] = (torch.rand(c.B, c.K, generator=g) + 0.5).to(dev) if c.fe else None
    t['oscale'] = (torch.rand(c.B, c.N, generator=g) + 0.5).to(dev) if c.fe else None
    return t


def run_case(c, dev, t=None):
    """The case's one C-ABI call on `dev`: {'out' | 'gin' | 'gw': tensor}."""
    from histogan_amd._lib import check, lib, ptr, raw_stream
    t = t or make_inputs(c, dev)
    st = raw_stream(dev)
    Ho, Wo = (c.H - 1) // c.stride + 1, (c.W - 1) // c.stride + 1
    nb = _ws_bytes(c)
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
    wsp = None if c.ws == 'none' else ws.data_ptr()
    if c.op == 'wgrad':
        gw = torch.full((c.N, c.K, c.ksize, c.ksize), float('nan'), device=dev)
        check(lib.hg_conv2d_wgrad(t['x'].data_ptr(), t['gout'].data_ptr(), gw.data_ptr(), ptr(t['iscale']), ptr(t['oscale']), c.B, c.K, c.N,
                                  c.H, c.W, c.ksize, c.stride, wsp, nb, st), 'hg_conv2d_wgrad')
        return {'gw': gw}
    Co, Ci, mode = (c.K, c.N, 1) if c.op == 'dgrad' else (c.N, c.K, 0)
    wt = torch.empty(lib.hg_conv_packed_elems(Co, Ci, c.ksize, mode), device=dev)
    check(lib.hg_conv_pack_weights(t['w'].data_ptr(), wt.data_ptr(), Co, Ci, c.ksize, mode, st), 'hg_conv_pack_weights')
    if c.op == 'dgrad':
        gin = torch.full((c.B, c.N, c.H, c.W), float('nan'), device=dev)
        check(lib.hg_conv2d_dgrad(t['gout'].data_ptr(), wt.data_ptr(), gin.data_ptr(), ptr(t['iscale']), ptr(t['oscale']), c.B, c.K, c.N,
                                  c.H, c.W, c.ksize, c.stride, wsp, nb, st), 'hg_conv2d_dgrad')
        return {'gin': gin}
    out = torch.full((c.B, c.N, Ho, Wo), float('nan'), device=dev)
    check(lib.hg_conv2d_fwd(t['x'].data_ptr(), wt.data_ptr(), out.data_ptr(), ptr(t['iscale']), ptr(t['oscale']), None, c.B, c.K, c.N,
                            c.H, c.W, c.ksize, c.stride, wsp, nb, st), 'hg_conv2d_fwd')
    return {'out': out}


def reference(c, t):
    """The same product from F.conv2d and its autograd in fp64."""
    d = lambda v: None if v is None else v.double()
    w, isc, osc, pad = d(t['w']), d(t['iscale']), d(t['oscale']), c.ksize // 2
    sc = lambda v, s: v if s is None else v * s[:, :, None, None]
    if c.op == 'fwd':
        return sc(F.conv2d(sc(d(t['x']), isc), w, stride=c.stride, padding=pad), osc)
    if c.op == 'dgrad':
        x = torch.zeros(c.B, c.N, c.H, c.W, dtype=torch.float64, device=w.device, requires_grad=True)
        gx, = torch.autograd.grad(F.conv2d(x, w, stride=c.stride, padding=pad), x, sc(d(t['gout']), isc))
        return sc(gx, osc)
    wr = w.clone().requires_grad_(True)
    gw, = torch.autograd.grad(F.conv2d(sc(d(t['x']), isc), wr, stride=c.stride, padding=pad), wr, sc(d(t['gout']), osc))
    return gw


def wgrad_splits(c):
    """Pixel splits (slabs) of the weight-gradient launch, from the workspace it asks for: one slab is ksize^2 x Kp x Np floats,
    the channel counts rounded up to the block's extent (16 on the 16x16 MFMA tile, else 32 per wave along that axis)."""
    mt = 16 if c.N <= 16 and c.K <= 16 else 32
    if mt == 16:
        wn = wk = 1
    elif c.stride == 2:
        wn = wk = 2 if c.N > 32 and c.K > 32 else 1
    else:
        wn, wk = (2 if c.N > 32 else 1), (2 if c.K > 32 else 1)
    up = lambda v, m: (v + m - 1) // m * m
    slab = c.ksize ** 2 * up(c.K, wk * mt) * up(c.N, wn * mt) * 4
    nb = _ws_bytes(c)
    assert nb % slab == 0
    return nb // slab


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_route_is_the_planned_one_and_matches_fp64(c, gpu_device):
    from histogan_amd import _lib as L
    if c.op == 'wgrad':
        assert wgrad_splits(c) == c.route
    else:
        r = L.conv_route(c.B, c.K, c.N, c.H, c.W, c.ksize, c.stride, dgrad=c.op == 'dgrad', fe=c.fe, workspace_bytes=_ws_bytes(c))
        assert (L.HG_CONV_KIND[r.kind], L.HG_CONV_TILE[r.tile], r.kchunk, r.ksplit) == c.route
        assert r.cus == 256 and r.reduce == (r.ksplit > 1)
    t = make_inputs(c, gpu_device)
    (name, got), = run_case(c, gpu_device, t).items()
    ref = reference(c, t)
    assert got.shape == ref.shape
    assert relmax(got.cpu().numpy(), ref.cpu().numpy()) <= (5e-6 if name == 'gw' else 2e-6)
