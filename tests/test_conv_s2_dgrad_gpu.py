"""The stride-2 data gradient whose blocks compute all four output-parity classes from one staged tile (hg_conv.hip
k_conv_allclass: the 16x256, 32x256 and 64x64 tiles of a PARITY4 route without fused extras), at the smallest shapes at which
its paths can go wrong, straight through the C ABI as tests/test_conv_route_gpu.py does (whose case type, inputs and fp64
reference this file shares): odd maps (the classes' extents differ, 4-byte stores), even maps (8-byte stores; the same on a
base that is only 4-byte aligned), K tails, many tiles, batch tails, channel blocks, the K split with a full / short / missing
workspace.  Plus one case each of the launches that keep one class per block: the 64x256 and 128x128 tiles, the fused extras,
and the PER_CLASS route.

Every case first asserts the route it was chosen for.  The result is written into a view inside a larger buffer pre-filled
with NaN: every element of the view must be finite (no missed pixel), every guard element before and behind it untouched (no
store outside the tensor), the values within 2e-6 (max-norm relative) of F.conv2d's autograd in fp64, and two calls bit-equal."""
import pytest
import torch

from conftest import relmax
from test_conv_route_gpu import P4, PC, Case, _ws_bytes, case_id, make_inputs, reference

GUARD = 64   # floats before and behind the view: keeps the 256-byte alignment of the allocation's start modulo 8 bytes


def D(B, K, N, H, W, route, fe=False, ws='full'):
    return Case(B, K, N, H, W, 3, 2, fe, 'dgrad', ws, route=route)


# (case, guard floats)
CASES = [
    # 16x256 tile: odd x odd maps; even maps; K no multiple of the chunk; >= 64 pixel tiles per class
    (D(2, 5, 7, 21, 23, (P4, '16x256', 4, 1)), GUARD),
    (D(2, 5, 7, 20, 24, (P4, '16x256', 4, 1)), GUARD),
    (D(2, 5, 7, 20, 24, (P4, '16x256', 4, 1)), GUARD - 1),   # even maps on a 4-byte aligned base: 4-byte stores
    (D(3, 18, 16, 22, 24, (P4, '16x256', 4, 1)), GUARD),
    (D(2, 5, 7, 255, 257, (P4, '16x256', 4, 1)), GUARD),
    # 32x256 tile
    (D(2, 5, 20, 21, 23, (P4, '32x256', 4, 1)), GUARD),
    (D(3, 34, 32, 22, 24, (P4, '32x256', 4, 1)), GUARD),
    # 64x64 tile, small maps: the smallest map of the route; a batch tail inside a tile, two channel blocks, mixed parity
    (D(2, 5, 7, 5, 7, (P4, '64x64', 8, 1)), GUARD),
    (D(2, 5, 7, 2, 2, (P4, '64x64', 8, 1)), GUARD),
    (D(7, 9, 70, 3, 4, (P4, '64x64', 8, 1)), GUARD),
    # ... K no multiple of the chunk on maps too small for the wide tiles (their classes are at most 8 pixels wide, so the
    # route answers the 64x64 tile for them whatever the channel count; the same K at 22 x 24 is in the wide tiles' lists above)
    (D(3, 18, 16, 6, 8, (P4, '64x64', 8, 1)), GUARD),
    (D(3, 34, 32, 10, 12, (P4, '64x64', 8, 1)), GUARD),
    # ... the K split (half the split planned per class) with the full workspace, one byte less, none
    (D(3, 128, 70, 4, 6, (P4, '64x64', 8, 2)), GUARD),
    (D(3, 128, 70, 4, 6, (P4, '64x64', 8, 1), ws='short'), GUARD),
    (D(3, 128, 70, 4, 6, (P4, '64x64', 8, 1), ws='none'), GUARD),
    (D(3, 256, 70, 4, 6, (P4, '64x64', 8, 4)), GUARD),
    (D(3, 256, 70, 4, 6, (P4, '64x64', 8, 1), ws='short'), GUARD),
    (D(3, 256, 70, 4, 6, (P4, '64x64', 8, 1), ws='none'), GUARD),
    # one class per block: input and output scales; the 64x256 and 128x128 tiles; one launch per class
    (D(3, 256, 70, 4, 6, (P4, '64x64', 8, 4), fe=True), GUARD),
    (D(8, 4, 40, 255, 257, (P4, '64x256', 4, 1)), GUARD),
    (D(1, 4, 136, 259, 261, (P4, '128x128', 4, 1)), GUARD),
    (D(2, 5, 7, 17, 17, (PC, '16x256', 4, 1)), GUARD),
]


def dgrad_guarded(c, t, wt, guard, dev):
    """hg_conv2d_dgrad of the case into a view `guard` floats inside a NaN buffer: (buffer, view)."""
    from histogan_amd._lib import check, lib, ptr, raw_stream
    n = c.B * c.N * c.H * c.W
    buf = torch.full((guard + n + GUARD,), float('nan'), device=dev)
    gin = buf[guard:guard + n].view(c.B, c.N, c.H, c.W)
    nb = _ws_bytes(c)
    ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=dev)
    check(lib.hg_conv2d_dgrad(t['gout'].data_ptr(), wt.data_ptr(), gin.data_ptr(), ptr(t['iscale']), ptr(t['oscale']), c.B, c.K, c.N,
                              c.H, c.W, 3, 2, None if c.ws == 'none' else ws.data_ptr(), nb, raw_stream(dev)), 'hg_conv2d_dgrad')
    return buf, gin


@pytest.mark.gpu
@pytest.mark.parametrize('c,guard', CASES, ids=lambda v: case_id(v) if isinstance(v, Case) else 'g%d' % v)
def test_s2_dgrad_matches_fp64_inside_its_tensor(c, guard, gpu_device):
    from histogan_amd import _lib as L
    r = L.conv_route(c.B, c.K, c.N, c.H, c.W, 3, 2, dgrad=True, fe=c.fe, workspace_bytes=_ws_bytes(c))
    assert (L.HG_CONV_KIND[r.kind], L.HG_CONV_TILE[r.tile], r.kchunk, r.ksplit) == c.route
    assert r.reduce == (r.ksplit > 1)
    t = make_inputs(c, gpu_device)
    wt = torch.empty(L.lib.hg_conv_packed_elems(c.K, c.N, 3, 1), device=gpu_device)
    L.check(L.lib.hg_conv_pack_weights(t['w'].data_ptr(), wt.data_ptr(), c.K, c.N, 3, 1, L.raw_stream(gpu_device)), 'hg_conv_pack_weights')
    buf, gin = dgrad_guarded(c, t, wt, guard, gpu_device)
    n = gin.numel()
    assert bool(torch.isfinite(gin).all()), 'a pixel of the data gradient was not written'
    # the guards still hold the fill's bits
    fill = torch.full((1,), float('nan'), device=gpu_device).view(torch.int32)
    bits = buf.view(torch.int32)
    assert bool((bits[:guard] == fill).all()) and bool((bits[guard + n:] == fill).all()), 'a store outside the tensor'
    ref = reference(c, t)
    err = relmax(gin.cpu().numpy(), ref.cpu().numpy())
    print('%s: relmax %.3g' % (case_id(c), err))
    assert err <= 2e-6
    _, again = dgrad_guarded(c, t, wt, guard, gpu_device)
    assert torch.equal(gin, again), 'two calls differ'
