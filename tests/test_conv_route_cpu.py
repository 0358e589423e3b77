"""hg_conv2d_route without a GPU (256 CUs assumed): the route query against the two older host queries it generalises
(hg_conv2d_plan, hg_conv2d_workspace_bytes) over a grid of arguments, and the rules a route must obey -- slab size, "too
little workspace: no K split", the 1-pixel-wide stride-2 data gradient, the 2-channel K chunks with and without fused extras,
and the return codes of invalid arguments."""
import ctypes
import itertools

import pytest

BS = (1, 2, 32, 64)
CH = (3, 16, 17, 32, 33, 64, 65, 128, 512, 2048)
HS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 256)
EINVAL, EUNSUPPORTED = -1, -5
SINGLE, PARITY4, PER_CLASS = range(3)
T16, T32, T64W, T128, T128SM, T64 = range(6)


@pytest.fixture(scope='module')
def L():
    from histogan_amd import build
    build.build()
    import histogan_amd._lib as L
    if L.conv_route(32, 256, 128, 64, 64, 3).cus != 256:
        pytest.skip('route expectations are written for the 256 CUs of an MI355X')
    return L


def grid():
    for ksize, stride in ((3, 1), (1, 1), (3, 2)):
        for H in HS:
            for W, B, K, N in itertools.product((H, 1, H + 1), BS, CH, CH):
                if B * max(K, N) * H * W < 1 << 31:
                    yield B, K, N, H, W, ksize, stride


def test_plain_route_is_the_plan_and_sizes_the_workspace(L):
    """fe = 0, any workspace: hg_conv2d_route == hg_conv2d_plan wherever the latter answers (every output, the stride-1 data
    gradient); its slab bytes == hg_conv2d_workspace_bytes for both directions and strides; the slabs are ksplit outputs
    (the one-launch stride-2 data gradient on the 64 x 64 tile: the split planned per class, of which it launches half);
    one byte less than that and the launch does not split."""
    plan = (ctypes.c_int32 * 5)()
    n = splits = halved = 0
    for B, K, N, H, W, ksize, stride in grid():
        for dgrad in (0, 1):
            r = L.conv_route(B, K, N, H, W, ksize, stride, dgrad=dgrad)
            args = (B, K, N, H, W, ksize, stride, dgrad)
            rc = L.lib.hg_conv2d_plan(*args, plan)
            if dgrad and stride == 2:
                assert rc == EUNSUPPORTED and r.kind in (PARITY4, PER_CLASS), args
            else:
                assert rc == 0 and r.kind == SINGLE, args
                assert (r.tile, r.ksplit, r.kchunk, min(r.blocks, 0x7fffffff), r.cus) == tuple(plan), args
            assert r.slab_bytes == L.lib.hg_conv2d_workspace_bytes(*args), args
            assert r.reduce == (r.ksplit > 1) and (r.slab_bytes > 0 or r.ksplit == 1), args
            Ho, Wo = (H, W) if dgrad else ((H - 1) // stride + 1, (W - 1) // stride + 1)
            out_bytes = B * N * Ho * Wo * 4
            if r.kind == PARITY4 and r.tile == T64:
                planned = r.slab_bytes // out_bytes
                assert r.slab_bytes == planned * out_bytes and r.ksplit == max(planned // 2, 1), args
                halved += planned > 1
            elif r.ksplit > 1:
                assert r.slab_bytes == r.ksplit * out_bytes, args
            else:
                assert r.slab_bytes == 0, args
            if r.slab_bytes:
                s = L.conv_route(B, K, N, H, W, ksize, stride, dgrad=dgrad, workspace_bytes=r.slab_bytes - 1)
                assert (s.ksplit, s.reduce, s.slab_bytes, s.kind, s.tile) == (1, 0, 0, r.kind, r.tile), args
                s = L.conv_route(B, K, N, H, W, ksize, stride, dgrad=dgrad, workspace_bytes=0)     # NULL: may plan another tile
                assert (s.ksplit, s.reduce, s.slab_bytes) == (1, 0, 0), args
                splits += 1
            n += 1
    assert n > 50000 and splits > 2000 and halved > 100


def test_one_pixel_wide_images_never_split_the_stride2_data_gradient(L):
    for B, K, N, H in itertools.product(BS, CH, CH, HS):
        for Hi, Wi in ((H, 1), (1, H)):
            r = L.conv_route(B, K, N, Hi, Wi, 3, 2, dgrad=True)
            assert (r.kind, r.ksplit, r.slab_bytes, r.reduce) == (PER_CLASS, 1, 0, 0)


def test_shapes_of_the_splitk_gpu_test_split(L):
    for B, K, N, H in [(32, 2048, 1024, 8), (16, 2048, 2048, 4), (64, 1024, 2048, 2), (32, 1024, 512, 16)]:
        assert L.conv_route(B, K, N, H, H, 3).ksplit > 1         # (the forward: what that test asks hg_conv2d_plan)


def test_fused_extras_keep_the_long_chunks_on_the_two_larger_tiles(L):
    """3x3 stride-1 launches: where the plain launch takes the 2-channel K chunks on the 64 x 256 or 128 x 128 tile, the launch
    with scales / noise / LeakyReLU takes the 4-channel ones (hg_conv2d_plan used to answer 2 for both); on the 32 x 256 tile
    both take 2; everywhere else fe changes nothing."""
    seen = {T32: 0, T64W: 0, T128: 0}
    for B, K, N, H, W, ksize, stride in grid():
        if (ksize, stride) != (3, 1):
            continue
        for dgrad in (0, 1):
            r0, r1 = (L.conv_route(B, K, N, H, W, 3, 1, dgrad=dgrad, fe=fe) for fe in (0, 1))
            assert (r0.kind, r0.tile, r0.ksplit, r0.blocks, r0.slab_bytes) == (r1.kind, r1.tile, r1.ksplit, r1.blocks, r1.slab_bytes)
            if r0.tile in (T64W, T128) and r0.kchunk == 2:
                assert r1.kchunk == 4
                seen[r0.tile] += 1
            else:
                assert r1.kchunk == r0.kchunk
                seen[T32] += r0.tile == T32 and r0.kchunk == 2
    assert all(seen.values()), seen
    # bench.py's roofline layer and the 64-channel layer of the generator at batch 32
    assert [L.conv_route(32, 256, 128, 64, 64, 3, fe=fe).kchunk for fe in (0, 1)] == [2, 4]
    assert [L.conv_route(32, 128, 64, 128, 128, 3, fe=fe).kchunk for fe in (0, 1)] == [2, 4]
    assert [L.conv_route(32, 64, 32, 256, 256, 3, fe=fe).kchunk for fe in (0, 1)] == [2, 2]


def test_stride2_data_gradient_forms(L):
    """Small maps: one launch on the 64 x 64 tile with the halved split; large maps: one launch on the tile planned for the
    smallest class, without fused extras only; with them, and between the two forms, one launch per class."""
    r = L.conv_route(8, 128, 128, 4, 4, 3, 2, dgrad=True)
    assert (r.kind, r.tile, r.kchunk) == (PARITY4, T64, 8) and r.ksplit > 1 and r.reduce
    r = L.conv_route(2, 16, 16, 128, 128, 3, 2, dgrad=True)
    assert (r.kind, r.tile, r.kchunk, r.ksplit, r.slab_bytes) == (PARITY4, T16, 4, 1, 0)
    assert L.conv_route(2, 16, 16, 128, 128, 3, 2, dgrad=True, fe=True).kind == PER_CLASS
    assert L.conv_route(2, 16, 16, 17, 17, 3, 2, dgrad=True).kind == PER_CLASS     # classes of 9 and 8 rows: two tiles
    for Hi, Wi in ((1, 1), (1, 9), (9, 1)):
        assert L.conv_route(2, 16, 16, Hi, Wi, 3, 2, dgrad=True).kind == PER_CLASS


def test_invalid_arguments_return_the_codes_of_the_calls(L):
    R, Q = L.HgConvRoute, L.HgConvQuery

    def rc(args=(1, 4, 4, 8, 8, 3, 1), dgrad=0, qsize=ctypes.sizeof(Q), rsize=ctypes.sizeof(R)):
        q = Q(qsize, dgrad, *args, 0, 1, 0)
        return L.lib.hg_conv2d_route(ctypes.byref(q), ctypes.byref(R(struct_size=rsize)))

    assert rc() == 0 and rc(dgrad=1) == 0
    plan = (ctypes.c_int32 * 5)()
    for bad in [(0, 4, 4, 8, 8, 3, 1), (1, 0, 4, 8, 8, 3, 1), (1, 4, -1, 8, 8, 3, 1), (1, 4, 4, 0, 8, 3, 1), (1, 4, 4, 8, 0, 3, 1),
                (1, 4, 4, 8, 8, 5, 1), (1, 4, 4, 8, 8, 2, 1), (1, 4, 4, 8, 8, 3, 3), (1, 4, 4, 8, 8, 3, 0), (1, 4, 4, 8, 8, 1, 2)]:
        for dgrad in (0, 1):
            assert rc(bad, dgrad) == EINVAL == L.lib.hg_conv2d_plan(*bad, dgrad, plan)
            assert L.lib.hg_conv2d_workspace_bytes(*bad, dgrad) == 0
        assert L.lib.hg_conv2d_wgrad_workspace_bytes(*bad) == 0
    assert rc((1, 4, 4, 8, 8, 3, 2), dgrad=1) == 0 and L.lib.hg_conv2d_plan(1, 4, 4, 8, 8, 3, 2, 1, plan) == EUNSUPPORTED
    assert L.lib.hg_conv2d_plan(1, 4, 4, 8, 8, 3, 1, 0, None) == EINVAL
    assert rc((64, 2048, 16, 256, 256, 3, 1)) == EUNSUPPORTED          # 2^33 input elements: the calls refuse them too
    assert rc(qsize=8) == EINVAL and rc(rsize=8) == EINVAL
    assert L.lib.hg_conv2d_route(None, ctypes.byref(R(struct_size=ctypes.sizeof(R)))) == EINVAL
    assert L.lib.hg_conv2d_route(ctypes.byref(Q(ctypes.sizeof(Q), 0, 1, 4, 4, 8, 8, 3, 1, 0, 1, 0)), None) == EINVAL
    assert L.lib.hg_version() >= 108 and 'hg_conv2d_route' in L.EXPORTS
    assert (ctypes.sizeof(Q), ctypes.sizeof(R)) == (56, 48)
