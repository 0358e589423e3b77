"""hg_wino_route / hg_wino_wgrad_route without a GPU (256 CUs assumed): the two route queries against the older host queries
they generalise (hg_wino_packed_elems, hg_wino_workspace_bytes, hg_wino_supported and their weight-gradient counterparts) over
a grid of arguments, the rules a route must obey -- the K splits cover the chunks exactly once, "too little workspace: no K
split, same kernel and tiles", when the XCD block order may be taken, which reduce follows a weight gradient --, the scan
record profiles/wino_route_scan.json (tools/wino_route_scan.py writes it from scan() below), the return codes of invalid
arguments, and the argument checks hg_wino_conv2d / hg_wino_wgrad make before they touch a device."""
import ctypes
import itertools
import json
import os

import pytest

BS = (1, 2, 3, 9, 32, 33)
CH = (8, 16, 32, 36, 40, 64, 72, 128, 136, 200, 520, 1040, 2048)
HS = (2, 4, 6, 8, 10, 16, 18, 32, 34, 64, 66, 128)
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -4, -5
KNOBS = ('HG_WINO_VARIANT', 'HG_WINO_KSPLIT', 'HG_WINO_WG_SPLITS', 'HG_WINO_PERSIST')
RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'wino_route_scan.json')
GEOM = ('variant', 'nblk', 'nch', 'lTW', 'lTH', 'lNI', 'bt_x', 'bt_y', 'blocks', 'xcd')


@pytest.fixture(scope='module')
def L():
    from histogan_amd import build
    build.build()
    import histogan_amd._lib as L
    if L.wino_route(32, 256, 128, 64, 64).cus != 256:
        pytest.skip('route expectations are written for the 256 CUs of an MI355X')
    if any(k in os.environ for k in KNOBS):
        pytest.skip('route expectations are written for the planner, not for what the HG_WINO_* knobs force')
    return L


class Asker:
    """The two queries on reused structs (the grid asks ~600 000 times)."""

    def __init__(self, L):
        self.L = L
        self.q = L.HgWinoQuery(struct_size=ctypes.sizeof(L.HgWinoQuery))
        self.unlimited = ctypes.c_size_t(-1).value

    def _fill(self, shape, ws):
        q = self.q
        q.B, q.K, q.N, q.H, q.W = shape
        q.have_workspace = int(ws is None or ws > 0)
        q.workspace_bytes = self.unlimited if ws is None else ws

    def fwd(self, shape, ws=None, fe=0):
        self._fill(shape, ws)
        self.q.fe = fe
        r = self.L.HgWinoRoute(struct_size=ctypes.sizeof(self.L.HgWinoRoute))
        return self.L.lib.hg_wino_route(ctypes.byref(self.q), ctypes.byref(r)), r

    def wgrad(self, shape, ws=None):
        self._fill(shape, ws)
        r = self.L.HgWinoWgradRoute(struct_size=ctypes.sizeof(self.L.HgWinoWgradRoute))
        return self.L.lib.hg_wino_wgrad_route(ctypes.byref(self.q), ctypes.byref(r)), r


def grid():
    """Every shape stays under the size limits of the planners (2^31 elements per tensor, 2^30 bytes per block's images and
    per packed operand: the largest tensor here has 33 * 2048 * 128 * 128 = 1.1e9 elements); the limits have a test of their own."""
    return itertools.product(BS, CH, CH, HS, HS)


def scan(L):
    """The grid through both queries, every invariant asserted; returns the counts profiles/wino_route_scan.json records."""
    lib, ask = L.lib, Asker(L)
    c = dict(shapes=0, forward_routes=0, forward_ksplit=0, forward_ksplit_ge4=0, forward_short_last_split=0, forward_empty_splits=0,
             forward_xcd=0, forward_xcd_ksplit=0, forward_persistent=0, forward_persistent_ksplit=0, forward_variant1=0,
             wgrad_routes=0, wgrad_empty_splits=0, wgrad_xcd=0, wgrad_persistent=0, wgrad_persistent_xcd=0,
             wgrad_reduce_groups={'1': 0, '8': 0, '32': 0})
    smallest_empty = None
    for shape in grid():
        B, K, N, H, W = shape
        c['shapes'] += 1
        # ---- forward / data gradient
        rc, r = ask.fwd(shape)
        served = lib.hg_wino_packed_elems(N, K, 0) > 0            # (H and W are even and >= 2 all over the grid)
        assert rc == (0 if served else EUNSUPPORTED), shape
        assert lib.hg_wino_supported(*shape) == (r.supported if served else 0), shape
        if not served:
            assert lib.hg_wino_workspace_bytes(*shape) == 0, shape
        else:
            c['forward_routes'] += 1
            assert r.cus == 256 and r.variant == (N <= 32) and r.nch == K // (4 if r.variant else 8), shape
            assert r.nblk == -(-N // (32 if r.variant else 64)) and r.lTW + r.lTH + r.lNI == (7 if r.variant else 6), shape
            assert r.bt_x == -(-(W // 2) // (1 << r.lTW)) and r.bt_y == -(-(H // 2) // (1 << r.lTH)), shape
            assert r.blocks == r.nblk * r.bt_x * r.bt_y * -(-B // (1 << r.lNI)), shape
            assert r.slab_bytes == lib.hg_wino_workspace_bytes(*shape), shape
            assert r.slab_bytes == (r.ksplit * B * N * H * W * 4 if r.ksplit > 1 else 0) and r.reduce == (r.ksplit > 1), shape
            assert 1 <= r.ksplit <= 16 and (r.ksplit == 1 or r.nch // r.ksplit >= 8), shape
            assert r.chunks_per_split == -(-r.nch // r.ksplit) and 1 <= r.last_split_chunks <= r.chunks_per_split, shape
            assert 0 <= r.empty_splits < r.ksplit, shape
            assert (r.ksplit - r.empty_splits - 1) * r.chunks_per_split + r.last_split_chunks == r.nch, shape
            assert r.grid == min(r.blocks * r.ksplit, r.cus) and r.persistent == (r.blocks * r.ksplit > r.grid), shape
            if r.xcd:
                assert 2 <= r.nblk < 8 and r.blocks % r.nblk == 0 and (r.blocks // r.nblk) % 8 == 0 and r.grid % 8 == 0, shape
            geom = [getattr(r, n) for n in GEOM]
            rc1, r1 = ask.fwd(shape, fe=1)                         # the input scale picks a kernel instance, nothing else
            assert rc1 == 0 and r1.fe == 1 and r.fe == 0 and [getattr(r1, n) for n in GEOM] + [r1.ksplit] == geom + [r.ksplit], shape
            if r.ksplit > 1:
                for ws in (r.slab_bytes - 1, 0):                   # one byte too few; no workspace
                    rc2, s = ask.fwd(shape, ws)
                    assert rc2 == 0 and (s.ksplit, s.reduce, s.slab_bytes, s.empty_splits) == (1, 0, 0, 0), shape
                    assert (s.chunks_per_split, s.last_split_chunks) == (s.nch, s.nch), shape
                    assert [getattr(s, n) for n in GEOM] == geom and s.supported == r.supported, shape
                    assert s.grid == min(s.blocks, s.cus), shape
                rc2, s = ask.fwd(shape, r.slab_bytes)              # exactly enough
                assert rc2 == 0 and s.ksplit == r.ksplit, shape
            c['forward_ksplit'] += r.ksplit > 1
            c['forward_ksplit_ge4'] += r.ksplit >= 4
            c['forward_short_last_split'] += r.last_split_chunks < r.chunks_per_split
            c['forward_xcd'] += r.xcd
            c['forward_xcd_ksplit'] += r.xcd and r.ksplit > 1
            c['forward_persistent'] += r.persistent
            c['forward_persistent_ksplit'] += r.persistent and r.ksplit > 1
            c['forward_variant1'] += r.variant
            if r.empty_splits:
                c['forward_empty_splits'] += 1
                key = (B * K * N * H * W, shape)
                smallest_empty = key if smallest_empty is None else min(smallest_empty, key)
        # ---- weight gradient
        rc, g = ask.wgrad(shape)
        nb = lib.hg_wino_wgrad_workspace_bytes(*shape)
        pow2 = (H // 2) & (H // 2 - 1) == 0 and (W // 2) & (W // 2 - 1) == 0
        assert rc == (0 if pow2 else EUNSUPPORTED) and (nb > 0) == pow2, shape
        assert lib.hg_wino_wgrad_supported(*shape) == (g.supported if pow2 else 0), shape
        if pow2:
            c['wgrad_routes'] += 1
            assert g.cus == 256 and g.slab_bytes == nb, shape
            assert 1 <= g.splits <= g.nchunks, shape
            assert (1 << g.lPW) * (1 << g.lPH) * (1 << g.lPI) == 8, shape
            assert (W // 2) == 1 << (g.lPW + g.lcg) and (H // 2) == 1 << (g.lPH + g.lrg), shape
            assert g.nchunks == -(-B // (1 << g.lPI)) << (g.lcg + g.lrg), shape
            assert (g.ktiles, g.ntiles) == (-(-K // 64), -(-N // 64)), shape
            assert g.slab_bytes == g.splits * 16 * g.ktiles * 64 * g.ntiles * 64 * 4, shape
            assert g.reduce_groups == (32 if g.splits >= 16 else 8 if g.splits >= 4 else 1), shape
            assert g.xcd == (g.splits % 8 == 0), shape
            assert g.chunks_per_split == -(-g.nchunks // g.splits) and 1 <= g.last_split_chunks <= g.chunks_per_split, shape
            assert 0 <= g.empty_splits < g.splits, shape
            assert (g.splits - g.empty_splits - 1) * g.chunks_per_split + g.last_split_chunks == g.nchunks, shape
            blocks = g.ktiles * g.ntiles * g.splits
            assert g.grid == min(blocks, g.cus) and g.persistent == (blocks > g.grid), shape
            c['wgrad_empty_splits'] += g.empty_splits > 0
            c['wgrad_xcd'] += g.xcd
            c['wgrad_persistent'] += g.persistent
            c['wgrad_persistent_xcd'] += g.persistent and g.xcd
            c['wgrad_reduce_groups'][str(g.reduce_groups)] += 1
    c['forward_empty_splits_smallest_shape'] = list(smallest_empty[1]) if smallest_empty else None
    return c


def test_routes_obey_their_rules_over_the_grid_and_match_the_scan_record(L):
    """Every invariant of scan(); and the record: how often each branch is planned over the grid -- in particular how many
    forward routes have a K split that owns no chunk (the comment at make_plan, hg_wino.hip, and the GPU case that follows
    from it, tests/test_wino_route_gpu.py)."""
    c = scan(L)
    assert c['shapes'] == len(BS) * len(CH) ** 2 * len(HS) ** 2
    assert c['forward_routes'] > 100000 and c['forward_ksplit'] > 1000 and c['forward_xcd'] > 1000 and c['forward_persistent'] > 1000
    assert c['wgrad_routes'] > 30000 and all(c['wgrad_reduce_groups'].values()) and c['wgrad_empty_splits'] > 100
    with open(RECORD) as f:
        rec = json.load(f)
    assert rec['counts'] == c
    assert rec['grid'] == {'B': list(BS), 'K': list(CH), 'N': list(CH), 'H': list(HS), 'W': list(HS)}


def test_size_limits_and_odd_maps_are_unsupported(L):
    ask = Asker(L)
    for shape in [(1, 64, 64, 3, 4), (1, 64, 64, 4, 5), (1, 64, 64, 0, 4), (1, 64, 64, 4, 0), (1, 64, 64, 1, 1),
                  (0, 64, 64, 4, 4), (1, 0, 64, 4, 4), (1, 64, -1, 4, 4)]:
        assert ask.fwd(shape)[0] == EUNSUPPORTED and ask.wgrad(shape)[0] == EUNSUPPORTED, shape
        assert L.lib.hg_wino_supported(*shape) == 0 and L.lib.hg_wino_workspace_bytes(*shape) == 0
        assert L.lib.hg_wino_wgrad_supported(*shape) == 0 and L.lib.hg_wino_wgrad_workspace_bytes(*shape) == 0
    assert ask.fwd((1, 36, 64, 4, 4))[0] == EUNSUPPORTED and ask.fwd((1, 36, 32, 4, 4))[0] == 0       # K % 8 / K % 4
    assert ask.fwd((1, 36, 64, 4, 4))[0] == EUNSUPPORTED and ask.wgrad((1, 36, 64, 4, 4))[0] == 0     # (no such rule there)
    assert ask.fwd((64, 2048, 16, 256, 256))[0] == EUNSUPPORTED       # 2^33 input elements
    assert ask.fwd((64, 16, 2048, 256, 256))[0] == EUNSUPPORTED       # 2^33 output elements
    assert ask.fwd((1, 16384, 64, 256, 256))[0] == EUNSUPPORTED       # one block's image: 2^32 bytes
    assert ask.fwd((1, 8192, 64, 256, 256))[0] == 0
    assert ask.wgrad((1, 16384, 64, 256, 256))[0] == EUNSUPPORTED and ask.wgrad((1, 64, 16384, 256, 256))[0] == EUNSUPPORTED
    assert ask.wgrad((1, 8192, 64, 256, 256))[0] == 0
    assert ask.wgrad((1, 64, 64, 12, 8))[0] == EUNSUPPORTED           # six tiles per column


def test_invalid_arguments_return_the_codes_of_the_calls(L):
    Q, R, G = L.HgWinoQuery, L.HgWinoRoute, L.HgWinoWgradRoute
    assert (ctypes.sizeof(Q), ctypes.sizeof(R), ctypes.sizeof(G)) == (40, 96, 88)
    unlimited = ctypes.c_size_t(-1).value

    def rc(fn, RT, qsize=ctypes.sizeof(Q), rsize=None, have=1, ws=unlimited, shape=(4, 64, 64, 8, 8)):
        q = Q(qsize, *shape, 0, have, ws)
        return fn(ctypes.byref(q), ctypes.byref(RT(struct_size=ctypes.sizeof(RT) if rsize is None else rsize)))

    for fn, RT in ((L.lib.hg_wino_route, R), (L.lib.hg_wino_wgrad_route, G)):
        assert rc(fn, RT) == 0
        assert rc(fn, RT, qsize=8) == EINVAL and rc(fn, RT, qsize=0) == EINVAL and rc(fn, RT, rsize=8) == EINVAL
        assert fn(None, ctypes.byref(RT(struct_size=ctypes.sizeof(RT)))) == EINVAL
        assert fn(ctypes.byref(Q(ctypes.sizeof(Q), 4, 64, 64, 8, 8, 0, 1, unlimited)), None) == EINVAL
    # the weight gradient refuses a missing and a short workspace, as hg_wino_wgrad does; the route is filled all the same
    nb = L.lib.hg_wino_wgrad_workspace_bytes(4, 64, 64, 8, 8)
    assert rc(L.lib.hg_wino_wgrad_route, G, have=0, ws=0) == EINVAL
    assert rc(L.lib.hg_wino_wgrad_route, G, ws=nb - 1) == EWORKSPACE and rc(L.lib.hg_wino_wgrad_route, G, ws=nb) == 0
    q, g = Q(ctypes.sizeof(Q), 4, 64, 64, 8, 8, 0, 1, nb - 1), G(struct_size=ctypes.sizeof(G))
    assert L.lib.hg_wino_wgrad_route(ctypes.byref(q), ctypes.byref(g)) == EWORKSPACE and g.slab_bytes == nb and g.splits >= 1
    # the forward launches without a workspace (no split): no error
    assert rc(L.lib.hg_wino_route, R, have=0, ws=0, shape=(1, 136, 40, 2, 2)) == 0
    assert L.lib.hg_version() >= 112 and 'hg_wino_route' in L.EXPORTS and 'hg_wino_wgrad_route' in L.EXPORTS


def test_helpers_raise_and_fill(L):
    r = L.wino_route(2, 128, 72, 10, 34)
    assert (r.ksplit, r.reduce) == (2, 1) and r.slab_bytes == L.lib.hg_wino_workspace_bytes(2, 128, 72, 10, 34)
    assert L.wino_route(2, 128, 72, 10, 34, workspace_bytes=0).ksplit == 1
    assert L.wino_route(2, 128, 72, 10, 34, fe=True).fe == 1
    assert L.wino_wgrad_route(9, 64, 64, 2, 2).reduce_groups == 1
    with pytest.raises(L.HgError):
        L.wino_route(2, 128, 72, 9, 34)
    with pytest.raises(L.HgError):
        L.wino_wgrad_route(9, 64, 64, 2, 2, workspace_bytes=0)


def test_argument_checks_of_the_launch_calls_need_no_device(L):
    """hg_wino_conv2d / hg_wino_wgrad refuse these before they plan or launch anything: the pointers are never read."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    B, K, N, H, W = 2, 64, 64, 8, 8

    def conv(iscale=None, oscale=None, bias=None, noise_w=None, noise_img=None, noise_S=0, slope=0.0, addend=None, H=H, W=W):
        return L.lib.hg_wino_conv2d(p, p, p, iscale, oscale, bias, noise_w, noise_img, noise_S, slope, addend, B, K, N, H, W, None, 0, None)

    assert conv(noise_img=p, noise_S=8) == EINVAL and conv(noise_w=p) == EINVAL          # noise image and weight: both or none
    assert conv(noise_img=p, noise_w=p, noise_S=9) == EINVAL                              # odd
    assert conv(noise_img=p, noise_w=p, noise_S=6) == EINVAL                              # smaller than the map
    assert conv(noise_img=p, noise_w=p, noise_S=8, H=4, W=10) == EINVAL                   # narrower than the map
    assert conv(slope=-0.1) == EINVAL
    for extra in (dict(iscale=p), dict(oscale=p), dict(noise_img=p, noise_w=p, noise_S=8), dict(slope=0.2)):
        assert conv(addend=p, **extra) == EINVAL, extra
    assert conv(H=7) == EUNSUPPORTED and conv(W=9) == EUNSUPPORTED
    assert conv(addend=p, bias=p, H=7) == EUNSUPPORTED                                    # (a valid epilogue: the plan refuses)
    assert L.lib.hg_wino_conv2d(None, p, p, None, None, None, None, None, 0, 0.0, None, B, K, N, H, W, None, 0, None) == EINVAL
    assert L.lib.hg_wino_conv2d(p, None, p, None, None, None, None, None, 0, 0.0, None, B, K, N, H, W, None, 0, None) == EINVAL
    assert L.lib.hg_wino_conv2d(p, p, None, None, None, None, None, None, 0, 0.0, None, B, K, N, H, W, None, 0, None) == EINVAL

    wg = lambda ws=p, nb=1 << 40, H=H, W=W, a=p, b=p, c=p: L.lib.hg_wino_wgrad(a, b, c, B, K, N, H, W, ws, nb, None)
    assert wg(H=12) == EUNSUPPORTED and wg(W=20) == EUNSUPPORTED and wg(H=7) == EUNSUPPORTED   # 6, 10 tiles; odd
    assert wg(ws=None) == EINVAL and wg(a=None) == EINVAL and wg(b=None) == EINVAL and wg(c=None) == EINVAL
    assert wg(nb=L.lib.hg_wino_wgrad_workspace_bytes(B, K, N, H, W) - 1) == EWORKSPACE
