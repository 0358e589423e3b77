"""One case per branch the Winograd host side (hg_wino.hip make_plan / make_wg_plan) can plan, straight through the C ABI (the
Python dispatch would refuse most of these shapes: they are the smallest that reach a branch on a 256-CU chip, not the ones
that beat the direct kernels).  Every case first asserts that hg_wino_route / hg_wino_wgrad_route still answer the route it was
chosen for -- a planning change shows up as that assertion, not as a silently untested branch -- and then compares with
F.conv2d / torch.nn.grad in fp64 at the bars of tests/test_wino_gpu.py: 2e-6 output and data gradient, 4e-6 weight gradient,
max-norm relative.

Forward branches (k_wino, k_wino_reduce): the XCD block order with 2 and 3 channel blocks, on a ragged map, with a K split; the
persistent tile loop where only some workgroups take a second tile, with a K split (the prefetched next tile belongs to another
split), on the 32-channel variant, with 8 channel blocks, together with the XCD order; K splits with a shorter last split and
4, 8, 16 splits; the noise row wrap of the reduce (W % 4 == 2); the fall-back to no split on a short or missing workspace.  No
forward case has an empty K split: the planner never takes one (see make_plan; tests/test_wino_route_cpu.py scans for them).
Each forward case also runs as the data gradient (K and N swapped, flipped operand) where that operand exists, with the route
of that launch asserted as well.

Weight-gradient branches (k_wino_wgrad, k_wino_wgrad_reduce<1|8|32>): the ten chunk patterns (lPW, lPH, lPI), each with an image
tail inside the chunk where lPI > 0; the three reduce variants; the persistent loop without and with the XCD order; blocks
with 0, 1, 2 and 3 chunks; empty splits (zero slabs).

Every call writes into an output placed between two sentinel bands and pre-filled with NaN, on a workspace pre-filled with NaN
(a slab element the reduce reads but no block wrote shows up), and runs twice (bit-identical results).
profiles/wino_route_gpu.json has the route and the measured error of every case (largest: 4.6e-7 output / data gradient,
3.0e-7 weight gradient)."""
import collections

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GUARD = 4096            # floats on either side of an output (a multiple of 4: the output keeps its 16-byte alignment)
SENTINEL = 12345.5    # (exact in fp32)

# B, K, N, H, W as hg_wino_conv2d takes them.  want: route fields the case was chosen for.  dg: those of the data-gradient
# launch (B, N, K, H, W), None where that operand does not exist.  ws: 'full' = the workspace the query asks for, 'short' =
# one byte less, 'none' = NULL.  tiles = blocks * ksplit, the work items of the launch (grid = min(tiles, 256)).
Fwd = collections.namedtuple('Fwd', 'B K N H W want dg ws', defaults=('full',))
FWD = [
    # XCD order, 2 channel blocks, ragged in both directions (17 x 5 tiles on 16 x 4 block tiles), one tile per workgroup
    Fwd(2, 32, 72, 10, 34, dict(variant=0, xcd=1, nblk=2, ksplit=1, tiles=16, persistent=0, ragged=True),
        dict(variant=1, ksplit=2, tiles=8, persistent=0)),
    # XCD order, 3 channel blocks
    Fwd(2, 32, 192, 10, 34, dict(variant=0, xcd=1, nblk=3, ksplit=1, tiles=24, persistent=0),
        dict(variant=1, ksplit=6, chunks_per_split=8, tiles=24)),
    # XCD order with a K split; the reduce's noise row wrap (W = 34)
    Fwd(2, 128, 72, 10, 34, dict(variant=0, xcd=1, nblk=2, ksplit=2, chunks_per_split=8, tiles=32, persistent=0, reduce=1),
        dict(variant=0, xcd=1, ksplit=1, tiles=16)),
    Fwd(2, 128, 72, 10, 34, dict(variant=0, xcd=1, nblk=2, ksplit=1, tiles=16, reduce=0, slab_bytes=0), None, 'short'),
    Fwd(2, 128, 72, 10, 34, dict(variant=0, xcd=1, nblk=2, ksplit=1, tiles=16, reduce=0, slab_bytes=0), None, 'none'),
    # persistent: 264 tiles on 256 workgroups, eight of them take a second tile
    Fwd(33, 32, 72, 10, 34, dict(variant=0, xcd=0, ksplit=1, tiles=264, grid=256, persistent=1),
        dict(variant=1, ksplit=2, tiles=132, persistent=0)),
    # persistent with a K split: 528 tiles, the next tile of workgroups 8 ... 255 belongs to the other split
    Fwd(33, 192, 72, 10, 34, dict(variant=0, xcd=0, ksplit=2, chunks_per_split=12, tiles=528, grid=256, persistent=1),
        dict(variant=0, nblk=3, xcd=0, ksplit=1, tiles=396, persistent=1)),
    Fwd(33, 192, 72, 10, 34, dict(variant=0, ksplit=1, tiles=264, persistent=1, reduce=0, slab_bytes=0), None, 'short'),
    Fwd(33, 192, 72, 10, 34, dict(variant=0, ksplit=1, tiles=264, persistent=1, reduce=0, slab_bytes=0), None, 'none'),
    # XCD order, K split and persistent together: 576 tiles
    Fwd(8, 192, 72, 66, 34, dict(variant=0, xcd=1, nblk=2, ksplit=2, tiles=576, grid=256, persistent=1),
        dict(variant=0, xcd=1, nblk=3, ksplit=1, tiles=432, persistent=1)),
    # the 32-channel variant, persistent: 288 tiles
    Fwd(32, 32, 16, 34, 66, dict(variant=1, ksplit=1, tiles=288, grid=256, persistent=1, ragged=True),
        dict(variant=1, ksplit=1, tiles=288, persistent=1)),
    # the 32-channel variant, persistent with a K split of 3: 396 tiles
    Fwd(33, 192, 16, 18, 34, dict(variant=1, ksplit=3, chunks_per_split=16, tiles=396, grid=256, persistent=1),
        dict(variant=0, nblk=3, ksplit=1, tiles=594, persistent=1)),
    # 8 channel blocks (channel block fastest), persistent: 288 tiles
    Fwd(9, 32, 512, 10, 34, dict(variant=0, xcd=0, nblk=8, ksplit=1, tiles=288, grid=256, persistent=1),
        dict(variant=1, ksplit=13, chunks_per_split=10, last_split_chunks=8, tiles=234)),
    # K splits with a shorter last split (odd and even chunk counts), up to 16 splits; batch tail inside the image group
    Fwd(1, 136, 40, 2, 2, dict(variant=0, ksplit=2, chunks_per_split=9, last_split_chunks=8, tiles=2),
        dict(variant=0, nblk=3, ksplit=1, tiles=3)),
    Fwd(1, 136, 16, 2, 2, dict(variant=1, ksplit=4, chunks_per_split=9, last_split_chunks=7, tiles=4),
        dict(variant=0, nblk=3, ksplit=1, tiles=3)),
    Fwd(1, 520, 40, 2, 2, dict(variant=0, ksplit=8, chunks_per_split=9, last_split_chunks=2, tiles=8),
        dict(variant=0, nblk=9, ksplit=1, tiles=9)),
    Fwd(1, 1040, 16, 2, 2, dict(variant=1, ksplit=16, chunks_per_split=17, last_split_chunks=5, tiles=16),
        dict(variant=0, nblk=17, ksplit=1, tiles=17)),
]

# B, K, N, H, W as hg_wino_wgrad takes them; want: route fields the case was chosen for (blocks = ktiles * ntiles * splits)
Wg = collections.namedtuple('Wg', 'B K N H W want')
WG = [
    # the ten chunk patterns; B = 3: an image tail inside the chunk wherever lPI > 0; 72 channels: padded, 2 x 2 channel tiles
    Wg(3, 72, 72, 2, 2, dict(pattern=(0, 0, 3), nchunks=1, splits=1)),
    Wg(3, 72, 72, 4, 2, dict(pattern=(0, 1, 2), nchunks=1, splits=1)),
    Wg(3, 72, 72, 8, 2, dict(pattern=(0, 2, 1), nchunks=2, splits=2)),
    Wg(3, 72, 72, 16, 2, dict(pattern=(0, 3, 0), nchunks=3, splits=3)),
    Wg(3, 72, 72, 2, 4, dict(pattern=(1, 0, 2), nchunks=1, splits=1)),
    Wg(3, 72, 72, 4, 4, dict(pattern=(1, 1, 1), nchunks=2, splits=2)),
    Wg(3, 72, 72, 8, 4, dict(pattern=(1, 2, 0), nchunks=3, splits=3)),
    Wg(3, 72, 72, 2, 8, dict(pattern=(2, 0, 1), nchunks=2, splits=2)),
    Wg(3, 72, 72, 4, 8, dict(pattern=(2, 1, 0), nchunks=3, splits=3)),
    Wg(3, 72, 72, 2, 16, dict(pattern=(3, 0, 0), nchunks=3, splits=3)),
    # the three reduce variants
    Wg(9, 64, 64, 2, 2, dict(reduce_groups=1, splits=2)),
    Wg(1, 64, 64, 2, 64, dict(reduce_groups=8, splits=4)),
    Wg(3, 330, 72, 4, 64, dict(reduce_groups=32, splits=22, xcd=0, blocks=264, grid=256, persistent=1, empty_splits=10)),
    # 3 chunks per block (odd, > 2), 20 empty splits, XCD order
    Wg(33, 72, 72, 2, 64, dict(chunks_per_split=3, last_split_chunks=3, splits=64, empty_splits=20, xcd=1, persistent=0)),
    # blocks with 2, 1 and 0 chunks
    Wg(33, 72, 200, 2, 16, dict(chunks_per_split=2, last_split_chunks=1, splits=32, empty_splits=15, xcd=1)),
    # persistent with the XCD order
    Wg(1, 200, 520, 4, 64, dict(splits=8, xcd=1, blocks=288, grid=256, persistent=1, reduce_groups=8)),
    # the smallest shape hg_wino_wgrad_supported accepts
    Wg(2, 72, 72, 64, 64, dict(supported=1, splits=64, chunks_per_split=4, xcd=1, reduce_groups=32, pattern=(3, 0, 0))),
]


def _id(c):
    return '%dx%d->%d-%dx%d%s' % (c.B, c.K, c.N, c.H, c.W, '' if getattr(c, 'ws', 'full') == 'full' else '-ws_' + c.ws)


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _p(t):
    return None if t is None else t.data_ptr()


class Guarded:
    """An output of `shape` inside a larger buffer: NaN where the call must write, sentinel bands on both sides."""

    def __init__(self, shape, dev):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.out = self.buf[GUARD:GUARD + n].view(shape)
        self.out.fill_(float('nan'))
        assert self.out.data_ptr() % 16 == 0

    def check(self, what):
        n = self.out.numel()
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + n:] == SENTINEL).all()), what + ': guard band'
        assert not bool(torch.isnan(self.out).any()), what + ': output not fully written'
        return self.out


def _assert_route(r, want, H, W, what):
    got = {}
    for k in want:
        if k == 'tiles':
            got[k] = r.blocks * r.ksplit
        elif k == 'ragged':
            got[k] = (r.bt_x << r.lTW) * 2 > W and (r.bt_y << r.lTH) * 2 > H
        elif k == 'pattern':
            got[k] = (r.lPW, r.lPH, r.lPI)
        elif k == 'blocks' and hasattr(r, 'ktiles'):
            got[k] = r.ktiles * r.ntiles * r.splits
        else:
            got[k] = getattr(r, k)
    assert got == want, what
    assert r.cus == 256, what


def _wino(x, u, N, ws_mode, **ep):
    """One hg_wino_conv2d call: guarded NaN output, NaN workspace of the size the route asks for."""
    from histogan_amd import _lib as L
    B, K, H, W = x.shape
    nb = L.lib.hg_wino_workspace_bytes(B, K, N, H, W)
    ws = torch.full((max(nb // 4, 4),), float('nan'), dtype=torch.float32, device=x.device)
    wsp, wsb = {'full': (ws.data_ptr(), nb), 'short': (ws.data_ptr(), nb - 1), 'none': (None, 0)}[ws_mode]
    g = Guarded((B, N, H, W), x.device)
    L.check(L.lib.hg_wino_conv2d(x.data_ptr(), u.data_ptr(), g.out.data_ptr(), _p(ep.get('iscale')), _p(ep.get('oscale')),
                                 _p(ep.get('bias')), _p(ep.get('noise_w')), _p(ep.get('noise_img')), ep.get('noise_S', 0),
                                 ep.get('slope', 0.0), _p(ep.get('addend')), B, K, N, H, W, wsp, wsb, L.raw_stream(x.device)),
            'hg_wino_conv2d')
    return g


def _pack(w, mode):
    from histogan_amd import _lib as L
    Co, Ci = w.shape[:2]
    u = torch.empty(L.lib.hg_wino_packed_elems(Co, Ci, mode), dtype=torch.float32, device=w.device)
    L.check(L.lib.hg_wino_pack_weights(w.data_ptr(), u.data_ptr(), Co, Ci, mode, L.raw_stream(w.device)), 'hg_wino_pack_weights')
    return u


def _three_epilogues(tag, x, u, N, conv64, ws_mode, g):
    """bias only / the generator epilogue / bias + addend of one launch shape against fp64; conv64(x64) is the plain product."""
    B, K, H, W = x.shape
    dev = x.device
    bias = torch.randn(N, generator=g).to(dev)
    isc = (torch.randn(B, K, generator=g) * 0.3 + 1).to(dev)
    osc = (torch.rand(B, N, generator=g) + 0.5).to(dev)
    S = max(H, W) + 2
    nimg = torch.randn(B, S, S, generator=g).to(dev)
    nw = torch.randn(N, generator=g).to(dev)
    ad = torch.randn(B, N, H, W, generator=g).to(dev)
    base = conv64(x.double())
    b64 = bias.double()[None, :, None, None]
    gen = conv64(x.double() * isc.double()[:, :, None, None]) * osc.double()[:, :, None, None] + b64 \
        + nw.double()[None, :, None, None] * nimg.double()[:, None, :H, :W]
    runs = [('bias', dict(bias=bias), base + b64),
            ('generator', dict(iscale=isc, oscale=osc, bias=bias, noise_w=nw, noise_img=nimg, noise_S=S, slope=0.2), F.leaky_relu(gen, 0.2)),
            ('addend', dict(bias=bias, addend=ad), base + b64 + ad.double())]
    for name, ep, ref in runs:
        what = '%s %s' % (tag, name)
        out = _wino(x, u, N, ws_mode, **ep).check(what)
        err = _rel(out, ref)
        print('wino-route %s: %.3e' % (what, err))
        assert out.shape == ref.shape and err <= 2e-6, what
        assert torch.equal(out, _wino(x, u, N, ws_mode, **ep).check(what + ' (second call)')), what + ': not deterministic'


@pytest.mark.parametrize('c', FWD, ids=_id)
def test_forward_route_is_the_planned_one_and_matches_fp64(c, gpu_device):
    from histogan_amd import _lib as L
    B, K, N, H, W = c[:5]
    nb = L.lib.hg_wino_workspace_bytes(B, K, N, H, W)
    wsb = {'full': None, 'short': nb - 1, 'none': 0}[c.ws]
    assert c.ws == 'full' or nb > 0
    for fe in (0, 1):
        _assert_route(L.wino_route(B, K, N, H, W, fe=fe, workspace_bytes=wsb), c.want, H, W, 'fwd fe=%d' % fe)
    assert L.lib.hg_wino_packed_elems(N, K, 0) > 0
    g = torch.Generator().manual_seed(B * 131 + K + 7 * N + H)
    x = torch.randn(B, K, H, W, generator=g).to(gpu_device)
    w = (torch.randn(N, K, 3, 3, generator=g) / (K * 9) ** 0.5).to(gpu_device)
    w64 = w.double()
    _three_epilogues('fwd ' + _id(c), x, _pack(w, 0), N, lambda v: F.conv2d(v, w64, padding=1), c.ws, g)
    if c.dg is None:
        assert c.ws != 'full' or L.lib.hg_wino_packed_elems(N, K, 1) == 0
        return
    # the data gradient of that convolution: a launch with N input and K output channels on the flipped operand
    assert L.lib.hg_wino_packed_elems(N, K, 1) > 0
    for fe in (0, 1):
        _assert_route(L.wino_route(B, N, K, H, W, fe=fe), c.dg, H, W, 'dgrad fe=%d' % fe)
    go = torch.randn(B, N, H, W, generator=g).to(gpu_device)
    _three_epilogues('dgrad ' + _id(c), go, _pack(w, 1), K, lambda v: torch.nn.grad.conv2d_input((B, K, H, W), w64, v, padding=1),
                     'full', g)


def _wgrad(x, go, what):
    from histogan_amd import _lib as L
    B, K, H, W = x.shape
    N = go.shape[1]
    nb = L.lib.hg_wino_wgrad_workspace_bytes(B, K, N, H, W)
    ws = torch.full((nb // 4,), float('nan'), dtype=torch.float32, device=x.device)
    g = Guarded((N, K, 3, 3), x.device)
    L.check(L.lib.hg_wino_wgrad(x.data_ptr(), go.data_ptr(), g.out.data_ptr(), B, K, N, H, W, ws.data_ptr(), nb, L.raw_stream(x.device)),
            'hg_wino_wgrad')
    return g.check(what)


@pytest.mark.parametrize('c', WG, ids=_id)
def test_wgrad_route_is_the_planned_one_and_matches_fp64(c, gpu_device):
    from histogan_amd import _lib as L
    B, K, N, H, W = c[:5]
    r = L.wino_wgrad_route(B, K, N, H, W)
    _assert_route(r, c.want, H, W, 'wgrad')
    assert r.slab_bytes == L.lib.hg_wino_wgrad_workspace_bytes(B, K, N, H, W)
    g = torch.Generator().manual_seed(B * 17 + K + 3 * N + H + 5 * W)
    x = torch.randn(B, K, H, W, generator=g).to(gpu_device)
    go = torch.randn(B, N, H, W, generator=g).to(gpu_device)
    ref = torch.nn.grad.conv2d_weight(x.double(), (N, K, 3, 3), go.double(), padding=1)
    what = 'wgrad ' + _id(c)
    gw = _wgrad(x, go, what)
    err = _rel(gw, ref)
    print('wino-route %s: %.3e' % (what, err))
    assert gw.shape == ref.shape and err <= 4e-6, what
    assert torch.equal(gw, _wgrad(x, go, what + ' (second call)')), what + ': not deterministic'
