"""hg_rgbuv_hist_route on the CPU (no kernel is launched, no GPU needed): the kernel route the library decides once per call
-- the one its workspace sizes and launches are made from -- against the table of DESIGN.md section 4 ("Route"), restated
here independently of the C++ (`model`), and against the families the GPU parity tests expect their cases to run on."""
import ctypes
import itertools
import math

import pytest
import torch

from test_hist_weight_gpu import GPU_PIN_EXTRA
from test_hist_weight_grad_gpu import CASES, WANT

THR, RBF, IQ = 0, 1, 2
RGBUV, RGCHROMA, DIRECT = 0, 1, 2
NONE, BILINEAR, SAMPLING = 0, 1, 2
BOUNDS = [(-3.0, 3.0), (-3.0, 1.0), (0.5, 3.0)]


@pytest.fixture(scope='module')
def L():
    from histogan_amd import build
    build.build()
    import histogan_amd._lib as L
    return L


def params(L, h=64, method=IQ, sigma=0.02, lo=-3.0, hi=3.0, proj=RGBUV, green=0, intensity=1, resize=NONE, B=2, C=3,
           H=40, W=48, weight=None):
    p = L.HgHistParams()
    p.struct_size = ctypes.sizeof(L.HgHistParams)
    p.B, p.C, p.H, p.W = B, C, H, W
    p.stride_b, p.stride_c, p.stride_h, p.stride_w = C * H * W, H * W, W, 1
    p.resize_mode = resize
    p.Hs, p.Ws = (H, W) if resize == NONE else (24, 24)
    if resize == SAMPLING:
        p.row_idx = p.col_idx = 0x1000           # never dereferenced: the query launches nothing
    p.h, p.lo, p.hi, p.method, p.sigma = h, lo, hi, method, sigma
    p.intensity_scale, p.green_only, p.projection = intensity, green, proj
    if weight is not None:                       # (stride_b, stride_h, stride_w)
        p.weight = 0x2000
        p.weight_stride_b, p.weight_stride_h, p.weight_stride_w = weight
    return p


def route(L, p, weight_grad=0):
    r = L.hist_route(p, weight_grad)
    return L.HG_ROUTE_FWD[r.fwd], L.HG_ROUTE_BWD[r.bwd], r.planes_rt, r.rbf_radius


def model(h, method, sigma, lo, hi, proj, green, intensity, resize, weight_grad, rbf_dense=None, bwd_planes=None):
    """DESIGN.md section 4, "Route": (fwd, bwd, planes_rt, rbf_radius)."""
    grid_fits = h * h * 8 <= 156 * 1024
    three_planes = proj == RGBUV and not green
    three_fit = 3 * h * h * 8 <= 150 * 1024
    single = h >= 2 and (hi - lo) / (h - 1) > (abs(lo) + abs(hi)) / h * (1 + 1e-9)
    if method == THR and grid_fits:
        if three_planes and single and three_fit:
            if intensity or weight_grad:
                return 'THR_LEAN', 'THR_LEAN', 0, 0
            return 'THR_LEAN', ('ZERO' if resize == NONE else 'THR_GATHER'), 0, 0
        return 'THR_SCATTER', 'THR_GATHER', 0, 0
    if method == RBF and grid_fits and h >= 2 and hi > lo and rbf_dense != '1':
        R = math.ceil(5.2565 * sigma / ((hi - lo) / (h - 1)))
        if 1 <= R <= 2:
            return 'RBF_SCATTER', 'RBF_GATHER', 0, R
    mirrored = lo == -hi and h <= 64 and proj == RGBUV
    planes = False
    if method != THR and h <= 128:
        planes = {'1': True, '0': False}.get(bwd_planes, not mirrored)
    if planes:
        return 'DENSE', 'PLANES', -(-h // 32), 0
    return 'DENSE', ('MIRRORED' if mirrored else 'GENERIC'), 0, 0


def test_routes_of_the_gpu_parity_cases(L):
    """Every case of tests/test_hist_weight_grad_gpu.py::WANT, with and without the map's gradient, at its own shape."""
    from histogan_amd import hist as HH
    dense = {'dense fwd + k_hist_bwd': 'MIRRORED', 'dense fwd + k_hist_bwd (green)': 'MIRRORED',
             'dense fwd + k_hist_bwd_planes': 'PLANES', 'dense fwd + k_hist_bwd_generic': 'GENERIC'}
    assert sorted(WANT) == list(range(len(CASES)))
    for i, (proj, kw, shape, layout, pre_relu) in enumerate(CASES):
        cfg = HH.HistConfig(projection=proj, **kw)
        x = torch.empty(*shape)
        p, keep = HH._make_params(x, cfg, pre_relu, torch.empty(shape[0], shape[2], shape[3]))
        resized = p.resize_mode != NONE
        step = (cfg.hi - cfg.lo) / (cfg.h - 1)
        for wg in (0, 1):
            got = route(L, p, wg)
            if WANT[i] in dense:
                want = ('DENSE', dense[WANT[i]], -(-cfg.h // 32) if dense[WANT[i]] == 'PLANES' else 0, 0)
            elif WANT[i] == 'truncated RBF scatter / gather':
                want = ('RBF_SCATTER', 'RBF_GATHER', 0, math.ceil(5.2565 * cfg.sigma / step))
            elif WANT[i] == 'thresholding scatter / gather':
                want = ('THR_SCATTER', 'THR_GATHER', 0, 0)
            else:
                assert WANT[i] == 'lean scatter'
                bwd = 'THR_LEAN' if (cfg.intensity_scale or wg) else ('THR_GATHER' if resized else 'ZERO')
                want = ('THR_LEAN', bwd, 0, 0)
            assert got == want, (i, wg, got, want)
    # both ZERO cases of the list (OWN_CASES) and a resized lean case without intensity_scale (3) are in it
    assert [i for i, c in enumerate(CASES) if c[1].get('intensity_scale') is False and WANT[i] == 'lean scatter'] == [3, 16, 17]


PIN_EXTRA_WANT = [           # tests/test_hist_weight_gpu.py::GPU_PIN_EXTRA at 1 x 3 x 40 x 48 (no resize)
    ('DENSE', 'MIRRORED', 0, 0),
    ('DENSE', 'PLANES', 2, 0),
    ('DENSE', 'MIRRORED', 0, 0),            # 5.2565 * 0.5 / (6 / 31) = 13.6 bins: dense
    ('RBF_SCATTER', 'RBF_GATHER', 0, 2),    # 5.2565 * 0.02 / (6 / 63) = 1.10 bins
    ('DENSE', 'GENERIC', 0, 0),
    ('THR_SCATTER', 'THR_GATHER', 0, 0),    # spacing 2.5 / 15 < window 3.5 / 16
    ('THR_SCATTER', 'THR_GATHER', 0, 0),
]


def test_routes_of_the_extra_mask_pins(L):
    from histogan_amd import hist as HH
    assert len(PIN_EXTRA_WANT) == len(GPU_PIN_EXTRA)
    for (proj, kw), want in zip(GPU_PIN_EXTRA, PIN_EXTRA_WANT):
        p, keep = HH._make_params(torch.empty(1, 3, 40, 48), HH.HistConfig(projection=proj, **kw))
        assert route(L, p) == want, (kw, route(L, p), want)


def test_both_sides_of_every_threshold(L):
    r = lambda wg=0, **kw: route(L, params(L, **kw), wg)[:3]
    # lean: all three 64-bit grids in 150 KB -- 3 * 80^2 * 8 = 153 600 B is exactly 150 KB, so the last lean size is 80
    # (not 79, as the documents said before this test existed), 3 * 81^2 * 8 = 157 464 B
    assert 3 * 79 * 79 * 8 < 3 * 80 * 80 * 8 == 150 * 1024 < 3 * 81 * 81 * 8
    assert r(method=THR, h=79) == r(method=THR, h=80) == ('THR_LEAN', 'THR_LEAN', 0)
    assert r(method=THR, h=81) == ('THR_SCATTER', 'THR_GATHER', 0)
    # scatter: one grid in 156 KB = 159 744 B -- 141^2 * 8 = 159 048 B fits (the documents said 140), 142^2 * 8 = 161 312 B
    assert 140 * 140 * 8 < 141 * 141 * 8 <= 156 * 1024 < 142 * 142 * 8
    assert r(method=THR, h=140) == r(method=THR, h=141) == ('THR_SCATTER', 'THR_GATHER', 0)
    assert r(method=THR, h=142) == ('DENSE', 'GENERIC', 0)
    assert r(method=RBF, sigma=0.01, h=141)[0] == 'RBF_SCATTER' and r(method=RBF, sigma=0.01, h=142) == ('DENSE', 'GENERIC', 0)
    # k_hist_bwd up to one 64-bin block, the planes kernel up to 128, the generic one beyond
    assert r(h=64) == ('DENSE', 'MIRRORED', 0) and r(h=65) == ('DENSE', 'PLANES', 3)
    assert r(h=128) == ('DENSE', 'PLANES', 4) and r(h=129) == ('DENSE', 'GENERIC', 0)
    assert r(h=32, lo=-3.0, hi=1.0) == ('DENSE', 'PLANES', 1) and r(h=33, lo=-3.0, hi=1.0) == ('DENSE', 'PLANES', 2)
    assert r(h=64, proj=RGCHROMA, lo=0.0, hi=1.0) == ('DENSE', 'PLANES', 2) and r(h=64, green=1) == ('DENSE', 'MIRRORED', 0)
    # `single`: spacing (hi - lo) / (h - 1) against the window (|lo| + |hi|) / h
    assert (1.0 + 3.0) / 15 > (3.0 + 1.0) / 16 and (3.0 - 0.5) / 15 < (0.5 + 3.0) / 16
    assert r(method=THR, h=16, lo=-3.0, hi=1.0)[0] == 'THR_LEAN' and r(method=THR, h=16, lo=0.5, hi=3.0)[0] == 'THR_SCATTER'
    assert r(method=THR, h=1)[0] == 'THR_SCATTER'                            # no spacing at all
    assert r(method=THR, h=16, green=1)[0] == 'THR_SCATTER' and r(method=THR, h=16, proj=DIRECT, lo=0.0, hi=1.0)[0] == 'THR_SCATTER'


GRID = list(itertools.product((1, 2, 16, 32, 33, 40, 64, 65, 79, 80, 81, 96, 128, 129, 136, 140, 141, 142), (THR, RBF, IQ), (0.02, 0.05, 0.5), BOUNDS,
                              (RGBUV, RGCHROMA, DIRECT), (0, 1), (0, 1), (NONE, BILINEAR, SAMPLING)))


def test_the_whole_grid_follows_the_table(L):
    """The query against `model` over the grid; uses_proj_cache == (fwd == DENSE) == hg_rgbuv_hist_uses_proj_cache; ZERO
    exactly for lean thresholding without intensity_scale, without a resize and without weight_grad; the forward does not
    depend on weight_grad."""
    seen = set()
    for h, method, sigma, (lo, hi), proj, green, intensity, resize in GRID:
        if method == THR and sigma != 0.02:
            continue
        kw = dict(h=h, method=method, sigma=sigma, lo=lo, hi=hi, proj=proj, green=green, intensity=intensity, resize=resize)
        p = params(L, weight=(40 * 48, 48, 1), **kw)
        for wg in (0, 1):
            r = L.hist_route(p, wg)
            got = route(L, p, wg)
            assert got == model(weight_grad=wg, **kw), (kw, wg, got)
            assert r.uses_proj_cache == (got[0] == 'DENSE') == L.lib.hg_rgbuv_hist_uses_proj_cache(ctypes.byref(p))
            lean = got[0] == 'THR_LEAN'
            assert (got[1] == 'ZERO') == (lean and not intensity and resize == NONE and not wg)
            assert (r.bwd_workgroups == 0) == (got[1] == 'ZERO') and r.fwd_slices >= 1
            seen.add(got[:2])
        assert route(L, p, 0)[0] == route(L, p, 1)[0]
    assert len({f for f, _ in seen}) == 4 and len({b for _, b in seen}) == 7       # every family was reached


def test_the_three_switches_move_the_route_as_documented(L, monkeypatch):
    for name in ('HG_RBF_DENSE', 'HG_THR_EXACT', 'HG_BWD_PLANES'):
        monkeypatch.delenv(name, raising=False)
    narrow = params(L, method=RBF, sigma=0.02, h=64)
    sym64, asym40, h136 = params(L, h=64), params(L, h=40, lo=-3.0, hi=1.0), params(L, h=136)
    lean = params(L, method=THR, h=64)
    assert route(L, narrow) == ('RBF_SCATTER', 'RBF_GATHER', 0, 2)
    monkeypatch.setenv('HG_RBF_DENSE', '1')                      # read on every call: no reload
    assert route(L, narrow) == ('DENSE', 'MIRRORED', 0, 0)
    monkeypatch.setenv('HG_RBF_DENSE', '0')
    assert route(L, narrow) == ('RBF_SCATTER', 'RBF_GATHER', 0, 2)
    monkeypatch.delenv('HG_RBF_DENSE')
    # three states: unset, 1 = force, 0 = forbid; never beyond h = 128, never for the scatter routes
    assert route(L, sym64) == ('DENSE', 'MIRRORED', 0, 0) and route(L, asym40) == ('DENSE', 'PLANES', 2, 0)
    monkeypatch.setenv('HG_BWD_PLANES', '1')
    assert route(L, sym64) == ('DENSE', 'PLANES', 2, 0) and route(L, asym40) == ('DENSE', 'PLANES', 2, 0)
    assert route(L, h136) == ('DENSE', 'GENERIC', 0, 0) and route(L, lean)[:2] == ('THR_LEAN', 'THR_LEAN')
    monkeypatch.setenv('HG_BWD_PLANES', '0')
    assert route(L, sym64) == ('DENSE', 'MIRRORED', 0, 0) and route(L, asym40) == ('DENSE', 'GENERIC', 0, 0)
    monkeypatch.setenv('HG_BWD_PLANES', '2')                     # neither: as unset
    assert route(L, sym64) == ('DENSE', 'MIRRORED', 0, 0) and route(L, asym40) == ('DENSE', 'PLANES', 2, 0)
    monkeypatch.delenv('HG_BWD_PLANES')
    # HG_THR_EXACT picks the classification inside the lean kernels, not the route; every workspace size stays
    # (the flag itself, Route::exact_only, is not part of hg_hist_route: that make_route still READS the switch is only shown
    # on the GPU, by the A/B parity of tests/test_hist_gpu.py::test_fast_window_classification_is_exact)
    f0, b0, f1, b1 = (ctypes.c_size_t() for _ in range(4))
    assert L.lib.hg_rgbuv_hist_workspace_bytes(ctypes.byref(lean), ctypes.byref(f0), ctypes.byref(b0)) == 0
    before = route(L, lean)
    monkeypatch.setenv('HG_THR_EXACT', '1')
    assert route(L, lean) == before == ('THR_LEAN', 'THR_LEAN', 0, 0)
    assert L.lib.hg_rgbuv_hist_workspace_bytes(ctypes.byref(lean), ctypes.byref(f1), ctypes.byref(b1)) == 0
    assert (f0.value, b0.value) == (f1.value, b1.value)
    # the whole grid under the two route-moving switches
    for rbf_dense, bwd_planes in (('1', None), (None, '1'), (None, '0')):
        for name, v in (('HG_RBF_DENSE', rbf_dense), ('HG_BWD_PLANES', bwd_planes)):
            monkeypatch.setenv(name, v) if v is not None else monkeypatch.delenv(name, raising=False)
        for h, method, sigma, (lo, hi), proj, green, intensity, resize in GRID[::7]:
            kw = dict(h=h, method=method, sigma=sigma, lo=lo, hi=hi, proj=proj, green=green, intensity=intensity, resize=resize)
            assert route(L, params(L, **kw)) == model(weight_grad=0, rbf_dense=rbf_dense, bwd_planes=bwd_planes, **kw), kw


def test_route_answers_size_the_workspaces_consistently(L):
    """fwd_slices is the S of the forward workspace: slab_tot [B][S * nbd^2] fp64 and slabs [B][S][P h^2] fp32, each rounded
    up to 256 bytes."""
    up = lambda n: (n + 255) // 256 * 256
    for kw in (dict(h=64, H=150, W=150), dict(h=64, method=THR, H=150, W=150), dict(h=96, H=41, W=45),
               dict(h=16, method=RBF, sigma=0.05, green=1), dict(h=33, proj=DIRECT, lo=0.0, hi=1.0, resize=BILINEAR)):
        p = params(L, **kw)
        r = L.hist_route(p)
        f = ctypes.c_size_t()
        assert L.lib.hg_rgbuv_hist_workspace_bytes(ctypes.byref(p), ctypes.byref(f), None) == 0
        planes = 1 if (p.green_only or p.projection) else 3
        nbd = -(-p.h // (32 if p.h <= 32 else 64))
        assert f.value == up(p.B * r.fwd_slices * nbd * nbd * 8) + up(p.B * r.fwd_slices * planes * p.h * p.h * 4), kw
    assert L.hist_route(params(L, h=64, H=150, W=150)).fwd_slices >= 2


def test_refusals(L):
    R = L.HgHistRoute
    q = lambda p, wg, out: L.lib.hg_rgbuv_hist_route(None if p is None else ctypes.byref(p), wg, None if out is None else ctypes.byref(out))
    out = R(struct_size=ctypes.sizeof(R))
    assert L.lib.hg_version() >= 106 and ctypes.sizeof(R) == 32
    assert q(params(L), 0, out) == 0
    assert q(None, 0, out) == -1 and q(params(L), 0, None) == -1
    stale = params(L)
    stale.struct_size -= 8
    assert q(stale, 0, out) == -1
    assert q(params(L), 0, R(struct_size=0)) == -1 and q(params(L), 0, R(struct_size=ctypes.sizeof(R) + 4)) == -1
    assert q(params(L, method=7), 0, out) == -2 and q(params(L, resize=9), 0, out) == -3
    # weight_grad validates like hg_rgbuv_hist_bwd_w: a map is required and must own every element
    own, bcast = params(L, weight=(40 * 48, 48, 1)), params(L, weight=(0, 48, 1))
    n = ctypes.c_size_t()
    assert q(params(L), 1, out) == -1 == L.lib.hg_rgbuv_hist_bwd_w_workspace_bytes(ctypes.byref(params(L)), ctypes.byref(n))
    assert q(bcast, 1, out) == -5 == L.lib.hg_rgbuv_hist_bwd_w_workspace_bytes(ctypes.byref(bcast), ctypes.byref(n))
    assert q(bcast, 0, out) == 0 and q(own, 1, out) == 0
