"""Per-pixel weighted (masked) histograms on the HIP kernels (hg_hist_params.weight, include/hg_hist.h).

The same pins as tests/test_hist_weight_cpu.py, through every kernel family the dispatcher of hg_hist.hip can take, under
the bars tests/test_hist_gpu.py applies to the unweighted kernels (forward 1e-5, gradient 1e-4, max-norm relative):
binary mask == the oracle on the selected pixels (reference arithmetic), the Lab block's fractional-weight pin, a
double-precision statement of the definition for fractional weights and resizing, and the exactness properties
(ones == None bit for bit, zero weight, clamping, repeatability).  Which family a case runs on is asserted through the
library's own queries, so a case cannot pass on the wrong path.

HG_WEIGHT_PARITY_JSON=<path>: the worst measured errors per kernel family are written there after the assertions."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import test_hist_weight_cpu as C
from conftest import relmax
from hist_weight_ref import (BWD_TOL, FWD_TOL, gather_selected, make_block, oracle_hist, random_mask, sample_image)

pytestmark = pytest.mark.gpu

RECORD = {}


def _note(family, e_f, e_b):
    r = RECORD.setdefault(family, {'forward': 0.0, 'gradient': 0.0, 'cases': 0})
    r['forward'], r['gradient'], r['cases'] = max(r['forward'], e_f), max(r['gradient'], e_b), r['cases'] + 1


@pytest.fixture(scope='module', autouse=True)
def _parity_record():
    yield
    path = os.environ.get('HG_WEIGHT_PARITY_JSON')
    if path and RECORD:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        try:
            head = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=root, capture_output=True, text=True).stdout.strip()
        except OSError:
            head = ''
        with open(path, 'w') as f:
            json.dump({'what': 'weighted histogram: worst max-norm relative error per kernel family (tests/test_hist_weight_gpu.py)',
                       'bars': {'forward': FWD_TOL, 'gradient': BWD_TOL}, 'commit': head or os.environ.get('HG_COMMIT', ''),
                       'families': RECORD}, f, indent=1, sort_keys=True)


def family(x, proj, kw):
    """The kernel family hg_hist.hip dispatches (x, block) to, as the library itself answers (hg_rgbuv_hist_route: the
    decision its launches and workspace sizes are made from).  Returns (label, forward split-K slices)."""
    from histogan_amd import hist as HH
    from histogan_amd._lib import HG_ROUTE_BWD, HG_ROUTE_FWD, hist_route, lib
    cfg = HH.HistConfig(projection=proj, **{k: (list(v) if k == 'hist_boundary' else v) for k, v in kw.items()})
    p, keep = HH._make_params(x, cfg)
    r = hist_route(p)
    assert r.uses_proj_cache == lib.hg_rgbuv_hist_uses_proj_cache(ctypes.byref(p))
    fwd, bwd = HG_ROUTE_FWD[r.fwd], HG_ROUTE_BWD[r.bwd]
    if fwd == 'DENSE':
        label = {'MIRRORED': 'dense fwd + k_hist_bwd' + (' (green)' if cfg.green_only else ''),
                 'PLANES': 'dense fwd + k_hist_bwd_planes', 'GENERIC': 'dense fwd + k_hist_bwd_generic'}[bwd]
    else:
        label = {'RBF_SCATTER': 'truncated RBF scatter / gather', 'THR_LEAN': 'lean scatter',
                 'THR_SCATTER': 'thresholding scatter / gather'}[fwd]
    return label, r.fwd_slices


GPU_PIN_EXTRA = [
    ('rgbuv', dict(method='inverse-quadratic', sigma=0.02, h=64, insz=64)),                        # T = 2, shared reciprocals
    ('rgbuv', dict(method='inverse-quadratic', sigma=0.02, h=40, insz=64, hist_boundary=[-3.0, 1.0])),   # planes, 3 planes
    ('rgbuv', dict(method='RBF', sigma=0.5, h=32, insz=64)),                                       # wide RBF: dense
    ('rgbuv', dict(method='RBF', sigma=0.02, h=64, insz=64)),                                      # default sigma: radius 1
    ('rgbuv', dict(method='inverse-quadratic', sigma=0.05, h=136, insz=64)),                       # beyond the MFMA backward
    ('rgbuv', dict(method='thresholding', h=16, insz=64, hist_boundary=[0.5, 3.0])),               # two bins can hit
    ('rgbuv', dict(method='thresholding', h=128, insz=64, green_only=True)),
]


@pytest.mark.parametrize('proj,kw', C.PIN_CASES + GPU_PIN_EXTRA)
def test_binary_mask_equals_oracle_on_the_selected_pixels(proj, kw, gpu_device):
    fam, _ = family(torch.empty(1, 3, 40, 48, device=gpu_device), proj, kw)
    e_f, e_b, outside = C.pin_binary_mask(proj, kw, gpu_device)
    print(f'mask pin [{fam}] {proj} {kw}: fwd {e_f:.2e} grad {e_b:.2e}')
    assert e_f <= FWD_TOL and e_b <= BWD_TOL
    assert outside == 0.0
    _note(fam, e_f, e_b)


@pytest.mark.parametrize('method,want,min_slices', [('inverse-quadratic', 'dense fwd + k_hist_bwd', 2), ('thresholding', 'lean scatter', 1)])
def test_binary_mask_at_a_size_that_splits_the_pixels(method, want, min_slices, gpu_device):
    """2 x 3 x 150 x 150, h = 64, a different mask per image: the dense MFMA kernels with several split-K slices per
    image, and the lean scatter kernels (three planes, 16-byte loads of image and weight map)."""
    kw = dict(method=method, sigma=0.02, h=64, insz=150)
    g = torch.Generator().manual_seed(21)
    x = sample_image(2, 3, 150, 150, g)
    a, b = 100, 120
    mask = random_mask(2, 150, 150, a * b, g)
    fam, slices = family(x.to(gpu_device), 'rgbuv', kw)
    assert fam == want and slices >= min_slices, (fam, slices)
    blk = make_block('rgbuv', gpu_device, **kw)
    xg = x.clone().to(gpu_device).requires_grad_(True)
    out = blk(xg, weight=mask.to(gpu_device))
    go = torch.randn(out.shape, generator=g)
    out.backward(go.to(gpu_device))
    xo = gather_selected(x, mask, a, b).detach().clone().requires_grad_(True)
    ref = oracle_hist(xo, 'rgbuv', **kw)
    ref.backward(go)
    gx = xg.grad.cpu()
    e_f = relmax(out.detach().cpu().numpy(), ref.detach().numpy())
    e_b = relmax(gather_selected(gx, mask, a, b).numpy(), xo.grad.numpy())
    print(f'mask pin 2x3x150x150 [{fam}, {slices} slices]: fwd {e_f:.2e} grad {e_b:.2e}')
    assert e_f <= FWD_TOL and e_b <= BWD_TOL
    assert float((gx * (1 - mask).unsqueeze(1)).abs().max()) == 0.0 and torch.isfinite(gx).all()
    _note(fam + ' (150 x 150)', e_f, e_b)


@pytest.mark.parametrize('method,mkw', C.METHODS)
def test_lab_block_fractional_weight_equals_oracle_on_scaled_channel0(method, mkw, gpu_device):
    e_f, e_b = C.pin_lab_fractional(method, mkw, gpu_device)
    print(f'lab pin {method}: fwd {e_f:.2e} grad {e_b:.2e}')
    assert e_f <= FWD_TOL and e_b <= BWD_TOL
    fam, _ = family(torch.empty(2, 3, 36, 44, device=gpu_device), 'direct', dict(method=method, intensity_scale=True, h=16, insz=64, **mkw))
    _note(fam + ' (Lab pin)', e_f, e_b)


GPU_DEF_EXTRA = [
    ('rgbuv', dict(h=64, insz=48, resizing='interpolation', method='inverse-quadratic', sigma=0.02), (3, 3, 96, 72), 'strided', True),
    ('rgbuv', dict(h=64, insz=150, method='thresholding'), (2, 3, 64, 64), 'strided', False),       # lean, strided map: sampled loads
    ('rgbuv', dict(h=64, insz=150, method='thresholding'), (2, 4, 64, 64), 'bhw', True),            # lean, 16-byte loads, C = 4
    ('rgbuv', dict(h=136, insz=24, resizing='interpolation', method='inverse-quadratic', sigma=0.05), (2, 3, 40, 56), 'bhw', False),
    ('rgbuv', dict(h=96, insz=32, resizing='interpolation', method='inverse-quadratic', sigma=0.03), (2, 3, 40, 56), 'b1hw', False),
    ('rgbuv', dict(h=64, insz=40, resizing='interpolation', method='RBF', sigma=0.02), (2, 3, 64, 48), 'bhw', False),
]


# three planes whose LDS grids do not fit together (h = 81): the plane-after-plane branch of the scatter forwards.  A list of
# its own, appended after every other: the case indices of tests/test_hist_weight_grad_gpu.py stay what they were.
GPU_DEF_PLANES = [
    ('rgbuv', dict(h=81, insz=64, method='thresholding'), (2, 3, 24, 28), 'bhw', False),
    ('rgbuv', dict(h=81, insz=64, method='RBF', sigma=0.02), (2, 3, 24, 28), 'bhw', False),
]


@pytest.mark.parametrize('proj,kw,shape,layout,pre_relu', C.DEF_CASES + GPU_DEF_EXTRA + GPU_DEF_PLANES)
def test_fractional_weights_and_resizing_match_the_definition(proj, kw, shape, layout, pre_relu, gpu_device):
    fam, _ = family(torch.empty(*shape, device=gpu_device), proj, kw)
    e_f, e_b = C.check_definition(proj, kw, shape, layout, pre_relu, gpu_device)
    print(f'definition [{fam}] {proj} {kw} {shape} {layout}: fwd {e_f:.2e} grad {e_b:.2e}')
    assert e_f <= FWD_TOL and e_b <= BWD_TOL
    _note(fam + ' (fractional / resized)', e_f, e_b)


EXACT_CASES = [
    ('rgbuv', dict(h=64, insz=150, method='inverse-quadratic'), (2, 3, 64, 64)),                                   # k_hist_fwd / k_hist_bwd, shared reciprocals
    ('rgbuv', dict(h=32, insz=32, resizing='interpolation', method='inverse-quadratic', sigma=0.05), (2, 3, 48, 56)),
    ('rgbuv', dict(h=32, insz=64, method='RBF', sigma=0.4, green_only=True), (2, 3, 40, 48)),
    ('rgbuv', dict(h=40, insz=64, method='inverse-quadratic', hist_boundary=[-3.0, 1.0]), (2, 4, 40, 48)),         # k_hist_bwd_planes
    ('rgchroma', dict(h=32, insz=24, resizing='sampling', method='inverse-quadratic', intensity_scale=True), (2, 3, 40, 56)),
    ('direct', dict(h=16, insz=64, method='RBF', sigma=0.3, intensity_scale=True), (2, 3, 40, 48)),
    ('rgbuv', dict(h=136, insz=64, method='inverse-quadratic', sigma=0.05), (1, 3, 24, 32)),                       # k_hist_bwd_generic
    ('rgbuv', dict(h=64, insz=150, method='thresholding'), (2, 3, 64, 64)),                                        # lean, 16-byte loads
    ('rgbuv', dict(h=64, insz=48, resizing='interpolation', method='thresholding'), (2, 3, 72, 96)),               # lean, sampled
    ('rgbuv', dict(h=32, insz=64, method='thresholding', green_only=True), (2, 3, 40, 48)),                        # k_hist_thr_fwd / _bwd
    ('direct', dict(h=16, insz=64, method='thresholding', intensity_scale=True), (2, 3, 40, 48)),
    ('rgbuv', dict(h=64, insz=64, method='RBF', sigma=0.02), (2, 3, 40, 48)),                                      # k_hist_rbf_fwd / _bwd
]


@pytest.mark.parametrize('proj,kw,shape', EXACT_CASES)
def test_exactness_properties(proj, kw, shape, gpu_device):
    """Equalities, not tolerances: weight=ones is weight=None bit for bit (forward and gradient) -- with the untouched
    unweighted tests this is what shows the unweighted path did not move; an all-zero map gives an all-zero histogram and
    an all-zero finite gradient; values outside [0, 1] behave as clamped; a weighted call repeats bit for bit.
    (The bilinear cases resize by 3/2, 7/4 and 2: the taps' lambdas are then exact in fp32 and the resized map of ones is
    exactly 1.  At other scales the definition's fp32 fma form gives 1 +- 1 ulp -- as aten does for a constant image --
    and ones == None holds to that ulp only: test_ones_under_an_inexact_bilinear_scale.)"""
    g = torch.Generator().manual_seed(4)
    x = sample_image(*shape, g)
    B, _, H, W = shape
    blk = make_block(proj, gpu_device, **kw)
    go = None

    def run(weight):
        nonlocal go
        xr = x.clone().to(gpu_device).requires_grad_(True)
        out = blk(xr) if weight is None else blk(xr, weight=weight.to(gpu_device))
        if go is None:
            go = torch.randn(out.shape, generator=torch.Generator().manual_seed(8)).to(gpu_device)
        out.backward(go)
        return out.detach().clone(), xr.grad.clone()

    h0, g0 = run(None)
    h1, g1 = run(torch.ones(B, H, W))
    assert torch.equal(h0, h1) and torch.equal(g0, g1)
    hz, gz = run(torch.zeros(B, 1, H, W))
    assert float(hz.abs().max()) == 0.0 and float(gz.abs().max()) == 0.0 and bool(torch.isfinite(gz).all())
    w = torch.rand(B, H, W, generator=g) * 3 - 1
    ha, ga = run(w)
    hb, gb = run(w.clamp(0, 1))
    assert torch.equal(ha, hb) and torch.equal(ga, gb)
    hc, gc = run(w)                                                     # repeat run: bit-identical
    assert torch.equal(ha, hc) and torch.equal(ga, gc)
    if H <= kw['insz'] and W <= kw['insz']:                             # no resize: w_n == 0 means exactly no gradient
        assert float((ga * (w.clamp(0, 1) == 0).unsqueeze(1).to(gpu_device)).abs().max()) == 0.0


@pytest.mark.parametrize('method', ['inverse-quadratic', 'thresholding'])
def test_ones_under_an_inexact_bilinear_scale(method, gpu_device):
    """64 x 80 -> 48 x 48 (scales 4/3 and 5/3): the map of ones is resized like a colour channel, four products and three
    fma roundings per pixel, so w_n = 1 + d with |d| <= 7 * 2^-24 = 4.2e-7.  The raw histogram and its sum are linear in
    the weights, so every normalised bin moves by at most 2 * 4.2e-7 relative: bound 1e-6 on the forward (max-norm); the
    gradient is held to the gradient bar.  Found when the exactness test above first used this shape."""
    g = torch.Generator().manual_seed(4)
    x = sample_image(2, 3, 64, 80, g)
    blk = make_block('rgbuv', gpu_device, h=64, insz=48, resizing='interpolation', method=method)
    res = []
    for w in (None, torch.ones(2, 64, 80, device=gpu_device)):
        xr = x.clone().to(gpu_device).requires_grad_(True)
        out = blk(xr) if w is None else blk(xr, weight=w)
        out.backward(torch.linspace(-1, 1, 64, device=gpu_device).expand_as(out))
        res.append((out.detach().cpu().numpy(), xr.grad.cpu().numpy()))
    e_f, e_b = relmax(res[1][0], res[0][0]), relmax(res[1][1], res[0][1])
    print(f'ones vs None, inexact bilinear scale, {method}: fwd {e_f:.2e} grad {e_b:.2e}')
    assert e_f <= 1e-6 and e_b <= BWD_TOL


def test_weight_argument_errors_and_device_handling(gpu_device):
    x = torch.rand(2, 3, 20, 24, device=gpu_device)
    for proj in ('rgbuv', 'rgchroma', 'direct'):
        blk = make_block(proj, gpu_device, h=8, insz=32)
        with pytest.raises(ValueError, match='requires grad'):
            blk(x, weight=torch.rand(2, 20, 24, device=gpu_device, requires_grad=True))
        for bad in (torch.rand(2, 24, 20), torch.rand(1, 20, 24), torch.rand(2, 3, 20, 24), torch.rand(20, 24)):
            with pytest.raises(ValueError, match='weight must have shape'):
                blk(x, weight=bad.to(gpu_device))
    blk = make_block('rgbuv', 'cuda', h=8, insz=32)
    w = torch.rand(2, 20, 24)
    ref = blk(x, weight=w.to(gpu_device))
    assert torch.equal(blk(x.cpu(), weight=w), ref)                    # CPU x and CPU map are moved like x
    assert torch.equal(blk(x, weight=w), ref)                          # a CPU map follows a GPU x
    assert torch.equal(blk(x, weight=w.double().to(gpu_device)), ref)  # other float types are converted
    from histogan_amd.hist import HistConfig, rgbuv_hist
    assert torch.equal(rgbuv_hist(x, HistConfig(h=8, insz=32), False, w.to(gpu_device)), ref)


@pytest.mark.parametrize('method', ['inverse-quadratic', 'thresholding'])
def test_abi_null_weight_ignores_strides_and_zero_stride_broadcasts(method, gpu_device):
    """include/hg_hist.h: NULL weight = no map whatever the strides say; a stride of 0 broadcasts (one map for the batch)."""
    from histogan_amd import hist as HH
    from histogan_amd._lib import check, lib
    g = torch.Generator().manual_seed(6)
    x = sample_image(4, 3, 32, 40, g).to(gpu_device)
    cfg = HH.HistConfig(h=32, insz=64, method=method)
    blk = make_block('rgbuv', gpu_device, h=32, insz=64, method=method)
    p, keep = HH._make_params(x, cfg)
    p.weight, p.weight_stride_b, p.weight_stride_h, p.weight_stride_w = None, -(1 << 40), 12345, -7
    fwd_b, _ = HH._ws_bytes(p)
    out, sums = torch.empty(4, 3, 32, 32, device=gpu_device), torch.empty(4, device=gpu_device)
    ws = torch.empty(max(fwd_b, 4), dtype=torch.uint8, device=gpu_device)
    check(lib.hg_rgbuv_hist_fwd(ctypes.byref(p), x.data_ptr(), out.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                HH._stream(x.device)), 'fwd')
    assert torch.equal(out, blk(x))
    w1 = torch.rand(1, 32, 40, generator=g).to(gpu_device)
    wb = w1.expand(4, 32, 40)
    assert wb.stride(0) == 0
    res = []
    for w in (wb, wb.contiguous()):
        xr = x.clone().requires_grad_(True)
        o = blk(xr, weight=w)
        o.backward(torch.ones_like(o) * torch.linspace(-1, 1, 32, device=gpu_device))
        res.append((o.detach(), xr.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][0], blk(x))
