"""Differentiable weight maps (`weight_grad=True`) on the HIP kernels: hg_rgbuv_hist_bwd_w (include/hg_hist.h).

The map's gradient of every backward family of hg_hist.hip against the double-precision definition
(tests/hist_weight_ref.py::definition, differentiated with respect to w) under the project's gradient bar BWD_TOL = 1e-4,
max-norm relative; x.grad bit-equal to the same call with a detached map; exact zeros under the clamp's mask (rows at -0.3
and 1.4 in every map); repeatability; map layouts; the trainer's hist_alpha_grad.  Which family a case runs on is asserted
through the dispatcher's own answers (test_hist_weight_gpu.family).

HG_WEIGHT_PARITY_JSON=<path>: the worst measured error per kernel family is written there after the assertions."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import test_hist_weight_grad_cpu as WC
from conftest import relmax
from hist_weight_ref import BWD_TOL, make_block, sample_image
from test_hist_weight_cpu import DEF_CASES
from test_hist_weight_gpu import EXACT_CASES, GPU_DEF_EXTRA, GPU_DEF_PLANES, family

pytestmark = pytest.mark.gpu

RECORD = {}


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
            json.dump({'what': 'gradient of the weight map: worst max-norm relative error per kernel family against the fp64 '
                               'definition (tests/test_hist_weight_grad_gpu.py)',
                       'bars': {'weight_gradient': BWD_TOL}, 'commit': head or os.environ.get('HG_COMMIT', ''),
                       'families': RECORD}, f, indent=1, sort_keys=True)


def _note(fam, e):
    r = RECORD.setdefault(fam, {'weight_gradient': 0.0, 'cases': 0})
    r['weight_gradient'], r['cases'] = max(r['weight_gradient'], e), r['cases'] + 1


# on top of the shared lists: thresholding without intensity_scale and without a resize -- the backward that is a plain
# clear of grad_x for a constant map (lean, 16-byte loads) -- and the same through sampled loads (an odd pixel count)
OWN_CASES = [
    ('rgbuv', dict(h=16, insz=64, method='thresholding', intensity_scale=False), (2, 3, 40, 48), 'bhw', False),
    ('rgbuv', dict(h=16, insz=64, method='thresholding', intensity_scale=False), (2, 3, 41, 45), 'b1hw', True),
]
CASES = DEF_CASES + GPU_DEF_EXTRA + OWN_CASES + GPU_DEF_PLANES
WANT = {           # case index -> the family it must run on: every backward family at least once
    0: 'dense fwd + k_hist_bwd',                # T = 1, bilinear
    1: 'dense fwd + k_hist_bwd',                # T = 1, sampling, C = 4
    2: 'lean scatter',                          # bilinear
    3: 'lean scatter',                          # sampling, no intensity_scale
    4: 'truncated RBF scatter / gather',
    5: 'dense fwd + k_hist_bwd_planes',         # three planes, asymmetric boundary
    6: 'dense fwd + k_hist_bwd (green)',
    7: 'dense fwd + k_hist_bwd_planes',         # rg-chroma
    8: 'dense fwd + k_hist_bwd_planes',         # Lab, sampling
    9: 'thresholding scatter / gather',         # Lab, no intensity_scale
    10: 'dense fwd + k_hist_bwd',               # T = 2, shared reciprocals
    11: 'lean scatter',                         # strided map: sampled loads
    12: 'lean scatter',                         # 16-byte loads, C = 4
    13: 'dense fwd + k_hist_bwd_generic',       # h = 136
    14: 'dense fwd + k_hist_bwd_planes',        # h = 96
    15: 'truncated RBF scatter / gather',       # bilinear
    16: 'lean scatter',
    17: 'lean scatter',
    18: 'thresholding scatter / gather',        # h = 81, three planes: plane-after-plane forward
    19: 'truncated RBF scatter / gather',       # h = 81, three planes, radius 2
}


@pytest.mark.parametrize('i', range(len(CASES)))
def test_weight_gradient_matches_the_definition(i, gpu_device):
    proj, kw, shape, layout, pre_relu = CASES[i]
    fam, _ = family(torch.empty(*shape, device=gpu_device), proj, kw)
    assert fam == WANT[i], (i, fam)
    e, gref, gw, gx = WC.check_weight_grad(proj, kw, shape, layout, pre_relu, gpu_device)
    print(f'weight gradient [{fam}] {proj} {kw} {shape} {layout}: {e:.2e}')
    if kw.get('method') == 'thresholding' and kw.get('intensity_scale') is False:
        assert float(gx.abs().max()) == 0.0 and float(gw.abs().max()) > 0.0            # no colour gradient, a map gradient
    assert e <= BWD_TOL
    _note(fam, e)


@pytest.mark.parametrize('method,want,min_slices', [('inverse-quadratic', 'dense fwd + k_hist_bwd', 2), ('thresholding', 'lean scatter', 1)])
def test_weight_gradient_at_a_size_that_splits_the_pixels(method, want, min_slices, gpu_device):
    """2 x 3 x 150 x 150, h = 64, a fractional map: several split-K slices / backward workgroups per image on the dense
    path, the 16-byte loads and stores of the lean scatter path."""
    kw = dict(method=method, sigma=0.02, h=64, insz=150)
    shape = (2, 3, 150, 150)
    fam, slices = family(torch.empty(*shape, device=gpu_device), 'rgbuv', kw)
    assert fam == want and slices >= min_slices, (fam, slices)
    e, gref, gw, gx = WC.check_weight_grad('rgbuv', kw, shape, 'bhw', False, gpu_device, seed=21)
    print(f'weight gradient 2x3x150x150 [{fam}, {slices} slices]: {e:.2e}')
    assert e <= BWD_TOL
    _note(fam + ' (150 x 150)', e)


@pytest.mark.parametrize('proj,kw,shape,binary', [
    ('rgbuv', dict(h=64, insz=150, method='inverse-quadratic'), (2, 3, 64, 64), True),
    ('rgbuv', dict(h=64, insz=150, method='thresholding'), (2, 3, 64, 64), True),
    ('rgbuv', dict(h=32, insz=32, resizing='interpolation', method='inverse-quadratic', sigma=0.05), (2, 3, 48, 56), False),
    ('direct', dict(h=16, insz=64, method='RBF', sigma=0.3, intensity_scale=True), (2, 3, 40, 48), False),
])
def test_scaling_the_whole_map_changes_nothing(proj, kw, shape, binary, gpu_device):
    """No reference needed: the normalised histogram is invariant to scaling the whole map (up to the 1e-6 in the
    normaliser), so sum_n w_n dL/dw_n ~ 0 -- held relative to sum_n |w_n dL/dw_n| under the gradient bar.  (The resize is
    linear in the map, so this holds at the input resolution as long as the map stays inside the clamp.)"""
    g = torch.Generator().manual_seed(13)
    x = sample_image(*shape, g).to(gpu_device)
    B, _, H, W = shape
    w = torch.rand(B, H, W, generator=g)
    w = (w > 0.4).float() if binary else 0.05 + 0.9 * w
    wd = w.to(gpu_device).requires_grad_(True)
    out = make_block(proj, gpu_device, **kw)(x, weight=wd, weight_grad=True)
    out.backward(torch.randn(out.shape, generator=g).to(gpu_device))
    t = (wd.detach() * wd.grad).double()
    num, den = float(t.sum().abs()), float(t.abs().sum())
    print(f'scale invariance {proj} {kw}: |sum| {num:.3e} of {den:.3e}')
    assert den > 0 and num <= BWD_TOL * den
    if binary:                                                          # unselected pixels have a gradient too (Iy_n A_n)
        assert float((wd.grad * (1 - wd.detach())).abs().max()) > 0.0


@pytest.mark.parametrize('proj,kw,shape', [c for c in EXACT_CASES if c[1].get('resizing') != 'sampling'])
def test_weight_gradient_repeats_bit_for_bit(proj, kw, shape, gpu_device):
    """No resize and the bilinear adjoint (a gather) are deterministic; the sampling adjoint's atomics are exempt, as they
    are for grad_x."""
    g = torch.Generator().manual_seed(4)
    x = sample_image(*shape, g).to(gpu_device)
    B, _, H, W = shape
    w = (torch.rand(B, H, W, generator=g) * 1.6 - 0.3).to(gpu_device)
    blk = make_block(proj, gpu_device, **kw)
    res = []
    for _ in range(2):
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        out = blk(xr, weight=wr, weight_grad=True)
        out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(8)).to(gpu_device))
        res.append((out.detach(), xr.grad, wr.grad))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    outside = ((w < 0) | (w > 1))
    assert bool(outside.any()) and float((res[0][2] * outside).abs().max()) == 0.0
    assert bool(torch.isfinite(res[0][2]).all()) and float(res[0][2].abs().max()) > 0.0


@pytest.mark.parametrize('method', ['inverse-quadratic', 'thresholding'])
def test_map_expanded_over_the_batch(method, gpu_device):
    """One (1, H, W) leaf expanded to the batch (stride 0): the C ABI refuses a broadcast map, so the binding materialises
    it and autograd reduces the gradient to the leaf.  Held elementwise against the fp64 batch sum of the gradient a
    contiguous copy of the map gets: an fp32 sum of four terms in any order is within 3 roundings of it, each at most
    2^-24 of sum |terms| (4 * 2^-24 asserted, one more for the final rounding of the fp64 value)."""
    g = torch.Generator().manual_seed(6)
    x = sample_image(4, 3, 32, 40, g).to(gpu_device)
    blk = make_block('rgbuv', gpu_device, h=32, insz=64, method=method)
    w1 = torch.rand(1, 32, 40, generator=g).to(gpu_device).requires_grad_(True)
    wb = w1.expand(4, 32, 40)
    assert wb.stride(0) == 0
    wc = wb.detach().contiguous().requires_grad_(True)
    go = torch.randn(4, 3, 32, 32, generator=g).to(gpu_device)
    blk(x, weight=wb, weight_grad=True).backward(go)
    blk(x, weight=wc, weight_grad=True).backward(go)
    assert w1.grad.shape == (1, 32, 40) and wc.grad.shape == (4, 32, 40)
    ref, mag = wc.grad.double().sum(dim=0, keepdim=True), wc.grad.double().abs().sum(dim=0, keepdim=True)
    assert float(mag.max()) > 0.0
    assert bool(((w1.grad.double() - ref).abs() <= 4 * 2.0 ** -24 * mag).all())


def test_c_abi_refuses_what_the_binding_materialises(gpu_device):
    import ctypes
    from histogan_amd import hist as HH
    from histogan_amd._lib import lib
    x = torch.rand(2, 3, 16, 16, device=gpu_device)
    w = torch.rand(1, 16, 16, device=gpu_device).expand(2, 16, 16)
    p, keep = HH._make_params(x, HH.HistConfig(h=16, insz=32), False, w)
    n = ctypes.c_size_t()
    assert lib.hg_rgbuv_hist_bwd_w_workspace_bytes(ctypes.byref(p), ctypes.byref(n)) == -5
    a = x.data_ptr()
    assert lib.hg_rgbuv_hist_bwd_w(ctypes.byref(p), a, a, a, a, a, a, a, 1 << 20, None) == -5


def test_trainer_steps_with_a_differentiable_alpha(gpu_device, tmp_path):
    from histoGAN import Trainer
    tr = Trainer('rgbawg', str(tmp_path / 'r'), str(tmp_path / 'm'), 32, 2, transparent=True, batch_size=2, hist_bin=16,
                 hist_insz=32, hist_alpha_weight=True, hist_alpha_grad=True)
    assert tr.hist_alpha_weight is True and tr.hist_alpha_grad is True
    tr.run_evaluate = tr.run_save = False
    tr.set_synthetic_data_src()
    for _ in range(3):
        tr.train(alpha=2)
    assert np.isfinite(tr.d_loss) and np.isfinite(tr.g_loss) and np.isfinite(tr.h_loss)


def test_histogram_loss_reaches_the_alpha_channel(gpu_device):
    """hellinger_loss(histBlock(img, pre_relu=True, weight=alpha, weight_grad=True)) puts a gradient into channel 3 of the
    image the alpha was taken from; without the flag (the detached map of hist_alpha_weight alone) it puts none."""
    from histogan_amd.hist import hellinger_loss
    from histogan_amd.trainer import _alpha_weight, _alpha_weight_grad
    g = torch.Generator().manual_seed(3)
    base = (torch.rand(2, 4, 32, 32, generator=g) * 1.2 - 0.1).to(gpu_device)
    blk = make_block('rgbuv', gpu_device, h=16, insz=32)
    target = blk(torch.rand(2, 3, 32, 32, generator=g).to(gpu_device)).detach()
    img = base.clone().requires_grad_(True)
    hellinger_loss(target, blk(img, pre_relu=True, weight=_alpha_weight_grad(img), weight_grad=True), 2.0).backward()
    ga, gc = img.grad[:, 3].clone(), img.grad[:, :3].clone()
    assert bool(torch.isfinite(img.grad).all()) and float(ga.abs().max()) > 0.0
    a = base[:, 3]
    assert float((ga * ((a < 0) | (a > 1))).abs().max()) == 0.0
    img2 = base.clone().requires_grad_(True)
    hellinger_loss(target, blk(img2, pre_relu=True, weight=_alpha_weight(img2)), 2.0).backward()
    assert float(img2.grad[:, 3].abs().max()) == 0.0
    assert torch.equal(img2.grad[:, :3], gc)                            # the colours' gradient is the same either way
