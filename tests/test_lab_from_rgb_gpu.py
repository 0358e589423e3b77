"""`LabHistBlock(from_rgb=True)` on the MI355X: the HG_PROJ_LAB projection of include/hg_hist.h on every kernel route a
one-plane projection takes, forward and backward, against the fp64 definition of tests/lab_ref.py; the stand-alone
conversions of histogan_amd/post.py; and the cross-check against the reference-checked `direct` path.

Bars (tests/test_hist_planes_gpu.py): histogram relmax <= 1e-5, grad_x and grad_weight relmax <= 1e-4.  Every shape is the
smallest that reaches its kernel; inputs come from torch.rand with Generator().manual_seed(0) unless a case says otherwise."""
import numpy as np
import pytest
import torch

import lab_ref as R
from conftest import relmax

pytestmark = pytest.mark.gpu

IQ16 = dict(h=16)


def _block(**kw):
    from histogram_classes.LabHistBlock import LabHistBlock
    return LabHistBlock(device='cuda', from_rgb=True, **kw)


def _route(x, kw, weight=None, weight_grad=False):
    from histogan_amd import _lib as L
    from histogan_amd.hist import _make_params
    p, keep = _make_params(x, _block(**kw)._config(), False, weight)
    r = L.hist_route(p, weight_grad)
    return L.HG_ROUTE_FWD[r.fwd], L.HG_ROUTE_BWD[r.bwd], r.planes_rt, r.rbf_radius


def _inputs(shape, h, wshape=None, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(*shape, generator=gen)
    go = torch.rand(shape[0], 1, h, h, generator=gen)
    w = None if wshape is None else torch.rand(*wshape, generator=gen) * 1.4 - 0.2     # values below 0 and above 1 present
    return x, go, w


def _run(dev, x, go, kw, w=None, weight_grad=False, x_dev=None, use_kw=None):
    """(hist, grad_x, grad_weight) of the module on the GPU, as CPU tensors.  use_kw: pass weight_grad explicitly."""
    xr = (x.to(dev) if x_dev is None else x_dev).detach().requires_grad_(True)
    wr = None if w is None else w.to(dev).requires_grad_(weight_grad)
    args = {} if w is None else {'weight': wr}
    if weight_grad or use_kw:
        args['weight_grad'] = weight_grad
    out = _block(**kw)(xr, **args)
    assert out.dtype == torch.float32 and out.is_cuda and out.shape == go.shape
    if out.requires_grad:
        out.backward(go.to(dev))
    gx = xr.grad if xr.grad is not None else torch.zeros_like(xr)
    gw = None if not weight_grad else wr.grad
    return out.detach().cpu(), gx.cpu(), None if gw is None else gw.cpu()


def _compare(tag, got, ref, weight_grad=False):
    e_f = relmax(got[0].numpy(), ref[0])
    e_b = relmax(got[1].numpy(), ref[1])
    e_w = relmax(got[2].numpy(), ref[2]) if weight_grad else 0.0
    print(f'{tag}: fwd {e_f:.2e}  grad_x {e_b:.2e}  grad_w {e_w:.2e}')
    assert np.isfinite(got[0].numpy()).all() and np.isfinite(got[1].numpy()).all()
    assert e_f <= R.FWD_TOL, (tag, e_f)
    assert e_b <= R.BWD_TOL, (tag, e_b)
    assert e_w <= R.BWD_TOL, (tag, e_w)


def test_reference_helper_is_anchored():
    assert R.check_anchors() <= 1e-3


# (name, shape, ctor kwargs, forward route, backward route, planes_rt, rbf_radius)
ROUTE_CASES = [
    ('dense_t1_ragged', (2, 3, 20, 28), dict(h=16, intensity_scale=False), 'DENSE', 'PLANES', 1, 0),
    ('dense_t1_ragged_intensity', (2, 3, 20, 28), dict(h=16, intensity_scale=True), 'DENSE', 'PLANES', 1, 0),
    ('planes_t2_h64', (2, 3, 40, 40), dict(h=64, intensity_scale=True), 'DENSE', 'PLANES', 2, 0),
    ('planes_t4_h128', (1, 3, 32, 32), dict(h=128, intensity_scale=True), 'DENSE', 'PLANES', 4, 0),
    ('generic_h130', (1, 3, 16, 16), dict(h=130, intensity_scale=True), 'DENSE', 'GENERIC', 0, 0),
    ('rbf_scatter_gather', (2, 3, 20, 28), dict(h=32, method='RBF', sigma=0.01, intensity_scale=True), 'RBF_SCATTER', 'RBF_GATHER', 0, 2),
    ('rbf_dense', (2, 3, 20, 28), dict(h=32, method='RBF', sigma=0.05, intensity_scale=True), 'DENSE', 'PLANES', 1, 0),
]


@pytest.mark.parametrize('name,shape,kw,fwd,bwd,rt,radius', ROUTE_CASES, ids=[c[0] for c in ROUTE_CASES])
def test_routes_forward_backward(name, shape, kw, fwd, bwd, rt, radius, gpu_device):
    x, go, _ = _inputs(shape, kw['h'])
    assert _route(x.to(gpu_device), kw) == (fwd, bwd, rt, radius)
    _compare(name, _run(gpu_device, x, go, kw), R.fwd_bwd(x, go, **kw))


def test_thresholding_scatter_gather(gpu_device):
    kw = dict(h=16, method='thresholding', intensity_scale=True)
    x, go, _ = _inputs((2, 3, 20, 28), 16)
    assert _route(x.to(gpu_device), kw)[:2] == ('THR_SCATTER', 'THR_GATHER')
    # the 0/1 windows are discontinuous: the comparison is meaningful when no coordinate sits within rounding distance of
    # a window edge (correct implementations disagree by at most 6e-8 in a coordinate)
    bins = torch.linspace(0, 1, 16, dtype=torch.float64)
    edges = torch.cat([bins - 1.0 / 32, bins + 1.0 / 32])
    margin = float((R.coordinates(x, **kw).unsqueeze(-1) - edges).abs().min())
    print(f'thresholding: smallest distance of a coordinate to a window edge {margin:.2e}')
    assert margin >= 1e-6
    _compare('thr', _run(gpu_device, x, go, kw), R.fwd_bwd(x, go, **kw))


RESIZE_CASES = [
    ('bilinear_37x53_to_24', (2, 3, 37, 53), dict(h=16, insz=24, intensity_scale=True)),
    ('bilinear_20x50_to_32', (2, 3, 20, 50), dict(h=16, insz=32, intensity_scale=True)),
    ('sampling_45x70', (2, 3, 45, 70), dict(h=16, insz=32, resizing='sampling', intensity_scale=True)),
]


@pytest.mark.parametrize('name,shape,kw', RESIZE_CASES, ids=[c[0] for c in RESIZE_CASES])
def test_resizes(name, shape, kw, gpu_device):
    x, go, _ = _inputs(shape, kw['h'])
    _compare(name, _run(gpu_device, x, go, kw), R.fwd_bwd(x, go, **kw))


def test_input_layouts(gpu_device):
    kw = dict(h=16, intensity_scale=True)
    x, go, _ = _inputs((2, 3, 20, 28), 16)
    ref = R.fwd_bwd(x, go, **kw)
    # C = 4: the first three channels are used, the fourth gets a zero gradient
    x4 = torch.cat([x, torch.rand(2, 1, 20, 28, generator=torch.Generator().manual_seed(5))], dim=1)
    got = _run(gpu_device, x4, go, kw)
    assert bool((got[1][:, 3] == 0).all())
    _compare('C=4', (got[0], got[1][:, :3], None), ref)
    # channels-last storage (permuted strides)
    xl = x.permute(0, 2, 3, 1).contiguous().to(gpu_device).permute(0, 3, 1, 2)
    assert not xl.is_contiguous()
    _compare('channels-last', _run(gpu_device, x, go, kw, x_dev=xl), ref)
    # another float type is converted
    _compare('float64', _run(gpu_device, x, go, kw, x_dev=x.double().to(gpu_device)), ref)


@pytest.mark.parametrize('name,shape,kw', [('none', (2, 3, 20, 28), dict(h=16, intensity_scale=True)), RESIZE_CASES[0]],
                         ids=['no_resize', 'bilinear'])
def test_weight_maps(name, shape, kw, gpu_device):
    B, _, H, W = shape
    x, go, w = _inputs(shape, kw['h'], wshape=(B, 1, H, W))
    assert bool((w < 0).any()) and bool((w > 1).any())
    const = _run(gpu_device, x, go, kw, w=w)
    _compare(f'map {name}', const, R.fwd_bwd(x, go, w=w, **kw))
    wg = _run(gpu_device, x, go, kw, w=w, weight_grad=True)
    _compare(f'map gradient {name}', wg, R.fwd_bwd(x, go, w=w, weight_grad=True, **kw), weight_grad=True)
    assert bool((wg[2][(w < 0) | (w > 1)] == 0).all())
    # the keyword changes nothing but the map's gradient
    off = _run(gpu_device, x, go, kw, w=w, use_kw=True)
    for a in (wg, off):
        assert torch.equal(a[0], const[0]) and torch.equal(a[1], const[1])


def test_edge_pixels(gpu_device):
    kw = dict(h=16, intensity_scale=True)
    x = R.edge_image()
    go = torch.rand(1, 1, 16, 16, generator=torch.Generator().manual_seed(0))
    got = _run(gpu_device, x, go, kw)
    _compare('edge', got, R.fwd_bwd(x, go, **kw))
    out_of_range = (x < 0) | (x > 1)
    assert int(out_of_range.sum()) == 2 and bool((got[1][out_of_range] == 0).all())


def _strided(gen, dev):
    big = torch.rand(2, 3, 40, 56, generator=gen).to(dev)
    return big[:, :, ::2, 1::2]


def test_standalone_conversions(gpu_device):
    from histogan_amd import post
    gen = torch.Generator().manual_seed(0)
    images = [torch.rand(2, 3, 20, 28, generator=gen).to(gpu_device), R.edge_image().to(gpu_device), _strided(gen, gpu_device)]
    tol = 2.0 ** -23
    for x in images:
        lab = post.srgb_to_lab(x)
        assert lab.dtype == torch.float32 and lab.is_contiguous() and lab.shape == x.shape
        ref_lab = R.convert_image(x.cpu())
        e1 = float((lab.cpu().double() - ref_lab).abs().max())
        lab32 = ref_lab.float()                                   # the fp32 Lab values the helper produced
        src = lab32.to(gpu_device)
        if not x.is_contiguous():                                 # the inverse from a strided view too
            pad = torch.zeros(2, 3, 40, 56, device=gpu_device)
            pad[:, :, ::2, 1::2] = src
            src = pad[:, :, ::2, 1::2]
        rgb = post.lab_to_srgb(src)
        e2 = float((rgb.cpu().double() - R.convert_image(lab32, inverse=True)).abs().max())
        print(f'srgb_to_lab {tuple(x.shape)} contiguous={x.is_contiguous()}: {e1:.2e}   lab_to_srgb: {e2:.2e}')
        assert e1 <= tol and e2 <= tol
        assert float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0
    assert post.srgb_to_lab(images[0][0]).shape == (3, 20, 28)    # (3, H, W) comes back as (3, H, W)
    with pytest.raises(ValueError, match='from_rgb=True'):
        post.srgb_to_lab(images[0].clone().requires_grad_(True))


@pytest.mark.parametrize('shape,kw', [((2, 3, 20, 28), dict(h=16, intensity_scale=True)),
                                      ((2, 3, 45, 70), dict(h=16, insz=32, resizing='sampling', intensity_scale=True))],
                         ids=['no_resize', 'sampling'])
def test_fused_projection_equals_convert_then_direct(shape, kw, gpu_device):
    """Ties the new path to the reference-checked one: converting per pixel commutes with a resize that only picks pixels."""
    from histogan_amd import post
    from histogram_classes.LabHistBlock import LabHistBlock
    x, _, _ = _inputs(shape, kw['h'])
    xd = x.to(gpu_device)
    fused = _block(**kw)(xd)
    two_step = LabHistBlock(device='cuda', **kw)(post.srgb_to_lab(xd))
    e = relmax(fused.cpu().numpy(), two_step.cpu().numpy())
    print(f'fused vs srgb_to_lab + direct {shape}: relmax {e:.2e}, bit-identical: {torch.equal(fused, two_step)}')
    assert e <= 1e-5


def test_refusals(gpu_device, monkeypatch):
    from histogan_amd import hist as HH
    from histogram_classes.LabHistBlock import LabHistBlock
    x, go, _ = _inputs((2, 3, 20, 28), 16)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        HH.rgbuv_hist(x, HH.HistConfig(h=16, projection='lab'))
    # device='cpu' is the HIP-free implementation: it never reaches the autograd Function that launches the kernels
    def boom(*a, **k):
        raise AssertionError('device="cpu" reached the HIP path')
    monkeypatch.setattr(HH.RGBuvHistFunction, 'apply', boom)
    out = LabHistBlock(h=16, device='cpu', from_rgb=True)(x.to(gpu_device))
    assert out.device.type == 'cpu' and relmax(out.numpy(), R.fwd_bwd(x, go, h=16)[0]) <= R.FWD_TOL
