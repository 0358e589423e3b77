"""GPU parity of the plane-after-plane branch of the scatter forwards (k_hist_thr_fwd / k_hist_rbf_fwd with ALL3 = false):
three planes whose 64-bit LDS grids do not fit together (81 <= h <= 141), so one grid is filled, flushed and cleared per
plane, and the matching gathers (k_hist_thr_bwd / k_hist_rbf_bwd).  Every other thresholding / RBF case with h > 80 is
green_only: one plane, which takes the all-grids-at-once branch.  Bars and norms of tests/test_hist_gpu.py; the oracle is
oracle/rgbuv_hist.py.  Each case first asks the library's own route query whether it is where it claims to be."""
import pytest
import torch

from conftest import relmax
from test_hist_gpu import BWD_TOL, FWD_TOL, _block

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 24, 28)


def _image(seed):
    """As test_thresholding_scatter_matches_oracle: values in [-0.1, 1.1], exact zeros, exact ones, one constant plane."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(*SHAPE, generator=g) * 1.2 - 0.1
    x[0, 2] = 0.25
    x[0, :, :4] = 0.0
    x[1, :, 5:9, 5:9] = 1.0
    return x, g


def _route(x, kw):
    from histogan_amd import hist as HH
    from histogan_amd._lib import HG_ROUTE_FWD, hist_route
    cfg = HH.HistConfig(projection='rgbuv', **{k: (list(v) if k == 'hist_boundary' else v) for k, v in kw.items()})
    p, keep = HH._make_params(x, cfg)
    r = hist_route(p)
    return HG_ROUTE_FWD[r.fwd], r.rbf_radius


def _check(kw, want_fwd, gpu_device, want_radius=None):
    from oracle import rgbuv_hist as O
    h = kw['h']
    x, g = _image(h + (0 if want_radius is None else 1))
    assert not kw.get('green_only', False)
    fwd, radius = _route(x.to(gpu_device), kw)
    assert fwd == want_fwd and 3 * h * h * 8 > 150 * 1024, (fwd, h)      # three planes, grids that do not fit together
    if want_radius is not None:
        assert radius == want_radius, radius
    blk = _block(kw)
    xg = x.to(gpu_device).requires_grad_(True)
    out = blk(xg)
    go = torch.randn(out.shape, generator=g)
    out.backward(go.to(gpu_device))
    xo = x.clone().requires_grad_(True)
    ref = O.rgbuv_hist(xo, **kw)
    assert out.shape == ref.shape == (SHAPE[0], 3, h, h)
    e_f = relmax(out.detach().cpu().numpy(), ref.detach().numpy())
    print(f'plane-after-plane {kw}: fwd {e_f:.2e}')
    assert e_f <= FWD_TOL
    if kw['method'] == 'thresholding' and not kw.get('intensity_scale', True):
        # counts only: the window has no slope -- exactly zero, through the gather and the resize adjoint
        assert not ref.requires_grad
        assert float(xg.grad.abs().max()) == 0.0
    else:
        ref.backward(go)
        gr = xo.grad.numpy()
        assert bool(torch.isfinite(xo.grad).all())
        e_b = relmax(xg.grad.cpu().numpy(), gr)
        print(f'plane-after-plane {kw}: grad {e_b:.2e}')
        assert e_b <= BWD_TOL
    assert torch.equal(blk(x.to(gpu_device)), out.detach())              # integer LDS atomics: order-independent


THR_PLANE_CASES = [
    dict(h=81, insz=64, intensity_scale=True),                                   # smallest h of the branch, one bin per value
    dict(h=81, insz=64, hist_boundary=[0.5, 3.0]),                               # eps = 3.5/81 > spacing 2.5/80: two windows can hit
    dict(h=141, insz=20, intensity_scale=False, resizing='interpolation'),       # largest grid that fits; gradient exactly zero
    dict(h=96, insz=20, resizing='sampling'),
]


@pytest.mark.parametrize('kw', THR_PLANE_CASES)
def test_thresholding_plane_after_plane_matches_oracle(kw, gpu_device):
    _check(dict(method='thresholding', **kw), 'THR_SCATTER', gpu_device)


RBF_PLANE_CASES = [
    (dict(h=81, insz=64, sigma=0.01), 1),                                        # spacing 0.075: radius 1
    (dict(h=81, insz=64, sigma=0.02), 2),                                        # radius 2
    (dict(h=96, insz=20, sigma=0.015, hist_boundary=[-2.0, 3.0], resizing='interpolation'), 2),
]


@pytest.mark.parametrize('kw,radius', RBF_PLANE_CASES)
def test_rbf_plane_after_plane_matches_oracle(kw, radius, gpu_device):
    _check(dict(method='RBF', **kw), 'RBF_SCATTER', gpu_device, want_radius=radius)
