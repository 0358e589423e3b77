"""Differentiable weight maps (`weight_grad=True`), `device='cpu'` path, host glue and the C-ABI argument checks.  No GPU.

The map's gradient is held against the double-precision statement of the definition (tests/hist_weight_ref.py::definition,
differentiated by autograd with respect to w) under the project's gradient bar BWD_TOL = 1e-4, max-norm relative: dL/dw_n
is the per-pixel sum that dL/dIy already contributes to grad_x under that bar.  Maps come from make_weight (exact 0 and 1
rows) with two rows at -0.3 and two at 1.4 on top, so the clamp's mask (0 <= w <= 1 passes, both ends inclusive) is
exercised in every case."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import relmax
from hist_weight_ref import BWD_TOL, definition, make_block, sample_image
from test_hist_weight_cpu import DEF_CASES, make_weight

NEG_ROWS, POS_ROWS, ZERO_ROWS, ONE_ROWS = slice(6, 8), slice(9, 11), slice(0, 4), slice(-4, None)


def masked_weight(layout, B, H, W, gen):
    """make_weight's map (rows 0..3 exactly 0, the last four exactly 1) with rows 6, 7 at -0.3 and rows 9, 10 at 1.4."""
    w = make_weight(layout, B, H, W, gen)
    v = w[:, 0] if w.dim() == 4 else w
    v[:, NEG_ROWS] = -0.3
    v[:, POS_ROWS] = 1.4
    return w


def definition_grad_w(x, w, go, proj, kw, pre_relu):
    """(dL/dw, dL/dx) of <definition(x, w), go>, fp64 numpy; thresholding on the fp32 projection, as definition_fwd_bwd."""
    dt = torch.float32 if kw.get('method') == 'thresholding' else torch.float64
    xr = x.detach().clone().requires_grad_(True)
    wr = w.detach().clone().contiguous().requires_grad_(True)
    hist = definition(xr, wr, projection=proj, pre_relu=pre_relu, proj_dtype=dt, **kw)
    hist.backward(go.double())
    gx = xr.grad if xr.grad is not None else torch.zeros_like(xr)
    return wr.grad.double().numpy(), gx.double().numpy()


def on_device(w, layout, device):
    """The map on `device` in the layout of the case (the strided view stays non-contiguous there)."""
    if layout == 'strided' and device != 'cpu':
        buf = torch.zeros(w.shape[0], w.shape[1], 2 * w.shape[2], device=device)
        buf[:, :, ::2] = w.to(device)
        wd = buf[:, :, ::2]
        assert not wd.is_contiguous()
        return wd
    return w.clone().to(device)


def check_weight_grad(proj, kw, shape, layout, pre_relu, device, seed=9):
    """Returns (error of the map's gradient against the definition, its reference, the block's map gradient (CPU), the map).
    Asserts what needs no tolerance: the shape of the gradient, x.grad bit-equal to the call with a detached map, exact zeros
    under the clamp's mask."""
    g = torch.Generator().manual_seed(seed)
    x = sample_image(*shape, g)
    B, _, H, W = shape
    w = masked_weight(layout, B, H, W, g)
    blk = make_block(proj, device, **kw)
    call = (lambda xi, **k: blk(xi, pre_relu=True, **k)) if pre_relu else blk

    xg = x.clone().to(device).requires_grad_(True)
    wd = on_device(w, layout, device).requires_grad_(True)
    out = call(xg, weight=wd, weight_grad=True)
    go = torch.randn(out.shape, generator=g)
    out.backward(go.to(device))
    assert wd.grad is not None and wd.grad.shape == wd.shape

    x2 = x.clone().to(device).requires_grad_(True)
    out2 = call(x2, weight=wd.detach())
    assert torch.equal(out2, out.detach())
    if out2.requires_grad:
        out2.backward(go.to(device))
    gx2 = x2.grad if x2.grad is not None else torch.zeros_like(x2)
    gx1 = xg.grad if xg.grad is not None else torch.zeros_like(xg)
    assert torch.equal(gx1, gx2), 'x.grad moved with weight_grad=True'

    gw = wd.grad.detach().cpu().reshape(B, H, W)
    gref, gxref = definition_grad_w(x, w.reshape(B, H, W), go, proj, kw, pre_relu)
    assert float(gw[:, NEG_ROWS].abs().max()) == 0.0 and float(gw[:, POS_ROWS].abs().max()) == 0.0
    assert np.abs(gref[:, NEG_ROWS]).max() == 0.0 and np.abs(gref[:, POS_ROWS]).max() == 0.0
    assert np.abs(gref).max() > 0
    return relmax(gw.double().numpy(), gref), gref, gw, gx1.detach().cpu()


@pytest.mark.parametrize('proj,kw,shape,layout,pre_relu', DEF_CASES)
def test_cpu_weight_gradient_matches_the_definition(proj, kw, shape, layout, pre_relu):
    e, gref, gw, _ = check_weight_grad(proj, kw, shape, layout, pre_relu, 'cpu')
    print(f'cpu weight gradient {proj} {kw} {layout}: {e:.2e}')
    assert e <= BWD_TOL


def test_cpu_clamp_mask_is_inclusive_at_both_ends():
    """Rows at exactly 0 and exactly 1 receive gradient (torch.clamp's rule), rows at -0.3 and 1.4 exactly none."""
    proj, kw, shape, layout, pre_relu = DEF_CASES[6]                 # no resize: the map's rows are the histogram's
    assert shape[2] <= kw['insz'] and shape[3] <= kw['insz']
    _, gref, gw, _ = check_weight_grad(proj, kw, shape, layout, pre_relu, 'cpu')
    assert float(gw[:, NEG_ROWS].abs().max()) == 0.0 and float(gw[:, POS_ROWS].abs().max()) == 0.0
    assert float(gw[:, ZERO_ROWS].abs().max()) > 0.0 and float(gw[:, ONE_ROWS].abs().max()) > 0.0


@pytest.mark.parametrize('proj', ['rgbuv', 'rgchroma', 'direct'])
def test_cpu_b1hw_map_gets_a_gradient_of_its_shape_and_errors(proj):
    x = torch.rand(2, 3, 20, 24)
    blk = make_block(proj, 'cpu', h=8, insz=32)
    w = torch.rand(2, 1, 20, 24, requires_grad=True)
    blk(x, weight=w, weight_grad=True).sum().backward()              # the sum is ~1 per image: tiny but defined
    assert w.grad.shape == (2, 1, 20, 24)
    blk(x, weight=w, weight_grad=True)[:, :, 2, 3].sum().backward()
    assert float(w.grad.abs().max()) > 0.0
    with pytest.raises(ValueError, match='weight_grad=True needs a weight map'):
        blk(x, weight_grad=True)
    with pytest.raises(ValueError, match='requires grad'):           # the default keyword keeps refusing such a map
        blk(x, weight=torch.rand(2, 20, 24, requires_grad=True))
    with pytest.raises(ValueError, match='requires grad'):
        blk(x, weight=torch.rand(2, 20, 24, requires_grad=True), weight_grad=False)
    assert torch.equal(blk(x, weight=w.detach(), weight_grad=True), blk(x, weight=w.detach()))
    assert not torch.cuda.is_initialized(), 'the CPU path initialised the GPU'


def test_keyword_reaches_every_layer():
    import inspect
    from histogan_amd import hist as HH
    from histogan_amd import hist_cpu as HC
    assert inspect.signature(HH.run_block).parameters['weight_grad'].default is False
    assert inspect.signature(HC.hist_cpu).parameters['weight_grad'].default is False
    assert list(inspect.signature(HH.rgbuv_hist_wgrad).parameters) == ['x', 'cfg', 'pre_relu', 'weight']
    assert inspect.signature(HH.check_weight).parameters['weight_grad'].default is False


@pytest.fixture(scope='module')
def L():
    from histogan_amd import build
    build.build()
    import histogan_amd._lib as L
    return L


def _params(L, **kw):
    p = L.HgHistParams()
    p.struct_size = ctypes.sizeof(L.HgHistParams)
    p.B, p.C, p.H, p.W = 2, 3, 16, 16
    p.stride_b, p.stride_c, p.stride_h, p.stride_w = 3 * 256, 256, 16, 1
    p.Hs, p.Ws, p.resize_mode = 16, 16, 0
    p.h, p.lo, p.hi, p.method, p.sigma = 64, -3.0, 3.0, 2, 0.02
    p.intensity_scale, p.green_only = 1, 0
    p.weight, p.weight_stride_b, p.weight_stride_h, p.weight_stride_w = 0x1000, 256, 16, 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_abi_version_and_workspace_of_the_weight_gradient(L):
    assert L.lib.hg_version() >= 105
    assert {'hg_rgbuv_hist_bwd_w', 'hg_rgbuv_hist_bwd_w_workspace_bytes'} <= set(L.EXPORTS)
    f, b, n = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    q = lambda **kw: L.lib.hg_rgbuv_hist_bwd_w_workspace_bytes(ctypes.byref(_params(L, **kw)), ctypes.byref(n))
    assert q() == 0
    assert L.lib.hg_rgbuv_hist_workspace_bytes(ctypes.byref(_params(L)), ctypes.byref(f), ctypes.byref(b)) == 0
    assert n.value == b.value                                       # no resize: the gradient goes straight to grad_weight
    # bilinear 16 x 16 -> 8 x 8: one more plane of B * 64 floats (rounded up to 256 bytes) than hg_rgbuv_hist_bwd
    rs = dict(Hs=8, Ws=8, resize_mode=1)
    assert q(**rs) == 0
    assert L.lib.hg_rgbuv_hist_workspace_bytes(ctypes.byref(_params(L, **rs)), ctypes.byref(f), ctypes.byref(b)) == 0
    assert n.value == b.value + 2 * 64 * 4
    assert q(weight=0) == -1                                        # HG_EINVAL: no map to differentiate
    assert q(weight_stride_b=0) == -5 and q(weight_stride_h=0) == -5 and q(weight_stride_w=0) == -5   # HG_EUNSUPPORTED
    assert q(method=7) == -2 and q(struct_size=8) == -1


def test_abi_weight_gradient_arguments_rejected_before_any_launch(L):
    """NULL grad_weight, NULL p->weight, a zero stride and a short workspace all return before anything is enqueued (the
    pointers below are not device memory: a launch would fault)."""
    n = ctypes.c_size_t()
    p = _params(L, Hs=8, Ws=8, resize_mode=1)
    assert L.lib.hg_rgbuv_hist_bwd_w_workspace_bytes(ctypes.byref(p), ctypes.byref(n)) == 0
    a = 0x1000
    call = lambda p, gw, nbytes: L.lib.hg_rgbuv_hist_bwd_w(ctypes.byref(p), a, a, a, a, a, gw, a, nbytes, None)
    assert call(p, None, n.value) == -1                             # grad_weight == NULL: HG_EINVAL
    assert call(_params(L, weight=0), a, n.value) == -1             # p->weight == NULL: HG_EINVAL
    assert call(_params(L, weight_stride_b=0), a, n.value) == -5    # broadcast map: HG_EUNSUPPORTED
    assert call(_params(L, weight_stride_w=0), a, n.value) == -5
    assert call(p, a, n.value - 1) == -4                            # HG_EWORKSPACE
    assert call(p, a, 0) == -4
    assert L.lib.hg_rgbuv_hist_bwd_w(ctypes.byref(p), None, None, None, None, None, a, None, 0, None) == -1
    # hg_rgbuv_hist_bwd itself still accepts its own (smaller) workspace size and a broadcast map: checked up to the launch
    f, b = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.lib.hg_rgbuv_hist_workspace_bytes(ctypes.byref(p), ctypes.byref(f), ctypes.byref(b)) == 0
    assert b.value < n.value
    assert L.lib.hg_rgbuv_hist_bwd(ctypes.byref(p), a, a, a, a, a, a, b.value - 1, None) == -4


def test_trainer_flag_needs_the_alpha_weight():
    from histogan_amd.trainer import Trainer
    with pytest.raises(ValueError, match='hist_alpha_grad=True needs hist_alpha_weight=True'):
        Trainer('t', '/nonexistent/results', '/nonexistent/models', 32, 2, transparent=True, hist_alpha_grad=True)


def test_generated_alpha_with_its_graph():
    """The differentiable twin of _alpha_weight: ordinary images keep the graph to their alpha channel; an image whose alpha
    is nowhere positive is weighed by constant ones and sends no gradient to its alpha."""
    from histogan_amd.trainer import _alpha_weight, _alpha_weight_grad
    base = torch.rand(3, 4, 8, 8)
    base[0, 3] = -0.2                      # fully transparent
    base[1, 3, :4] = -1.0                  # half transparent
    base[2, 3, 0] = 1.7                    # partly beyond 1
    img = base.clone().requires_grad_(True)
    w = _alpha_weight_grad(img)
    assert w.shape == (3, 8, 8) and w.requires_grad
    assert torch.equal(w.detach().clamp(0, 1), _alpha_weight(img))  # the histogram clamps: the same weights as the constant map
    assert torch.equal(w[0].detach(), torch.ones(8, 8))
    blk = make_block('rgbuv', 'cpu', h=8, insz=32)
    out = blk(img, pre_relu=True, weight=w, weight_grad=True)
    (out * torch.linspace(-1, 1, 8)).sum().backward()
    ga = img.grad[:, 3]
    assert float(ga[0].abs().max()) == 0.0                          # all transparent: no gradient to its alpha
    assert float(ga[1, 4:].abs().max()) > 0.0 and float(ga[1, :4].abs().max()) == 0.0
    assert float(ga[2, 1:].abs().max()) > 0.0 and float(ga[2, 0].abs().max()) == 0.0
    assert float(img.grad[:, :3].abs().max()) > 0.0
